"""Every optimizer-step kernel of csrc/optim.hip at every row of tests/optim_matrix.py ROWS, exact, guarded.

The block sums, the bf16 wire, the whole-buffer clip, the finalize on hand-made partials, Adam + EMA + the bf16 image
on both templates and the cast run every row on the exact and on the soft family (the capped-grid rows on the exact
family alone). The recorded launch plan must name the row's kernel and grid. After every call nothing but the declared
outputs may have changed, bit for bit -- inputs, the workspace past nb floats, an absent ema or params_bf16, the state
words a branch leaves alone. Then the statements of tests/optim_matrix.py: bitwise partials, norms, moments and
parameters in the exact family, the K u T bounds in the soft one, a bitwise EMA, bf16 image and wire in both, the
state words against the numpy.float32 model, the same partial from every entry point. A second identical call gives
identical bits. Each test prints its worst error / bound per quantity and family.

Also every error return: -1 or -3, nothing launched, nothing written."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_matrix as OM

pytestmark = pytest.mark.gpu


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = OM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert OM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _within(got, ref, lim, what, tag, seen):
    assert not bool(torch.isnan(got).any()), f"{tag}: {what} holds NaN"
    err = (got - ref).abs()
    w = float((err / lim.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    seen[what] = max(seen.get(what, 0.0), w)
    assert bool((err <= lim).all()), f"{tag}: {what} worst error / bound {w:.3f}"


def _same(got, ref, what, tag):
    assert OM.same_bits(got, ref), f"{tag}: {what} differs from its bitwise value " \
        f"in {int((got != ref).sum()) if got.shape == ref.shape else 'shape'} elements"


def _report(tag, seen):
    print(f"{tag}: max(err / bound) " + (", ".join(f"{k} {v:.3f}" for k, v in sorted(seen.items())) or "bitwise"))


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _rejected(L, g, fn, tag, code=-1):
    rc, ops = OM.recorded(L, fn)
    assert rc == code, f"{tag}: returned {rc}, documented {code}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: a rejected call changed {g.changed()}"


def _words_match(got, want, tag, upto=8):
    for i in range(upto):
        same = (np.isnan(got[i]) and np.isnan(want[i])) or got[i].tobytes() == want[i].tobytes()
        assert same, f"{tag}: state[{i}] is {got[i]!r}, the model says {want[i]!r}"


def _check_partials(p, g, kind, tag, seen):
    got, ref = p.partials().double(), OM.block_sums(g)
    _within(got, ref, OM.K_N * OM.U24 * ref, "partial", tag, seen)
    if kind == "exact":
        assert torch.equal(got, ref), f"{tag}: a partial is not the integer sum of squares"
    return got


# ----------------------------------------------------------------------------------------------------------------
# the block sums and the bf16 wire
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", OM.rows_of(OM.SUMSQ, OM.WIDEN), ids=OM.row_id)
def test_block_sum_rows(row):
    L = _L()
    n = row.dims[0]
    assert L.sdmi_norm_block() == OM.NORM_BLK and L.sdmi_optim_workspace() == OM.optim_workspace()
    assert L.sdmi_optim_workspace_for(n) == OM.optim_workspace_for(n)
    wire, partial = row.entry == OM.WIDEN, OM.opt(row, "partial", 1)
    for kind in OM.FAMILIES:
        tag, seen = f"{OM.row_id(row)} {kind}", {}
        g = OM.norm_case(kind, n, wire)
        p = OM.NormProblem(g, kind, wire=wire)
        gd = p.guard(ws=bool(partial), dst=wire)
        call = (lambda: p.widen(L, _stream(), partial=bool(partial))) if wire else (lambda: p.sumsq(L, _stream()))
        _run(L, call, row.launches, tag)
        _unchanged(gd, tag)
        if wire:
            _same(p.dst.data.cpu(), g.float(), "the widened gradients", tag)
        if partial:
            first = _check_partials(p, g, kind, tag, seen)
            assert call() == 0
            torch.cuda.synchronize()
            assert torch.equal(p.partials().double(), first), f"{tag}: a second identical call gives other bits"
        _report(tag, seen)


@pytest.mark.parametrize("row", OM.rows_of(OM.CLIP), ids=OM.row_id)
def test_clip_rows_and_the_same_partial_from_every_entry_point(row):
    L = _L()
    n = row.dims[0]
    for kind in OM.FAMILIES:
        tag, seen = f"{OM.row_id(row)} {kind}", {}
        g = OM.norm_case(kind, n, True)          # values exact in bf16, so the wire carries the same gradients
        s = OM.NORM_STATE[kind]
        p = OM.NormProblem(g, kind, wire=True)
        gd = p.guard(ws=True, state=True)
        _run(L, lambda: p.clip(L, _stream()), row.launches, tag)
        _unchanged(gd, tag)
        whole = _check_partials(p, g, kind, tag, seen)
        words = p.words()
        ref = float(torch.sqrt(OM.block_sums(g).sum())) / (s["scale"] * s["div"])
        _within(torch.tensor([float(words[0])], dtype=torch.float64), torch.tensor([ref], dtype=torch.float64),
                torch.tensor([OM.norm_bound(ref)], dtype=torch.float64), "norm", tag, seen)
        assert words[0] == OM.norm_model(float(whole.sum()), s["scale"], s["div"])[0], f"{tag}: state[0] is not the norm of its partials"
        if kind == "exact":
            assert words[0] == OM.norm_model(float(OM.block_sums(g).sum()), s["scale"], s["div"])[0]
        _words_match(words, OM.finalize_model(words[0], p.start, s["maxn"], 2000, 0, s["div"]), tag)
        # the pieces: block-aligned ranges through sdmi_sumsq_blocks, then the wire, each followed by the finalize
        cuts = [0] + [b * OM.NORM_BLK for b in range(1, p.nb)][-1:] + [n]      # (three blocks: two and one)
        for name in ("pieces", "wire"):
            q = OM.NormProblem(g, kind, wire=True)
            gd = q.guard(ws=True, state=True, dst=name == "wire")
            if name == "pieces":
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    assert q.sumsq(L, _stream(), lo, hi) == 0
            else:
                assert q.widen(L, _stream()) == 0
            assert L.sdmi_clip_finalize(OM.ptr(q.ws.data), q.nb, s["maxn"], OM.ptr(q.state.data), 2000, 0, s["div"],
                                        _stream()) == 0
            torch.cuda.synchronize()
            _unchanged(gd, f"{tag} {name}")
            assert torch.equal(q.partials().double(), whole), f"{tag}: the {name} give other partials than the whole buffer"
            _words_match(q.words(), words, f"{tag} {name}")
        _report(tag, seen)


# ----------------------------------------------------------------------------------------------------------------
# the finalize: partial counts, every branch of the state machine, the loss flag
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", OM.rows_of(OM.FIN), ids=OM.row_id)
def test_finalize_rows(row):
    L = _L()
    k = row.dims[0]
    for kind in OM.FAMILIES:
        tag = f"{OM.row_id(row)} {kind}"
        parts = OM.finalize_parts(kind, k)
        start = np.array([OM.NAN, OM.NAN, 8.0, 1.0, 5.0, OM.NAN, 1.5, 0.0], dtype=OM.f32)
        p = OM.FinalizeProblem(parts, start)
        gd = p.guard()
        _run(L, lambda: p.run(L, _stream(), 1.0, 3, 1, 1.0), row.launches, tag)
        _unchanged(gd, tag)
        words = p.words()
        assert words[0] == OM.norm_model(OM.partials_sum(parts), 8.0, 1.0)[0], f"{tag}: state[0] is not bitwise the norm"
        _words_match(words, OM.finalize_model(words[0], start, 1.0, 3, 1, 1.0), tag)


@pytest.mark.parametrize("case", OM.STATE_CASES, ids=lambda c: c["name"])
def test_state_machine_cases(case):
    L = _L()
    c, tag = case, case["name"]
    start = OM.state_words(c)
    parts = OM.case_partials(c)
    for trip in range(2):                       # the second trip starts from the same words: every bit repeats
        if c["grads"] is not None:
            p = OM.NormProblem(torch.tensor(c["grads"], dtype=torch.float64), "exact")
            p.state.put(torch.from_numpy(start))
            gd = p.guard(ws=True, state=True)
            _run(L, lambda: p.clip(L, _stream(), maxn=c["maxn"], gi=c["gi"], mode=c["mode"], div=c["div"]),
                 [("sumsq_block_kernel", 1), ("norm_finalize_kernel", 1)], tag)
        else:
            p = OM.FinalizeProblem(parts, start)
            gd = p.guard()
            _run(L, lambda: p.run(L, _stream(), c["maxn"], c["gi"], c["mode"], c["div"]), [("norm_finalize_kernel", 1)], tag)
        _unchanged(gd, tag)
        words = p.words()
        norm = OM.norm_model(float(np.sum(parts.astype(np.float64))), c["scale"], c["div"])[0]
        _words_match(words[:1], np.array([norm]), tag, upto=1)
        _words_match(words, OM.finalize_model(words[0], start, c["maxn"], c["gi"], c["mode"], c["div"]), tag)
        assert (int(words[5]), float(words[2]), float(words[3]), float(words[4])) == c["want"], f"{tag}: {words}"


@pytest.mark.parametrize("case", OM.FLAG_CASES, ids=str)
def test_loss_flag(case):
    L = _L()
    mode, value, want = case
    src, dst = OM.Win(1, "cuda").put(torch.tensor([value])), OM.Win(1, "cuda")
    gd = OM.Guard()
    gd.add("src", src)
    gd.add("dst", dst, [(0, 1)])
    _run(L, lambda: L.sdmi_loss_flag(OM.ptr(src.data), OM.ptr(dst.data), mode, _stream()), [("loss_flag_kernel", 1)], str(case))
    _unchanged(gd, str(case))
    assert dst.data.cpu().numpy()[0].tobytes() == OM.f32(want).tobytes(), f"{case}: wrote {float(dst.data[0])}"


# ----------------------------------------------------------------------------------------------------------------
# Adam + EMA + the bf16 image
# ----------------------------------------------------------------------------------------------------------------
def _adam_outputs(p):
    return {k: getattr(p, k).data.cpu() for k in p.OUT}


@pytest.mark.parametrize("row", OM.rows_of(OM.ADAM), ids=OM.row_id)
def test_adam_rows(row):
    L = _L()
    for kind in OM.FAMILIES[:1] if OM.opt(row, "big") else OM.FAMILIES:
        tag, seen = f"{OM.row_id(row)} {kind}", {}
        c = OM.row_case(kind, row)
        p = OM.AdamProblem(c, row)
        gd = p.guard()
        _run(L, lambda: p.run(L, _stream()), row.launches, tag)
        _unchanged(gd, tag)        # (a skipped step declares no output: p, m, v, ema and the image are untouched)
        out = _adam_outputs(p)
        if not p.skip:
            if kind == "exact":
                want = OM.adam_closed_form(c)
                for k in "mvp":
                    _same(out[k], want[k], k, tag)
                if p.with_ema:
                    _same(out["ema"], want["e"], "ema", tag)
            else:
                ref = OM.adam_reference(c)
                for k, K in (("m", OM.K_M), ("v", OM.K_V), ("p", OM.K_P)):
                    _within(out[k].double(), ref[k], K * OM.U24 * ref["T_" + k], k, tag, seen)
            if p.with_ema:
                e64, T_e, e_bits = OM.ema_reference(c, out["p"].double())
                _same(out["ema"], e_bits.float(), "ema against fma32(alpha, p, fl(ema decay))", tag)
                if kind == "soft":
                    _within(out["ema"].double(), e64, OM.K_E * OM.U24 * T_e, "ema", tag, seen)
            if p.with_pb:
                _same(out["pb"], out["p"].to(torch.bfloat16), "params_bf16 against RNE of the stored parameter", tag)
        first = p.raw()
        q = OM.AdamProblem(c, row)
        assert q.run(L, _stream()) == 0
        torch.cuda.synchronize()
        for a, b in zip(first, q.raw()):
            assert OM.same_bits(a.cpu(), b.cpu()), f"{tag}: a second identical call gives other bits"
        _report(tag, seen)


def test_v_is_the_abi_definition_and_differs_from_torch_by_the_complement_gap():
    """The GPU's v against both float64 models on a first step (m = v = 0, as the step the torch comparison of
    tests/test_gradscaler_gpu.py starts from): within K_V u of the ABI's, complement_gap away from torch's."""
    L = _L()
    row = [r for r in OM.rows_of(OM.ADAM) if r.dims == (1027,) and not r.opt][0]
    c = dict(OM.row_case("soft", row))
    c["m"], c["v"] = torch.zeros_like(c["m"]), torch.zeros_like(c["v"])
    p = OM.AdamProblem(c, row)
    assert p.run(L, _stream()) == 0
    torch.cuda.synchronize()
    v = p.v.data.cpu().double()
    abi = OM.adam_reference(c)
    torch_model = OM.adam_reference(c, comp2=OM.complement_torch(0.999), comp1=OM.complement_torch(0.9))
    gap = OM.complement_gap(0.999)
    d_abi = float(((v - abi["v"]).abs() / abi["v"]).max())
    d_torch = ((v - torch_model["v"]).abs() / torch_model["v"])
    print(f"v on the GPU: {d_abi:.3e} relative from the ABI's float64 model ({d_abi / OM.U24:.2f} u), "
          f"{float(d_torch.min()):.4e} .. {float(d_torch.max()):.4e} from torch's; complement gap {gap:.4e}")
    assert d_abi <= OM.K_V * OM.U24
    assert bool(((d_torch - gap).abs() <= (OM.K_V + 1) * OM.U24).all())


# ----------------------------------------------------------------------------------------------------------------
# the cast
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", OM.rows_of(OM.CAST), ids=OM.row_id)
def test_cast_rows(row):
    L = _L()
    for kind in OM.FAMILIES[:1] if OM.opt(row, "big") else OM.FAMILIES:
        tag = f"{OM.row_id(row)} {kind}"
        x = OM.cast_case(kind, row.dims[0])
        p = OM.CastProblem(x)
        gd = p.guard()
        _run(L, lambda: p.run(L, _stream()), row.launches, tag)
        _unchanged(gd, tag)
        _same(p.dst.data.cpu(), x.float().to(torch.bfloat16), "the image against RNE", tag)


# ----------------------------------------------------------------------------------------------------------------
# error returns (only arguments the host code rejects before any launch)
# ----------------------------------------------------------------------------------------------------------------
def test_norm_entry_points_reject_without_launching():
    L = _L()
    n = OM.NORM_BLK + 1
    p = OM.NormProblem(OM.norm_case("exact", n, True), "exact", wire=True)
    g, s = p.guard(), _stream()
    for name in ("grads", "state", "ws"):
        _rejected(L, g, lambda: p.clip(L, s, **{name: None}), f"clip: {name} null")
    for v in (0, -1):
        _rejected(L, g, lambda: p.clip(L, s, n=v), f"clip: n = {v}")
    _rejected(L, g, lambda: p.clip(L, s, grads=OM.ptr(p.g.data[1:])), "clip: grads 4 bytes off")
    _rejected(L, g, lambda: p.clip(L, s, ws_bytes=4 * p.nb - 4), "clip: ws_bytes = 4 nb - 4", code=-3)
    fixed = lambda: L.sdmi_clip_unscale(OM.ptr(p.g.data), OM.NORM_BLOCKS * OM.NORM_BLK + 1, 1.0,  # noqa: E731
                                        OM.ptr(p.state.data), OM.ptr(p.ws.data), 2000, 0, 1.0, s)
    _rejected(L, g, fixed, "clip_unscale: more blocks than the fixed workspace", code=-3)
    for name in ("grads", "partial"):
        _rejected(L, g, lambda: p.sumsq(L, s, **{name: None}), f"sumsq: {name} null")
    _rejected(L, g, lambda: p.sumsq(L, s, n=-1), "sumsq: n = -1")
    _rejected(L, g, lambda: p.sumsq(L, s, grads=OM.ptr(p.g.data[1:])), "sumsq: grads 4 bytes off")
    _rejected(L, g, lambda: p.sumsq(L, s, n=0), "sumsq: n = 0 is a no-op", code=0)
    for name in ("src", "dst"):
        _rejected(L, g, lambda: p.widen(L, s, **{name: None}), f"widen: {name} null")
    _rejected(L, g, lambda: p.widen(L, s, n=-1), "widen: n = -1")
    _rejected(L, g, lambda: p.widen(L, s, src=OM.ptr(p.src.data[1:])), "widen: src 2 bytes off")
    _rejected(L, g, lambda: p.widen(L, s, dst=OM.ptr(p.dst.data[1:])), "widen: dst 4 bytes off")
    _rejected(L, g, lambda: p.widen(L, s, n=0), "widen: n = 0 is a no-op", code=0)


def test_finalize_and_loss_flag_reject_without_launching():
    L = _L()
    p = OM.FinalizeProblem((9.0, 16.0), OM.state_words(OM.STATE_CASES[0]))
    g, s = p.guard(writes=False), _stream()
    for name in ("partial", "state"):
        _rejected(L, g, lambda: p.run(L, s, 1.0, 3, 0, 1.0, **{name: None}), f"finalize: {name} null")
    for v in (0, -1):
        _rejected(L, g, lambda: p.run(L, s, 1.0, 3, 0, 1.0, n=v), f"finalize: n = {v}")
    src, dst = OM.ptr(p.parts.data), OM.ptr(p.state.data)
    _rejected(L, g, lambda: L.sdmi_loss_flag(None, dst, 0, s), "loss_flag: src null")
    _rejected(L, g, lambda: L.sdmi_loss_flag(src, None, 0, s), "loss_flag: dst null")
    for mode in (-1, 2):
        _rejected(L, g, lambda: L.sdmi_loss_flag(src, dst, mode, s), f"loss_flag: mode {mode}")


def test_adam_and_cast_reject_without_launching():
    L = _L()
    row = [r for r in OM.rows_of(OM.ADAM) if r.dims == (1027,) and not r.opt][0]
    for pb in (1, 0):                                  # sdmi_adam_ema_bf16 and sdmi_adam_ema
        p = OM.AdamProblem(OM.row_case("exact", row), row._replace(opt=(("pb", pb),)))
        g, s = p.guard(writes=False), _stream()
        for name in ("p", "g", "m", "v", "state"):
            _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"adam pb={pb}: {name} null")
        _rejected(L, g, lambda: p.run(L, s, n=-1), f"adam pb={pb}: n = -1")
        _rejected(L, g, lambda: p.run(L, s, n=0), f"adam pb={pb}: n = 0 is a no-op", code=0)
    c = OM.CastProblem(OM.cast_case("exact", 1027))
    g = c.guard(writes=False)
    for name in ("src", "dst"):
        _rejected(L, g, lambda: c.run(L, s, **{name: None}), f"cast: {name} null")
    _rejected(L, g, lambda: c.run(L, s, n=-1), "cast: n = -1")
    _rejected(L, g, lambda: c.run(L, s, src=OM.ptr(c.src.data[1:])), "cast: src 4 bytes off")
    _rejected(L, g, lambda: c.run(L, s, dst=OM.ptr(c.dst.data[1:])), "cast: dst 2 bytes off")
    _rejected(L, g, lambda: c.run(L, s, n=0), "cast: n = 0 is a no-op", code=0)
