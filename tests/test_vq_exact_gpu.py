"""Every VQ latent-interface kernel of csrc/vqvae.hip at every row of tests/vq_matrix.py ROWS, exact, guarded.

sdmi_vq_quantize and sdmi_vq_bwd run every row on the exact and on the soft family, with the row's strides and with
operands that are column windows of wider NaN-filled buffers; the backward with three index distributions;
sdmi_pointwise_in on both families. The recorded launch plan must name the row's kernels and grids. After every call
nothing but the declared outputs may have changed, bit for bit -- inputs, pad columns, rows past the end, the
workspaces beyond what the launch writes, an absent xq and absent dw / db included. Then the statements of
tests/vq_matrix.py: bitwise xq, zq, dz_enc and the pointwise output with zero pads, an admissible index (the first
minimum of the integer d^2 in the exact family), the bounds on the loss, the four sums and demb (bitwise in the exact
family), exact zeros in the rows of unused codes. A second identical call gives identical bits. Each test prints its
worst error / bound per quantity and family.

Also the error returns: -1, nothing launched, nothing written."""
import ctypes

import pytest
import torch

from tests import vq_matrix as VM

pytestmark = pytest.mark.gpu
FAMILIES = ("exact", "soft")


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = VM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert VM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _within(got, ref, lim, what, tag, seen):
    assert not bool(torch.isnan(got).any()), f"{tag}: {what} holds NaN"
    err = (got - ref).abs()
    w = float((err / lim.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    seen[what] = max(seen.get(what, 0.0), w)
    assert bool((err <= lim).all()), f"{tag}: {what} worst error / bound {w:.3f}"


def _same(got, ref, what, tag):
    assert got.shape == ref.shape and torch.equal(got, ref), \
        f"{tag}: {what} differs in {int((got != ref).sum())} elements from its bitwise value"


def _report(tag, seen):
    print(f"{tag}: max(err / bound) " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(seen.items())))


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _repeatable(p, call, tag):
    first = p.raw()
    assert call() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, p.raw()):
        assert torch.equal(VM.bits(a), VM.bits(b)), f"{tag}: a second identical call gives other bits"


# ----------------------------------------------------------------------------------------------------------------
# sdmi_vq_quantize
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", VM.rows_of(VM.QUANT), ids=VM.row_id)
def test_quantize_rows(row):
    L = _L()
    B, HW, C, K = row.dims
    P = B * HW
    assert L.sdmi_vq_workspace(P) == VM.quant_workspace(P)
    for kind in FAMILIES:
        c, seen = VM.quant_case(kind, B, HW, C, K, VM.opt(row, "conv")), {}
        x, e = VM.conv_chain(c["z"], c["w"], c["b"]), c["codebook"]
        d64 = VM.dist2(x, e)
        if kind == "soft":
            adm, best = VM.admissible(x, e)
            one = adm.sum(1) == 1
            assert int((~one).sum()) <= 0.01 * P, "more than 1 % of the pixels have several admissible codes"
            tol = VM.K_D * VM.U24 * VM.dist_scale(x, e) + 2.0 ** -22 * d64
        for layout in VM.LAYOUTS:
            tag = f"{VM.row_id(row)} {kind} {layout}"
            p = VM.QuantProblem(c, row, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            out = p.outputs()
            idx = out["idx"]
            assert bool(((idx >= 0) & (idx < K)).all()), f"{tag}: an index outside the codebook"
            if VM.opt(row, "xq"):
                _same(out["xq"], x, "xq", tag)
            if kind == "exact":
                wrong = idx != d64.argmin(1)
                assert not bool(wrong.any()), \
                    f"{tag}: {int(wrong.sum())} indices are not the first minimum, e.g. pixel {int(wrong.nonzero()[0])}"
                _same(out["zq"], e[idx], "zq against q", tag)
            else:
                rows = torch.arange(P)
                assert bool(adm[rows, idx].all()), f"{tag}: {int((~adm[rows, idx]).sum())} inadmissible indices"
                assert bool((idx[one] == best[one]).all()), f"{tag}: an index differs from the only admissible code"
                gap = (d64[rows, idx] - d64[rows, best]) / (tol[rows, idx] + tol[rows, best])
                seen["index"] = max(seen.get("index", 0.0), float(gap.max()))
            _same(out["zq"], VM.zq_reference(x, e, idx), "zq", tag)
            loss, S = VM.loss_reference(x, e, idx)
            got = torch.tensor([out["loss"]], dtype=torch.float64)
            _within(got, loss.reshape(1), VM.K_S * VM.U24 * loss.reshape(1), "loss", tag, seen)
            assert not bool(torch.isnan(out["partial"]).any()), f"{tag}: a partial was not written"
            if kind == "exact":
                want = VM.exact_loss(S, P * C)
                assert out["loss"] == want, f"{tag}: loss {out['loss']!r} is not fl(S fl(1 / n)) = {want!r}"
            _repeatable(p, lambda: p.run(L, _stream()), tag)
        _report(f"{VM.row_id(row)} {kind}", seen)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_vq_bwd
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", VM.DISTS)
@pytest.mark.parametrize("row", VM.rows_of(VM.BWD), ids=VM.row_id)
def test_backward_rows(row, dist):
    L = _L()
    B, HW, C, K = row.dims
    ld_out = VM.opt(row, "ld")[2]
    assert L.sdmi_vq_bwd_workspace() == VM.bwd_workspace()
    for kind in FAMILIES:
        c, seen = VM.bwd_case(kind, B, HW, C, K, dist, VM.opt(row, "add"), VM.opt(row, "lw")), {}
        ref = VM.bwd_reference(c)
        unused = ref["count"] == 0
        for layout in VM.LAYOUTS:
            tag = f"{VM.row_id(row)} {dist} {kind} {layout}"
            p = VM.BwdProblem(c, row, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            out = p.outputs()
            _same(out["dz"][:, :C], ref["dz"], "dz_enc", tag)
            assert ld_out == C or bool((VM.bits(p.dz[:, C:].contiguous()) == 0).all()), \
                f"{tag}: the pad columns of dz_enc are not zero"
            for name in p.OUT:
                if not p.given(name):
                    continue
                _within(out[name], ref[name], VM.sum_bound(ref["T_" + name]), name, tag, seen)
                if kind == "exact":
                    _same(out[name], ref[name], name, tag)
            _within(out["demb"], ref["demb"], VM.demb_bound(ref["demb"], ref["T_demb"]), "demb", tag, seen)
            assert bool((out["demb"][unused] == 0).all()), f"{tag}: the row of an unused code is not zero"
            if kind == "exact":
                _same(out["demb"], ref["demb"], "demb", tag)
            _repeatable(p, lambda: p.run(L, _stream()), tag)
        _report(f"{VM.row_id(row)} {dist} {kind}", seen)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_pointwise_in
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", VM.rows_of(VM.POINT), ids=VM.row_id)
def test_pointwise_rows(row):
    L = _L()
    B, C, HW, cout, ld = row.dims
    for kind in FAMILIES:
        tag = f"{VM.row_id(row)} {kind}"
        c = VM.point_case(kind, B, C, HW, cout, VM.opt(row, "bias"))
        p = VM.PointProblem(c, row)
        g = p.guard()
        _run(L, lambda: p.run(L, _stream()), row.launches, tag)
        _unchanged(g, tag)
        _same(p.out[:, :cout].cpu().double(), VM.point_reference(c), "the output", tag)
        assert ld == cout or bool((VM.bits(p.out[:, cout:].contiguous()) == 0).all()), \
            f"{tag}: the pad columns are not zero"


# ----------------------------------------------------------------------------------------------------------------
# error returns
# ----------------------------------------------------------------------------------------------------------------
def _rejected(L, g, fn, tag):
    rc, ops = VM.recorded(L, fn)
    assert rc == -1, f"{tag}: returned {rc}, documented -1"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: a rejected call changed {g.changed()}"


def test_quantize_rejects_without_launching():
    L = _L()
    row = VM.rows_of(VM.QUANT)[4]                      # (3, 35, 8, 37), ldz = 8, w + b, xq
    c = VM.quant_case("exact", *row.dims, VM.opt(row, "conv"))
    p = VM.QuantProblem(c, row, VM.CONTIGUOUS)
    g, s = p.guard(writes=False), _stream()
    for name in ("z", "codebook", "zq", "idx", "ws", "loss"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"quantize: {name} null")
    for name in ("K", "B", "HW", "C"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"quantize: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, C=9, ldz=16), "quantize: C = 9")
    _rejected(L, g, lambda: p.run(L, s, ldz=7), "quantize: ldz < C")


def test_backward_rejects_without_launching():
    L = _L()
    row = VM.rows_of(VM.BWD)[3]                        # (3, 343, 8, 130), every option present
    c = VM.bwd_case("exact", *row.dims, "uniform", VM.opt(row, "add"), VM.opt(row, "lw"))
    p = VM.BwdProblem(c, row, VM.CONTIGUOUS)
    g, s = p.guard(writes=False), _stream()
    for name in ("dzin", "zq", "w_post", "xq", "idx", "codebook", "z_enc", "w_pre", "dz_enc", "ws", "demb"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"backward: {name} null")
    for name in ("K", "B", "HW", "C"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"backward: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, C=9, ld_dzin=16, ldz=16, ld_out=16), "backward: C = 9")
    for name in ("ld_dzin", "ldz", "ld_out"):
        _rejected(L, g, lambda: p.run(L, s, **{name: 7}), f"backward: {name} < C")


def test_pointwise_rejects_without_launching():
    L = _L()
    row = VM.rows_of(VM.POINT)[4]                      # (1, 4, 40, 6, 8), bias
    B, C, HW, cout, ld = row.dims
    p = VM.PointProblem(VM.point_case("exact", B, C, HW, cout, 1), row)
    g, s = p.guard(writes=False), _stream()
    for name in ("z", "w", "out"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"pointwise: {name} null")
    for name in ("B", "C", "HW", "cout"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"pointwise: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, ld=cout - 1), "pointwise: ld < cout")
