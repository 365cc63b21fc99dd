"""Every DiT row and patch-layout kernel of csrc/dit.hip at every row of tests/dit_matrix.py ROWS, exact, guarded.

The row kernels and finalize run every row on the exact and on the soft family, with contiguous operands and with
operands that are column windows of NaN-filled buffers in which every stride and offset differs; the patch kernels at
the row's ld. The recorded launch plan must name the row's kernels and grids. After every call nothing but the logical
output windows may have changed, bit for bit -- inputs, pad columns, rows past the end, the partial rows of absent
pointers and the mse workspace beyond the partials written included.

Both families, every element: the componentwise bounds of tests/dit_matrix.py on the kernel's own xo, mean and rstd,
and the bitwise statements (xo, dx16, dv, the layouts, the zero pad columns). Exact family: psh, finalize, the loss and
mean at a power-of-two C are bitwise, the constant row gives y == shift, and the bf16 and the fp32 stream give the
same mean and rstd bits. Each test prints its worst error / bound per quantity and family.

Also the error returns: nothing launched, nothing written."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dit_matrix as DM

pytestmark = pytest.mark.gpu
FAMILIES = ("exact", "soft")


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = DM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert DM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _within(got, ref, lim, what, tag, seen):
    assert not bool(torch.isnan(got).any()), f"{tag}: {what} holds NaN"
    err = (got - ref).abs()
    w = float((err / lim.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    seen[what] = max(seen.get(what, 0.0), w)
    assert bool((err <= lim).all()), f"{tag}: {what} worst error / bound {w:.3f}"


def _same(got, ref, what, tag):
    assert torch.equal(got, ref), f"{tag}: {what} differs in {int((got != ref).sum())} elements from its bitwise value"


def _report(row, kind, seen):
    print(f"{DM.row_id(row)} {kind}: max(err / bound) " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(seen.items())))


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


# ----------------------------------------------------------------------------------------------------------------
# sdmi_ln_mod_fwd
# ----------------------------------------------------------------------------------------------------------------
def _forward_once(L, row, c, layout, f32, want, tag, seen):
    """One guarded forward; returns the float64 copies of mean and rstd."""
    B, N, C = row.dims
    res, mod = DM.opt(row, "res"), DM.opt(row, "mod")
    p = DM.LnProblem(c, layout, f32)
    g = p.guard({"y", "mean", "rstd"} | ({"xo"} if res != "none" else set()))
    rc, ops = DM.recorded(L, lambda: p.fwd(L, res, mod, _stream()))
    assert rc == 0, f"{tag}: returned {rc}"
    if want is not None:
        assert DM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()
    _unchanged(g, tag)
    xo = DM.xo_reference(c, res, f32)
    if res != "none":
        _same(p.out("xo"), xo, "xo", tag)
    mean, rstd = p.mean.get(B * N), p.rstd.get(B * N)
    st = DM.row_stats(xo)
    bm, br = DM.stats_bounds(c["kind"], C, st)
    _within(mean, st["mean"], bm, "mean", tag, seen)
    _within(rstd, st["rstd"], br, "rstd", tag, seen)
    ref, lim, _ = DM.y_reference(c, xo, mean, rstd, mod)
    y = p.out("y")
    _within(y, ref, lim, "y", tag, seen)
    if c["kind"] == "exact" and c["const"] is not None:
        i = c["const"]
        assert float(mean[i]) == 2.0, f"{tag}: the constant row's mean"
        want_y = c["shift"][i // N] if mod else torch.zeros(C, dtype=torch.float64)
        _same(y[i], want_y, "y of the constant row", tag)
    return mean, rstd


@pytest.mark.parametrize("row", DM.rows_of(DM.LN_FWD), ids=DM.row_id)
def test_forward_rows(row):
    L = _L()
    B, N, C = row.dims
    f32 = DM.opt(row, "f32")
    for kind in FAMILIES:
        c, seen = DM.ln_case(kind, B, N, C, f32 if kind == "soft" else 0), {}
        stats = []
        for layout in DM.LAYOUTS:
            tag = f"{DM.row_id(row)} {kind} {layout}"
            stats.append(_forward_once(L, row, c, layout, f32, row.launches, tag, seen))
        if kind == "exact":
            # the same numbers on the other stream type: the same statistics, bit for bit
            other = _forward_once(L, row, c, DM.WINDOWS, 1 - f32, None, f"{DM.row_id(row)} exact, other stream", seen)
            for a in stats:
                assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]), \
                    f"{DM.row_id(row)}: mean / rstd differ between the bf16 and the fp32 stream or between layouts"
        _report(row, kind, seen)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_ln_mod_bwd
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DM.rows_of(DM.LN_BWD), ids=DM.row_id)
def test_backward_rows(row):
    L = _L()
    B, N, C = row.dims
    f32, mod, dres, gate, dx16 = (DM.opt(row, k) for k in ("f32", "mod", "dres", "gate", "dx16"))
    parts = [j for j, on in enumerate((mod in ("both", "psh"), mod in ("both", "psc"), gate)) if on]
    for kind in FAMILIES:
        c, seen = DM.ln_case(kind, B, N, C, f32 if kind == "soft" else 0), {}
        mean, rstd = DM.host_stats(c["x"])
        bw = DM.bwd_reference(c, mean, rstd, mod, dres)
        psh, Tsh = DM.chunk_sums(c["dy"], c)
        psc, Tsc = DM.chunk_sums(c["dy"] * bw["xh"], c)
        for layout in DM.LAYOUTS:
            tag = f"{DM.row_id(row)} {kind} {layout}"
            p = DM.LnProblem(c, layout, f32)
            p.mean.put(mean)
            p.rstd.put(rstd)
            g = p.guard({"dx"} | ({"dx16"} if dx16 else set()) | ({"dv"} if gate else set()), parts)
            _run(L, lambda: p.bwd(L, mod, dres, gate, dx16, _stream()), row.launches, tag)
            _unchanged(g, tag)
            dx = p.out("dx")
            _within(dx, bw["dx"], DM.dx_bound(bw["dx"], bw["T"], f32), "dx", tag, seen)
            if dx16:
                _same(p.out("dx16"), DM.bf16(dx), "dx16", tag)
            if 0 in parts:
                _within(p.partial(0), psh, DM.sum_bound(Tsh), "psh", tag, seen)
                if kind == "exact":
                    _same(p.partial(0), psh, "psh", tag)
            if 1 in parts:
                _within(p.partial(1), psc, DM.sum_bound(Tsc), "psc", tag, seen)
            if gate:
                _same(p.out("dv"), DM.dv_reference(c, dx), "dv", tag)
                pg, Tg = DM.chunk_sums(dx * c["v"], c)
                _within(p.partial(2), pg, DM.sum_bound(Tg), "pg", tag, seen)
        _report(row, kind, seen)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_mod_finalize
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DM.rows_of(DM.FINALIZE), ids=DM.row_id)
def test_finalize_rows(row):
    L = _L()
    for kind in FAMILIES:
        ws, seen = DM.finalize_case(kind, *row.dims), {}
        ref, T = DM.finalize_reference(ws)
        for layout in DM.LAYOUTS:
            tag = f"{DM.row_id(row)} {kind} {layout}"
            p = DM.FinalizeProblem(ws, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            got = p.out.cpu().double()
            _within(got, ref, DM.sum_bound(T, ref=ref), "finalize", tag, seen)
            if kind == "exact":
                _same(got, DM.bf16(ref), "finalize", tag)
        _report(row, kind, seen)


# ----------------------------------------------------------------------------------------------------------------
# the patch layout and the MSE
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DM.rows_of(DM.TO_NCHW), ids=DM.row_id)
def test_tokens_to_nchw_rows(row):
    L = _L()
    B, C, H, W, p = row.dims
    f32 = DM.opt(row, "f32")
    dt = torch.float32 if f32 else torch.bfloat16
    for kind in FAMILIES:
        tag = f"{DM.row_id(row)} {kind}"
        img = DM.patch_case(kind, *row.dims)["img"]
        img = img if f32 else DM.bf16(img)
        q = DM.PatchProblem(row.dims, DM.opt(row, "pad"))
        src, win = q.tokens(dt, DM.tokens_of(img, p))
        dst = q.image()
        g = DM.Guard()
        g.add("tokens", src)
        g.add("image", dst, [(0, q.n)])
        _run(L, lambda: L.sdmi_tokens_to_nchw(DM.ptr(win), f32, q.ld, B, C, H, W, p, DM.ptr(dst.data), _stream()),
             row.launches, tag)
        _unchanged(g, tag)
        _same(dst.get(B, C, H, W), img, "the image", tag)


@pytest.mark.parametrize("row", DM.rows_of(DM.TO_TOKENS), ids=DM.row_id)
def test_nchw_to_tokens_rows(row):
    L = _L()
    B, C, H, W, p = row.dims
    for kind in FAMILIES:
        tag = f"{DM.row_id(row)} {kind}"
        img = DM.patch_case(kind, *row.dims)["img"]
        q = DM.PatchProblem(row.dims, DM.opt(row, "pad"))
        src = q.image(img)
        dst, win = q.tokens(torch.bfloat16)
        g = DM.Guard()
        g.add("image", src)
        g.add("tokens", dst, [("w", 0, q.ld)])
        _run(L, lambda: L.sdmi_nchw_to_tokens_bf16(DM.ptr(src.data), B, C, H, W, p, DM.ptr(win), q.ld, _stream()),
             row.launches, tag)
        _unchanged(g, tag)
        got = win.cpu().double()
        _same(got[:, :q.K], DM.bf16(DM.tokens_of(img, p)), "the tokens", tag)
        assert bool((DM.bits(win[:, q.K:].contiguous()) == 0).all()), f"{tag}: the pad columns are not zero"


@pytest.mark.parametrize("row", DM.rows_of(DM.MSE), ids=DM.row_id)
def test_mse_patch_rows(row):
    L = _L()
    B, C, H, W, p = row.dims
    by_dev, with_grad = DM.opt(row, "gs") == "dev", DM.opt(row, "grad")
    blocks = row.launches[0][1]
    assert L.sdmi_mse_workspace() == 4 * DM.MSE_CAP
    for kind in FAMILIES:
        tag, seen = f"{DM.row_id(row)} {kind}", {}
        c = DM.patch_case(kind, *row.dims)
        m = DM.mse_reference(c, row.dims)
        q = DM.PatchProblem(row.dims, DM.opt(row, "pad"))
        pred, pwin = q.tokens(torch.float32, c["pred"])   # (its pad columns hold NaN: the kernel must not read them)
        pred_ptr = DM.ptr(pwin)
        grad, gwin = q.tokens(torch.bfloat16)
        target = q.image(c["target"])
        ws, loss = DM.Flat(DM.MSE_CAP, "cuda"), DM.Flat(1, "cuda")
        gdev = DM.Flat(1, "cuda").put(torch.tensor(c["gscale"]))
        g = DM.Guard()
        g.add("pred", pred)
        g.add("target", target)
        g.add("gscale_dev", gdev)
        g.add("grad", grad, [("w", 0, q.ld)] if with_grad else [])
        g.add("workspace", ws, [(0, blocks)])
        g.add("loss", loss, [(0, 1)])
        # by value the kernel must ignore the device scalar's absence; through the pointer the value argument
        gval = -3.0 if by_dev else c["gscale"]
        _run(L, lambda: L.sdmi_mse_patch(pred_ptr, q.ld, DM.ptr(target.data), B, C, H, W, p, gval,
                                         DM.ptr(gdev.data) if by_dev else None, DM.ptr(gwin) if with_grad else None,
                                         DM.ptr(ws.data), DM.ptr(loss.data), _stream()), row.launches, tag)
        _unchanged(g, tag)
        got = loss.get(1)
        _within(got, m["loss"].reshape(1), DM.K_SUM * DM.U24 * m["loss"].reshape(1), "loss", tag, seen)
        assert not bool(torch.isnan(ws.get(DM.MSE_CAP)[:blocks]).any()), f"{tag}: a partial was not written"
        if kind == "exact":
            want = float(np.float32(float(m["S"])) * (np.float32(1.0) / np.float32(m["n"])))
            assert float(got) == want, f"{tag}: loss {float(got)!r} is not fl(S fl(1 / n)) = {want!r}"
        if with_grad:
            gg = gwin.cpu().double()
            _within(gg[:, :q.K], m["grad"], DM.grad_bound(m["grad"]), "grad", tag, seen)
            assert bool((DM.bits(gwin[:, q.K:].contiguous()) == 0).all()), f"{tag}: the pad columns are not zero"
            if kind == "exact" and DM.is_pow2(B * C * H * W):
                _same(gg[:, :q.K], m["grad"], "grad", tag)
        _report(row, kind, seen)


# ----------------------------------------------------------------------------------------------------------------
# error returns
# ----------------------------------------------------------------------------------------------------------------
def _rejected(L, guards, fn, want, tag):
    rc, ops = DM.recorded(L, fn)
    assert rc == want, f"{tag}: returned {rc}, documented {want}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    for g in guards:
        assert g.changed() is None, f"{tag}: a rejected call changed {g.changed()}"


def _off(p, nbytes=2):
    return ctypes.c_void_p(p.value + nbytes)


def test_row_kernels_reject_without_launching():
    """-1 for C % 8 != 0, C > 512, rows % N != 0; -2 for v without xo, shift without scale (and scale without shift),
    psh or psc without scale, gate without v, dv or pg; -3 for a pointer that is not 16-byte aligned or a row stride
    that is no multiple of 8. Every argument list stays inside its buffers even if it were launched."""
    L = _L()
    B, N, C = 2, 4, 64
    c = DM.ln_case("exact", B, N, C)
    for f32 in (0, 1):
        p = DM.LnProblem(c, DM.WINDOWS, f32)
        mean, rstd = DM.host_stats(c["x"])
        p.mean.put(mean)
        p.rstd.put(rstd)
        g = [p.guard(set())]
        s = _stream()

        def fwd(res="gate", mod=1, **kw):
            return lambda: p.fwd(L, res, mod, s, **kw)

        def bwd(mod="both", dres=1, gate=1, dx16=1, **kw):
            return lambda: p.bwd(L, mod, dres, gate, dx16, s, **kw)
        for name, mk in (("fwd", fwd), ("bwd", bwd)):
            _rejected(L, g, mk(C=C - 4), -1, f"{name}: C % 8 != 0")
            _rejected(L, g, mk(C=520), -1, f"{name}: C > 512")
            _rejected(L, g, mk(N=3), -1, f"{name}: rows % N != 0")
            _rejected(L, g, mk(rows=0), -1, f"{name}: no rows")
            _rejected(L, g, mk(x=_off(DM.ptr(p.win["x"]))), -3, f"{name}: x not 16-byte aligned")
            _rejected(L, g, mk(ldx=p.ld("x") + 4), -3, f"{name}: ldx % 8 != 0")
            _rejected(L, g, mk(ld_mod=p.mod.ld + 4), -3, f"{name}: ld_mod % 8 != 0")
        _rejected(L, g, fwd(xo=None), -2, "fwd: v without xo")
        _rejected(L, g, fwd(scale=None), -2, "fwd: shift without scale")
        _rejected(L, g, fwd(shift=None), -2, "fwd: scale without shift")
        _rejected(L, g, fwd(y=_off(DM.ptr(p.win["y"]))), -3, "fwd: y not 16-byte aligned")
        _rejected(L, g, fwd(ldxo=p.ld("xo") + 2), -3, "fwd: ldxo % 8 != 0")
        _rejected(L, g, fwd(gate=_off(DM.ptr(p.gate))), -3, "fwd: gate not 16-byte aligned")
        _rejected(L, g, bwd(mod="both", scale=None), -2, "bwd: psh and psc without scale")
        _rejected(L, g, bwd(mod="psh", scale=None), -2, "bwd: psh without scale")
        _rejected(L, g, bwd(mod="psc", scale=None), -2, "bwd: psc without scale")
        _rejected(L, g, bwd(v=None), -2, "bwd: gate without v")
        _rejected(L, g, bwd(dv=None), -2, "bwd: gate without dv")
        _rejected(L, g, bwd(pg=None), -2, "bwd: gate without pg")
        _rejected(L, g, bwd(dx=_off(DM.ptr(p.win["dx"]), 8)), -3, "bwd: dx not 16-byte aligned")
        _rejected(L, g, bwd(lddy=p.ld("dy") + 1), -3, "bwd: lddy % 8 != 0")
        _rejected(L, g, bwd(ld16=p.ld("dx16") + 4), -3, "bwd: ld16 % 8 != 0")
        _rejected(L, g, bwd(dv=_off(DM.ptr(p.win["dv"]))), -3, "bwd: dv not 16-byte aligned")


def test_patch_entry_points_reject_without_launching():
    """ld < p p C and H % p != 0 (W % p != 0 likewise) return -1 on the four patch entry points; sdmi_mod_finalize
    returns -1 for ws_ld < W and ldo < W."""
    L = _L()
    dims = B, C, H, W, p = 2, 3, 4, 6, 2
    c = DM.patch_case("exact", *dims)
    q = DM.PatchProblem(dims, 3)
    s = _stream()
    tok32, w32 = q.tokens(torch.float32, c["pred"])
    tok16, w16 = q.tokens(torch.bfloat16)
    img, out = q.image(c["target"]), q.image()
    ws, loss = DM.Flat(DM.MSE_CAP, "cuda"), DM.Flat(1, "cuda")
    g = DM.Guard()
    for name, b in (("tokens32", tok32), ("tokens16", tok16), ("image", img), ("out", out), ("ws", ws), ("loss", loss)):
        g.add(name, b)
    calls = (
        ("tokens_to_nchw", lambda ld, H, W: L.sdmi_tokens_to_nchw(DM.ptr(w32), 1, ld, B, C, H, W, p, DM.ptr(out.data),
                                                                  s)),
        ("nchw_to_tokens", lambda ld, H, W: L.sdmi_nchw_to_tokens_bf16(DM.ptr(img.data), B, C, H, W, p, DM.ptr(w16), ld,
                                                                      s)),
        ("mse_patch", lambda ld, H, W: L.sdmi_mse_patch(DM.ptr(tok32.window(0, q.ld)), ld, DM.ptr(img.data), B, C, H, W,
                                                        p, 1.0, None, DM.ptr(w16), DM.ptr(ws.data), DM.ptr(loss.data),
                                                        s)),
        ("mse_patch without grad", lambda ld, H, W: L.sdmi_mse_patch(DM.ptr(tok32.window(0, q.ld)), ld,
                                                                     DM.ptr(img.data), B, C, H, W, p, 1.0, None, None,
                                                                     DM.ptr(ws.data), DM.ptr(loss.data), s)),
    )
    for name, f in calls:
        _rejected(L, [g], lambda: f(q.K - 1, H, W), -1, f"{name}: ld < p p C")
        _rejected(L, [g], lambda: f(q.ld, H - 1, W), -1, f"{name}: H % p != 0")
        _rejected(L, [g], lambda: f(q.ld, H, W - 1), -1, f"{name}: W % p != 0")
    fin = DM.FinalizeProblem(DM.finalize_case("exact", 2, 8, 96), DM.WINDOWS)
    fg = fin.guard(writes=False)
    _rejected(L, [fg], lambda: fin.run(L, s, ws_ld=95), -1, "finalize: ws_ld < W")
    _rejected(L, [fg], lambda: fin.run(L, s, ldo=95), -1, "finalize: ldo < W")
    _rejected(L, [fg], lambda: fin.run(L, s, chunks=0), -1, "finalize: no chunks")
