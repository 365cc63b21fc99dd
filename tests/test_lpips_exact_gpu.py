"""Every kernel of csrc/lpips.hip at every row of tests/lpips_matrix.py ROWS, exact, guarded.

Each row runs through the C ABI (sdmi._lib) in every data family of its kernel -- the distance rows also in both
layouts, contiguous and as column windows of wider NaN-filled buffers with ld, ld_add and ld_dy all different, the
backward rows on both sides. The recorded launch plan must name the row's kernels and grids. After every call nothing but
the declared outputs may have changed, bit for bit (ws is exactly sdmi_lpips_dist_workspace bytes between NaN pads).
Then the statements of tests/lpips_matrix.py: prep, image_grad, the pool pair, val given the partials and mean bitwise;
rn, the partials and dy within K_RN, K_D, K_G (bitwise in the exact family). A second identical call gives identical
bits. Each distance test prints its worst ratio per statement.

Also one engine-level case: a NaN pixel in image 0 gives a NaN distance and a NaN gradient at that pixel, as the
restatement of the reference module (tests/lpips_ref.py) does on the CPU."""
import ctypes
import functools

import pytest
import torch

from tests import lpips_matrix as M
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
opt = M.opt


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = M.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert M.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _repeatable(raw, call, tag):
    first = raw()
    assert call() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, raw()):
        assert torch.equal(M.bits(a), M.bits(b)), f"{tag}: a second identical call gives other bits"


def _again(p, first, L, tag):
    """A second call of a problem whose inputs were put back: the same bits as `first`."""
    assert p.run(L, _stream()) == 0
    torch.cuda.synchronize()
    for a, b in zip(first, p.raw()):
        assert torch.equal(M.bits(a), M.bits(b)), f"{tag}: a second identical call gives other bits"


def _bitwise(got, ref, what, tag):
    assert M.same_bits(got, ref), f"{tag}: {what} is not its bitwise value"


# ----------------------------------------------------------------------------------------------------------------
# the distance pair
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _fwd_refs(kind, B, P, C):
    c = M.dist_case(kind, B, P, C)
    d, Mx = M.pixel_terms(c)
    return c, M.rn_reference(c), M.block_sums(d, C), M.block_sums(Mx, C)


@pytest.mark.parametrize("row", M.rows_of(M.DFWD), ids=M.row_id)
def test_distance_forward_rows(row):
    L = _L()
    B, P, C = row.dims
    full = bool(opt(row, "full"))
    nb = M.blocks(P, C)
    assert L.sdmi_lpips_dist_workspace(B, P, C) == M.workspace(B, P, C) == 4 * B * nb
    worst = dict(rn=0.0, partial=0.0)
    for kind in M.KINDS:
        c, rn64, S64, Mb = _fwd_refs(kind, B, P, C)
        live = (c["f"] != 0).any(-1)
        for layout in M.LAYOUTS:
            tag = f"{M.row_id(row)} {kind} {layout}"
            p = M.DistProblem(c, row, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            part = p.ws.data.cpu().view(B, nb)
            assert not bool(torch.isnan(part).any()), f"{tag}: a partial was not written"
            if kind == "exact":
                assert M.same_bits(part, S64.float()) and torch.equal(part.double(), S64), f"{tag}: the partials are not the exact sums"
            else:
                assert bool((part[Mb == 0] == 0).all()), f"{tag}: a partial is non-zero where every term is zero"
                if bool((Mb > 0).any()):
                    r = float(((part.double() - S64).abs()[Mb > 0] / (M.K_D * M.U24 * Mb[Mb > 0])).max())
                    assert r <= 1.0, f"{tag}: |partial - S64| / (K_D u M) = {r:.3f}"
                    worst["partial"] = max(worst["partial"], r)
            if full:
                rn = p.rn.get(2, B * P)
                assert not bool(torch.isnan(rn).any()), f"{tag}: an inverse norm was not written"
                assert bool((rn[~live] == M.RN_ZERO).all()), f"{tag}: rn of an all-zero row is not fl32(1e12)"
                if kind == "exact":
                    assert M.same_bits(p.rn.data.cpu().view(2, B * P)[live], rn64[live].float()) and torch.equal(rn[live], rn64[live]), \
                        f"{tag}: rn is not exact"
                elif bool(live.any()):
                    r = float(((rn - rn64).abs()[live] / (M.K_RN * M.U24 * rn64[live])).max())
                    assert r <= 1.0, f"{tag}: |rn - rn64| / (K_RN u rn64) = {r:.3f}"
                    worst["rn"] = max(worst["rn"], r)
            want = M.val_from_partials(part, P, c["prev"] if full else None)
            _bitwise(p.val.data.cpu(), want, "val given the partials", tag)
            first_raw = p.raw()
            if kind == "exact" and not full and bool((S64 == 0).all()):
                assert bool((M.bits(p.val.data.cpu()) == 0).all()), f"{tag}: identical images do not give +0"
            if full:        # (accumulate: the second call starts from the same prior value)
                p.val.put(c["prev"])
            _again(p, first_raw, L, tag)
    print(f"{M.row_id(row)}: max |rn - rn64| / bound {worst['rn']:.3f}, max |partial - S64| / bound {worst['partial']:.3f}")


@pytest.mark.parametrize("row", M.rows_of(M.DBWD), ids=M.row_id)
def test_distance_backward_rows(row):
    L = _L()
    B, P, C = row.dims
    full = bool(opt(row, "full"))
    worst, beyond = 0.0, 0.0
    for kind in M.KINDS:
        c = M.dist_case(kind, B, P, C)
        for side in (0, 1):
            ref, T = M.dy_reference(c, side, full)
            dead = c["f"][side] <= 0
            for layout in M.LAYOUTS:
                tag = f"{M.row_id(row)} {kind} side {side} {layout}"
                p = M.DistProblem(c, row, layout, side)
                g = p.guard()
                _run(L, lambda: p.run(L, _stream()), row.launches, tag)
                _unchanged(g, tag)
                raw = p.dy.cpu()
                dy = raw.double()
                assert not bool(torch.isnan(dy).any()), f"{tag}: dy holds a NaN (an element was not written)"
                assert bool((M.bits(raw.contiguous())[dead] == 0).all()), f"{tag}: dy is not +0 where the activation is <= 0"
                if kind == "exact":
                    # (ref64 is an fp32 value, but for the bare rows off a power of two: one fp32 rounding there)
                    assert M.same_bits(raw, ref.float().to(BF)), \
                        f"{tag}: dy differs in {int((dy != M.bf16(ref.float())).sum())} elements from its bitwise value"
                    if full:    # identical pairs hand the addend on untouched
                        same = ((c["f"][0] == c["f"][1]).all(-1))[:, None] & ~dead
                        assert M.same_bits(raw.contiguous()[same], c["addend"].to(BF)[same])
                else:
                    r = M.dy_within(dy, ref, T)
                    assert r <= 1.0, f"{tag}: |dy - ref64| / (K_G u T + bf16 ulp / 2) = {r:.3f}"
                    worst, beyond = max(worst, r), max(beyond, M.dy_beyond_rounding(dy, ref, T))
                _repeatable(p.raw, lambda: p.run(L, _stream()), tag)
    print(f"{M.row_id(row)}: max |dy - ref64| / bound {worst:.3f}; max (|dy - ref64| - bf16 ulp / 2) / (K_G u T) {beyond:.3f}")


def test_distance_backward_passes_under_a_nan_activation():
    """dy = a <= 0 ? 0 : df + addend, torch's threshold_backward: under a NaN activation the (NaN) gradient passes; the
    rows without a NaN are untouched by it."""
    L = _L()
    row = next(r for r in M.rows_of(M.DBWD) if r.dims == (3, 9, 64) and opt(r, "full"))
    c = dict(M.dist_case("soft", *row.dims))
    c["f"] = c["f"].clone()
    c["f"][0, 4, 17] = float("nan")
    p = M.DistProblem(c, row, M.CONTIGUOUS, side=0)
    assert p.run(L, _stream()) == 0
    torch.cuda.synchronize()
    dy = p.dy.cpu().double()
    assert bool(torch.isnan(dy[4, 17])), "the gradient under a NaN activation is finite"
    live = c["f"][0, 4] > 0
    assert bool(torch.isnan(dy[4][live]).all()) and bool((dy[4][c["f"][0, 4] == 0] == 0).all())
    clean = M.DistProblem(M.dist_case("soft", *row.dims), row, M.CONTIGUOUS, side=0)
    assert clean.run(L, _stream()) == 0
    torch.cuda.synchronize()
    others = torch.arange(27) != 4
    assert torch.equal(M.bits(p.dy.cpu().contiguous())[others], M.bits(clean.dy.cpu().contiguous())[others])


# ----------------------------------------------------------------------------------------------------------------
# the pool pair
# ----------------------------------------------------------------------------------------------------------------
def _rows_buf(rows, C, dtype, values=None):
    b = M.Buf(rows, C, dtype, DEV)
    w = b.window(0, C)
    if values is not None:
        w.copy_(values.reshape(rows, C).to(dtype))
    return b, w


@pytest.mark.parametrize("row", M.rows_of(M.POOLF, M.POOLB), ids=M.row_id)
def test_pool_rows(row):
    L = _L()
    N, H, W, C = row.dims
    OH, OW = H // 2, W // 2
    for kind in ("ties", "special"):
        tag = f"{M.row_id(row)} {kind}"
        c = M.pool_case(kind, N, H, W, C)
        xb, x = _rows_buf(N * H * W, C, BF, c["x"])
        g = M.Guard()
        g.add("x", xb)
        if row.entry == M.POOLF:
            yb, y = _rows_buf(N * OH * OW, C, BF)
            g.add("y", yb, [("w", 0, C)])
            call = lambda: L.sdmi_maxpool2_fwd(M.ptr(x), N, H, W, C, M.ptr(y), _stream())  # noqa: E731
            want = M.pool_model(c["x"])[0].reshape(-1, C)
            out, outb = y, yb
        else:
            dyb, dy = _rows_buf(N * OH * OW, C, BF, c["dy"])
            dxb, dx = _rows_buf(N * H * W, C, BF)
            g.add("dy", dyb)
            g.add("dx", dxb, [("w", 0, C)])
            call = lambda: L.sdmi_maxpool2_bwd(M.ptr(x), M.ptr(dy), N, H, W, C, M.ptr(dx), _stream())  # noqa: E731
            want = M.pool_bwd_model(c["x"], c["dy"]).reshape(-1, C)
            out, outb = dx, dxb
        _run(L, call, row.launches, tag)
        _unchanged(g, tag)
        _bitwise(out, want, "the output", tag)
        _repeatable(lambda: [outb.buf.clone()], call, tag)


# ----------------------------------------------------------------------------------------------------------------
# prep, image_grad, mean
# ----------------------------------------------------------------------------------------------------------------
def _flat(values):
    return M.Flat(values.numel(), DEV).put(values)


@pytest.mark.parametrize("row", M.rows_of(M.PREP), ids=M.row_id)
def test_prep_rows(row):
    L = _L()
    B, H, W = row.dims
    n0, n1, normalize = opt(row, "nhwc0"), opt(row, "nhwc1"), opt(row, "normalize")
    shift, scale = _flat(torch.tensor(M.SHIFT)), _flat(torch.tensor(M.SCALE))
    for kind in ("soft", "special"):
        tag = f"{M.row_id(row)} {kind}"
        c = M.image_case(kind, B, H, W)
        src = [_flat(M.nhwc8(x) if flat else x) for x, flat in zip(c["ims"], (n0, n1))]
        ob, out = _rows_buf(2 * B * H * W, 8, BF)
        g = M.Guard()
        for name, f in (("in0", src[0]), ("in1", src[1]), ("shift", shift), ("scale", scale)):
            g.add(name, f)
        g.add("out", ob, [("w", 0, 8)])
        call = lambda: L.sdmi_lpips_prep(M.ptr(src[0].data), n0, M.ptr(src[1].data), n1, B, H, W, M.ptr(shift.data),  # noqa: E731
                                         M.ptr(scale.data), normalize, M.ptr(out), _stream())
        _run(L, call, row.launches, tag)
        _unchanged(g, tag)
        _bitwise(out, M.prep_reference(c["ims"], normalize), "the packed batch", tag)
        assert bool((M.bits(out[:, 3:].contiguous()) == 0).all()), f"{tag}: channels 3..7 are not +0"
        _repeatable(lambda: [ob.buf.clone()], call, tag)


@pytest.mark.parametrize("row", M.rows_of(M.IGRAD), ids=M.row_id)
def test_image_grad_rows(row):
    L = _L()
    B, H, W = row.dims
    HW, mode = H * W, opt(row, "mode")
    mse, with_nchw, with_acc = mode.startswith("mse"), "nchw" in mode, mode != "nchw"
    scale = _flat(torch.tensor(M.SCALE))
    for kind in ("soft", "special"):
        c = M.image_case(kind, B, H, W)
        for normalize in (0, 1):
            tag = f"{M.row_id(row)} {kind} normalize {normalize}"
            db, d = _rows_buf(B * HW, 8, BF, c["d"])
            nchw = M.Flat(3 * B * HW, DEV)
            ab, acc = _rows_buf(B * HW, 8, BF, None if mse else c["acc"])
            pred, target = _flat(M.nhwc8(c["pred"])), _flat(c["target"])
            g = M.Guard()
            for name, f in (("d", db), ("scale", scale), ("pred", pred), ("target", target)):
                g.add(name, f)
            g.add("out_nchw", nchw, [(0, 3 * B * HW)] if with_nchw else [])
            # the add mode rewrites 8 bytes of a row (channels 0..3); the whole mode all 16
            g.add("acc", ab, [("w", 0, 8 if mse else 4)] if with_acc else [])
            call = lambda: L.sdmi_lpips_image_grad(  # noqa: E731
                M.ptr(d), B, H, W, M.ptr(scale.data), normalize, M.ptr(nchw.data) if with_nchw else None,
                M.ptr(acc) if with_acc else None, M.ptr(pred.data) if mse else None, M.ptr(target.data) if mse else None, _stream())
            _run(L, call, row.launches, tag)
            _unchanged(g, tag)
            want = M.image_grad_reference(c, B, H, W, normalize, mode)
            if with_nchw:
                _bitwise(nchw.data.view(B, 3, H, W), want["nchw"], "out_nchw", tag)
            if with_acc:
                _bitwise(acc, want["acc"], "acc", tag)
                pads = M.bits(acc[:, 3:].contiguous().cpu())
                if mse:
                    assert bool((pads == 0).all()), f"{tag}: channels 3..7 of the whole acc are not +0"
                else:
                    assert torch.equal(pads, M.bits(c["acc"][:, 3:].contiguous())), f"{tag}: a pad channel of acc changed"
            if not with_acc or mse:     # (the add mode is not idempotent)
                _repeatable(lambda: [nchw.buf.clone(), ab.buf.clone()], call, tag)


@pytest.mark.parametrize("row", M.rows_of(M.MEAN), ids=M.row_id)
def test_mean_rows(row):
    L = _L()
    B, = row.dims
    for kind in ("soft", "special"):
        tag = f"{M.row_id(row)} {kind}"
        c = M.mean_case(kind, B)
        val, out = _flat(c["val"]), M.Flat(1, DEV)
        g = M.Guard()
        g.add("val", val)
        g.add("out", out, [(0, 1)])
        call = lambda: L.sdmi_lpips_mean(M.ptr(val.data), B, c["scale"], M.ptr(out.data), _stream())  # noqa: E731
        _run(L, call, row.launches, tag)
        _unchanged(g, tag)
        _bitwise(out.data, M.mean_reference(c), "the mean", tag)
        _repeatable(lambda: [out.buf.clone()], call, tag)


# ----------------------------------------------------------------------------------------------------------------
# refusals launch nothing and write nothing
# ----------------------------------------------------------------------------------------------------------------
def test_distance_rejects_without_launching():
    L = _L()
    fwd = next(r for r in M.rows_of(M.DFWD) if r.dims == (3, 257, 64) and opt(r, "full"))
    bwd = next(r for r in M.rows_of(M.DBWD) if r.dims == (3, 257, 64) and opt(r, "full"))
    for row, bad in ((fwd, [dict(f=None), dict(w=None), dict(ws=None), dict(val=None), dict(C=96), dict(ld=56), dict(ld=68),
                            dict(B=0), dict(P=0), dict(B=65536)]),
                     (bwd, [dict(f=None), dict(w=None), dict(rn=None), dict(dy=None), dict(C=96), dict(ld=56), dict(ld_dy=68),
                            dict(ld_add=56), dict(side=2), dict(side=-1), dict(P=-1), dict(B=65536)])):
        p = M.DistProblem(M.dist_case("exact", *row.dims), row, M.CONTIGUOUS)
        g = p.guard(writes=False)
        for over in bad:
            rc, ops = M.recorded(L, lambda: p.run(L, _stream(), **over))
            torch.cuda.synchronize()
            assert rc == -1 and ops == [], f"{M.row_id(row)} {over}: returned {rc}, launched {ops}"
            assert g.changed() is None, f"{M.row_id(row)} {over}: the refused call changed {g.changed()}"


# ----------------------------------------------------------------------------------------------------------------
# the whole chain passes a NaN on, as the reference module does
# ----------------------------------------------------------------------------------------------------------------
def test_engine_passes_a_nan_pixel_on():
    from sdmi.lpips_engine import MIN_SIDE, LPIPSEngine
    sd = R.seeded_state()
    out, im = R.images(1, MIN_SIDE, MIN_SIDE, 5)
    out = out.clone()
    out[0, 1, 5, 7] = float("nan")
    a = out.clone().requires_grad_(True)
    val_ref = R.lpips(sd, a, im)
    val_ref.sum().backward()
    assert bool(torch.isnan(val_ref).all()) and bool(torch.isnan(a.grad[0, :, 5, 7]).all())
    eng = LPIPSEngine({k: v.cuda() for k, v in sd.items()}, DEV)
    val, ctx = eng.forward(out.cuda(), im.cuda())
    g0, g1 = eng.backward(ctx, None, want=(True, False))
    torch.cuda.synchronize()
    assert g1 is None and bool(torch.isnan(val).all()), f"val {val.tolist()} of an image with a NaN pixel"
    assert bool(torch.isnan(g0[0, :, 5, 7]).all()), "the gradient at the NaN pixel is finite"
    # and nothing of it without the NaN
    clean, _ = eng.forward(im.cuda(), im.cuda(), need_backward=False)
    assert bool((clean == 0).all())
