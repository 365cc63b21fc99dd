"""Every kernel of csrc/lsq.hip, exact and guarded (statements: tests/lsq_ref.py; launches: DESIGN.md section 17).

Operands and outputs sit between NaN pads; after a call only the declared outputs may have changed, bit for bit; a second
identical call gives identical bits; the recorded launch plan names the kernels and grids DESIGN.md declares. y, the
codes, dx, d_pre and pre are bitwise the torch expression on the CPU (autograd of the restatement is the judge for dx);
ds lies within K_LSQ u g sum |t_i| of the float64 sum of the fp32 terms. Flat operands are run 16-byte aligned (a front
pad of 64 floats) and misaligned (65), which takes the element-by-element path with the same order of additions.
Each test prints its worst |ds - ds64| / bound."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lsq_ref as R
from tests.attn_matrix import launches_match, recorded
from tests.norm_matrix import Guard, bits, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRONTS = (64, 65)


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Box:
    """n elements between NaN pads (front elements before, 256 after); `data` is the logical window."""

    def __init__(self, n, dtype=torch.float32, front=64, values=None):
        self.buf = torch.full((front + n + 256,), float("nan"), dtype=dtype, device=DEV)
        self.n, self.front = n, front
        self.data = self.buf[front:front + n]
        if values is not None:
            self.data.copy_(values.reshape(-1).to(dtype))

    def cpu(self, *shape):
        return self.data.cpu().view(*shape) if shape else self.data.cpu()


def _run(L, call, want, tag):
    rc, ops = recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert launches_match(ops, want), f"{tag}: launched {ops}, DESIGN.md section 17 says {want}"
    torch.cuda.synchronize()


def _guard(ins, outs):
    g = Guard()
    for k, b in ins.items():
        g.add(k, b)
    for k, b in outs.items():
        g.add(k, b, [(0, b.n)])
    return g


def _check(g, outs, call, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"
    first = [b.buf.clone() for b in outs.values()]
    assert call() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, outs.values()):
        assert torch.equal(bits(a), bits(b.buf)), f"{tag}: a second identical call gives other bits"


def _same(got, ref, what, tag):
    ok = torch.equal(bits(got.contiguous()), bits(ref.contiguous().to(got.dtype)))
    if not ok:  # +-0 and NaN payloads aside, count the differing elements
        d = int((bits(got.contiguous()) != bits(ref.contiguous().to(got.dtype))).sum())
        raise AssertionError(f"{tag}: {what} differs in {d} of {got.numel()} elements from its bitwise value")


def _autograd(x, dy, step, bit):
    xr, sr = x.clone().requires_grad_(True), step.clone().requires_grad_(True)
    y = R.quant_lsq(xr, bit, sr)
    y.backward(dy)
    return y.detach(), xr.grad, float(sr.grad)


def _ds_ok(ds, t, g, tag):
    ref, bound = R.ds64(t, g), R.sum_bound(t, g)
    ratio = abs(ds - ref) / bound if bound else (0.0 if ds == ref else float("inf"))
    assert ratio <= 1.0, f"{tag}: ds {ds!r} is {ratio:.3f} bounds from {ref!r}"
    return ratio


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("bit", R.KERNEL_BITS)
@pytest.mark.parametrize("n", R.KERNEL_SIZES)
def test_flat_quantiser(n, bit, front):
    L, st = _L(), _stream()
    qp, g = R.qp_of(bit), R.g_of(bit, n)
    fb = R.flat_blocks(n)
    worst = 0.0
    for fam in R.STEP_FAMILIES:
        tag = f"n={n} bit={bit} front={front} {fam}"
        c = R.quant_case(n, bit, fam)
        ins = dict(x=Box(n, front=front, values=c["x"]), dy=Box(n, front=front, values=c["dy"]),
                   step=Box(1, values=c["step"]))
        y, codes = Box(n, front=front), Box(n, front=front)
        gd = _guard(ins, dict(y=y, codes=codes))

        def fwd():
            return L.sdmi_lsq_quant_fwd(ptr(ins["x"].data), n, ptr(ins["step"].data), g, qp, ptr(y.data),
                                        ptr(codes.data), st)
        _run(L, fwd, [("lsq_quant_fwd_kernel", fb)], tag)
        _check(gd, dict(y=y, codes=codes), fwd, tag)
        y_ref, dx_ref, _ = _autograd(c["x"], c["dy"], c["step"], bit)
        tm = R.terms(c["x"], c["dy"], c["step"], bit)
        _same(y.cpu(), y_ref, "y", tag)
        _same(codes.cpu(), tm["q"], "codes", tag)
        if fam == "dyadic" and n >= 11:
            assert codes.cpu()[:3].tolist() == [min(v, qp) for v in (0.0, 2.0, 2.0)], tag
            assert not torch.signbit(y.cpu()[10]) and float(y.cpu()[10]) == 0.0, f"{tag}: -0.0 must give torch's +0"
        dx, ws, ds = Box(n, front=front), Box(256), Box(1)
        gd = _guard(ins, dict(dx=dx, ds=ds))
        gd.add("workspace", ws, [(0, fb)])

        def bwd():
            return L.sdmi_lsq_quant_bwd(ptr(ins["x"].data), ptr(ins["dy"].data), n, ptr(ins["step"].data), g, qp, None,
                                        0.0, ptr(dx.data), ptr(ws.data), ptr(ds.data), st)
        _run(L, bwd, [("lsq_quant_bwd_kernel", fb), ("lsq_finish_kernel", 1)], tag)
        _check(gd, dict(dx=dx, ds=ds, ws=ws), bwd, tag)
        _same(dx.cpu(), dx_ref, "dx", tag)
        if fam == "dyadic" and n >= 11:  # exactly +-Qp passes the gradient, one ulp beyond does not
            assert bool((dx.cpu()[6:8] != 0).all()) and bool((dx.cpu()[8:10] == 0).all()), tag
        worst = max(worst, _ds_ok(float(ds.cpu()), tm["t"], R.g32(bit, n), tag))
    print(f"n={n} bit={bit} front={front}: worst |ds - ds64| / bound {worst:.3f}")


@pytest.mark.parametrize("bit", (4, 8))
def test_flat_quantiser_nan_and_scaled_gradient(bit):
    L, st = _L(), _stream()
    n = 1025
    qp, g = R.qp_of(bit), R.g_of(bit, n)
    c = R.quant_case(n, bit, "soft", nan=True)
    x, dyb, step = Box(n, values=c["x"]), Box(n, values=c["dy"]), Box(1, values=c["step"])
    y, dx, ws, ds = Box(n), Box(n), Box(256), Box(1)
    assert L.sdmi_lsq_quant_fwd(ptr(x.data), n, ptr(step.data), g, qp, ptr(y.data), None, st) == 0
    assert L.sdmi_lsq_quant_bwd(ptr(x.data), ptr(dyb.data), n, ptr(step.data), g, qp, None, 0.0, ptr(dx.data),
                                ptr(ws.data), ptr(ds.data), st) == 0
    torch.cuda.synchronize()
    y_ref, dx_ref, ds_ref = _autograd(c["x"], c["dy"], c["step"], bit)
    assert bool(torch.isnan(y.cpu()[n // 2])) and int(torch.isnan(y.cpu()).sum()) == 1  # a NaN passes to y alone
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(y_ref))
    _same(dx.cpu(), dx_ref, "dx", "nan")  # a NaN v is outside: autograd's dx there is 0
    assert np.isnan(ds_ref) and bool(torch.isnan(ds.cpu()).all())  # and the step gradient is NaN, as in torch
    # the other operand's step scales the incoming gradient first: dy' = fl(se_scale dy)
    c = R.quant_case(n, bit, "soft")
    sc = torch.tensor(0.0173)
    g_sc = R.g_of(8, 777)
    up = c["dy"] * R.effective_step(sc, 8, 777)
    x, scb = Box(n, values=c["x"]), Box(1, values=sc)
    assert L.sdmi_lsq_quant_bwd(ptr(x.data), ptr(dyb.data), n, ptr(step.data), g, qp, ptr(scb.data), g_sc, ptr(dx.data),
                                ptr(ws.data), ptr(ds.data), st) == 0
    torch.cuda.synchronize()
    _, dx_ref, _ = _autograd(c["x"], up, c["step"], bit)
    _same(dx.cpu(), dx_ref, "dx (scaled)", "scaled")
    _ds_ok(float(ds.cpu()), R.terms(c["x"], up, c["step"], bit)["t"], R.g32(bit, n), "scaled")


# (B, C, P): one element; a ragged tail with 5 -> 8 channels; two channel groups with padding; rows (P = 1); more than one
# trip of the capped grid (33 000 pixels x 2 groups = 66 000 items > 65 536; 297 000 elements > 262 144)
LAYOUT_SHAPES = ((1, 1, 1), (2, 5, 63), (3, 18, 30), (7, 24, 1), (2, 9, 16500))


def _layout_case(B, C, P, bit, seed):
    gen = torch.Generator().manual_seed(seed)
    n = B * C * P
    step = torch.tensor(0.0371)
    se = R.effective_step(step, bit, n)
    x = torch.randn(B, C, P, generator=gen) * (0.6 * R.qp_of(bit)) * se
    pl = torch.tensor(R.planted(bit))[:n] * R.effective_step(torch.tensor(0.0625), bit, n)
    x.view(-1)[:pl.numel()] = pl
    return x, step, gen


@pytest.mark.parametrize("bit", R.KERNEL_BITS)
@pytest.mark.parametrize("B,C,P", LAYOUT_SHAPES)
def test_input_quantiser_layout(B, C, P, bit):
    L, st = _L(), _stream()
    n, ld = B * C * P, (C + 7) // 8 * 8
    qp, g = R.qp_of(bit), R.g_of(bit, n)
    tag = f"({B},{C},{P}) bit={bit}"
    x, step, gen = _layout_case(B, C, P, bit, 7 * n + bit)
    ins = dict(x=Box(n, values=x), step=Box(1, values=step))
    codes = Box(B * P * ld, torch.bfloat16)
    gd = _guard(ins, dict(codes=codes))

    def fwd():
        return L.sdmi_lsq_in_fwd(ptr(ins["x"].data), B, C, P, ptr(ins["step"].data), g, qp, ptr(codes.data), ld, st)
    _run(L, fwd, [("lsq_in_fwd_kernel", R.item_blocks(B * P * (ld // 8)))], tag)
    _check(gd, dict(codes=codes), fwd, tag)
    q = R.terms(x, torch.zeros_like(x), step, bit)["q"]
    want = torch.zeros(B, P, ld)
    want[:, :, :C] = q.permute(0, 2, 1)
    got = codes.cpu(B, P, ld)
    _same(got, want.to(torch.bfloat16), "codes", tag)
    assert bool((got[:, :, C:].float() == 0).all()), f"{tag}: pad columns are not zero"
    assert torch.equal(got.float()[:, :, :C], q.permute(0, 2, 1)), f"{tag}: the codes are not exact in bf16"
    # backward on the data-gradient GEMM's NHWC result, scaled by the weight's step
    G = torch.full((B, P, ld), float("nan"))
    G[:, :, :C] = torch.randn(B, P, C, generator=gen)
    s_w, g_w = torch.tensor(0.0173), R.g_of(4, 432)
    ins = dict(x=ins["x"], step=ins["step"], G=Box(B * P * ld, values=G), s_w=Box(1, values=s_w))
    dx, ws, ds = Box(n), Box(256), Box(1)
    gd = _guard(ins, dict(dx=dx, ds=ds))
    gd.add("workspace", ws, [(0, R.flat_blocks(n))])

    def bwd():
        return L.sdmi_lsq_in_bwd(ptr(ins["x"].data), ptr(ins["G"].data), ld, B, C, P, ptr(ins["step"].data), g, qp,
                                 ptr(ins["s_w"].data), g_w, ptr(dx.data), ptr(ws.data), ptr(ds.data), st)
    _run(L, bwd, [("lsq_in_bwd_kernel", R.flat_blocks(n)), ("lsq_finish_kernel", 1)], tag)
    _check(gd, dict(dx=dx, ds=ds, ws=ws), bwd, tag)
    up = G[:, :, :C].permute(0, 2, 1).contiguous() * R.effective_step(s_w, 4, 432)
    _, dx_ref, _ = _autograd(x, up, step, bit)
    _same(dx.cpu(B, C, P), dx_ref, "dx", tag)
    r = _ds_ok(float(ds.cpu()), R.terms(x, up, step, bit)["t"], R.g32(bit, n), tag)
    print(f"{tag}: |ds - ds64| / bound {r:.3f}")


# every mode at 8 bit; the full stage, forward and backward, at the other widths too (no_quant has no width)
@pytest.mark.parametrize("mode,bit", [("full", 2), ("full", 4), ("full", 8), ("full", 9), ("no_bias_no_w", 8),
                                      ("have_pre", 8), ("have_pre", 2), ("no_quant", 8)])
@pytest.mark.parametrize("B,C,P", LAYOUT_SHAPES)
def test_output_stage(B, C, P, mode, bit):
    L, st = _L(), _stream()
    n, ld = B * C * P, (C + 7) // 8 * 8
    qp, g = R.qp_of(bit), R.g_of(bit, n)
    tag = f"({B},{C},{P}) {mode} bit={bit}"
    gen = torch.Generator().manual_seed(13 * n + len(mode))
    acc = torch.full((B, P, ld), float("nan"))
    acc[:, :, :C] = torch.randint(-40000, 40000, (B, P, C), generator=gen).float()
    bias = torch.randn(C, generator=gen) if mode != "no_bias_no_w" else None
    s_in, s_w = torch.tensor(0.0213), (torch.tensor(0.0057) if mode != "no_bias_no_w" else None)
    g_in, g_w = R.g_of(8, 1200), R.g_of(4, 540)
    f = R.effective_step(s_in, 8, 1200) * (R.effective_step(s_w, 4, 540) if s_w is not None else torch.tensor(1.0))
    pre = acc[:, :, :C] * f
    if bias is not None:
        pre = pre + bias
    if mode == "have_pre":
        pre = acc[:, :, :C].clone()
    s_out = pre.abs().max() / (1.2 * qp)  # a few elements beyond +-Qp
    ins = dict(s_in=Box(1, values=s_in), s_w=Box(1, values=s_w if s_w is not None else torch.ones(())),
               bias=Box(C, values=bias if bias is not None else torch.zeros(C)), s_out=Box(1, values=s_out))
    accb, y = Box(B * P * ld, values=acc), Box(n)
    gd = _guard(ins, dict(y=y))
    cols = torch.zeros(B * P, ld, dtype=torch.bool)
    cols[:, :C] = mode != "have_pre"
    snap = accb.buf.clone()

    def fwd():
        return L.sdmi_lsq_out_fwd(ptr(accb.data), ld, B, C, P, ptr(ins["s_in"].data), g_in,
                                  ptr(ins["s_w"].data) if s_w is not None else None, g_w,
                                  ptr(ins["bias"].data) if bias is not None else None, ptr(ins["s_out"].data), g,
                                  0 if mode == "no_quant" else qp, 1 if mode == "have_pre" else 0, ptr(y.data), st)
    _run(L, fwd, [("lsq_out_fwd_kernel", R.flat_blocks(n))], tag)
    bad = gd.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"
    now = accb.buf.clone()
    keep = torch.ones_like(now, dtype=torch.bool)
    keep[accb.front:accb.front + accb.n] = ~cols.view(-1).to(DEV)
    assert torch.equal(bits(now)[keep], bits(snap)[keep]), f"{tag}: the accumulator changed outside columns < C"
    _same(accb.cpu(B, P, ld)[:, :, :C], pre, "pre", tag)
    y_ref = pre if mode == "no_quant" else R.quant_lsq(pre, bit, s_out)
    _same(y.cpu(B, C, P), y_ref.permute(0, 2, 1), "y", tag)
    if mode == "no_quant":
        return
    # backward: d_pre as NHWC bf16 with zero pads, and ds_out
    dy = torch.randn(B, C, P, generator=gen)
    dyb, dpre, ws, ds = Box(n, values=dy), Box(B * P * ld, torch.bfloat16), Box(256), Box(1)
    nb = R.item_blocks(B * P * (ld // 8))
    gd = _guard(dict(dy=dyb, s_out=ins["s_out"], pre=accb), dict(dpre=dpre, ds=ds))
    gd.add("workspace", ws, [(0, nb)])

    def bwd():
        return L.sdmi_lsq_out_bwd(ptr(accb.data), ld, ptr(dyb.data), B, C, P, ptr(ins["s_out"].data), g, qp,
                                  ptr(dpre.data), ld, ptr(ws.data), ptr(ds.data), st)
    _run(L, bwd, [("lsq_out_bwd_kernel", nb), ("lsq_finish_kernel", 1)], tag)
    _check(gd, dict(dpre=dpre, ds=ds, ws=ws), bwd, tag)
    up = dy.permute(0, 2, 1).contiguous()
    _, dx_ref, _ = _autograd(pre, up, s_out, bit)
    want = torch.zeros(B, P, ld)
    want[:, :, :C] = dx_ref
    _same(dpre.cpu(B, P, ld), want.to(torch.bfloat16), "d_pre", tag)
    r = _ds_ok(float(ds.cpu()), R.terms(pre, up, s_out, bit)["t"], R.g32(bit, n), tag)
    print(f"{tag}: |ds - ds64| / bound {r:.3f}")


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("n", R.KERNEL_SIZES)
def test_step_initialiser_and_scale(n, front):
    L, st = _L(), _stream()
    gen = torch.Generator().manual_seed(n)
    fb = R.flat_blocks(n)
    for bit, kind in ((8, "randn"), (4, "randn"), (8, "zero"), (8, "nan")):
        tag = f"n={n} bit={bit} {kind}"
        x = torch.randn(n, generator=gen) * 3.7
        if kind == "zero":
            x = torch.zeros(n)
            x[n // 2] = -0.0
        if kind == "nan":
            x[n // 3] = float("nan")
        xb, step, ws = Box(n, front=front, values=x), Box(1, values=torch.tensor(0.123)), Box(256)
        gd = _guard(dict(x=xb), dict(step=step))
        gd.add("workspace", ws, [(0, fb)])

        def init():
            return L.sdmi_lsq_init_step(ptr(xb.data), n, R.qp_of(bit), ptr(ws.data), ptr(step.data), st)
        _run(L, init, [("lsq_absmax_kernel", fb), ("lsq_init_finish_kernel", 1)], tag)
        _check(gd, dict(step=step, ws=ws), init, tag)
        got = step.cpu()[0]
        if kind == "zero":
            assert float(got) == float(np.float32(0.123)), f"{tag}: the step was touched at range 0"
        elif kind == "nan":
            assert bool(torch.isnan(got)), tag
        else:
            _same(got.reshape(1), R.init_step(x, bit).reshape(1), "step", tag)
    # scale: out = fl(x se) or fl(x / se)
    x = torch.randn(n, generator=gen)
    s = torch.tensor(0.0371)
    g = R.g_of(4, n)
    se = R.effective_step(s, 4, n)
    xb, sb, out = Box(n, front=front, values=x), Box(1, values=s), Box(n, front=front)
    for divide, ref in ((0, x * se), (1, x / se)):
        gd = _guard(dict(x=xb, s=sb), dict(out=out))

        def scale():
            return L.sdmi_lsq_scale(ptr(xb.data), n, ptr(sb.data), g, divide, ptr(out.data), st)
        _run(L, scale, [("lsq_scale_kernel", fb)], f"scale n={n}")
        _check(gd, dict(out=out), scale, f"scale n={n}")
        _same(out.cpu(), ref, "out", f"scale n={n} divide={divide}")


def test_error_returns_launch_nothing():
    L, st = _L(), _stream()
    x, step, y, ws = Box(64), Box(1, values=torch.tensor(0.1)), Box(64), Box(256)
    codes = Box(64, torch.bfloat16)
    snap = [b.buf.clone() for b in (y, ws, codes)]
    g = 0.01
    calls = (
        lambda: L.sdmi_lsq_quant_fwd(ptr(x.data), 64, ptr(step.data), g, 300, ptr(y.data), None, st),  # 10 bits
        lambda: L.sdmi_lsq_quant_fwd(ptr(x.data), 64, ptr(step.data), g, 0, ptr(y.data), None, st),
        lambda: L.sdmi_lsq_quant_fwd(ptr(x.data), 0, ptr(step.data), g, 127, ptr(y.data), None, st),
        lambda: L.sdmi_lsq_quant_fwd(ptr(x.data), 64, None, g, 127, ptr(y.data), None, st),
        lambda: L.sdmi_lsq_quant_fwd(ptr(x.data), 64, ptr(step.data), g, 127, None, None, st),
        lambda: L.sdmi_lsq_in_fwd(ptr(x.data), 2, 5, 4, ptr(step.data), g, 127, ptr(codes.data), 4, st),  # ld < C
        lambda: L.sdmi_lsq_in_fwd(ptr(x.data), 2, 5, 4, ptr(step.data), g, 127, ptr(codes.data), 6, st),  # ld % 8
        lambda: L.sdmi_lsq_in_fwd(ptr(x.data), 2, 5, 4, ptr(step.data), g, 127, ptr(codes.data[1:]), 8, st),  # align
        lambda: L.sdmi_lsq_out_fwd(ptr(x.data), 4, 2, 5, 4, None, g, None, g, None, ptr(step.data), g, 127, 0,
                                   ptr(y.data), st),
        lambda: L.sdmi_lsq_out_fwd(ptr(x.data), 8, 2, 5, 4, None, g, None, g, None, None, g, 127, 0, ptr(y.data), st),
        lambda: L.sdmi_lsq_init_step(ptr(x.data), 64, 127, None, ptr(step.data), st),
    )
    for i, call in enumerate(calls):
        rc, ops = recorded(L, call)
        assert rc == -1 and ops == [], f"call {i}: returned {rc}, launched {ops}"
    torch.cuda.synchronize()
    for a, b in zip(snap, (y, ws, codes)):
        assert torch.equal(bits(a), bits(b.buf))
