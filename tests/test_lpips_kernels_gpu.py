"""The LPIPS kernels (csrc/lpips.hip) one by one, every output in a NaN-guarded buffer (tests/gemm_matrix.Guarded):
* the 2x2 max-pool pair bit-exact against F.max_pool2d on the same bf16 device tensors (odd edges, ties);
* the layer distance and its backward against float64 torch on the same bf16 inputs, with planted all-zero feature
  rows, to the bounds of the project's other fp32-reduction kernels (tests/test_vqvae_train_gpu.py);
* image scaling in and out bit-exact against the torch expression;
* the implicit-conv GEMM combinations the LPIPS engine launches that no other exact test runs (A_CONV with the ReLU
  epilogue and with the ReLU-gradient mask), on exact integer data."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_matrix as GM
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


def _k():
    from sdmi import kernels
    return kernels


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ---- max-pool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ties", [((3, 6, 10, 64), False), ((2, 5, 7, 128), False), ((2, 2, 2, 512), False),
                                         ((2, 5, 7, 128), True), ((3, 6, 10, 64), True)])
def test_maxpool_pair_bit_exact(shape, ties):
    K = _k()
    B, H, W, C = shape
    g = torch.Generator().manual_seed(21)
    if ties:  # small integers (as ReLU outputs: many zeros): equal values in almost every window
        x = torch.randint(0, 3, shape, generator=g).to(BF)
    else:
        x = torch.randn(shape, generator=g).to(BF)
    OH, OW = H // 2, W // 2
    dy = torch.randn(B, OH, OW, C, generator=g).to(BF)
    xd = x.to(DEV)
    xt = xd.permute(0, 3, 1, 2).detach().requires_grad_(True)
    yt = F.max_pool2d(xt, 2, 2)
    yt.backward(dy.to(DEV).permute(0, 3, 1, 2))
    y_ref, dx_ref = yt.detach().permute(0, 2, 3, 1), xt.grad.permute(0, 2, 3, 1)
    y = GM.Guarded(B * OH * OW, C, C, BF, DEV)
    dx = GM.Guarded(B * H * W, C, C, BF, DEV)
    K.maxpool2_fwd(xd.view(-1, C), B, H, W, C, y.view)
    K.maxpool2_bwd(xd.view(-1, C), dy.to(DEV).view(-1, C), B, H, W, C, dx.view)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.view), _bits(y_ref.reshape(-1, C)))
    assert torch.equal(dx.view.float(), dx_ref.reshape(-1, C).float())  # +0 / -0 of an unrouted element compare equal
    assert y.outside_untouched() and dx.outside_untouched()
    if ties:  # an all-equal window routes its whole gradient to (0, 0)
        eq = (x[:, 0:2 * OH:2, 0:2 * OW:2] == x[:, 1:2 * OH:2, 0:2 * OW:2]) & \
             (x[:, 0:2 * OH:2, 0:2 * OW:2] == x[:, 0:2 * OH:2, 1:2 * OW:2]) & \
             (x[:, 0:2 * OH:2, 0:2 * OW:2] == x[:, 1:2 * OH:2, 1:2 * OW:2])
        assert eq.any()
        got = dx.view.cpu().view(B, H, W, C)
        assert torch.equal(got[:, 0:2 * OH:2, 0:2 * OW:2][eq], dy[eq])
        assert (got[:, 1:2 * OH:2, 1:2 * OW:2][eq] == 0).all()


# ---- distance ------------------------------------------------------------------------------------------------------
def _dist_inputs(B, P, C, seed):
    """A tap as ReLU outputs (half the entries zero), bf16, with all-zero rows planted in f0 only, f1 only and both
    (as many of the three as there are (sample, pixel) pairs to spare)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(2, B * P, C, generator=g)).to(BF)
    T = B * P
    spots = [] if T == 1 else [(T // 3, (0,)), ((2 * T) // 3, (1,)), (T - 1, (0, 1))]
    if T == 3:
        spots = [(0, (0,)), (1, (1,)), (2, (0, 1))]
    for r, sides in spots:
        for s in sides:
            f[s, r] = 0
    w = torch.randn(C, generator=g).abs() / C
    gv = torch.rand(B, generator=g) + 0.5
    return f.reshape(2 * B * P, C), w, gv, spots


def _dist_ref(f, w, gv, B, P, C, addend, side):
    """float64 autograd of val[b] = mean_p sum_c w_c (u0 - u1)^2; the tap gradient goes through the tap's ReLU."""
    fl = f.double().requires_grad_(True)
    u = F.normalize(fl.view(2, B, P, C), dim=-1, eps=1e-12)
    val = (((u[0] - u[1]) ** 2) * w.double()).sum(-1).mean(-1)
    (val * gv.double()).sum().backward()
    fs = f.view(2, B * P, C)[side].double()
    gr = fl.grad.view(2, B * P, C)[side]
    if addend is not None:
        gr = gr + addend.double()
    return val.detach(), torch.where(fs > 0, gr, torch.zeros_like(gr))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 6, 1600])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_dist_fwd_bwd_vs_float64(C, P, B):
    K = _k()
    f, w, gv, spots = _dist_inputs(B, P, C, seed=C + P + B)
    side = (C // 64 + P + B) % 2  # both sides over the matrix
    with_add = (C + P) % 3 == 0
    addend = None
    if with_add:
        addend = (torch.randn(B * P, C, generator=torch.Generator().manual_seed(4)) * 1e-3).to(BF)
    val_ref, g_ref = _dist_ref(f, w, gv, B, P, C, addend, side)
    fd, wd, gd = f.to(DEV), w.to(DEV), gv.to(DEV)
    add_d = addend.to(DEV) if with_add else None
    runs = []
    for _ in range(2):
        val = GM.Guarded(1, B, B, F32, DEV)
        rn = GM.Guarded(1, 2 * B * P, 2 * B * P, F32, DEV)
        dy = GM.Guarded(B * P, C, C, BF, DEV)
        K.lpips_dist_fwd(fd, wd, B, P, C, val.view[0], False, rn.view[0])
        K.lpips_dist_bwd(fd, wd, rn.view[0], B, P, C, side, dy.view, g=gd, addend=add_d)
        torch.cuda.synchronize()
        assert val.outside_untouched() and rn.outside_untouched() and dy.outside_untouched()
        runs.append((val.view[0].cpu(), rn.view[0].cpu(), dy.view.cpu()))
    v, rn, dy = runs[0]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], runs[1])), "two runs differ bitwise"
    assert torch.isfinite(v).all() and torch.isfinite(rn).all() and torch.isfinite(dy.float()).all()
    err_v = (v.double() - val_ref).abs()
    print(f"C={C} P={P} B={B}: val rel err {(err_v / val_ref.abs().clamp_min(1e-30)).max().item():.2e}, "
          f"grad worst |err| / (1e-2 |ref| + 1e-6) {((dy.double() - g_ref).abs() / (1e-2 * g_ref.abs() + 1e-6)).max():.3f}")
    assert (err_v <= 1e-4 * val_ref.abs() + 1e-7).all(), (v, val_ref)
    assert ((dy.double() - g_ref).abs() <= 1e-2 * g_ref.abs() + 1e-6).all()
    for r, sides in spots:  # planted rows: exact zeros on their own side
        if side in sides:
            assert (dy[r] == 0).all()


def test_dist_accumulates_over_taps_and_scales():
    """accumulate adds the tap's mean to val in place; gscale multiplies the per-sample gradient factor."""
    K = _k()
    B, P, C = 2, 37, 128
    f, w, gv, _ = _dist_inputs(B, P, C, seed=8)
    fd, wd = f.to(DEV), w.to(DEV)
    one = torch.empty(B, device=DEV)
    rn = torch.empty(2 * B * P, device=DEV)
    K.lpips_dist_fwd(fd, wd, B, P, C, one, False, rn)
    acc = torch.tensor([0.25, -3.0], device=DEV)
    K.lpips_dist_fwd(fd, wd, B, P, C, acc, True)
    assert torch.equal(acc, torch.tensor([0.25, -3.0], device=DEV) + one)
    a, b = (GM.Guarded(B * P, C, C, BF, DEV) for _ in range(2))
    K.lpips_dist_bwd(fd, wd, rn, B, P, C, 0, a.view, g=torch.full((B,), 0.5, device=DEV))
    K.lpips_dist_bwd(fd, wd, rn, B, P, C, 0, b.view, gscale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.view), _bits(b.view))
    mean = torch.empty(1, device=DEV)
    K.lpips_mean(one, B, 0.5, mean)
    assert torch.equal(mean, (one[0] + one[1]).reshape(1) * 0.5)


# ---- image scaling in / out ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("layouts", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 33, 40)])
def test_prep_bit_exact(shape, layouts, normalize):
    K = _k()
    B, H, W = shape
    g = torch.Generator().manual_seed(31)
    ims = [torch.rand(B, 3, H, W, generator=g) * 2 - 1 for _ in range(2)]
    shift, scale = torch.tensor(R.SHIFT), torch.tensor(R.SCALE)
    want = []
    for x in ims:
        v = 2 * x - 1 if normalize else x
        v = (v - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)
        want.append(F.pad(v.permute(0, 2, 3, 1).reshape(-1, 3), (0, 5)))
    want = torch.cat(want).to(BF)
    src = []
    for x, flat in zip(ims, layouts):
        if flat:  # the training engine's NHWC fp32 [B*H*W][8]; the pad channels hold junk the kernel must not read into c < 3
            t = torch.full((B * H * W, 8), 7.0)
            t[:, :3] = x.permute(0, 2, 3, 1).reshape(-1, 3)
            src.append(t.to(DEV))
        else:
            src.append(x.to(DEV))
    out = GM.Guarded(2 * B * H * W, 8, 8, BF, DEV)
    K.lpips_prep(src[0], layouts[0], src[1], layouts[1], B, H, W, shift.to(DEV), scale.to(DEV), normalize, out.view)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.view.cpu()), _bits(want))
    assert (out.view[:, 3:] == 0).all() and out.outside_untouched()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 33, 40)])
def test_image_grad_bit_exact(shape, normalize):
    K = _k()
    B, H, W = shape
    g = torch.Generator().manual_seed(32)
    d = torch.randn(B * H * W, 8, generator=g).to(BF)  # channels 3..7 hold junk
    scale = torch.tensor(R.SCALE)
    gimg = d[:, :3].float() / scale * (2.0 if normalize else 1.0)
    nchw = GM.Guarded(1, B * 3 * H * W, B * 3 * H * W, F32, DEV)
    prev = torch.randn(B * H * W, 8, generator=g).to(BF)
    acc = GM.place(prev, 8, DEV, tail=8)
    K.lpips_image_grad(d.to(DEV), B, H, W, scale.to(DEV), normalize, out_nchw=nchw.view[0])
    K.lpips_image_grad(d.to(DEV), B, H, W, scale.to(DEV), normalize, acc_nhwc=acc.view)
    torch.cuda.synchronize()
    want = gimg.view(B, H * W, 3).permute(0, 2, 1).reshape(-1)
    assert torch.equal(_bits(nchw.view[0].cpu()), _bits(want))
    got = acc.view.cpu()
    assert torch.equal(_bits(got[:, :3]), _bits((prev[:, :3].float() + gimg).to(BF)))
    assert torch.equal(_bits(got[:, 3:]), _bits(prev[:, 3:]))  # pad channels untouched
    assert nchw.outside_untouched() and acc.outside_untouched()
    # the trainer's form: acc written whole = sdmi_mse's gradient 2 (pred - target) / n + the image gradient, one rounding
    target = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    pred = torch.full((B * H * W, 8), 7.0)  # pad channels hold junk
    pred[:, :3] = (target + 0.1 * torch.randn(B, 3, H, W, generator=g)).permute(0, 2, 3, 1).reshape(-1, 3)
    whole = GM.Guarded(B * H * W, 8, 8, BF, DEV)
    K.lpips_image_grad(d.to(DEV), B, H, W, scale.to(DEV), normalize, acc_nhwc=whole.view,
                       mse=(pred.to(DEV), target.to(DEV)))
    torch.cuda.synchronize()
    mse_g = 2 * (pred[:, :3] - target.permute(0, 2, 3, 1).reshape(-1, 3)) / float(B * 3 * H * W)
    got = whole.view.cpu()
    assert torch.equal(_bits(got[:, :3]), _bits((mse_g + gimg).to(BF)))
    assert (got[:, 3:] == 0).all() and whole.outside_untouched()


# ---- GEMM descriptor combinations of the engine not run exactly elsewhere -------------------------------------------
def _int_conv(B, H, W, cin, cout, seed):
    x = GM.ints((B, cin, H, W), seed).double()
    w = GM.ints((cout, cin, 3, 3), seed + 1).double()
    GM.assert_exact_k(9 * cin)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])  # noqa: E731
    return x, w, flat


@pytest.mark.parametrize("case", ["conv1_1", "c64", "c128_ragged"])
def test_conv_bias_relu_exact(case):
    """A_CONV + bias + act 2 (the VGG forward layers; conv1_1 with cin padded 3 -> 8)."""
    K = _k()
    B, H, W, cin, cout = {"conv1_1": (2, 9, 7, 3, 64), "c64": (2, 6, 10, 64, 128), "c128_ragged": (1, 5, 5, 128, 256)}[case]
    x, w, flat = _int_conv(B, H, W, cin, cout, 41)
    bias = GM.ints((cout,), 43).to(F32)
    ref = F.relu(F.conv2d(x, w, bias.double(), padding=1))
    cp = 8 if cin == 3 else cin
    xp = F.pad(flat(x), (0, cp - cin))
    wpk = F.pad(w.permute(0, 2, 3, 1), (0, cp - cin)).reshape(cout, 9 * cp)
    xg, wg = GM.place(xp, cp, DEV), GM.place(wpk, 9 * cp, DEV)
    out = GM.Guarded(B * H * W, cout, cout + 8, BF, DEV)
    K.conv_fwd(xg.view, B, H, W, cp, cp, wg.view, cout, 3, 3, 1, 1, out.view, cout + 8, bias=bias.to(DEV), act=2)
    torch.cuda.synchronize()
    assert torch.equal(out.view.cpu(), GM.to_c(flat(ref), BF))
    assert out.outside_untouched()


@pytest.mark.parametrize("case", ["c64_mask", "c128_mask", "to_image"])
def test_conv_dgrad_relu_mask_exact(case):
    """A_CONV + act 3 + aux (data gradient through the previous layer's ReLU), and the 8-column data gradient of
    conv1_1 (no mask): flipped-tap transposed weights as the engine packs them."""
    K = _k()
    B, H, W, cout, cin, mask = {"c64_mask": (2, 6, 10, 64, 64, True), "c128_mask": (1, 5, 7, 128, 64, True),
                                "to_image": (2, 9, 7, 64, 3, False)}[case]
    dy, w, flat = _int_conv(B, H, W, cout, cin, 51)  # dy (B, cout, H, W); w here is the transposed-role weight
    # dx = conv_transpose(dy, W) = conv2d(dy, flip(W)^T): w is already (cin, cout, 3, 3) in that role
    ref = flat(F.conv2d(dy, w, padding=1))
    cp = 8 if cin == 3 else cin
    wpk = F.pad(w.permute(0, 2, 3, 1).reshape(cin, 9 * cout), (0, 0, 0, cp - cin))
    ref = F.pad(ref, (0, cp - cin))
    aux = None
    if mask:
        a = GM.ints((B * H * W, cin), 53).to(BF)
        ref = torch.where(a.double() > 0, ref, torch.zeros_like(ref))
        aux = GM.place(a, cin + 8, DEV)
    dg, wg = GM.place(flat(dy), cout, DEV), GM.place(wpk, 9 * cout, DEV)
    out = GM.Guarded(B * H * W, cp, cp, BF, DEV)
    K.conv_fwd(dg.view, B, H, W, cout, cout, wg.view, cp, 3, 3, 1, 1, out.view, cp, act=3 if mask else 0,
               aux=aux.view if mask else None)
    torch.cuda.synchronize()
    assert torch.equal(out.view.cpu(), GM.to_c(ref, BF))
    assert out.outside_untouched()


def _same_with_nan(got, ref):
    n = torch.isnan(ref)
    return torch.equal(torch.isnan(got), n) and torch.equal(got[~n], ref[~n])


@pytest.mark.parametrize("pad", [8, 4], ids=["vec", "scalar"])
@pytest.mark.parametrize("case", ["conv1_1", "c64", "c128_ragged"])
def test_conv_bias_relu_passes_nan(case, pad):
    """act 2 is torch's relu: a NaN accumulator stays NaN after the bias (v <= 0 ? 0 : v, not fmaxf(v, 0), which
    returns 0). One NaN planted in the input reaches the 3x3 neighbourhood of its pixel in every output channel;
    everything else is the exact integer result of test_conv_bias_relu_exact. pad: the output's row stride is
    cout + pad -- a multiple of 8 takes the 8-wide epilogue (Epi::finish8), cout + 4 the per-element one (act1)."""
    K = _k()
    B, H, W, cin, cout = {"conv1_1": (2, 9, 7, 3, 64), "c64": (2, 6, 10, 64, 128), "c128_ragged": (1, 5, 5, 128, 256)}[case]
    x, w, flat = _int_conv(B, H, W, cin, cout, 41)
    x[B - 1, cin - 1, 2, 3] = float("nan")
    bias = GM.ints((cout,), 43).to(F32)
    ref = flat(F.relu(F.conv2d(x, w, bias.double(), padding=1)))
    assert int(torch.isnan(ref).sum()) == 9 * cout and not torch.isnan(ref).all()
    cp = 8 if cin == 3 else cin
    xp = F.pad(flat(x), (0, cp - cin))
    wpk = F.pad(w.permute(0, 2, 3, 1), (0, cp - cin)).reshape(cout, 9 * cp)
    xg, wg = GM.place(xp, cp, DEV), GM.place(wpk, 9 * cp, DEV)
    out = GM.Guarded(B * H * W, cout, cout + pad, BF, DEV)
    K.conv_fwd(xg.view, B, H, W, cp, cp, wg.view, cout, 3, 3, 1, 1, out.view, cout + pad, bias=bias.to(DEV), act=2)
    torch.cuda.synchronize()
    assert _same_with_nan(out.view.cpu().double(), GM.to_c(ref, BF).double())
    assert out.outside_untouched()


@pytest.mark.parametrize("pad", [0, 4], ids=["vec", "scalar"])
@pytest.mark.parametrize("case", ["c64_mask", "c128_mask"])
def test_conv_dgrad_relu_mask_passes_under_nan(case, pad):
    """act 3 is torch's threshold_backward: the gradient is zeroed where aux <= 0 and passes everywhere else, under a
    NaN activation too (not `aux > 0 ? v : 0`). The data of test_conv_dgrad_relu_mask_exact with NaNs planted in aux.
    pad: the output's row stride is cin + pad -- cin takes the 8-wide epilogue, cin + 4 the per-element one (act1)."""
    K = _k()
    B, H, W, cout, cin = {"c64_mask": (2, 6, 10, 64, 64), "c128_mask": (1, 5, 7, 128, 64)}[case]
    dy, w, flat = _int_conv(B, H, W, cout, cin, 51)
    ref = flat(F.conv2d(dy, w, padding=1))
    wpk = w.permute(0, 2, 3, 1).reshape(cin, 9 * cout)
    a = GM.ints((B * H * W, cin), 53).to(BF)
    a.view(-1)[::7] = float("nan")
    ref = torch.where(a.double() <= 0, torch.zeros_like(ref), ref)
    planted = torch.isnan(a)
    assert (ref[planted] != 0).any() and not torch.isnan(ref).any()
    aux = GM.place(a, cin + 8, DEV)
    dg, wg = GM.place(flat(dy), cout, DEV), GM.place(wpk, 9 * cout, DEV)
    out = GM.Guarded(B * H * W, cin, cin + pad, BF, DEV)
    K.conv_fwd(dg.view, B, H, W, cout, cout, wg.view, cin, 3, 3, 1, 1, out.view, cin + pad, act=3, aux=aux.view)
    torch.cuda.synchronize()
    assert torch.equal(out.view.cpu(), GM.to_c(ref, BF))
    assert out.outside_untouched()
