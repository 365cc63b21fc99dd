"""Every epilogue feature of sdmi_gemm on each of its three writers: the register-staged kernel unsplit (variant 0),
an LDS-DMA kernel unsplit (variant 2: the 128-row LDS epilogue, variant 9: the 64-row one) and split-K (3 slices)
through the reducer. Exact integer data and guarded buffers as tests/test_gemm_variants_gpu.py: every addend is a
small integer (alpha = 0.5 halves an integer), so the fp32 epilogue is exact and C must torch.equal the float64
reference cast to C's dtype. SiLU is the one inexact feature: random values under the elementwise dot-product bound
propagated through SiLU's Lipschitz constant (<= 1.1) plus one fp32 ulp of the result."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_matrix as GM

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
# ragged against every tile; K = 264 is 4 k-tiles of 64 and a ragged fifth, which three slices share as 2 + 2 + 1 (a
# 4-tile K such as 200 would be planned as 3 slices and launched as 2 + 2)
M, N, KD = 125, 168, 264
N128 = 232  # variant 2 takes its 128-column tile here (the last tile more than half used), the 64-column one at N
assert GM.launched_slices(3, KD) == 3 and (KD + 63) // 64 % 3

# (id, requested variant, splits hint, expected variant)
WRITERS = [("v0", 1, 1, 0), ("dma2", 2, 1, 2), ("dma9", 9, 1, 9), ("splitk", 2, 3, 2)]

# variant 2's column tile per N of this file, by hand from the pick_tbn rules: 64 for N <= 64 and where the last
# 128-column tile would be at most half used (168, 163, 144), else 128; variants 0 and 9 always have 128 columns
TILE_V2 = {168: 64, 163: 64, 144: 64, 40: 64, 24: 64, 64: 64, 96: 128, N128: 128}


def _tile(var, n):
    return TILE_V2[n] if var == 2 else 128


def _k():
    from sdmi import kernels, _lib
    return kernels, _lib


def _ivec(n, seed, dtype):
    return GM.ints((n,), seed).to(dtype)


def _epi_ref(acc, *, bias=None, bias2=None, rowbias=None, rb_div=0, rb_mod=0, resid=None, alpha=1.0, act=0, aux=None):
    """v = act(alpha acc + bias + bias2 + rowbias[(m / rb_div) % rb_mod] + resid) in float64 (include/sdmi.h)."""
    v = alpha * acc.double()
    for b in (bias, bias2):
        if b is not None:
            v = v + b.double()[: v.shape[1]]
    if rowbias is not None:
        r = torch.arange(v.shape[0]) // max(1, rb_div)
        if rb_mod:
            r = r % rb_mod
        v = v + rowbias.double()[r][:, : v.shape[1]]
    if resid is not None:
        v = v + resid.double()
    if act == 2:
        v = v.clamp_min(0)
    if act == 3:
        v = torch.where(aux.double() > 0, v, torch.zeros_like(v))
    return v


# feature -> (gemm kwargs built from CPU tensors, reference kwargs); tensors are placed in guarded device buffers
def _feature(name, m, n):
    cpu, ref, opt = {}, {}, {}
    if name in ("bias", "all"):
        cpu["bias"] = ref["bias"] = _ivec(n, 31, F32)
    if name in ("bias2", "all"):
        cpu["bias2"] = ref["bias2"] = _ivec(n, 32, F32)
    if name in ("rowbias_div", "all"):
        cpu["rowbias"] = ref["rowbias"] = GM.ints((m // 25 + 1, n), 33).to(BF)
        opt.update(rb_div=25)
        ref.update(rb_div=25)
    if name == "rowbias_mod":
        cpu["rowbias"] = ref["rowbias"] = GM.ints((7, n), 34).to(BF)
        opt.update(rb_div=1, rb_mod=7)
        ref.update(rb_div=1, rb_mod=7)
    if name in ("resid", "all"):
        cpu["resid"] = ref["resid"] = GM.ints((m, n), 35).to(BF)
    if name in ("alpha", "all"):
        opt.update(alpha=0.5)
        ref.update(alpha=0.5)
    if name in ("relu", "all"):
        opt.update(act=2)
        ref.update(act=2)
    if name == "relu_grad":
        cpu["aux"] = ref["aux"] = GM.ints((m, n), 36).to(BF)
        opt.update(act=3)
        ref.update(act=3)
    return cpu, ref, opt


def _launch(kn, L, m, n, k, c_dtype, feature, *, ldc=None, c_offset=0, m_store=0, n_store=0):
    A0, B0 = GM.int_operands()
    cpu, refkw, opt = _feature(feature, m, n)
    keep, kw = [], dict(opt)
    for key, t in cpu.items():
        if t.dim() == 1:
            g = GM.place(t[None], t.shape[0] + 8, DEV, dtype=F32, tail=1)
            kw[key] = g.view[0]
        else:
            g = GM.place(t, n + 8, DEV)
            kw[key] = g.view
            kw[{"rowbias": "rb_ld", "resid": "ldr", "aux": "ld_aux"}[key]] = n + 8
        keep.append(g)
    c = GM.run_linear(kn, L, GM.A_ROW, GM.B_NK, m, n, k, A0[:m, :k], B0[:k, :n], c_dtype, DEV, ldc=ldc,
                      c_offset=c_offset, m_store=m_store, n_store=n_store, **kw)
    ref = _epi_ref(GM.int_ref(m, n, k), **refkw)
    return c, ref[: m_store or m, : n_store or n]


FEATURES = [  # (id, feature, N, C dtype, launch options)
    ("plain", "none", N, BF, {}),
    ("bias", "bias", N, BF, {}),
    ("bias2", "bias2", N, BF, {}),
    ("rowbias_div", "rowbias_div", N, BF, {}),
    ("rowbias_mod", "rowbias_mod", N, BF, {}),
    ("resid_ldr", "resid", N, BF, {}),
    ("alpha", "alpha", N, BF, {}),
    ("relu", "relu", N, BF, {}),
    ("relu_grad_aux", "relu_grad", N, BF, {}),
    ("f32", "bias", N, F32, {}),
    ("all", "all", N, BF, {}),
    ("all_f32", "all", N, F32, {}),
    ("n_store8", "bias", N, BF, dict(n_store=8)),
    ("n_store4", "bias", N, BF, dict(n_store=4)),
    ("m_store", "all", N, BF, dict(m_store=61)),
    ("scalar_ldc", "all", N, BF, dict(ldc=N + 3)),
    ("scalar_ldc_f32", "bias", N, F32, dict(ldc=N + 3)),
    ("scalar_n", "all", 163, BF, {}),
    ("scalar_c_offset", "all", N, BF, dict(c_offset=1)),
    ("scalar_m_n_store", "resid", 163, F32, dict(m_store=61, n_store=4)),
    # the same on variant 2's 128-column tile (and variant 0 / 9 at two whole tiles less 24 columns)
    ("t128_all", "all", N128, BF, {}),
    ("t128_all_f32", "all", N128, F32, {}),
    ("t128_relu_grad_aux", "relu_grad", N128, BF, {}),
    ("t128_rowbias_mod", "rowbias_mod", N128, BF, {}),
    ("t128_n_store8_m_store", "bias", N128, BF, dict(n_store=8, m_store=61)),
    ("t128_scalar_ldc", "all", N128, BF, dict(ldc=N128 + 3)),
    ("t128_scalar_c_offset", "resid", N128, F32, dict(c_offset=1)),
]


@pytest.mark.parametrize("writer", WRITERS, ids=[w[0] for w in WRITERS])
@pytest.mark.parametrize("feat", FEATURES, ids=[f[0] for f in FEATURES])
def test_epilogue_feature_exact(monkeypatch, writer, feat):
    kn, L = _k()
    _, req, hint, var = writer
    _, feature, n, c_dtype, opts = feat
    GM.force(monkeypatch, kn, hint, req)
    c, ref = _launch(kn, L, M, n, KD, c_dtype, feature, **opts)
    tag = f"{writer[0]} {feat[0]}"
    GM.check_log(kn, var, _tile(var, n), hint, tag)
    torch.cuda.synchronize()
    assert torch.equal(c.view.cpu(), GM.to_c(ref, c_dtype)), f"{tag}: C differs from the exact reference"
    assert c.outside_untouched(), f"{tag}: memory outside the m_store x n_store window changed"


@pytest.mark.parametrize("writer", WRITERS, ids=[w[0] for w in WRITERS])
@pytest.mark.parametrize("perm", [1, 2])
def test_epilogue_column_permute(monkeypatch, writer, perm):
    """perm 1 (torch conv-weight layout) and 2 (tap-major) with p_cvalid < p_cin: columns n = tap * 16 + c are stored
    at c * 9 + tap / tap * 8 + c for c < 8 only, the rest dropped; a row limit rides along."""
    kn, L = _k()
    _, req, hint, var = writer
    cin, taps, cvalid, n, m_store = 16, 9, 8, 144, 120
    GM.force(monkeypatch, kn, hint, req)
    A0, B0 = GM.int_operands()
    c = GM.run_linear(kn, L, GM.A_ROW, GM.B_NK, M, n, KD, A0[:M, :KD], B0[:KD, :n], F32, DEV, c_cols=taps * cvalid,
                      m_store=m_store, perm=(cin, taps, cvalid, perm), alpha=0.5)
    GM.check_log(kn, var, _tile(var, n), hint, writer[0])
    ref = GM.permuted(0.5 * GM.int_ref(M, n, KD)[:m_store].double().view(m_store, taps, cin), perm, cvalid)
    torch.cuda.synchronize()
    assert torch.equal(c.view.cpu(), GM.to_c(ref, F32))
    assert c.outside_untouched()


def _phase_weights(kn, w):
    """w [cin_t][cout_t][4][4] of a transposed conv -> the four packed 2x2 sub-pixel weights [cout_t][2*2*cin_t]."""
    out = []
    for ph in range(2):
        for pw in range(2):
            sub = w[:, :, kn.phase_taps(ph)][:, :, :, kn.phase_taps(pw)]
            out.append(sub.permute(1, 2, 3, 0).reshape(w.shape[1], -1))
    return out


@pytest.mark.parametrize("writer", WRITERS, ids=[w[0] for w in WRITERS])
@pytest.mark.parametrize("which", ["convT_fwd_phases", "conv_dgrad_phases"])
def test_epilogue_row_remap(monkeypatch, writer, which):
    """The stride-2 sub-pixel row remap (four launches interleave into one output) with a residual read at the
    remapped row (and a bias for the forward), against F.conv_transpose2d / torch.nn.grad.conv2d_input in float64 on
    the same integers (3 x 6 x 7 -> 12 x 14, 48 -> 40 channels; 2 x 5 x 4 -> 10 x 8, 80 -> 24 channels)."""
    kn, _ = _k()
    _, req, hint, var = writer
    # (x is the input of the transposed conv, or dy of a k4 s2 p1 conv whose input gradient is wanted: the same
    # function, so the two wrappers get different geometry) 4 ci = 192 / 320: 3 / 5 k-tiles, three real slices
    B, H, W, ci, co = (3, 6, 7, 48, 40) if which == "convT_fwd_phases" else (2, 5, 4, 80, 24)
    GM.assert_exact_k(16 * ci)
    assert GM.launched_slices(3, 4 * ci) == 3
    x = GM.ints((B, ci, H, W), 41).double()
    resid = GM.ints((B * 2 * H * 2 * W, co), 43)
    bias = _ivec(co, 44, F32)
    w = GM.ints((ci, co, 4, 4), 42).double()
    if which == "convT_fwd_phases":
        ref = F.conv_transpose2d(x, w, stride=2, padding=1) + bias.double()[None, :, None, None]
    else:
        ref = torch.nn.grad.conv2d_input((B, co, 2 * H, 2 * W), w, x, stride=2, padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, co) + resid.double()
    xg = GM.place(x.permute(0, 2, 3, 1).reshape(-1, ci), ci + 8, DEV)
    wph = [GM.place(p, 4 * ci, DEV) for p in _phase_weights(kn, w)]
    rg = GM.place(resid, co + 8, DEV)
    c = GM.Guarded(B * 4 * H * W, co, co + 8, BF, DEV)
    GM.force(monkeypatch, kn, hint, req)
    if which == "convT_fwd_phases":
        bg = GM.place(bias[None], co + 8, DEV, dtype=F32, tail=1)
        kn.convT_fwd_phases(xg.view, B, H, W, ci, ci + 8, [p.view for p in wph], co, c.view, co + 8, bias=bg.view[0],
                            resid=rg.view, ldr=co + 8)
    else:
        kn.conv_dgrad_phases(xg.view, B, 2 * H, 2 * W, ci, ci + 8, [p.view for p in wph], co, c.view, co + 8,
                             resid=rg.view, ldr=co + 8)
    assert len(kn.GEMM_LOG) == 4
    for i in range(4):
        GM.check_log(kn, var, _tile(var, co), hint, f"{writer[0]} {which} phase {i}", entry=i)
    torch.cuda.synchronize()
    assert torch.equal(c.view.cpu(), GM.to_c(ref, BF)), f"{writer[0]} {which}"
    assert c.outside_untouched()


@pytest.mark.parametrize("writer", WRITERS, ids=[w[0] for w in WRITERS])
def test_epilogue_silu_random_values(monkeypatch, writer):
    kn, L = _k()
    _, req, hint, var = writer
    GM.force(monkeypatch, kn, hint, req)
    A0, B0 = GM.rand_operands()
    c = GM.run_linear(kn, L, GM.A_ROW, GM.B_NK, M, N, KD, A0[:M, :KD], B0[:KD, :N], F32, DEV, act=1)
    GM.check_log(kn, var, _tile(var, N), hint, writer[0])
    ref, bound = GM.rand_ref(M, N, KD)
    res = F.silu(ref)
    lim = 1.1 * bound + 2.0 ** -23 * res.abs()
    torch.cuda.synchronize()
    err = (c.view.cpu().double() - res).abs()
    assert bool((err <= lim).all()), f"worst error / bound {(err / lim.clamp_min(1e-300)).max().item():.3f}"
    assert c.outside_untouched()


def _relerr(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


# GroupNorm-statistics epilogue: requested variant -> (expected variant, tile_n for C = 96, tile_n for C = 64)
GN_VARIANTS = {1: (0, 128, 128), 2: (2, 128, 64), 5: (5, 128, 128), 7: (7, 64, 64), 9: (9, 128, 128), 11: (11, 128, 128)}


@pytest.mark.parametrize("hint", [1, 3], ids=["unsplit", "splits3"])
@pytest.mark.parametrize("req", sorted(GN_VARIANTS))
@pytest.mark.parametrize("B,P,C", [(3, 16, 96), (2, 64, 64)])
def test_epilogue_groupnorm_statistics(monkeypatch, B, P, C, req, hint):
    """gn= on every variant the tuned table sends it to: dy bitwise the same launch without gn; dx / dgamma / dbeta of
    the streaming backward against the self-contained gn_bwd, under the tolerances
    test_groupnorm_bwd_from_gemm_statistics uses for that comparison (2e-3 / 1e-4)."""
    kn, _ = _k()
    var, t96, t64 = GN_VARIANTS[req]
    GM.force(monkeypatch, kn, hint, req)
    g = torch.Generator().manual_seed(B * P + C)
    Mr, G, kd = B * P, 32, KD  # 5 k-tiles: the split case runs three slices
    x = (torch.randn(Mr, C, generator=g) * 2 + 0.5).to(BF).to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.1 + 1).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV)
    g_up = torch.randn(Mr, kd, generator=g).to(BF).to(DEV)
    wt = (torch.randn(C, kd, generator=g) * 0.05).to(BF).to(DEV)
    add = torch.randn(Mr, C, generator=g).to(BF).to(DEV)
    for silu in (False, True):
        y = torch.empty_like(x)
        tab = kn.gn_fwd(x, B, P, C, G, gamma, beta, silu, y)
        dy_ref = torch.full((Mr, C), float("nan"), dtype=BF, device=DEV)
        dy = torch.full((Mr, C), float("nan"), dtype=BF, device=DEV)
        kn.linear_dgrad_t(g_up, wt, dy_ref)
        req_gn = kn.gn_request(x, tab, P, C, silu)
        assert req_gn is not None
        kn.linear_dgrad_t(g_up, wt, dy, gn=req_gn)
        for _ in range(2):
            GM.check_log(kn, var, t96 if C == 96 else t64, hint, f"gn req={req}")
            kn.GEMM_LOG.pop()
        torch.cuda.synchronize()
        assert torch.equal(dy, dy_ref), "dy changed by the statistics epilogue"
        dx_ref, dx = torch.empty_like(x), torch.empty_like(x)
        dg_ref, db_ref, dg, db = (torch.empty(C, device=DEV) for _ in range(4))
        kn.gn_bwd(x, dy_ref, dx_ref, tab, gamma, B, P, C, G, silu, dg_ref, db_ref, addend=add)
        kn.gn_bwd(x, dy, dx, tab, gamma, B, P, C, G, silu, dg, db, addend=add, gn=req_gn)
        torch.cuda.synchronize()
        assert _relerr(dx, dx_ref) < 2e-3, _relerr(dx, dx_ref)
        assert _relerr(dg, dg_ref) < 1e-4 and _relerr(db, db_ref) < 1e-4, (_relerr(dg, dg_ref), _relerr(db, db_ref))
