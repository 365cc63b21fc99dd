"""Every mainloop x operand mode x column tile x split of sdmi_gemm (tests/gemm_matrix.py ROWS), exact.

Integer operands in [-3, 3] with K * 9 < 2^24: an fp32 C must torch.equal the int64 matmul of the CPU, a bf16 C its
round-to-nearest-even; one random-valued launch per instantiation is held to the elementwise fp32 dot-product bound
2 K 2^-24 (|A| @ |B|) (+ 2^-8 |ref| for a bf16 C). No other tolerance appears in this file. After every launch the
library's own log must name the row's (variant, tile_n, splits) -- a silent fallback fails here, and so does a run with
SDMI_GEMM_VARIANT set -- and everything outside the output window must be bitwise untouched."""
import pytest
import torch

from tests import gemm_matrix as GM

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


def _k():
    from sdmi import kernels, _lib
    return kernels, _lib


def _m_for(row):
    tbm = GM.GEOM[row.var][0]
    return 2 * tbm - 8 if row.a == GM.A_COL else 2 * tbm - 3


def _check_c(c, ref, c_dtype, tag):
    torch.cuda.synchronize()
    assert torch.equal(c.view.cpu(), GM.to_c(ref, c_dtype)), f"{tag}: C differs from the exact reference"
    assert c.outside_untouched(), f"{tag}: memory outside the C window changed"


def _check_rand(c, ref, bound, c_dtype, tag):
    torch.cuda.synchronize()
    err = (c.view.cpu().double() - ref).abs()
    lim = GM.rand_bound(ref, bound, c_dtype)
    assert bool((err <= lim).all()), f"{tag}: worst error / bound {(err / lim.clamp_min(1e-300)).max().item():.3f}"
    assert c.outside_untouched(), f"{tag}: memory outside the C window changed"


def _reduction_outputs(red, m, k, group):
    """sum_out / sum_out2 / gsum guarded outputs of a col-major-A launch (None where the row has no reductions)."""
    if not red:
        return {}, None
    so, so2 = GM.Guarded(1, m, m, F32, DEV), GM.Guarded(1, m, m, F32, DEV)
    kw = dict(sum_out=so.view[0], sum_out2=so2.view[0])
    gs = None
    if red != "sum":
        gs = GM.Guarded((k + group - 1) // group, m, m + 16, BF, DEV)
        kw.update(gsum=gs.view, sum_group=group)
    return kw, (so, so2, gs)


def _check_reductions(outs, A, group, tag):
    """A [m][k] integers: sum_out exact, the bf16 gsum the RNE of the exact group sums."""
    so, so2, gs = outs
    ref = A.sum(1)
    assert torch.equal(so.view[0].cpu(), ref.float()) and torch.equal(so2.view[0].cpu(), ref.float()), f"{tag}: sum_out"
    assert so.outside_untouched() and so2.outside_untouched(), f"{tag}: memory outside sum_out changed"
    if gs is not None:
        k = A.shape[1]
        pad = torch.zeros(A.shape[0], (k + group - 1) // group * group, dtype=A.dtype)
        pad[:, :k] = A
        gref = pad.view(A.shape[0], -1, group).sum(2).t()
        assert torch.equal(gs.view.cpu(), GM.to_c(gref, BF)), f"{tag}: gsum"
        assert gs.outside_untouched(), f"{tag}: memory outside gsum changed"


LINEAR_ROWS = [r for r in GM.ROWS if r.a != GM.A_CONV and r.b != GM.B_KNCONV]


@pytest.mark.parametrize("row", LINEAR_ROWS, ids=GM.row_id)
def test_linear_modes_exact(monkeypatch, row):
    """a0b0, a0b1 and a2b1 rows: every N of the row x K in {below one stage, one ring trip, wrap + ragged tail, long}
    x splits in {1, 3}; the other C dtype and the scalar-store stride ldc = N + 3 at the wrap K; reduction rows also
    check sum_out / sum_out2 / gsum."""
    kn, L = _k()
    m = _m_for(row)
    red = row.extras.get("red")
    group = {"gsum_odd": 50, "gsum_many": 8}.get(red, 64)  # 64: at most 17 groups at the longest K of these rows
    dflt = F32 if row.a == GM.A_COL else BF
    A0, B0 = GM.int_operands()
    ks = GM.ks_for(row.var) + ([GM.K_MAX] if row.extras.get("kmax") else [])
    if red == "gsum_many":
        ks = [GM.K_LONG]  # 129 groups
    for n in row.extras["N"]:
        for k in ks:
            if k == GM.K_MAX and n != row.extras["N"][0]:
                continue
            GM.assert_exact_k(k)
            A, B, ref = A0[:m, :k], B0[:k, :n], GM.int_ref(m, n, k)
            for hint in GM.SPLIT_HINTS:
                GM.force(monkeypatch, kn, hint, row.req)
                sp = GM.logged_splits(hint, k)
                variants = [(dflt, None)]
                if k == GM.wrap_k(row.var):
                    variants += [(BF if dflt == F32 else F32, None), (dflt, n + 3)]
                for c_dtype, ldc in variants:
                    tag = f"{GM.row_id(row)} M={m} N={n} K={k} splits_hint={hint} {c_dtype} ldc={ldc}"
                    kw, outs = _reduction_outputs(red, m, k, group)
                    c = GM.run_linear(kn, L, row.a, row.b, m, n, k, A, B, c_dtype, DEV, ldc=ldc, **kw)
                    GM.check_log(kn, row.var, row.tile_n, sp, tag)
                    _check_c(c, ref, c_dtype, tag)
                    if outs:
                        _check_reductions(outs, A, group, tag)


@pytest.mark.parametrize("row", [r for r in LINEAR_ROWS if "red" not in r.extras], ids=GM.row_id)
def test_linear_modes_random_values(monkeypatch, row):
    """randn operands rounded to bf16 against the float64 product, elementwise bound, unsplit and split."""
    kn, L = _k()
    m, n, k = _m_for(row), row.extras["N"][0], GM.wrap_k(row.var)
    A0, B0 = GM.rand_operands()
    ref, bound = GM.rand_ref(m, n, k)
    for hint in GM.SPLIT_HINTS:
        GM.force(monkeypatch, kn, hint, row.req)
        for c_dtype in (BF, F32):
            tag = f"{GM.row_id(row)} M={m} N={n} K={k} splits_hint={hint} {c_dtype} randn"
            c = GM.run_linear(kn, L, row.a, row.b, m, n, k, A0[:m, :k], B0[:k, :n], c_dtype, DEV)
            GM.check_log(kn, row.var, row.tile_n, GM.logged_splits(hint, k), tag)
            _check_rand(c, ref, bound, c_dtype, tag)


def _run_conv(kn, case, n, c_dtype, ldo=None):
    """conv_fwd of an implicit-conv A case on guarded x (ldx = cin + 8), weights (ldw = K + 8) and output."""
    q = case["q"]
    cin, cin2 = q["cin"], q.get("cin2", 0)
    xg = GM.place(case["x"], cin + 8, DEV)
    x2g = GM.place(case["x2"], cin2 + 8, DEV) if cin2 else None
    wg = GM.place(case["wpk"][:n], case["K"] + 8, DEV)
    m = case["ref"].shape[0]
    ldo = ldo or n + 8
    c = GM.Guarded(m, n, ldo, c_dtype, DEV)
    kn.conv_fwd(xg.view, q["B"], q["H"], q["W"], cin, cin + 8, wg.view, n, q["k"], q["k"], q["s"], q["p"], c.view, ldo,
                x2=x2g.view if cin2 else None, cin2=cin2, ldw=case["K"] + 8)
    c.keep = (xg, x2g, wg)
    return c


CONV_ROWS = GM.rows(GM.A_CONV, GM.B_NK)


@pytest.mark.parametrize("row", CONV_ROWS, ids=GM.row_id)
def test_conv_a_exact(monkeypatch, row):
    """a1b0 rows: every conv case of the row (3x3 with cin 8 / 64 / 128, 4x4 s2, 1x1, 2x2 s1 / s2, the K-concatenated
    second source) x N x splits {1, 3}, against F.conv2d in float64 on the same integers; one random-valued launch per
    row under the elementwise bound."""
    kn, _ = _k()
    for name in row.extras["convs"]:
        case = GM.conv_case(name)
        for n in row.extras["N"]:
            for hint in GM.SPLIT_HINTS:
                GM.force(monkeypatch, kn, hint, row.req)
                for c_dtype, ldo in ((BF, None), (F32, n + 3)) if n == row.extras["N"][0] else ((BF, None),):
                    tag = f"{GM.row_id(row)} {name} N={n} K={case['K']} splits_hint={hint} {c_dtype} ldo={ldo}"
                    c = _run_conv(kn, case, n, c_dtype, ldo)
                    GM.check_log(kn, row.var, row.tile_n, GM.logged_splits(hint, case["K"]), tag)
                    _check_c(c, case["ref"][:, :n], c_dtype, tag)
    name, n = row.extras["convs"][-1], row.extras["N"][0]
    case = GM.conv_case(name, True)
    for hint in GM.SPLIT_HINTS:
        GM.force(monkeypatch, kn, hint, row.req)
        tag = f"{GM.row_id(row)} {name} N={n} splits_hint={hint} randn"
        c = _run_conv(kn, case, n, BF)
        GM.check_log(kn, row.var, row.tile_n, GM.logged_splits(hint, case["K"]), tag)
        _check_rand(c, case["ref"][:, :n], case["bound"][:, :n], BF, tag)


WCONV_ROWS = GM.rows(GM.A_COL, GM.B_KNCONV)


@pytest.mark.parametrize("row", WCONV_ROWS, ids=GM.row_id)
def test_conv_b_exact(monkeypatch, row):
    """a2b2 rows (conv weight gradients): every grid of the row x column permute {none, torch layout, tap-major} x
    splits {1, 3} against torch.nn.grad.conv2d_weight in float64; reduction rows check sum_out / gsum (one group per
    sample) as well; one random-valued launch per plain row under the elementwise bound."""
    kn, L = _k()
    red = row.extras.get("red")
    for name in row.extras["convs"]:
        m = 120 if name == "k3c128" else _m_for(row)
        case = GM.wconv_case(name, m)
        q, k = case["q"], case["K"]
        cin, taps = q["cin"], q["k"] * q["k"]
        n = taps * cin
        group = case["oh"] * case["ow"]
        geom = kn.conv_geom(q["H"], q["W"], cin, cin + 8, q["k"], q["k"], case["oh"], case["ow"], q["s"], q["s"],
                            -q["p"], -q["p"])
        for perm in ((0,) if red else GM.PERMS):
            ref = GM.permuted(case["ref"], perm, cin)
            for hint in GM.SPLIT_HINTS:
                GM.force(monkeypatch, kn, hint, row.req)
                tag = f"{GM.row_id(row)} {name} M={m} N={n} K={k} perm={perm} splits_hint={hint}"
                dyg, xg = GM.place(case["dy"], m + 8, DEV), GM.place(case["x"], cin + 8, DEV)
                kw, outs = _reduction_outputs(red, m, k, group)
                c = GM.Guarded(m, n, n + 8, F32, DEV)
                kn.gemm(m, n, k, dyg.view, L.A_COLMAJOR, m + 8, xg.view, L.B_KN_CONV, 0, c.view, n + 8, geom=geom,
                        perm=(cin, taps, cin, perm) if perm else None, **kw)
                GM.check_log(kn, row.var, row.tile_n, GM.logged_splits(hint, k), tag)
                _check_c(c, ref, F32, tag)
                if outs:
                    _check_reductions(outs, case["dy"].t().long(), group, tag)
    if red:
        return
    name = row.extras["convs"][-1]
    m = 120 if name == "k3c128" else _m_for(row)
    case = GM.wconv_case(name, m, True)
    q, k = case["q"], case["K"]
    cin, n = q["cin"], q["k"] * q["k"] * q["cin"]
    geom = kn.conv_geom(q["H"], q["W"], cin, cin + 8, q["k"], q["k"], case["oh"], case["ow"], q["s"], q["s"], -q["p"], -q["p"])
    for hint in GM.SPLIT_HINTS:
        GM.force(monkeypatch, kn, hint, row.req)
        tag = f"{GM.row_id(row)} {name} splits_hint={hint} randn"
        dyg, xg = GM.place(case["dy"], m + 8, DEV), GM.place(case["x"], cin + 8, DEV)
        c = GM.Guarded(m, n, n + 8, F32, DEV)
        kn.gemm(m, n, k, dyg.view, L.A_COLMAJOR, m + 8, xg.view, L.B_KN_CONV, 0, c.view, n + 8, geom=geom)
        GM.check_log(kn, row.var, row.tile_n, GM.logged_splits(hint, k), tag)
        _check_rand(c, case["ref"].reshape(m, -1), case["bound"].reshape(m, -1), F32, tag)


@pytest.mark.parametrize("mode", ["a0b0", "a1b0"])
def test_variant2_tile192_by_request(monkeypatch, mode):
    """Variant 2 takes its 128 x 192 tile by occupancy only beyond M = 21760; below that it runs on the descriptor's
    tile_n_hint = 192, which the Python wrapper never sets. So the wrapper's own descriptor (GEMM_CAPTURE) of an
    N = 384 launch is launched again with that hint through the C ABI, under the same exact checks."""
    import ctypes
    kn, L = _k()
    lib = L.lib()
    A0, B0 = GM.int_operands()
    m, n = 253, 384
    for k in (GM.ks_for(2) if mode == "a0b0" else [576]):
        for hint in GM.SPLIT_HINTS:
            GM.force(monkeypatch, kn, hint, 2)
            monkeypatch.setattr(kn, "GEMM_CAPTURE", [])
            if mode == "a0b0":
                c0 = GM.run_linear(kn, L, GM.A_ROW, GM.B_NK, m, n, k, A0[:m, :k], B0[:k, :n], BF, DEV)
                ref = GM.int_ref(m, n, k)
            else:
                case = GM.conv_case("3x3c64")
                c0 = _run_conv(kn, case, n, BF)
                ref = case["ref"][:, :n]
            tag = f"{mode} tile 192 N={n} K={k} splits_hint={hint}"
            GM.check_log(kn, 2, 128, GM.logged_splits(hint, k), tag)
            d = kn.GEMM_CAPTURE[-1]
            c = GM.Guarded(ref.shape[0], n, n + 8, BF, DEV)
            d.c, d.tile_n_hint = c.view.data_ptr(), 192
            var, tn, sp, wsb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
            L.check(lib.sdmi_gemm_kernel_info(ctypes.byref(d), ctypes.byref(var), ctypes.byref(tn)), "kernel_info")
            L.check(lib.sdmi_gemm_plan(ctypes.byref(d), ctypes.byref(sp), ctypes.byref(wsb)), "plan")
            assert (var.value, tn.value, sp.value) == (2, 192, GM.logged_splits(hint, k)), tag
            ws = torch.full((max(1, wsb.value // 4),), float("nan"), device=DEV)
            L.check(lib.sdmi_gemm(ctypes.byref(d), ws.data_ptr() if wsb.value else None, wsb.value, kn._stream()), "gemm")
            GM.RAN.add((d.a_mode, d.b_mode, 2, 192, sp.value > 1))
            _check_c(c, ref, BF, tag)
            del c0


def test_zz_instantiations_launched(request):
    """Reports how many distinct (mode, variant, tile_n, split) instantiations this process launched. When the whole
    file was selected (every other test of it is in the session), every row of the matrix and the instantiations the
    matrix exists for must have launched -- a row that silently stops launching fails here."""
    ran = GM.RAN
    print(f"\ndistinct (a_mode, b_mode, variant, tile_n, split) instantiations launched: {len(ran)}")
    mine = [i for i in request.session.items if i.module is request.module]
    whole_file = len(mine) == 2 * len(LINEAR_ROWS) - sum("red" in r.extras for r in LINEAR_ROWS) + len(CONV_ROWS) + \
        len(WCONV_ROWS) + 2 + 1
    if not whole_file:
        return
    assert {(r.a, r.b, r.var, r.tile_n) for r in GM.ROWS} | {(0, 0, 2, 192), (1, 0, 2, 192)} <= {x[:4] for x in ran}
    need = {(a, 0, v) for a in (0, 1) for v in (4, 7, 8, 9, 10)} | {(a, b, v) for a, b in ((0, 0), (0, 1), (1, 0))
                                                                   for v in (3, 5, 6)}
    assert need <= {(a, b, v) for a, b, v, _, _ in ran}
    assert {(0, 0, 4, 256), (0, 0, 4, 384), (1, 0, 4, 256), (1, 0, 4, 384)} <= {x[:4] for x in ran}
