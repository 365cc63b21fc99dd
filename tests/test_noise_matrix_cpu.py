"""The latent-noise test matrix cannot fall behind the kernels, its exact data is exact and its statements have teeth
(CPU only, no library call).

Each row of tests/noise_matrix.py ROWS launches what the restated host rules of csrc/latent_noise.hip give and stays
inside the launch budget; no row can be removed without a coverage check failing; every plant puts its extremes
where it says, with tie counts that are powers of two in the exact family; the exact family's S is exact in both
summation orders; the fp32 emulations of the soft family stay within K_S / 2 of the bound, K_S is at most 3 times the
largest emulated ratio, and each perturbed reference leaves its bitwise statement. The closed-form gradient -- tie
rule included -- equals torch autograd's on every planted case."""
import functools

import numpy as np
import pytest
import torch

from tests import noise_matrix as NM
from tests import vq_matrix as VM


def test_rows_follow_the_restated_rules():
    assert len({NM.row_id(r) for r in NM.ROWS}) == len(NM.ROWS)
    for r in NM.ROWS:
        assert list(r.launches) == NM.expected_launches(r.entry, r.dims, r.opt), NM.row_id(r)
        if r.entry == NM.RANGE:
            assert 4 * 4 * r.launches[0][1] == NM.workspace(r.dims[0])
            continue
        B, C, HW = r.dims
        assert 1 <= C <= NM.MAXC
        if r.entry == NM.FWD and NM.opt(r, "zin"):
            assert NM.opt(r, "ld") >= NM.opt(r, "cout") >= 1
        if r.entry == NM.BWD:
            assert NM.opt(r, "dzin") or NM.opt(r, "add")
            assert 4 * r.launches[0][1] <= NM.workspace(B * C * HW), "the S partials do not fit the workspace"


def test_the_bound_entry_points_and_their_host_side():
    """The bindings take what the problems of noise_matrix.py pass, and the host side of the library (loaded without
    a GPU: no launch happens here) sizes the workspace by the restated rule and rejects before it would launch."""
    import ctypes
    import os
    assert NM.ARITY == dict(sdmi_latent_noise_workspace=1, sdmi_latent_range=4, sdmi_latent_noise_fwd=14,
                            sdmi_latent_noise_bwd=14)
    from sdmi import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsdmi.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    for n in sorted({NM.numel(r) for r in NM.ROWS} | {1024, 262144, 262145, 10 ** 7}):
        assert L.sdmi_latent_noise_workspace(n) == NM.workspace(n), n
    assert L.sdmi_latent_noise_workspace(0) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sdmi_latent_range(None, 8, p, None) == -1 and L.sdmi_latent_range(p, 0, p, None) == -1
    assert L.sdmi_latent_noise_fwd(p, p, 1, 9, 8, 0.5, p, p, None, None, 0, None, 0, None) == -1
    assert L.sdmi_latent_noise_fwd(p, p, 1, 4, 2, 0.5, p, p, None, None, 4, p, 8, None) == -1      # zin without w_post
    assert L.sdmi_latent_noise_bwd(None, 0, None, None, p, p, 1, 4, 2, 0.5, p, p, p, None) == -1   # neither gradient
    # n_scale == 0 returns 0 before anything is launched or read
    assert L.sdmi_latent_noise_fwd(p, None, 1, 4, 2, 0.0, p, p, None, None, 0, None, 0, None) == 0
    assert L.sdmi_latent_noise_bwd(None, 0, None, p, None, p, 1, 4, 2, 0.0, p, p, p, None) == 0
    assert buf[0] == 0.0


def test_the_launch_budget():
    """Forward at n_scale != 0: the randn launch plus at most 2 (range + fwd); backward at most 2."""
    for r in NM.ROWS:
        assert len(r.launches) == {NM.RANGE: 1, NM.FWD: 1, NM.BWD: 2}[r.entry], NM.row_id(r)


def test_the_restated_rules_at_known_points():
    assert [NM.flat_blocks(n) for n in (1, 1024, 1025, 262144, 262145, 10 ** 7)] == [1, 1, 2, 256, 256, 256]
    assert [NM.pixel_blocks(p) for p in (1, 256, 257, 65536, 65537)] == [1, 1, 2, 256, 256]
    assert NM.workspace(1) == 16 and NM.workspace(32768) == 512 and NM.workspace(10 ** 6) == 4096
    # the vqvae-train shape: B = 8, C = 4, 32 x 32 latents
    assert NM.expected_launches(NM.FWD, (8, 4, 1024), (("zin", 1),)) == [("latent_noise_fwd_kernelILb1EE", 32)]
    assert NM.expected_launches(NM.BWD, (8, 4, 1024)) == [("latent_noise_dot_kernel", 32),
                                                          ("latent_noise_bwd_kernel", 32)]
    assert NM.block_of(3000).tolist()[1023:1025] == [0, 1] and int(NM.block_of(262149)[-1]) == 0
    for n in (1, 300, 1025, 4116, 262148):          # the S partials of the C = 1 case fit the shared workspace size
        assert 4 * NM.pixel_blocks(n) <= NM.workspace(n)


# ----------------------------------------------------------------------------------------------------------------
# coverage
# ----------------------------------------------------------------------------------------------------------------
def _need(found, what):
    assert found, f"ROWS has no row for: {what}"


def check_range_coverage():
    rows = NM.rows_of(NM.RANGE)
    _need([r for r in rows if r.dims[0] == 1], "range: n = 1")
    _need([r for r in rows if r.dims[0] == 5], "range: n = 5")
    _need([r for r in rows if r.dims[0] == NM.SPAN - 1], "range: one short of a workgroup's span")
    _need([r for r in rows if r.dims[0] == NM.SPAN + 1], "range: one past a workgroup's span")
    _need([r for r in rows if 2 < r.launches[0][1] < NM.CAP and r.dims[0] % NM.SPAN], "range: several workgroups, ragged")
    _need([r for r in rows if r.dims[0] > NM.CAP * NM.SPAN], "range: the partial cap and a second trip")


def check_fwd_coverage():
    rows = NM.rows_of(NM.FWD)
    _need([r for r in rows if NM.numel(r) == 1], "forward: n = 1")
    _need([r for r in rows if NM.numel(r) == 5], "forward: n = 5")
    for C in (1, 4, 8):
        _need([r for r in rows if r.dims[1] == C and NM.opt(r, "zin") and NM.opt(r, "ld") == 8 and
               NM.opt(r, "cout") == C], f"forward: C = {C} with ld = 8 for the fused pointwise")
    _need([r for r in rows if NM.pixels(r) == NM.NT - 1], "forward: one pixel short of a workgroup")
    _need([r for r in rows if NM.pixels(r) == NM.NT + 1], "forward: one pixel past a workgroup")
    _need([r for r in rows if NM.opt(r, "zin") and not NM.opt(r, "bias")], "forward: no bias")
    _need([r for r in rows if r.dims[0] > 1 and r.dims[2] % NM.NT and NM.opt(r, "zin")],
          "forward: a workgroup that straddles images, with the pointwise")
    _need([r for r in rows if NM.opt(r, "zin") and NM.opt(r, "ld") > 8 and NM.opt(r, "cout") != r.dims[1]],
          "forward: cout != C and pad columns past the eighth")
    _need([r for r in rows if not NM.opt(r, "zin") and r.dims[1] == 1 and NM.flat_blocks(NM.numel(r)) == 2],
          "forward: a flat tensor with two range partials")
    _need([r for r in rows if not NM.opt(r, "zin") and r.dims[1] > 1 and r.dims[0] > 2],
          "forward: several images and channels without the pointwise")
    _need([r for r in rows if NM.pixels(r) > NM.CAP * NM.NT and NM.numel(r) > NM.CAP * NM.SPAN], "forward: both caps")


def check_bwd_coverage():
    rows = NM.rows_of(NM.BWD)
    _need([r for r in rows if NM.numel(r) == 1], "backward: n = 1")
    _need([r for r in rows if NM.numel(r) == 5], "backward: n = 5")
    _need([r for r in rows if not NM.opt(r, "add")], "backward: dz_add absent")
    _need([r for r in rows if not NM.opt(r, "dzin") and NM.flat_blocks(NM.numel(r)) == 2],
          "backward: dzin absent, two range partials")
    for C in (1, 4, 8):
        _need([r for r in rows if r.dims[1] == C and NM.opt(r, "dzin")], f"backward: C = {C} with dzin")
    _need([r for r in rows if NM.pixels(r) == NM.NT - 1], "backward: one pixel short of a workgroup")
    _need([r for r in rows if NM.opt(r, "dzin") and NM.opt(r, "ld") > 8], "backward: a wide dzin")
    _need([r for r in rows if r.dims[0] > 2 and r.dims[1] > 1 and r.launches[0][1] == r.launches[1][1] > 1],
          "backward: several images, as many pixel as flat workgroups")
    _need([r for r in rows if NM.pixels(r) > NM.CAP * NM.NT and NM.numel(r) > NM.CAP * NM.SPAN], "backward: both caps")


COVERAGE = (check_range_coverage, check_fwd_coverage, check_bwd_coverage)


@pytest.mark.parametrize("check", COVERAGE, ids=lambda f: f.__name__)
def test_coverage(check):
    check()


def _noticed():
    for check in COVERAGE:
        try:
            check()
        except AssertionError:
            return True
    return False


def test_no_row_can_be_removed(monkeypatch):
    full = list(NM.ROWS)
    assert not _noticed()
    for r in full:
        monkeypatch.setattr(NM, "ROWS", [x for x in full if x is not r])
        assert _noticed(), f"ROWS without {NM.row_id(r)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# the plants
# ----------------------------------------------------------------------------------------------------------------
_SIZES = sorted({NM.numel(r) for r in NM.ROWS})


def _is_pow2(v):
    return v >= 1 and v & (v - 1) == 0


@pytest.mark.parametrize("n", _SIZES)
def test_plants(n):
    for plant in NM.PLANTS:
        z = NM.z_case("exact", n, plant)
        assert z.numel() == n
        mn, mx, cmn, cmx = NM.range_reference(z)
        val, cnt = NM.partials(z)
        if plant == "nan":
            assert mn != mn and mx != mx and (cmn, cmx) == (0, 0)
            assert int(torch.isnan(z).sum()) == 1 and int(torch.isnan(val[:, 0]).sum()) == 1
            assert bool(torch.isnan(NM.out_reference(z, torch.ones(n, dtype=torch.float64), NM.EXACT_SCALE)).all())
            continue
        assert bool((z % 1 == 0).all()) and float(z.abs().max()) <= 4
        assert _is_pow2(cmn) and _is_pow2(cmx) or plant in ("equal", "zeros"), (plant, cmn, cmx)
        # the partials merge to the whole tensor's range, counts included
        assert float(val[:, 0].min()) == mn and float(val[:, 1].max()) == mx
        assert int(cnt[:, 0][val[:, 0] == mn].sum()) == cmn and int(cnt[:, 1][val[:, 1] == mx].sum()) == cmx
        if plant in ("equal", "zeros"):
            assert (cmn, cmx) == (n, n) and mx - mn == 0
            eps = NM.eps_case("exact", n, torch.Generator().manual_seed(n))
            out = NM.out_reference(z, eps, NM.EXACT_SCALE)
            assert torch.equal(out, z)
            if plant == "equal":
                assert torch.equal(NM.bits(out.float()), NM.bits(z.float())), "all-equal: out is not z bitwise"
            else:
                assert len(set(NM.bits(z.float()).tolist())) == (2 if n > 1 else 1), "one sign of zero only"
            continue
        top, low = NM.plant_positions(n, plant)
        if n > 1:
            assert sorted(top) == (z == 4).nonzero().reshape(-1).tolist() and not set(top) & set(low)
            assert sorted(low) == (z == -4).nonzero().reshape(-1).tolist()
        if plant == "first":
            assert top == [0] and low == [n - 1]
        if plant == "seam" and n > NM.SPAN + 1:
            blk = NM.block_of(n)
            assert int(blk[top[0]]) != int(blk[top[1]]), "the two maxima are not on a workgroup seam"
        if plant == "spread" and n >= 2 * NM.SPAN:
            assert len(set(NM.block_of(n)[top].tolist())) >= min(NM.flat_blocks(n), len(top)) // 2 + 1
    for plant in NM.SOFT_PLANTS:
        z = NM.z_case("soft", n, plant)
        _, _, cmn, cmx = NM.range_reference(z)
        assert (cmn, cmx) == ((5, 3) if plant == "ties" and n >= 16 else (1, 1)) or n == 1


def test_opposite_signed_zeros():
    z = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=torch.float64)
    assert NM.range_reference(z) == (0.0, 0.0, 4, 4)
    assert float(NM.scale32(z, 0.2)) == 0.0


# ----------------------------------------------------------------------------------------------------------------
# the closed form against autograd
# ----------------------------------------------------------------------------------------------------------------
def _closed_form(z, g, eps, n_scale):
    """The gradient of sum(g * (z + (max - min) n_scale eps)) in float64: g plus the range term under the tie rule."""
    S = float((g * eps).sum())
    mn, mx = z.min(), z.max()
    at_max, at_min = z == mx, z == mn
    return g + n_scale * S * (at_max.double() / at_max.sum() - at_min.double() / at_min.sum())


def test_the_tie_rule_of_this_torch_build():
    x = torch.tensor([1.0, 3.0, 3.0, -2.0, -2.0, -2.0, 0.0], requires_grad=True)
    (x.max() - x.min()).backward()
    assert torch.allclose(x.grad, torch.tensor([0, .5, .5, -1 / 3, -1 / 3, -1 / 3, 0]), atol=1e-7)


@pytest.mark.parametrize("n", [n for n in _SIZES if n <= 5000])
def test_closed_form_gradient_matches_autograd(n):
    for kind, plants in (("exact", ("first", "seam", "spread", "equal")), ("soft", NM.SOFT_PLANTS)):
        for plant in plants:
            gen = torch.Generator().manual_seed(n)
            z0 = NM.z_case(kind, n, plant)
            eps, g = VM._rn(gen, n), VM._rn(gen, n)
            z = z0.clone().requires_grad_(True)
            out = z + (z.max() - z.min()) * 0.2 * eps
            (out * g).sum().backward()
            want = _closed_form(z0, g, eps, 0.2)
            assert torch.allclose(z.grad, want, rtol=1e-12, atol=1e-12), (n, kind, plant)
            # and the fp32 restatement the kernels are held to is that closed form, to fp32 accuracy
            c = dict(B=1, C=1, HW=n, add=g, dzin=None, w_post=None, eps=eps)
            terms, S64, T = NM.s_reference(c)
            r = NM.r_reference(c, z0, np.float32(S64), 0.2)
            tol = 1e-6 * (want.abs() + abs(0.2 * S64) + 0.2 * T * NM.U24 * 8)
            assert bool(((r - want).abs() <= tol).all()), (n, kind, plant)


# ----------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------
def _bcase(kind, r):
    return NM.bwd_case(kind, *r.dims, NM.opt(r, "dzin"), NM.opt(r, "add"))


@pytest.mark.parametrize("row", NM.rows_of(NM.BWD), ids=NM.row_id)
def test_exact_backward_family(row):
    c = _bcase("exact", row)
    for name in ("dzin", "add", "w_post"):
        if c[name] is not None:
            assert bool((c[name] % 1 == 0).all()) and float(c[name].abs().max()) <= 4
    assert bool(((4 * c["eps"]) % 1 == 0).all()) and float(c["eps"].abs().max()) <= 4
    assert NM.exact_margin(c) < 2 ** 24
    terms, S64, T = NM.s_reference(c)
    assert (4 * S64) % 1 == 0
    for order in NM.ORDERS:
        assert NM.emulate_S(terms, order) == S64, order
    assert float(np.float32(S64)) == S64
    n = NM.numel(row)
    for plant in NM.PLANTS:
        z = NM.z_case("exact", n, plant)
        ref = NM.r_reference(c, z, S64, NM.EXACT_SCALE)
        add = c["add"] if c["add"] is not None else torch.zeros(n, dtype=torch.float64)
        if plant in ("equal", "nan"):
            assert torch.equal(ref, add), f"{plant}: corr is not zero"
        if plant == "zeros":
            assert torch.equal(ref, add) and NM.range_reference(z)[2:] == (n, n)
        if plant in ("first", "seam", "spread") and S64 != 0 and n > 1:
            # the perturbed references leave the bitwise statement
            assert not torch.equal(NM.r_reference(c, z, S64, NM.EXACT_SCALE, count_off=1), ref), "tie count + 1"
            assert not torch.equal(NM.r_reference(c, z, S64, NM.EXACT_SCALE, flip_min=True), ref), "min sign"
        if plant == "equal" and S64 != 0:
            assert not torch.equal(NM.r_reference(c, z, S64, NM.EXACT_SCALE, both_is_max=True), ref), "doubly extremal"


@pytest.mark.parametrize("row", NM.rows_of(NM.FWD), ids=NM.row_id)
def test_exact_forward_family(row):
    B, C, HW = row.dims
    n = NM.numel(row)
    c = NM.fwd_case("exact", B, C, HW, NM.opt(row, "cout", 0), NM.opt(row, "bias", 0))
    for plant in ("first", "seam", "spread"):
        z = NM.z_case("exact", n, plant)
        out = NM.out_reference(z, c["eps"], NM.EXACT_SCALE)
        mn, mx, _, _ = NM.range_reference(z)
        assert torch.equal(out, z + (mx - mn) * NM.EXACT_SCALE * c["eps"]), "the exact forward is not exact"
        bumped = (out.float().view(torch.int32) + 1).view(torch.float32).double()
        assert not torch.equal(bumped, out), "1 ulp in out passes"
        if NM.opt(row, "zin"):
            zin = NM.zin_reference(c, out)
            o = VM.from_nchw(out, B, HW, C)
            want = o @ c["w"].T + (c["b"] if c["b"] is not None else 0.0)
            assert torch.equal(zin, NM.bf16(want)) and zin.shape == (B * HW, NM.opt(row, "cout"))


# ----------------------------------------------------------------------------------------------------------------
# the soft family: emulated ratios and K_S
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ratios(row):
    c = _bcase("soft", row)
    terms, S64, T = NM.s_reference(c)
    return {order: abs(NM.emulate_S(terms, order) - S64) / (NM.U24 * T) for order in NM.ORDERS}, S64, T


@pytest.mark.parametrize("row", NM.rows_of(NM.BWD), ids=NM.row_id)
def test_soft_backward_rows(row):
    m, S64, T = _ratios(row)
    print(f"{NM.row_id(row)}: emulated |S32 - S64| / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()))
    assert max(m.values()) <= NM.K_S / 2, m
    c = _bcase("soft", row)
    n = NM.numel(row)
    if n >= 16:
        for plant in NM.SOFT_PLANTS:
            z = NM.z_case("soft", n, plant)
            for ns in NM.SOFT_SCALES:
                ref = NM.r_reference(c, z, np.float32(S64), ns)
                assert not torch.equal(NM.r_reference(c, z, np.float32(S64), ns, count_off=1), ref)
                assert not torch.equal(NM.r_reference(c, z, np.float32(S64), ns, flip_min=True), ref)
    # a pixel dropped from the sum leaves the bound
    g = NM.g_reference(c)
    e = VM.from_nchw(c["eps"], *[c[k] for k in ("B", "HW", "C")])
    worst = (g * e).abs().sum(1).max()
    assert float(worst) > NM.sum_bound(T) or n < 16


def test_the_constant_is_twice_the_emulated_ratio():
    worst = {o: max(_ratios(r)[0][o] for r in NM.rows_of(NM.BWD)) for o in NM.ORDERS}
    print("largest emulated |S32 - S64| / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f"; K_S {NM.K_S}")
    top = max(worst.values())
    assert 2 * top <= NM.K_S <= 3 * top
    assert abs(worst["kernel"] - NM.MEASURED["kernel"]) < 5e-3 and abs(worst["pair"] - NM.MEASURED["pair"]) < 5e-3, \
        "the docstring's ratios are stale"


def test_sum_order_at_known_points():
    """The emulation at points worked out by hand."""
    big = 2.0 ** 24
    t = torch.zeros(600, 1)
    t[0, 0], t[1, 0], t[33, 0] = big, 1.0, 1.0            # lanes 0, 1 and 33 of wave 0: (1 + 33) meet before lane 0
    assert NM.emulate_S(t, "kernel") == big + 2
    t = torch.zeros(600, 1)
    t[0, 0], t[64, 0], t[300, 0] = big, 1.0, 1.0          # wave 0, wave 1 and the second workgroup, one by one
    assert NM.emulate_S(t, "kernel") == big
    t = torch.zeros(3, 2)
    t[0, 0], t[0, 1] = big, 1.0                           # one thread's channels in sequence
    assert NM.emulate_S(t, "kernel") == big
    part = torch.zeros(200)
    part[0], part[32], part[1] = big, 1.0, 1.0            # the last stage: lanes 0 and 32 meet first
    assert float(NM.last_stage(part)) == big
    part[32], part[3] = 0.0, 1.0                          # lanes 1 and 3 reach lane 0 as 2
    assert float(NM.last_stage(part)) == big + 2
