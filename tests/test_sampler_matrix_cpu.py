"""The sampler test matrix cannot fall behind the kernels, its references are the reference's arithmetic and its
noise bound has teeth (CPU only; the library is loaded only for the error returns, which come before any launch).

Each row of tests/sampler_matrix.py ROWS launches what the restated host rules give; no row can be removed without a
coverage check failing; the numpy.float32 models give the bits of the same expressions evaluated by torch on the CPU on
every row's data; every swept timestep holds elements whose unclamped x0 lies within 2 ulp of +1 and of -1 on both
sides; no DDIM pair in use has a NaN coefficient; the Philox model gives the published Random123 known answers; the
float32 emulation of the noise stays within its share of K_Z and every perturbed reference leaves the bound; the draws
follow from the integers with strict comparisons."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import sampler_matrix as SM

opt = SM.opt


def test_rows_follow_the_restated_rules():
    assert len({SM.row_id(r) for r in SM.ROWS}) == len(SM.ROWS)
    for r in SM.ROWS:
        assert list(r.launches) == SM.expected_launches(r.entry, r.dims, r.opt), SM.row_id(r)


def test_the_restated_rules_at_known_points():
    assert [SM.grid(n) for n in (1, 256, 257, 4096 * 256, 4096 * 256 + 1, 2 ** 40)] == [1, 1, 2, 4096, 4096, 4096]
    assert SM.grid(0) == 1 and SM.grid(8192 * 256 + 1, SM.ADDN_GRID_CAP) == 8192 and SM.grid(4096 * 256 + 1, 8192) == 4097
    assert SM.draw_items(5, 3, 4, 1) == 2 + 3 + 3 and SM.draw_items(5, 3, 4, 0) == 2 + 3
    assert SM.draw_items(SM.BIG4, 2, 8, 1) == 4096 * 256 + 1 + 4 + 2
    assert SM.expected_launches(SM.RANDN, (5,), (("adv", 1),)) == [(SM.K_RANDN, 1), (SM.K_ADV, 1)]
    assert SM.expected_launches(SM.DDPM, (257,), (("dec", 1),)) == [(SM.K_DDPM, 2), (SM.K_DEC, 1)]
    assert SM.draw_status(5, 3, 1000, 1, 1, 1, 4) == 0 and SM.draw_status(5, 3, 1000, 0, 0, 0, 0) == 0
    assert SM.draw_status(0, 3, 1000, 1, 1, 1, 4) == -1 and SM.draw_status(5, 3, 0, 1, 1, 1, 4) == -1
    assert SM.draw_status(5, 3, 1000, 1, 0, 1, 4) == -2 and SM.draw_status(5, 3, 1000, 1, 1, 1, 6) == -2
    assert SM.draw_status(5, 3, 1000, 1, 1, 1, 4, align=(0, 4, 0)) == -2
    assert SM.draw_status(5, 3, 1000, 1, 0, 1, 4, noise=0) == -1
    # the capped-grid rows reach the second turn of their loops
    assert SM.BIG > SM.GRID_CAP * SM.NT and SM.cdiv(SM.BIG4, 4) > SM.GRID_CAP * SM.NT


# ----------------------------------------------------------------------------------------------------------------
# coverage: every named branch has a row, and every row is the only one covering some named branch
# ----------------------------------------------------------------------------------------------------------------
def _is(r, entry, dims=None, **o):
    return r.entry == entry and (dims is None or r.dims == tuple(dims)) and dict(r.opt) == o


def _needs():
    need = []
    for tb in ("cond", "uncond", "syn"):
        need.append((f"ddpm at every t of {tb}", lambda r, tb=tb: _is(r, SM.DDPM, (67,), table=tb, sweep=1)))
    for tb in ("a", "b"):
        for eta in (0.0, 0.5, 1.0):
            need.append((f"ddim on every pair of {tb} at eta {eta}",
                         lambda r, tb=tb, eta=eta: _is(r, SM.DDIM, (67,), table=tb, eta=eta, sweep=1)))
    for n, _ in SM.EDGES:
        need.append((f"ddpm at n = {n}", lambda r, n=n: _is(r, SM.DDPM, (n,), t=500)))
        need.append((f"ddim at n = {n}", lambda r, n=n: _is(r, SM.DDIM, (n,))))
        need.append((f"affine at n = {n}", lambda r, n=n: _is(r, SM.AFF, (n,), t=500)))
    turn = lambda r: r.dims[0] > SM.GRID_CAP * SM.NT and r.launches[0][1] == SM.GRID_CAP  # noqa: E731
    for entry in (SM.DDPM, SM.DDIM, SM.AFF):
        need.append((f"{entry}: the second turn of the grid-stride loop", lambda r, e=entry: r.entry == e and turn(r)))
    need += [
        ("ddpm with a second output", lambda r: r.entry == SM.DDPM and opt(r, "prev2") == 1),
        ("ddpm without x0", lambda r: r.entry == SM.DDPM and opt(r, "x0") == 0),
        ("ddpm in place", lambda r: r.entry == SM.DDPM and opt(r, "alias") == 1 and opt(r, "t") > 0),
        ("ddpm reading abar[0] as abar[t - 1]", lambda r: r.entry == SM.DDPM and opt(r, "t") == 1 and r.dims[0] < SM.BIG),
        ("ddpm at the last table entry off the sweep", lambda r: r.entry == SM.DDPM and opt(r, "t") == 999),
        ("dec_t above zero", lambda r: r.entry == SM.DDPM and opt(r, "dec") and opt(r, "t") == 5),
        ("dec_t at zero", lambda r: r.entry == SM.DDPM and opt(r, "dec") and opt(r, "t") == 0),
        ("ddpm null z at t = 0", lambda r: r.entry == SM.DDPM and opt(r, "z") == 0 and opt(r, "t") == 0),
        ("ddpm null z at t > 0", lambda r: r.entry == SM.DDPM and opt(r, "z") == 0 and opt(r, "t") > 0),
        ("ddim null noise", lambda r: r.entry == SM.DDIM and opt(r, "noise") == 0),
        ("ddim with a second output", lambda r: r.entry == SM.DDIM and opt(r, "out2") == 1),
        ("ddim_dup with a null second output", lambda r: r.entry == SM.DDIM and opt(r, "dup") == 1 and not opt(r, "out2")),
        ("ddim in place", lambda r: r.entry == SM.DDIM and opt(r, "alias") == 1),
        ("ddim advance from idx 3", lambda r: _is(r, SM.DDIM, (257,), adv=1)),
        ("ddim advance at idx 0", lambda r: r.entry == SM.DDIM and opt(r, "adv") and opt(r, "idx") == 0),
        ("ddim advance without t_dev", lambda r: r.entry == SM.DDIM and opt(r, "adv") and opt(r, "tdev") == 0),
        ("ddim without t_dev and without advance", lambda r: r.entry == SM.DDIM and not opt(r, "adv") and opt(r, "tdev") == 0),
        ("affine null z", lambda r: r.entry == SM.AFF and opt(r, "z") == 0),
    ]
    for t in (999, 500, 1, 0):
        need.append((f"affine at t = {t}", lambda r, t=t: _is(r, SM.AFF, (67,), t=t)))
    for B in (1, 3, 5):
        for per in (1, 7, 256, 1000):
            need.append((f"add_noise at B = {B}, per = {per}", lambda r, B=B, per=per: _is(r, SM.ADDN, (B, per))))
    need.append(("add_noise: the second turn", lambda r: r.entry == SM.ADDN and r.dims[0] * r.dims[1] > SM.ADDN_GRID_CAP *
                 SM.NT and r.dims[0] > 1 and r.launches[0][1] == SM.ADDN_GRID_CAP))
    for n in (1, 2, 3, 4, 5, 1023, 1024, 1025):
        need.append((f"randn at n = {n}", lambda r, n=n: _is(r, SM.RANDN, (n,), seed=SM.SEED_HI, off=SM.OFF_HI)))
    for seed, off in SM.SEED_PAIRS[:4]:
        need.append((f"randn at seed {seed}, offset {off}", lambda r, s=seed, o=off: _is(r, SM.RANDN, (1025,), seed=s, off=o)))
    need.append(("randn advancing its offset", lambda r: r.entry == SM.RANDN and opt(r, "adv") == 1))
    need.append(("randn: the second turn", lambda r: r.entry == SM.RANDN and SM.cdiv(r.dims[0], 4) > SM.GRID_CAP * SM.NT))
    own = lambda r, k: isinstance(opt(r, k), tuple)  # noqa: E731
    need += [
        ("draw without text and keep", lambda r: r.entry == SM.DRAW and not opt(r, "txt") and not opt(r, "keep")),
        ("draw at p = 0.1 on a few samples", lambda r: _is(r, SM.DRAW, (5, 3, 4), T=1000, txt=1, keep=1, pt=0.1, pk=0.1)),
        ("draw at p_text 0 and p_keep 1", lambda r: r.entry == SM.DRAW and opt(r, "pt") == 0.0 and opt(r, "pk") == 1.0),
        ("draw at p_text 1 and p_keep 0", lambda r: r.entry == SM.DRAW and opt(r, "pt") == 1.0 and opt(r, "pk") == 0.0),
        ("draw at a sample's own uniforms, T = 2^31 - 1", lambda r: r.entry == SM.DRAW and own(r, "pt") and own(r, "pk") and
         opt(r, "T") == 2 ** 31 - 1),
        ("draw with text and no keep", lambda r: r.entry == SM.DRAW and opt(r, "txt") and not opt(r, "keep")),
        ("draw of 257 samples at p = 0.1", lambda r: r.entry == SM.DRAW and r.dims[1] == 257 and opt(r, "pt") == 0.1),
        ("draw at the last sample's own uniforms, T = 1", lambda r: r.entry == SM.DRAW and own(r, "pt") and opt(r, "T") == 1),
        ("draw: text and samples in the second turn", lambda r: r.entry == SM.DRAW and SM.cdiv(r.dims[0], 4) >=
         SM.GRID_CAP * SM.NT and opt(r, "txt") and opt(r, "keep")),
    ]
    return need


def _missing(rows, needs):
    return [what for what, pred in needs if not any(pred(r) for r in rows)]


def test_coverage():
    assert _missing(SM.ROWS, _needs()) == []


def test_no_row_can_be_removed():
    needs = _needs()
    for r in SM.ROWS:
        assert _missing([y for y in SM.ROWS if y is not r], needs), f"ROWS without {SM.row_id(r)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# error returns that come before any launch (no pointer below is ever dereferenced)
# ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_a_launch():
    from sdmi import _lib
    L = _lib.lib()
    host = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(host) + 15) // 16 * 16
    ddpm = [p, p, p, 16, p, p, p, p, p, p, p, 1, None]
    for i in (0, 1, 4, 5, 6, 7, 8, 9):
        assert L.sdmi_ddpm_prev(*(ddpm[:i] + [None] + ddpm[i + 1:])) == -1, i
        assert L.sdmi_ddpm_prev_dup(*(ddpm[:i] + [None] + ddpm[i + 1:10] + [p] + ddpm[10:])) == -1, i
    assert L.sdmi_ddpm_prev(*(ddpm[:3] + [0] + ddpm[4:])) == -1
    for fn in (L.sdmi_ddim_prev, L.sdmi_affine_step):
        a = [p, p, p, 16, 0.5, 0.75, 0.5, p, None]
        for i in (0, 1, 7):
            assert fn(*(a[:i] + [None] + a[i + 1:])) == -1, i
        assert fn(*(a[:3] + [0] + a[4:])) == -1 and fn(*(a[:3] + [-1] + a[4:])) == -1
    dev = [p, p, p, 16, p, p, p, p, p, 0.5, p, 1, None]
    for i in (0, 1, 4, 5, 6, 8, 10):
        assert L.sdmi_ddim_prev_dev(*(dev[:i] + [None] + dev[i + 1:])) == -1, i
        assert L.sdmi_ddim_prev_dev_dup(*(dev[:i] + [None] + dev[i + 1:11] + [p] + dev[11:])) == -1, i
    assert L.sdmi_ddim_prev_dev(*(dev[:3] + [0] + dev[4:])) == -1
    assert L.sdmi_randn(None, 16, 7, p, 1, None) == -1 and L.sdmi_randn(p, 16, 7, None, 1, None) == -1
    assert L.sdmi_randn(p, 0, 7, p, 1, None) == -1
    addn = [p, p, p, p, p, 2, 8, p, None]
    for i in (0, 1, 2, 3, 4, 7):
        assert L.sdmi_add_noise(*(addn[:i] + [None] + addn[i + 1:])) == -1, i
    for i in (5, 6):
        for v in (0, -1):
            assert L.sdmi_add_noise(*(addn[:i] + [v] + addn[i + 1:])) == -1, (i, v)

    def draw(n=16, B=2, T=1000, noise=1, t=1, txt=1, text=1, empty=1, re=8, align=(0, 0, 0)):
        q = lambda on, a=0: (p + a) if on else None  # noqa: E731
        rc = L.sdmi_step_draw(q(noise), n, q(t), B, T, q(text, align[0]), q(empty, align[1]), q(txt, align[2]), re, 0.1,
                              None, 0.1, 7, 1, None)
        assert rc == SM.draw_status(n, B, T, txt, text, empty, re, align, noise, t) != 0
        return rc

    assert [draw(noise=0), draw(t=0), draw(n=0), draw(B=0), draw(T=0), draw(T=-1)] == [-1] * 6
    assert [draw(text=0), draw(empty=0), draw(re=0), draw(re=6), draw(re=-4)] == [-2] * 5
    assert [draw(align=a) for a in ((4, 0, 0), (0, 8, 0), (0, 0, 4))] == [-2] * 3
    assert draw(noise=0, text=0) == -1


# ----------------------------------------------------------------------------------------------------------------
# the models are the reference's arithmetic: torch on the CPU gives the same bits on every row's data
# ----------------------------------------------------------------------------------------------------------------
def test_torchs_own_square_root_is_within_one_ulp_of_the_correctly_rounded_one():
    """The one substitution of the torch evaluation (sampler_matrix.tsqrt) changes a rounding, nothing else."""
    v = torch.from_numpy(np.concatenate([SM.table(k).abar for k in ("cond", "uncond", "syn")] + [SM.affine_coeffs()[2]]))
    exact, own = SM.tsqrt(v), torch.sqrt(v)
    assert bool(((SM.bits(exact) - SM.bits(own)).abs() <= 1).all())
    assert SM.same_bits(exact.numpy(), np.sqrt(v.numpy()))


def _ddpm_check(row):
    tab, t, x, e, z = SM.ddpm_row_case(row)
    zz = z if opt(row, "z", 1) else None
    prev, x0, x0u = SM.ddpm_model(tab, t, x, e, zz)
    for i, ti in enumerate(t):
        p, q = SM.ddpm_torch(tab, int(ti), x[i], e[i], None if zz is None else z[i])
        assert SM.same_bits(p, prev[i]) and SM.same_bits(q, x0[i]), f"{SM.row_id(row)} at t = {ti}"
    return tab, t, x, e, z, prev, x0, x0u


@pytest.mark.parametrize("row", SM.rows_of(SM.DDPM), ids=SM.row_id)
def test_ddpm_model_is_the_references_arithmetic(row):
    tab, t, x, e, z, prev, x0, x0u = _ddpm_check(row)
    n = x.shape[1]
    if n >= 16:     # the specials are there, the clamp keeps a NaN and the steps pass it on
        for k, a in enumerate((x, e, z)):
            assert np.isnan(a[:, 5 * k + 4]).all() and (a[:, 5 * k + 2] == SM.INF).all() and np.signbit(a[:, 5 * k + 1]).all()
        assert np.isnan(x0[:, 4]).all() and np.isnan(x0[:, 9]).all() and np.isnan(prev[:, 4]).all()
        assert bool((np.abs(x0[~np.isnan(x0)]) <= 1).all())
    if opt(row, "sweep"):
        assert list(t) == list(range(tab.T)) and bool((np.diff(tab.abar) < 0).all()) and 0 < tab.abar.min() and tab.abar.max() < 1
        two_ulp = 2 * 2.0 ** -23
        for target, at in SM.SEAM_AT.items():
            g = x0u[:, at:at + len(SM.SEAM_OFFSETS)].astype(np.float64)
            above, below = (g > target) & (g <= target + two_ulp), (g < target) & (g >= target - two_ulp)
            assert bool(above.any(1).all()) and bool(below.any(1).all()), f"no element beside {target} at some t"
            assert bool((x0[:, at:at + len(SM.SEAM_OFFSETS)] == SM.f32(target)).any(1).all())   # and the clamp acts there
    if opt(row, "z", 1) == 0 and opt(row, "t") > 0:   # null noise is +0 noise, not the t == 0 arm: a -0 mean becomes +0
        other, _, _ = SM.ddpm_model(tab, t, x, e, z)
        assert not SM.same_bits(other, prev)
        assert SM.same_bits(prev[:, 15], np.array([0.0], dtype=SM.f32)) and x[0, 15] == 0 and np.signbit(x[0, 15])


@pytest.mark.parametrize("row", SM.rows_of(SM.DDIM), ids=SM.row_id)
def test_ddim_model_is_the_references_arithmetic(row):
    abar, ts, tp, eta, x, e, nz = SM.ddim_row_case(row)
    nn = nz if opt(row, "noise", 1) else None
    sigma, c1, c2, inner = SM.ddim_coeffs(abar[ts], abar[tp], eta)
    assert not np.isnan(sigma).any() and not np.isnan(c1).any() and not np.isnan(c2).any() and bool((inner >= 0).all())
    # (the quadratic schedule repeats its first timesteps: t_prev == t gives sigma = 0 and c2 = 0, not a NaN)
    assert bool((sigma[abar[tp] > abar[ts]] > 0).all()) == (eta > 0) and bool((abar[tp] >= abar[ts]).all())
    want = SM.ddim_model(abar[ts], abar[tp], eta, x, e, nn)
    for i in range(len(ts)):
        got = SM.ddim_torch(abar[ts[i]], abar[tp[i]], eta, x[i], e[i], None if nn is None else nz[i])
        assert SM.same_bits(got, want[i]), f"{SM.row_id(row)} at pair ({ts[i]}, {tp[i]})"
    if opt(row, "sweep"):
        pairs = set(zip(ts.tolist(), tp.tolist()))
        assert len(ts) == 102 and {(1, 0), (999, 998), (981, 961), (801, 768)} <= pairs
    else:
        i = opt(row, "idx", SM.DDIM_IDX)
        assert (int(ts[0]), int(tp[0])) == (SM.DDIM_TS[i], SM.DDIM_TP[i])


def test_no_ddim_pair_has_a_nan_coefficient():
    """Over all t with t_prev = t - {1, 20, 41, 500}, both beta ranges and eta in {0, 0.5, 1}."""
    for tb in ("a", "b"):
        abar = SM.ddim_table(tb)
        for d in (1, 20, 41, 500):
            t = np.arange(d, 1000)
            for eta in (0.0, 0.5, 1.0):
                sigma, c1, c2, inner = SM.ddim_coeffs(abar[t], abar[t - d], eta)
                assert not np.isnan(sigma).any() and not np.isnan(c2).any() and bool((inner >= 0).all()), (tb, d, eta)


@pytest.mark.parametrize("row", SM.rows_of(SM.AFF), ids=SM.row_id)
def test_affine_model_is_the_references_arithmetic(row):
    c1, c2, var, x, e, z = SM.affine_row_case(row)
    zz = z if opt(row, "z", 1) else None
    want = SM.affine_model(c1, c2, var, x, e, zz)
    assert SM.same_bits(SM.affine_torch(c1, c2, var, x[0], e[0], None if zz is None else z[0]), want[0])
    if zz is None:      # + 0.0f: the -0 mean of element 15 becomes +0
        mean = SM.f32(c1) * x[0, 15] - SM.f32(c2) * e[0, 15]
        assert mean == 0 and np.signbit(mean) and want[0, 15] == 0 and not np.signbit(want[0, 15])
    assert (opt(row, "t") == 0) == (float(var) == 0.0)


@pytest.mark.parametrize("row", SM.rows_of(SM.ADDN), ids=SM.row_id)
def test_add_noise_model_is_the_references_arithmetic(row):
    tab, t, x0, eps = SM.addn_row_case(row)
    B, per = row.dims
    want = SM.add_noise_model(tab, t, x0, eps)
    assert SM.same_bits(SM.add_noise_torch(tab, t, x0, eps), want)
    assert len(set(t.tolist())) == B and (B == 1 or {0, 999} <= set(t.tolist()))
    if B > 1:       # b = i / (per + 1), clamped, is another result
        i = np.arange(B * per)
        b = np.minimum(i // (per + 1), B - 1)
        pert = tab.sa[t][b] * x0.reshape(-1) + tab.s1m[t][b] * eps.reshape(-1)
        assert not SM.same_bits(pert.reshape(B, per), want)


# ----------------------------------------------------------------------------------------------------------------
# Philox and the draws
# ----------------------------------------------------------------------------------------------------------------
def test_philox_gives_the_published_known_answers():
    for counter, key, want in SM.KNOWN_ANSWERS:
        got = SM.philox([np.array([c], dtype=np.uint64) for c in counter], key)[0]
        assert tuple(int(w) for w in got) == want
    # the layout: counter (q lo, q hi, off lo, off hi), key (seed lo, seed hi), on the third known answer
    q, off, seed = 0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822
    assert tuple(int(w) for w in SM._words(np.array([q], dtype=np.uint64), seed, off)[0]) == SM.KNOWN_ANSWERS[2][2]
    assert tuple(int(w) for w in SM.sample_words(7, 1, 3)[2]) == \
        tuple(int(w) for w in SM._words(np.array([2 ** 40 + 2], dtype=np.uint64), 7, 1)[0])
    for kw in (dict(rounds=9), dict(rounds=11), dict(bump="counter"), dict(swap_m=True)):
        got = SM.philox([np.array([c], dtype=np.uint64) for c in SM.KNOWN_ANSWERS[2][0]], SM.KNOWN_ANSWERS[2][1], **kw)[0]
        assert tuple(int(w) for w in got) != SM.KNOWN_ANSWERS[2][2], kw


def _noise_keys():
    keys = {(opt(r, "seed"), opt(r, "off"), SM.cdiv(r.dims[0], 4)) for r in SM.rows_of(SM.RANDN)}
    keys |= {(SM.DRAW_SEED, SM.DRAW_OFF, SM.cdiv(r.dims[0], 4)) for r in SM.rows_of(SM.DRAW)}
    return sorted(keys)


def test_the_noise_constant_is_twice_the_emulated_ratio_plus_the_library_allowance():
    worst, draws = 0.0, 0
    for seed, off, nq in _noise_keys():
        w = SM.noise_words(seed, off, nq)
        z, rad, theta = SM.noise_reference(w)
        assert np.isfinite(z).all() and bool((rad >= 0).all()) and bool((theta < 2 * math.pi).all())
        worst = max(worst, SM.worst_ratio(SM.noise_emulation(w), z, SM.noise_bound(rad, theta, 1.0)))
        draws += 4 * nq
    print(f"largest emulated |fp32 - float64| / (u rad (1 + theta)) over {draws} draws: {worst:.3f}")
    assert draws >= 2 ** 22
    base = SM.K_Z - SM.LIB_ALLOWANCE
    assert abs(worst - SM.EMULATED_RATIO) <= 0.005 and base == math.ceil(2 * worst) and 2 * worst <= base <= 3 * worst


PERTURBED = (
    ("cos and sin swapped", dict(swap=True), {}),
    ("pairs (0, 2) and (1, 3)", dict(pairs=((0, 2), (1, 3))), {}),
    ("u1 without its + 1", dict(plus1=False), {}),
    (">> 9", dict(shift=9), {}),
    ("a 23-bit uniform", dict(shift=9, scale=2.0 ** -23), {}),
    ("nine rounds", {}, dict(rounds=9)),
    ("eleven rounds", {}, dict(rounds=11)),
    ("the key bump on the counter", {}, dict(bump="counter")),
    ("the high word of off dropped", {}, dict(off_hi=False)),
    ("M0 and M1 swapped", {}, dict(swap_m=True)),
)


@pytest.mark.parametrize("case", PERTURBED, ids=lambda c: c[0])
def test_perturbed_noise_references_leave_the_bound(case):
    name, ref_kw, word_kw = case
    seed, off, nq = 7, 2 ** 32 + 1, SM.cdiv(SM.BIG4, 4)
    w = SM.noise_words(seed, off, nq)
    z, rad, theta = SM.noise_reference(w)
    pert, _, _ = SM.noise_reference(SM.perturbed_noise_words(seed, off, nq, **word_kw) if word_kw else w, **ref_kw)
    ratio = SM.worst_ratio(pert, z, SM.noise_bound(rad, theta))
    assert ratio > 1000, f"{name}: only {ratio:.1f} times the bound"


def test_the_high_words_of_seed_and_offset_change_every_block():
    low = SM.noise_words(7, 1, 257)
    for seed, off in ((2 ** 32 + 7, 1), (7, 2 ** 32 + 1)):
        assert bool((SM.noise_words(seed, off, 257) != low).any(1).all())
    assert bool((SM.sample_words(2 ** 32 + 7, 1, 5) != SM.sample_words(7, 1, 5)).any(1).all())


@pytest.mark.parametrize("row", SM.rows_of(SM.DRAW), ids=SM.row_id)
def test_draws_follow_from_the_integers_with_strict_comparisons(row):
    B, T = row.dims[1], opt(row, "T")
    pt, pk = SM.draw_probabilities(row)
    t, drop, keep, ut, uk = SM.draw_reference(SM.DRAW_SEED, SM.DRAW_OFF, B, T, pt, pk)
    w = SM.sample_words(SM.DRAW_SEED, SM.DRAW_OFF, B)
    assert [int(v) for v in t] == [(int(c) * T) >> 32 for c in w[:, 0]] and 0 <= t.min() and t.max() < T
    assert bool((ut < 1).all()) and bool((uk >= 0).all())
    assert pt == float(SM.f32(pt)) and pk == float(SM.f32(pk))
    if T > 1:       # shifting by 31 (clamped) is another t
        assert [min(((int(c) * T) >> 31), T - 1) for c in w[:, 0]] != [int(v) for v in t]
    if isinstance(opt(row, "pt"), tuple):
        b = opt(row, "pt")[1]
        assert pt == float(ut[b]) and not drop[b]                      # the strict < keeps the row
        assert SM.draw_reference(SM.DRAW_SEED, SM.DRAW_OFF, B, T, float(np.nextafter(SM.f32(pt), SM.f32(2))), pk)[1][b]
    if isinstance(opt(row, "pk"), tuple):
        b = opt(row, "pk")[1]
        assert pk == float(uk[b]) and keep[b] == 0                      # the strict > gives keep = 0
    if opt(row, "pt") == 0.0:
        assert not drop.any() and not keep.any()
    if opt(row, "pt") == 1.0:
        assert drop.all() and keep.all()
    if B == 257 and opt(row, "pt") == 0.1:
        assert 5 <= int(drop.sum()) <= 60 and 5 <= int((keep == 0).sum()) <= 60
        assert bool((drop != (keep == 0)).any())                        # drop and keep read different words
    text, empty = SM.text_case(B, max(row.dims[2], 4))
    assert len({r.tobytes() for r in text} | {empty.tobytes()}) == B + 1
