"""CPU checks of tests/kl_matrix.py: the rows against the restated host rules, the exact family's margins, the measured
summation constant K_KL, and that every perturbed reference leaves its statement. No library call is made."""
import numpy as np
import pytest
import torch

from tests import kl_matrix as KM


def test_bindings_have_the_documented_arity():
    assert KM.ARITY == {"sdmi_kl_workspace": 1, "sdmi_kl_bwd_workspace": 0, "sdmi_kl_sample": 17, "sdmi_kl_bwd": 25}


def test_rows_follow_the_host_rules():
    for r in KM.ROWS:
        assert list(r.launches) == KM.expected_launches(r.entry, r.dims, r.opt), KM.row_id(r)
        assert 2 * r.dims[1] <= KM.MAXC
    assert KM.pixel_blocks(1) == 1 and KM.pixel_blocks(256) == 1 and KM.pixel_blocks(257) == 2
    assert KM.pixel_blocks(65536) == 256 and KM.pixel_blocks(66000) == 256
    assert KM.workspace(66000) == 1024 and KM.bwd_workspace() == 256 * 92 * 4 and KM.PART == 92
    ids = [KM.row_id(r) for r in KM.ROWS]
    assert len(set(ids)) == len(ids)


def test_rows_cover_the_declared_shapes_and_options():
    shapes = {(1, 1, 1), (1, 3, 255), (2, 4, 257), (2, 4, 1025), (2, 4, 33000)}
    for entry, keys in ((KM.SAMPLE, ("eps", "zin", "bias", "kl")), (KM.BWD, ("eps", "dsample", "dmom", "kw"))):
        rows = KM.rows_of(entry)
        assert {r.dims for r in rows} == shapes
        for shape in shapes:
            for key in keys:
                seen = {bool(KM.opt(r, key)) for r in rows if r.dims == shape}
                assert seen == {True, False}, (entry, shape, key)
    # the grid-stride loop is reached: more pixels than one trip of the capped grid
    assert max(r.dims[0] * r.dims[2] for r in KM.ROWS) > KM.CAP * KM.NT
    assert any(KM.opt(r, "ld") > 8 for r in KM.rows_of(KM.SAMPLE)) and any(KM.opt(r, "ld_out") > 8 for r in KM.rows_of(KM.BWD))
    assert any(not KM.opt(r, "dzin") for r in KM.rows_of(KM.BWD))


def _sample_refs(c, row, exp32=KM.cpu_exp32, half=0.5, swap=False):
    z = c["z"]
    mom = KM.moments_reference(c, KM.opt(row, "bias"))
    mean, lv = KM.halves(mom, z, swap)
    std = KM.std_of(lv, exp32, half)
    eps = KM.rows_of_nchw(c["eps"], c["B"], c["HW"], z) if KM.opt(row, "eps") else None
    smp = KM.sample_reference(mom, z, eps, std, swap)
    return mom, std, smp


def test_exact_family_is_exact():
    """logvar == 0, std == 1, E - 1 == 0 and every sum's margin below 2^24 units of its last bit."""
    for row in KM.ROWS:
        B, z, HW = row.dims
        if row.entry == KM.SAMPLE:
            c = KM.sample_case("exact", B, z, HW, KM.opt(row, "bias"))
            mom, std, smp = _sample_refs(c, row)
            assert bool((mom[:, z:] == 0).all()) and bool((std == 1).all())
            terms = KM.kl_terms(mom, z, KM.cpu_exp32(mom[:, z:]))
            assert bool((terms.double() == mom[:, :z] ** 2).all())
            assert float(terms.abs().sum()) < 2.0 ** 24, KM.row_id(row)
        else:
            c = KM.bwd_case("exact", B, z, HW)
            one = torch.ones(B * HW, z)
            dmom = KM.dmom_reference(c, row, one, torch.zeros_like(one))
            assert bool((dmom * 8 == (dmom * 8).round()).all())
            for name, (terms, _) in KM.grad_terms(c, row, dmom).items():
                assert float(terms.abs().sum(0).max()) * 32 < 2.0 ** 24, (KM.row_id(row), name)
                got = KM.emulate_grad(terms.float()).double()
                assert torch.equal(got, terms.sum(0)), (KM.row_id(row), name)


def test_summation_constant_is_measured():
    worst, where = 0.0, None
    for row in KM.ROWS:
        B, z, HW = row.dims
        if row.entry == KM.SAMPLE:
            if not KM.opt(row, "kl"):
                continue
            c = KM.sample_case("soft", B, z, HW, KM.opt(row, "bias"))
            mom, _, _ = _sample_refs(c, row)
            terms = KM.kl_terms(mom, z, KM.cpu_exp32(mom[:, z:]))
            S32, S64, T = KM.emulate_kl_S(terms), float(terms.double().sum()), float(terms.double().abs().sum())
            ratio = abs(S32 - S64) / (KM.U24 * T)
            if ratio > worst:
                worst, where = ratio, (KM.row_id(row), "kl")
        else:
            c = KM.bwd_case("soft", B, z, HW)
            lv = c["moments"][:, z:].float()
            E = KM.cpu_exp32(lv)
            dmom = KM.dmom_reference(c, row, KM.std_of(lv), E - 1.0)
            for name, (terms, _) in KM.grad_terms(c, row, dmom).items():
                S32 = KM.emulate_grad(terms.float()).double()
                T = terms.abs().sum(0)
                assert bool((S32[T == 0] == 0).all())                     # (a sum whose every term is zero)
                ratio = float(((S32 - terms.sum(0)).abs()[T > 0] / (KM.U24 * T[T > 0])).max()) if bool((T > 0).any()) else 0.0
                if ratio > worst:
                    worst, where = ratio, (KM.row_id(row), name)
    print(f"largest |S32 - S64| / (u sum |terms|): {worst:.3f} at {where}")
    assert abs(worst - KM.MEASURED) <= 5e-3, (worst, where)
    assert 2 * worst <= KM.K_KL <= 3 * worst, (worst, KM.K_KL)


def _differs(a, b):
    return not torch.equal(a, b)


@pytest.mark.parametrize("row", [r for r in KM.rows_of(KM.SAMPLE) if KM.opt(r, "eps") and r.dims[2] > 1], ids=KM.row_id)
def test_perturbed_sample_references_leave_their_statements(row):
    B, z, HW = row.dims
    c = KM.sample_case("soft", B, z, HW, KM.opt(row, "bias"))
    mom, std, smp = _sample_refs(c, row)
    lv = mom[:, z:].float()
    assert KM.exp_within(std, np.float32(0.5) * lv) <= 1.0            # torch's CPU exp is a conforming expf
    # the 0.5 in std dropped: far outside the exp statement, and the sample moves
    _, std_p, smp_p = _sample_refs(c, row, half=1.0)
    assert KM.exp_within(std_p, np.float32(0.5) * lv) > 1e3
    assert _differs(smp_p, smp)
    # the halves swapped
    _, _, smp_s = _sample_refs(c, row, swap=True)
    assert _differs(smp_s, smp)
    # 1 ulp in the sample
    assert _differs(torch.nextafter(smp.float(), torch.full_like(smp.float(), 1e30)).double(), smp)


@pytest.mark.parametrize("row", [r for r in KM.rows_of(KM.BWD) if KM.opt(r, "kw") and r.dims[2] > 1], ids=KM.row_id)
def test_perturbed_backward_references_leave_their_statements(row):
    B, z, HW = row.dims
    for kind in KM.KINDS:
        c = KM.bwd_case(kind, B, z, HW)
        lv = c["moments"][:, z:].float()
        E = KM.cpu_exp32(lv)
        std, t = KM.std_of(lv), E - 1.0
        ref = KM.dmom_reference(c, row, std, t)
        # the -1 in dlogvar dropped
        assert _differs(KM.dmom_reference(c, row, std, t, minus_one=False, E32=E)[:, z:], ref[:, z:]), kind
        # 1 / B replaced by 1 / (B P)
        assert _differs(KM.dmom_reference(c, row, std, t, per_pixel=True), ref), kind
        # dmom_add ignored
        assert _differs(KM.dmom_reference(c, row, std, t, use_add=False), ref), kind
        # the perturbed gradients also leave the sums' bound where the term is visible at all (soft: kl_weight 1e-4)
        if kind == "exact":
            terms, _ = KM.grad_terms(c, row, ref)["db_pre"]
            bad, _ = KM.grad_terms(c, row, KM.dmom_reference(c, row, std, t, use_add=False))["db_pre"]
            assert _differs(bad.sum(0), terms.sum(0))


def test_kl_value_last_step():
    assert KM.kl_value(np.float32(8.0), 2) == 2.0
    assert KM.kl_value(np.float32(3.0), 3) == float(np.float32(1.5) / np.float32(3))
