"""Both latent kernels of the KL autoencoder (csrc/kl_latent.hip) at every row of tests/kl_matrix.py ROWS, exact, guarded.

sdmi_kl_sample and sdmi_kl_bwd run every row in both data families, with the operands contiguous and as column windows
of wider NaN-filled buffers. The recorded launch plan must name the row's kernels and grids. After every call nothing but
the declared outputs may have changed, bit for bit. Then the statements of tests/kl_matrix.py: moments, sample, zin
(zero pads included), the gradient of the moments and dh bitwise given the kernel's own expf (observed through the
kernel: device_exp), that expf within E_ULPS of the float64 exp, the KL sum and the four parameter-gradient sums within
K_KL u sum |terms| (equal in the exact family), kl bitwise from its partials. A second identical call gives identical bits.
Each test prints its worst |S - S64| / bound and its worst exp error in ulps.

Also the error returns (-1, nothing launched, nothing written)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kl_matrix as KM

pytestmark = pytest.mark.gpu


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = KM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert KM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _same(got, ref, what, tag):
    assert got.shape == ref.shape, f"{tag}: {what} has shape {tuple(got.shape)}, not {tuple(ref.shape)}"
    assert not bool(torch.isnan(got).any()), f"{tag}: {what} holds a NaN (an element was not written)"
    assert torch.equal(got, ref), \
        f"{tag}: {what} differs in {int((got != ref).sum())} elements from its bitwise value"


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _repeatable(p, call, tag):
    first = p.raw()
    assert call() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, p.raw()):
        assert torch.equal(KM.bits(a), KM.bits(b)), f"{tag}: a second identical call gives other bits"


def device_exp(L, x):
    """The kernel's own expf of an fp32 [P][z] tensor, through sdmi_kl_sample: mean 0 (zero weight rows), logvar = 2x
    (unit weights: 1 * 2x + 0 exactly), eps = 1, so sample = fl(0 + fl(expf(fl(0.5 * 2x)) * 1)) = expf(x)."""
    P, z = x.shape
    x = x.float()
    h = torch.cat([torch.zeros(P, z), 2.0 * x], 1).contiguous().cuda()
    w = torch.diag(torch.cat([torch.zeros(z), torch.ones(z)])).contiguous().cuda()
    eps = torch.ones(z * P, device="cuda")
    mom, smp = torch.empty(2 * z * P, device="cuda"), torch.full((z * P,), float("nan"), device="cuda")
    rc = L.sdmi_kl_sample(KM.ptr(h), 2 * z, KM.ptr(w), None, KM.ptr(eps), 1, z, P, KM.ptr(mom), KM.ptr(smp), None, None,
                          None, 0, None, None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return smp.cpu().view(z, P).t().contiguous()


def _exp_pair(L, lv, kind, tag):
    """(std32, E32, worst error in units of E_ULPS ulps); in the exact family logvar is 0 and both are 1 exactly."""
    half = np.float32(0.5) * lv
    std32, E32 = device_exp(L, half), device_exp(L, lv)
    worst = max(KM.exp_within(std32, half), KM.exp_within(E32, lv))
    assert worst <= 1.0, f"{tag}: the kernel's expf is {worst * KM.E_ULPS:.2f} ulps from the float64 exp"
    if kind == "exact":
        assert bool((std32 == 1).all()) and bool((E32 == 1).all()), f"{tag}: expf(0) is not 1"
    return std32, E32, worst


def _sum_check(got, S64, T, kind, what, tag):
    """got, S64, T: float64 tensors of one shape. Returns the worst |got - S64| / bound."""
    if kind == "exact":
        assert torch.equal(got, S64), f"{tag}: {what} is not the exact sum"
        return 0.0
    zero = T == 0
    assert bool((got[zero] == 0).all()), f"{tag}: {what} is non-zero where every term is zero"
    if not bool((~zero).any()):
        return 0.0
    ratio = float(((got - S64).abs()[~zero] / KM.sum_bound(T[~zero])).max())
    assert ratio <= 1.0, f"{tag}: {what}: |S - S64| / bound = {ratio:.3f}"
    return ratio


# ----------------------------------------------------------------------------------------------------------------
# sdmi_kl_sample
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", KM.rows_of(KM.SAMPLE), ids=KM.row_id)
def test_sample_rows(row):
    L = _L()
    B, z, HW = row.dims
    P, M = B * HW, 2 * z
    assert L.sdmi_kl_workspace(P) == KM.workspace(P)
    worst_s, worst_e = 0.0, 0.0
    for kind in KM.KINDS:
        c = KM.sample_case(kind, B, z, HW, KM.opt(row, "bias"))
        mom = KM.moments_reference(c, KM.opt(row, "bias"))
        lv = mom[:, z:].float()
        std32, E32, e = _exp_pair(L, lv, kind, f"{KM.row_id(row)} {kind}")
        worst_e = max(worst_e, e)
        eps = KM.rows_of_nchw(c["eps"], B, HW, z) if KM.opt(row, "eps") else None
        smp = KM.sample_reference(mom, z, eps, std32)
        for layout in KM.LAYOUTS:
            tag = f"{KM.row_id(row)} {kind} {layout}"
            p = KM.SampleProblem(c, row, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            _same(p.rows(p.moments, M), mom, "moments", tag)
            _same(p.rows(p.sample, z), smp, "sample", tag)
            if not KM.opt(row, "eps"):
                assert torch.equal(p.rows(p.sample, z), mom[:, :z]), f"{tag}: without eps the sample is not the mean"
            if KM.opt(row, "zin"):
                ld = KM.opt(row, "ld")
                _same(p.zin[:, :z].cpu().double(), KM.zin_reference(smp, c["w_post"], c["b_post"]), "zin", tag)
                assert bool((KM.bits(p.zin[:, z:].contiguous()) == 0).all()), f"{tag}: the pad columns of zin are not zero"
                assert p.zin.shape[1] == ld
            if KM.opt(row, "kl"):
                part = p.ws.data[:p.blocks].cpu()
                assert not bool(torch.isnan(part).any()), f"{tag}: a partial was not written"
                terms = KM.kl_terms(mom, z, E32)
                S = float(KM.last_stage(part))
                S64, T = terms.double().sum().reshape(1), terms.double().abs().sum().reshape(1)
                worst_s = max(worst_s, _sum_check(torch.tensor([S], dtype=torch.float64), S64, T, kind, "the KL sum", tag))
                assert float(p.kl.get(1)) == KM.kl_value(np.float32(S), B), f"{tag}: kl is not fl(fl(0.5 S) / B)"
            _repeatable(p, lambda: p.run(L, _stream()), tag)
    print(f"{KM.row_id(row)}: max(|S - S64| / bound) {worst_s:.3f}, worst expf error {worst_e * KM.E_ULPS:.2f} ulps")


# ----------------------------------------------------------------------------------------------------------------
# sdmi_kl_bwd
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", KM.rows_of(KM.BWD), ids=KM.row_id)
def test_backward_rows(row):
    L = _L()
    B, z, HW = row.dims
    P, M = B * HW, 2 * z
    assert L.sdmi_kl_bwd_workspace() == KM.bwd_workspace()
    worst_s = 0.0
    for kind in KM.KINDS:
        c = KM.bwd_case(kind, B, z, HW)
        lv = c["moments"][:, z:].float()
        std32, E32, _ = _exp_pair(L, lv, kind, f"{KM.row_id(row)} {kind}")
        dmom = KM.dmom_reference(c, row, std32, E32 - 1.0)
        sums = KM.grad_terms(c, row, dmom)
        for layout in KM.LAYOUTS:
            tag = f"{KM.row_id(row)} {kind} {layout}"
            p = KM.BwdProblem(c, row, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            _same(KM.rows_of_nchw(p.dmom.get(P * M), B, HW, M), dmom, "the gradient of the moments", tag)
            if KM.opt(row, "dh"):
                _same(p.dh[:, :M].cpu().double(), KM.dh_reference(dmom, c["w_pre"]), "dh", tag)
                assert bool((KM.bits(p.dh[:, M:].contiguous()) == 0).all()), f"{tag}: the pad columns of dh are not zero"
            for name, (terms, shape) in sums.items():
                n = terms.shape[1]
                got = getattr(p, name).get(n)
                worst_s = max(worst_s, _sum_check(got, terms.sum(0), terms.abs().sum(0), kind, name, tag))
            _repeatable(p, lambda: p.run(L, _stream()), tag)
    print(f"{KM.row_id(row)}: max(|S - S64| / bound) {worst_s:.3f}")


def test_device_loss_weight_multiplies_the_host_weight():
    """kl_weight 2 kw with the device scalar loss_w = 0.5 is kl_weight kw, bit for bit (the product is exact)."""
    L = _L()
    row = KM.rows_of(KM.BWD)[5]                         # (2, 4, 257), everything on
    assert row.dims == (2, 4, 257) and KM.opt(row, "kw")
    c = KM.bwd_case("soft", *row.dims)
    a, b = KM.BwdProblem(c, row, KM.CONTIGUOUS), KM.BwdProblem(c, row, KM.CONTIGUOUS, kw=2 * KM.SOFT_KW)
    lw = torch.tensor([0.5], device="cuda")
    assert a.run(L, _stream()) == 0 and b.run(L, _stream(), loss_w=KM.ptr(lw)) == 0
    torch.cuda.synchronize()
    for x, y in zip(a.raw(), b.raw()):
        assert torch.equal(KM.bits(x), KM.bits(y))


# ----------------------------------------------------------------------------------------------------------------
# error returns
# ----------------------------------------------------------------------------------------------------------------
def _rejected(L, g, fn, tag):
    rc, ops = KM.recorded(L, fn)
    assert rc == -1, f"{tag}: returned {rc}, documented -1"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: the call changed {g.changed()}"


def test_sample_rejects_without_launching():
    L = _L()
    row = KM.rows_of(KM.SAMPLE)[5]                      # (2, 4, 257), everything on
    assert row.dims == (2, 4, 257) and KM.opt(row, "kl") and KM.opt(row, "zin")
    p = KM.SampleProblem(KM.sample_case("exact", *row.dims, 1), row, KM.CONTIGUOUS)
    g, s = p.guard(writes=False), _stream()
    for name in ("h", "w_pre", "moments", "sample", "w_post", "ws"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"sample: {name} null")
    for name in ("B", "z", "HW"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"sample: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, z=5, ldh=16), "sample: 2z = 10")
    _rejected(L, g, lambda: p.run(L, s, ldh=7), "sample: ldh < 2z")
    _rejected(L, g, lambda: p.run(L, s, ld=3), "sample: ld < z")
    _rejected(L, g, lambda: p.run(L, s, B=2 ** 20, HW=2 ** 10), "sample: 2^31 elements")
    assert L.sdmi_kl_workspace(0) == 0 and L.sdmi_kl_workspace(-1) == 0


def test_backward_rejects_without_launching():
    L = _L()
    row = KM.rows_of(KM.BWD)[5]
    p = KM.BwdProblem(KM.bwd_case("exact", *row.dims), row, KM.CONTIGUOUS)
    g, s = p.guard(writes=False), _stream()
    for name in ("moments", "ws", "w_post", "sample", "w_pre", "h"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"backward: {name} null")
    _rejected(L, g, lambda: p.run(L, s, dzin=None), "backward: dw_post without dzin")
    none = dict(dh=None, dmom=None, dw_post=None, db_post=None, dw_pre=None, db_pre=None)
    _rejected(L, g, lambda: p.run(L, s, **none), "backward: no output")
    for name in ("B", "z", "HW"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"backward: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, z=5, ld_dzin=16, ld_out=16, ldh=16), "backward: 2z = 10")
    _rejected(L, g, lambda: p.run(L, s, ld_dzin=3), "backward: ld_dzin < z")
    _rejected(L, g, lambda: p.run(L, s, ld_out=7), "backward: ld_out < 2z")
    _rejected(L, g, lambda: p.run(L, s, ldh=7), "backward: ldh < 2z")
    _rejected(L, g, lambda: p.run(L, s, B=2 ** 20, HW=2 ** 10), "backward: 2^31 elements")
