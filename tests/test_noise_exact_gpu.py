"""Every latent-noise kernel of csrc/latent_noise.hip at every row of tests/noise_matrix.py ROWS, exact, guarded.

sdmi_latent_range, sdmi_latent_noise_fwd and sdmi_latent_noise_bwd run every row with every plant of the exact family
and, on the soft family, both n_scale with and without planted ties; the backward also with dzin as a column window of
a wider NaN-filled buffer. The recorded launch plan must name the row's kernels and grids. After every call nothing but
the declared outputs may have changed, bit for bit. Then the statements of tests/noise_matrix.py: the partials by
value, out, zin (zero pads included) and r bitwise, S within its bound and equal to S64 in the exact family. A second
identical call gives identical bits. Each test prints its worst |S - S64| / bound.

Also the error returns (-1, nothing launched, nothing written) and the n_scale == 0 calls that return 0 and launch
nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import noise_matrix as NM

pytestmark = pytest.mark.gpu


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = NM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert NM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _same(got, ref, what, tag):
    assert got.shape == ref.shape, f"{tag}: {what} has shape {tuple(got.shape)}, not {tuple(ref.shape)}"
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: {what} has NaN elsewhere than its reference"
    assert torch.equal(got[~nan], ref[~nan]), \
        f"{tag}: {what} differs in {int((got[~nan] != ref[~nan]).sum())} elements from its bitwise value"


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _repeatable(p, call, tag):
    first = p.raw()
    assert call() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, p.raw()):
        assert torch.equal(NM.bits(a), NM.bits(b)), f"{tag}: a second identical call gives other bits"


def _cases(n):
    """(family, plant, n_scale) of one row."""
    out = [("exact", plant, NM.EXACT_SCALE) for plant in NM.PLANTS]
    return out + [("soft", plant, ns) for plant in NM.SOFT_PLANTS for ns in NM.SOFT_SCALES]


# ----------------------------------------------------------------------------------------------------------------
# sdmi_latent_range
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", NM.rows_of(NM.RANGE), ids=NM.row_id)
def test_range_rows(row):
    L = _L()
    n = row.dims[0]
    assert L.sdmi_latent_noise_workspace(n) == NM.workspace(n)
    for kind, plant in [("exact", q) for q in NM.PLANTS] + [("soft", q) for q in NM.SOFT_PLANTS]:
        tag = f"{NM.row_id(row)} {kind} {plant}"
        z = NM.z_case(kind, n, plant)
        p = NM.RangeProblem(z)
        g = p.guard()
        _run(L, lambda: p.run(L, _stream()), row.launches, tag)
        _unchanged(g, tag)
        val, cnt = p.outputs()
        want_val, want_cnt = NM.partials(z)
        _same(val, want_val, "the partial extremes", tag)
        assert torch.equal(cnt, want_cnt), f"{tag}: the partial counts {cnt.tolist()} are not {want_cnt.tolist()}"
        _repeatable(p, lambda: p.run(L, _stream()), tag)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_latent_noise_fwd
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", NM.rows_of(NM.FWD), ids=NM.row_id)
def test_forward_rows(row):
    L = _L()
    B, C, HW = row.dims
    n, cout, ld = NM.numel(row), NM.opt(row, "cout", 0), NM.opt(row, "ld", 0)
    for kind, plant, ns in _cases(n):
        tag = f"{NM.row_id(row)} {kind} {plant} {ns}"
        c = NM.fwd_case(kind, B, C, HW, cout, NM.opt(row, "bias", 0))
        z = NM.z_case(kind, n, plant)
        p = NM.FwdProblem(c, z, row, ns)
        g = p.guard()
        _run(L, lambda: p.run(L, _stream()), row.launches, tag)
        _unchanged(g, tag)
        ref = NM.out_reference(z, c["eps"], ns)
        _same(p.out.get(n), ref, "out", tag)
        if plant == "equal":
            assert torch.equal(NM.bits(p.out.data), NM.bits(p.z.data)), f"{tag}: out is not z bitwise"
        if plant == "nan":
            assert bool(torch.isnan(p.out.data).all()), f"{tag}: an element of out is not NaN"
        if NM.opt(row, "zin"):
            _same(p.zin[:, :cout].cpu().double(), NM.zin_reference(c, ref), "zin", tag)
            assert ld == cout or bool((NM.bits(p.zin[:, cout:].contiguous()) == 0).all()), \
                f"{tag}: the pad columns of zin are not zero"
        _repeatable(p, lambda: p.run(L, _stream()), tag)


# ----------------------------------------------------------------------------------------------------------------
# sdmi_latent_noise_bwd
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", NM.rows_of(NM.BWD), ids=NM.row_id)
def test_backward_rows(row):
    L = _L()
    B, C, HW = row.dims
    n, worst = NM.numel(row), 0.0
    layouts = NM.LAYOUTS if NM.opt(row, "dzin") else NM.LAYOUTS[:1]
    for kind, plant, ns in _cases(n):
        c = NM.bwd_case(kind, B, C, HW, NM.opt(row, "dzin"), NM.opt(row, "add"))
        z = NM.z_case(kind, n, plant)
        terms, S64, T = NM.s_reference(c)
        for layout in layouts:
            tag = f"{NM.row_id(row)} {kind} {plant} {ns} {layout}"
            p = NM.BwdProblem(c, z, row, ns, layout)
            g = p.guard()
            _run(L, lambda: p.run(L, _stream()), row.launches, tag)
            _unchanged(g, tag)
            part = p.ws.data[:p.blocks].cpu()
            assert not bool(torch.isnan(part).any()), f"{tag}: a partial was not written"
            S = float(NM.last_stage(part))
            if kind == "exact":
                assert S == S64, f"{tag}: S = {S!r} is not the exact sum {S64!r}"
            else:
                lim = NM.sum_bound(T)
                worst = max(worst, abs(S - S64) / lim)
                assert abs(S - S64) <= lim, f"{tag}: |S - S64| / bound = {abs(S - S64) / lim:.3f}"
            _same(p.r.get(n), NM.r_reference(c, z, np.float32(S), ns), "r", tag)
            _repeatable(p, lambda: p.run(L, _stream()), tag)
    print(f"{NM.row_id(row)}: max(|S - S64| / bound) {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------
# the chain as the engines call it: range -> fwd on the kernel's own partials
# ----------------------------------------------------------------------------------------------------------------
def test_forward_on_the_range_kernels_own_partials():
    L = _L()
    row = NM.rows_of(NM.FWD)[3]                         # (1, 8, 257): three partials
    B, C, HW = row.dims
    n = NM.numel(row)
    c = NM.fwd_case("soft", B, C, HW, NM.opt(row, "cout"), 1)
    z = NM.z_case("soft", n, "ties")
    p = NM.FwdProblem(c, z, row, 0.2)
    p.ws.buf.fill_(float("nan"))
    rc, ops = NM.recorded(L, lambda: L.sdmi_latent_range(NM.ptr(p.z.data), n, NM.ptr(p.ws.data), _stream()) or
                          p.run(L, _stream()))
    assert rc == 0 and len(ops) == 2, ops                # the forward's budget: the randn launch plus these two
    torch.cuda.synchronize()
    _same(p.out.get(n), NM.out_reference(z, c["eps"], 0.2), "out", "range -> fwd")


# ----------------------------------------------------------------------------------------------------------------
# error returns and n_scale == 0
# ----------------------------------------------------------------------------------------------------------------
def _rejected(L, g, fn, tag, rc_want=-1):
    rc, ops = NM.recorded(L, fn)
    assert rc == rc_want, f"{tag}: returned {rc}, documented {rc_want}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: the call changed {g.changed()}"


def test_range_rejects_without_launching():
    L = _L()
    p = NM.RangeProblem(NM.z_case("exact", 3000, "first"))
    g, s = p.guard(writes=False), _stream()
    for name in ("z", "ws"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"range: {name} null")
    for v in (0, -1, 2 ** 31):
        _rejected(L, g, lambda: p.run(L, s, n=v), f"range: n = {v}")
    assert L.sdmi_latent_noise_workspace(0) == 0 and L.sdmi_latent_noise_workspace(-1) == 0


def _fwd_problem():
    row = NM.rows_of(NM.FWD)[2]                         # (1, 4, 255), zin, ld = 8, bias
    B, C, HW = row.dims
    c = NM.fwd_case("exact", B, C, HW, NM.opt(row, "cout"), 1)
    return NM.FwdProblem(c, NM.z_case("exact", NM.numel(row), "spread"), row, NM.EXACT_SCALE)


def test_forward_rejects_without_launching():
    L = _L()
    p = _fwd_problem()
    g, s = p.guard(writes=False), _stream()
    for name in ("z", "eps", "ws", "out", "w_post"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"forward: {name} null")
    for name in ("B", "C", "HW", "cout"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"forward: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, C=9), "forward: C = 9")
    _rejected(L, g, lambda: p.run(L, s, cout=9, ld=16), "forward: cout = 9")
    _rejected(L, g, lambda: p.run(L, s, ld=3), "forward: ld < cout")
    _rejected(L, g, lambda: p.run(L, s, B=2 ** 20, HW=2 ** 10), "forward: 2^31 elements")


def _bwd_problem():
    row = NM.rows_of(NM.BWD)[6]                         # (3, 4, 343), dzin and dz_add
    c = NM.bwd_case("exact", *row.dims, 1, 1)
    return NM.BwdProblem(c, NM.z_case("exact", NM.numel(row), "spread"), row, NM.EXACT_SCALE, NM.CONTIGUOUS)


def test_backward_rejects_without_launching():
    L = _L()
    p = _bwd_problem()
    g, s = p.guard(writes=False), _stream()
    _rejected(L, g, lambda: p.run(L, s, dzin=None, dz_add=None), "backward: dzin and dz_add null")
    for name in ("w_post", "eps", "z", "ws_range", "ws", "r"):
        _rejected(L, g, lambda: p.run(L, s, **{name: None}), f"backward: {name} null")
    for name in ("B", "C", "HW"):
        for v in (0, -1):
            _rejected(L, g, lambda: p.run(L, s, **{name: v}), f"backward: {name} = {v}")
    _rejected(L, g, lambda: p.run(L, s, C=9, ld_dzin=16), "backward: C = 9")
    _rejected(L, g, lambda: p.run(L, s, ld_dzin=3), "backward: ld_dzin < C")
    _rejected(L, g, lambda: p.run(L, s, B=2 ** 20, HW=2 ** 10), "backward: 2^31 elements")


def test_zero_scale_launches_nothing():
    """n_scale == 0: both calls return 0 without a launch, without reading eps (a null pointer here) and without
    writing anything."""
    L = _L()
    s = _stream()
    p = _fwd_problem()
    _rejected(L, p.guard(writes=False), lambda: p.run(L, s, n_scale=0.0, eps=None), "forward at n_scale = 0", 0)
    q = _bwd_problem()
    _rejected(L, q.guard(writes=False), lambda: q.run(L, s, n_scale=0.0, eps=None), "backward at n_scale = 0", 0)
