"""Every attention kernel instantiation (tests/attn_matrix.py ROWS), exact and guarded.

Selector-group data on every row: O, dQ, dK, dV and delta must torch.equal float64 maths with the kernels' rounding
points, lse lies within 8 fp32 ulps; the recorded launch plan must name the row's kernels and grids. The uniform family
sweeps ragged N and S (O == m bitwise, the backward exact for S a power of two); the soft family holds randn data to
componentwise bounds derived from the rounding points. Every case runs with contiguous operands and with operands that
are column windows of packed buffers, all NaN-guarded: nothing outside out, dq, dk, dv, lse[:B*H*N], delta[:B*H*N] and
the first sdmi_attn_bwd_workspace bytes of the workspace may change. Also the fused backward's counter slots across
more launches than slots, and the error returns (nothing launched, outputs untouched)."""
import ctypes
import functools

import pytest
import torch

from tests import attn_matrix as AM

pytestmark = pytest.mark.gpu

LAYOUTS = (AM.CONTIGUOUS, AM.PACKED)


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _forward(L, c, layout, want=None, tag=""):
    p = AM.Problem(c, layout)
    rc, ops = AM.recorded(L, lambda: p.fwd(L, _stream()))
    assert rc == 0, f"{tag}: sdmi_attn_fwd returned {rc}"
    if want is not None:
        assert AM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {want}"
    torch.cuda.synchronize()
    return p


def _backward(L, p, fused, want=None, tag=""):
    rc, ops = AM.recorded(L, lambda: p.bwd(L, _stream(), fused))
    assert rc == 0, f"{tag}: the backward returned {rc}"
    if want is not None:
        assert AM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {want}"
    torch.cuda.synchronize()
    return ops


def _check_forward_exact(p, ref, ulps, lse_scale, tag):
    assert torch.equal(p.out("o"), ref["O"]), f"{tag}: O differs from the exact reference"
    err = float((p.stat("lse") - ref["lse"]).abs().max())
    print(f"{tag}: lse error {err:.3e}, allowed {ulps * AM.ulp32(lse_scale):.3e}")
    assert err <= ulps * AM.ulp32(lse_scale), f"{tag}: lse off by {err}"
    bad = p.guards_ok(backward=False)
    assert bad is None, f"{tag}: forward changed memory: {bad}"


def _check_backward_exact(p, ref, tag):
    for name, key in (("dv", "dV"), ("dq", "dQ"), ("dk", "dK")):
        got = p.out(name)
        assert torch.equal(got, ref[key]), \
            f"{tag}: {key} differs from the exact reference in {int((got != ref[key]).sum())} elements"
    assert torch.equal(p.stat("delta"), ref["delta"]), f"{tag}: delta differs"
    bad = p.guards_ok(backward=True)
    assert bad is None, f"{tag}: backward changed memory: {bad}"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("row", AM.ROWS, ids=AM.row_id)
def test_selector_rows_exact(row, layout):
    L = _L()
    c = AM.selector_case(row.B, row.H, row.N, row.S, row.d, row.g)
    ref = AM.exact_reference(c)
    tag = f"{AM.row_id(row)} {layout}"
    p = _forward(L, c, layout, row.launches if row.entry == AM.FWD else None, tag)
    _check_forward_exact(p, ref, 8, ref["lse_scale"], tag)
    if row.entry != AM.FWD:
        _backward(L, p, row.entry == AM.FUSED, row.launches, tag)
        _check_backward_exact(p, ref, tag)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", AM.SWEEP_D)
def test_uniform_ragged_sweep(d, layout):
    """N, S in {1, 17, 64, 65, 128, 129, 257}^2, Q = 0 and K = 0: O == m bitwise and lse == log2 S within 4 fp32 ulps
    of max(1, log2 S); S a power of two: both backward forms exact (Q = 0: dK == 0; K = 0: dQ == 0)."""
    L = _L()
    for N in AM.SWEEP_LENS:
        for S in AM.SWEEP_LENS:
            for zero in ("q", "k"):
                c = AM.uniform_case(2, 3, N, S, d, zero)
                tag = f"uniform N{N} S{S} d{d} zero-{zero} {layout}"
                exact_bwd = S & (S - 1) == 0
                lse = torch.full((2, 3, N), float(torch.log2(torch.tensor(float(S), dtype=torch.float64))),
                                 dtype=torch.float64)
                ref = AM.exact_reference(c) if exact_bwd else dict(O=c["m"], lse=lse)
                p = _forward(L, c, layout, None, tag)
                _check_forward_exact(p, ref, 4, max(1.0, float(lse[0, 0, 0])), tag)
                if exact_bwd:
                    _backward(L, p, False, None, tag)
                    _check_backward_exact(p, ref, tag + " two-pass")
                    p = _forward(L, c, layout, None, tag)
                    _backward(L, p, True, None, tag)
                    _check_backward_exact(p, ref, tag + " fused")


@functools.lru_cache(maxsize=None)
def _soft(i):
    c = AM.soft_case(*AM.SOFT[i])
    return c, AM.soft_forward_reference(c)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("i", range(len(AM.SOFT)), ids=[f"B{s[0]}H{s[1]}-N{s[2]}-S{s[3]}-d{s[4]}" for s in AM.SOFT])
def test_soft_componentwise_bounds(i, layout):
    """randn data, the running maximum moves between key tiles. Every element, none excluded:
    |O - ref| <= 2^-7 (P |V|) + 2^-8 |ref|; |dV - ref| <= 2^-7 (P^T |dO|) + 2^-8 |ref|; with
    E = P (2^-7 (|dP| + |delta|) + 2^-8 sum_d |dO| |O|): |dQ - ref| <= s (E |K|) + 2^-8 |ref|,
    |dK - ref| <= s (E^T |Q|) + 2^-8 |ref|; |lse - ref| <= 8 fp32 ulps of max |score * c|. The float64 reference takes
    delta from the kernel's own bf16 O; the kernel's delta, an fp32 sum of d exact products, lies within
    (d + 1) 2^-24 sum_d |dO| |O| of it.

    lse where d % 16 == 8 (d = 24 here): the row sum comes out of the PV MFMA, a sum of bf16 P. A torch emulation of
    that rounding point (attn_matrix.emulate_lse_ones) exceeds the 8 ulps by a factor of 119.5 (1.82e-3 absolute), so
    the constant was too tight for these rows; twice that would be 3.7e-3. They are held to the tighter analytic
    bound instead, -log2(1 - 2^-9) = 2.82e-3 for the rounding of P plus the 8 ulps (the kernel measured 1.97e-3). The
    fp32 row sum of the other head dims stays at 8 ulps."""
    L = _L()
    c, fw = _soft(i)
    B, H, N, S, d = AM.SOFT[i]
    g4 = d <= 32 and N <= 256 and S <= 256 and B * H >= 512
    for fused in (False, True):
        tag = f"soft {AM.SOFT[i]} {layout} {'fused' if fused else 'two-pass'}"
        p = _forward(L, c, layout, None, tag)
        O = p.out("o")
        err, lim = (O - fw["O"]).abs(), fw["O_bound"] + 2.0 ** -8 * fw["O"].abs()
        print(f"{tag}: O worst error / bound {float((err / lim.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= lim).all()), f"{tag}: O worst error / bound {float((err / lim.clamp_min(1e-300)).max())}"
        lerr = float((p.stat("lse") - fw["lse"]).abs().max())
        lim = AM.lse_bound(d, fw["lse_scale"])
        print(f"{tag}: lse error {lerr:.3e}, allowed {lim:.3e}")
        assert lerr <= lim, f"{tag}: lse off by {lerr}, allowed {lim}"
        assert p.guards_ok(backward=False) is None, tag
        ops = _backward(L, p, fused, None, tag)
        if not fused:
            assert all(("ELi4EE" in name) == g4 for name, _ in ops), f"{tag}: launched {ops}"
        bw = AM.soft_backward_reference(c, fw, O)
        for name, key in (("dv", "dV"), ("dq", "dQ"), ("dk", "dK")):
            err, lim = (p.out(name) - bw[key]).abs(), bw[key + "_bound"]
            worst = float((err / lim.clamp_min(1e-300)).max())
            print(f"{tag}: {key} worst error / bound {worst:.3f}")
            assert bool((err <= lim).all()), f"{tag}: {key} worst error / bound {worst}"
        err, lim = (p.stat("delta") - bw["delta"]).abs(), bw["delta_bound"]
        worst = float((err / lim.clamp_min(1e-300)).max())
        print(f"{tag}: delta worst error / bound {worst:.3f}")
        assert bool((err <= lim).all()), f"{tag}: delta worst error / bound {worst}"
        bad = p.guards_ok(backward=True)
        assert bad is None, f"{tag}: backward changed memory: {bad}"


def test_fused_counter_slots_are_reused():
    """The arrival counters live in 4 slot regions used round-robin and must be back at zero when a slot comes round
    again: the 3-key-block fused backward six times in a row on one stream, then alternating with a shape of another
    query-tile count; every result bitwise the exact reference."""
    L = _L()
    rows = [r for r in AM.ROWS if r.entry == AM.FUSED and (r.d, r.N, r.S) == (32, 130, 257)] + AM.EXTRA
    assert len(rows) == 2 and -(-rows[0].N // 64) != -(-rows[1].N // 64)
    cases = [AM.selector_case(r.B, r.H, r.N, r.S, r.d, r.g) for r in rows]
    refs = [AM.exact_reference(c) for c in cases]
    for order in ((0,) * 6, (0, 1) * 3):
        probs = [_forward(L, cases[i], AM.PACKED) for i in order]
        for p in probs:  # back to back, no synchronisation in between
            assert p.bwd(L, _stream(), True) == 0
        torch.cuda.synchronize()
        for n, (i, p) in enumerate(zip(order, probs)):
            _check_backward_exact(p, refs[i], f"fused launch {n} of {order}")


# positions in the argument lists of the three entry points (include/sdmi.h)
FWD_PTR, FWD_LD, FWD_DIM = (0, 2, 4, 6), (1, 3, 5, 7), range(9, 14)
BWD_PTR, BWD_LD, BWD_DIM = (0, 2, 4, 6, 8, 12, 14, 16), (1, 3, 5, 7, 9, 13, 15, 17), range(18, 23)
FUS_PTR, FUS_LD, FUS_DIM = (0, 2, 4, 6, 8, 14, 16, 18), (1, 3, 5, 7, 9, 15, 17, 19), range(20, 25)


def _entry_points(L, p, ws, need):
    return (("sdmi_attn_fwd", L.sdmi_attn_fwd, p.args_fwd(), FWD_PTR, FWD_LD, FWD_DIM),
            ("sdmi_attn_bwd", L.sdmi_attn_bwd, p.args_bwd(), BWD_PTR, BWD_LD, BWD_DIM),
            ("sdmi_attn_bwd_fused", L.sdmi_attn_bwd_fused, p.args_bwd((AM._ptr(ws.window(0, 1)), need)), FUS_PTR, FUS_LD,
             FUS_DIM))


def _outputs_untouched(p, ws):
    bufs = [p.obuf[0], p.lse_buf, p.delta_buf, ws] + [b for b, _ in p.grads]
    return all(b.outside_untouched([]) for b in bufs) and p.guards_ok(backward=False) is None


def _rejected(L, fn, args, want, p, ws, tag):
    rc, ops = AM.recorded(L, lambda: fn(*args, _stream()))
    assert rc == want, f"{tag}: returned {rc}, expected {want}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert _outputs_untouched(p, ws), f"{tag}: a rejected call changed an output"


def test_error_returns_launch_nothing():
    """-1 for a non-positive dimension, -2 for d = 12 and d = 72, for a row stride that is no multiple of 8 and for a
    base pointer that is not 16-byte aligned, -3 for a missing or one-byte-short fused workspace with 3 key blocks;
    ws_bytes = 0 with one key block succeeds. Every rejected call returns before any launch (the recorded plan is
    empty) and leaves the NaN-filled outputs untouched."""
    L = _L()
    row = next(r for r in AM.ROWS if r.entry == AM.FUSED and (r.d, r.S) == (32, 257))
    c = AM.selector_case(row.B, row.H, row.N, row.S, row.d, row.g)
    p = AM.Problem(c, AM.PACKED)
    need = L.sdmi_attn_bwd_workspace(*p.dims)
    assert need == 3 * row.B * row.H * row.N * row.d * 4
    ws = AM.Buf(1, need // 4, torch.float32, "cuda", tail=64)
    for name, fn, args, ptrs, lds, dims in _entry_points(L, p, ws, need):
        for i in dims:
            for bad in (0, -1):
                a = list(args)
                a[i] = bad
                _rejected(L, fn, a, -1, p, ws, f"{name} argument {i} = {bad}")
        for bad in (12, 72):
            a = list(args)
            a[dims[-1]] = bad
            _rejected(L, fn, a, -2, p, ws, f"{name} d = {bad}")
        for i in lds:
            a = list(args)
            a[i] += 4
            _rejected(L, fn, a, -2, p, ws, f"{name} row stride {i} + 4")
        for i in ptrs:
            a = list(args)
            a[i] = ctypes.c_void_p(a[i].value + 8)
            _rejected(L, fn, a, -2, p, ws, f"{name} pointer {i} + 8 bytes")
    name, fn, args = _entry_points(L, p, ws, need)[2][:3]
    a = list(args)
    a[12] = None
    _rejected(L, fn, a, -3, p, ws, "fused: null workspace with 3 key blocks")
    a = list(args)
    a[13] = need - 1
    _rejected(L, fn, a, -3, p, ws, "fused: workspace one byte short")
    # one key block: no workspace needed
    row1 = next(r for r in AM.ROWS if r.entry == AM.FUSED and (r.d, r.S) == (32, 77))
    c1 = AM.selector_case(row1.B, row1.H, row1.N, row1.S, row1.d, row1.g)
    assert L.sdmi_attn_bwd_workspace(row1.B, row1.H, row1.N, row1.S, row1.d) == 0
    p1 = _forward(L, c1, AM.PACKED)
    a = list(p1.args_bwd((None, 0)))
    p1.keep_forward()
    rc, ops = AM.recorded(L, lambda: L.sdmi_attn_bwd_fused(*a, _stream()))
    assert rc == 0 and AM.launches_match(ops, row1.launches), (rc, ops)
    torch.cuda.synchronize()
    _check_backward_exact(p1, AM.exact_reference(c1), "fused without a workspace")
