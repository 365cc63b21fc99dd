"""The attention test matrix cannot fall behind the kernels, and its exact data is exact (CPU only, no library call).

tests/attn_matrix.py ROWS must name every instantiation the three host entry points of csrc/attention.hip can launch
(the list is stated here by hand as well), with both fused configurations for every DT; the expected kernels follow
the launch rules restated here; and the conditions of the exactness argument hold for every row, in float64."""
import math
import re

import pytest
import torch

from tests import attn_matrix as AM

# every instantiation sdmi_attn_fwd / sdmi_attn_bwd / sdmi_attn_bwd_fused can launch: 8 forward, 4 + 2 dq, 4 + 2 dkv,
# 4 fused (+ the delta kernel, no template)
ALL = {f"attn_fwd_kernelILi{dt}ELb{ones}EE" for dt in (1, 2, 3, 4) for ones in (0, 1)}
ALL |= {f"attn_bwd_{k}_kernelILi{dt}ELi2EE" for k in ("dq", "dkv") for dt in (1, 2, 3, 4)}
ALL |= {f"attn_bwd_{k}_kernelILi{dt}ELi4EE" for k in ("dq", "dkv") for dt in (1, 2)}
ALL |= {f"attn_bwd_fused_kernelILi{dt}EE" for dt in (1, 2, 3, 4)}
ALL |= {"attn_delta_kernel"}


def test_rows_cover_every_instantiation():
    assert len(ALL) == 8 + 6 + 6 + 4 + 1
    assert AM.instantiations() == ALL
    for dt in (1, 2, 3, 4):
        fused = [r for r in AM.ROWS if r.entry == AM.FUSED and r.launches[1][0] == f"attn_bwd_fused_kernelILi{dt}EE"]
        one_block = [r for r in fused if r.S <= 128 and -(-r.N // 64) >= 3]
        many = [r for r in fused if -(-r.S // 128) == 3 and -(-r.N // 64) == 3]
        assert one_block and many, f"fused DT = {dt} needs one key block with >= 3 query tiles and 3 x 3"
    g4 = [r for r in AM.ROWS if r.entry == AM.BWD and "ELi4EE" in r.launches[0][0]]
    assert {r.d for r in g4} == {8, 16, 24, 32}
    assert any(r.N > 128 and r.S > 128 and (r.N % 256 or r.S % 256) for r in g4), "a ragged, filled 256-row block"
    assert any(r.entry == AM.BWD and r.B * r.H == 511 and "ELi2EE" in r.launches[0][0] for r in AM.ROWS)
    assert sorted({r.d for r in AM.ROWS if r.entry == AM.FWD}) == [8, 16, 24, 32, 40, 48, 56, 64]


def test_rows_are_well_formed():
    """The hand-written expectations against the launch rules, restated independently of the rows."""
    assert len({AM.row_id(r) for r in AM.ROWS}) == len(AM.ROWS)
    for r in AM.ROWS + AM.EXTRA:
        assert r.B >= 2 and r.H >= 3 and r.d % 8 == 0 and 8 <= r.d <= 64 and r.g in (2, 4), r
        dt, bh = (r.d + 15) // 16, r.B * r.H
        tmpl = [tuple(map(int, re.findall(r"L[ib](\d)E", name))) for name, _ in r.launches]
        grids = [g for _, g in r.launches]
        if r.entry == AM.FWD:
            assert tmpl == [(dt, int(r.d % 16 == 8))] and grids == [-(-r.N // 128) * bh], r
        elif r.entry == AM.BWD:
            G = 4 if r.d <= 32 and r.N <= 256 and r.S <= 256 and bh * -(-min(r.N, r.S) // 256) >= 512 else 2
            assert tmpl == [(dt, G), (dt, G)], r
            assert grids == [-(-r.N // (64 * G)) * bh, -(-r.S // (64 * G)) * bh], r
            assert "dq" in r.launches[0][0] and "dkv" in r.launches[1][0], r
        else:
            assert tmpl == [(), (dt,)] and grids == [-(-r.B * r.N * r.H // 256), -(-r.S // 128) * bh], r
    for B, H, N, S, d in AM.SOFT:
        assert B >= 2 and H >= 3 and -(-S // 64) >= 3, "the soft family needs 3 key tiles or more"
    assert {d for _, _, _, _, d in AM.SOFT} >= {24, 64}
    assert any(d <= 32 and max(N, S) <= 256 and B * H >= 512 for B, H, N, S, d in AM.SOFT), "one G = 4 soft row"


def _case(r):
    return AM.selector_case(r.B, r.H, r.N, r.S, r.d, r.g)


def _check_exactness(c, ref, tag):
    """The conditions under which the kernels' outputs equal `ref` bitwise."""
    d, g = c["d"], c["g"]
    cc = float(AM.scale32(d)) * AM.LOG2E
    for name in ("Q", "K", "V", "dO"):
        assert AM.is_bf16(c[name]), f"{tag}: {name} is not exact in bf16"
    # every value at a rounding point is representable: P (1 / g), O, dS and dV are unchanged by the bf16 conversion
    P, s = ref["P"], ref["s"]
    assert AM.is_bf16(P) and torch.equal(P.sum(-1), torch.ones_like(P.sum(-1))), tag
    assert torch.equal(AM.bf16(P @ c["V"]), P @ c["V"]), f"{tag}: O is rounded"
    delta = (c["dO"] * ref["O"]).sum(-1, keepdim=True)
    dS = P * (c["dO"] @ c["V"].transpose(-1, -2) - delta)
    assert torch.equal(AM.bf16(dS), dS) and torch.equal(dS, ref["dS"]), f"{tag}: dS is rounded"
    assert torch.equal(AM.bf16(P.transpose(-1, -2) @ c["dO"]), P.transpose(-1, -2) @ c["dO"]), f"{tag}: dV is rounded"
    # every |partial sum| is below 2^24 in units of its granularity (1 / g for products with P, 1 / g^2 with dS)
    lim = 2.0 ** 24
    assert float((P @ c["V"].abs()).max()) * g < lim and float((P.transpose(-1, -2) @ c["dO"].abs()).max()) * g < lim
    assert float((c["dO"].abs() @ c["V"].abs().transpose(-1, -2)).max()) < lim
    assert float((dS.abs() @ c["K"].abs()).max()) * g * g < lim, tag
    assert float((dS.abs().transpose(-1, -2) @ c["Q"].abs()).max()) * g * g < lim, tag
    assert float((c["Q"].abs() @ c["K"].abs().transpose(-1, -2)).max()) < lim
    # the scale and the log-sum-exp stay small enough for the fp32 statistics
    assert ref["lse_scale"] < 2.0 ** 12 and cc > 0
    return dS


@pytest.mark.parametrize("row", AM.ROWS + AM.EXTRA, ids=AM.row_id)
def test_selector_data_is_exact(row):
    c = _case(row)
    ref = AM.exact_reference(c)
    tag = AM.row_id(row)
    B, H, N, S, d, g, nb = row.B, row.H, row.N, row.S, row.d, row.g, c["nb"]
    cc = float(AM.scale32(d)) * AM.LOG2E
    assert d - nb >= 2 and bool((c["Q"][..., nb:] == 0).all()) and float(c["K"][..., nb:].abs().max()) == 2
    assert float(c["V"].abs().max()) == 2 and float(c["dO"].abs().max()) == 1
    assert int((c["dO"] != 0).sum(-1).max()) <= 4
    # batches share codes and selections, differ in V and dO; heads differ
    assert torch.equal(c["Q"][0], c["Q"][1]) and torch.equal(c["K"][0, ..., :nb], c["K"][1, ..., :nb])
    assert not torch.equal(c["V"][0], c["V"][1]) and not torch.equal(c["dO"][0], c["dO"][1])
    assert not torch.equal(c["Q"][:, 0], c["Q"][:, 1]) and not torch.equal(c["K"][:, 0], c["K"][:, 1])
    # a condition, not a measurement: every non-selected key is >= 160 binary orders below the selected ones, and
    # the maximal scores are exactly the selected group
    s = ref["s"]
    sel = c["sel_keys"][None].expand(B, H, N, S)
    top = s.amax(-1, keepdim=True)
    assert torch.equal(s == top, sel), f"{tag}: the maximal scores are not the selected group"
    gap = ((top - s) * cc)[~sel]
    assert float(gap.min()) >= 160, f"{tag}: smallest exponent gap {float(gap.min())}"
    T = -(-S // 64)
    for h, hd in enumerate(c["heads"]):
        sizes = [len(hd["groups"][j]) for j in hd["selectable"]]
        assert all(n & (n - 1) == 0 and n <= g for n in sizes), tag
        assert sorted(k for m in hd["groups"] for k in m) == list(range(S)), tag
        chosen = [hd["groups"][j] for j in set(hd["sel"].tolist())]
        first = {min(m) // 64 for m in chosen}
        # rows meet their maximum in the first key tile, in the last, and (three tiles or more) in a middle one
        assert 0 in first and T - 1 in first and (T < 3 or first - {0, T - 1}), f"{tag} head {h}: first tiles {first}"
        assert any(len({k // 64 for k in m}) > 1 for m in chosen), f"{tag}: no selected group spans 64-key tiles"
        assert S <= 128 or any(len({k // 128 for k in m}) > 1 for m in chosen), f"{tag}: no group spans key blocks"
        assert any(len(m) == g for m in chosen)
    _check_exactness(c, ref, tag)
    for name in ("dQ", "dK", "dV", "O"):
        nz = (ref[name] != 0).sum((0, 2, 3))
        assert int(nz.min()) > 0, f"{tag}: {name} is zero in a head ({nz.tolist()})"
    em = AM.emulate_with_fuzz(c)
    for name in ("O", "dV", "dQ", "dK"):
        assert torch.equal(em[name], ref[name]), f"{tag}: {name} moves under a 5e-4 relative fuzz of P"


@pytest.mark.parametrize("N,S,d,g", [(33, 77, 8, 2), (130, 257, 16, 4), (100, 200, 64, 2), (40, 77, 24, 4),
                                     (70, 128, 56, 2)])
def test_fuzz_emulation_of_the_construction(N, S, d, g):
    c = AM.selector_case(2, 3, N, S, d, g)
    ref, em = AM.exact_reference(c), AM.emulate_with_fuzz(c)
    for name in ("O", "dV", "dQ", "dK"):
        assert torch.equal(em[name], ref[name]), name
    assert int((ref["dQ"] != 0).sum()) >= 100 and int((ref["dK"] != 0).sum()) >= 100


@pytest.mark.parametrize("d", AM.SWEEP_D)
def test_uniform_data_is_exact(d):
    for N in AM.SWEEP_LENS:
        for S in AM.SWEEP_LENS:
            for zero in ("q", "k"):
                c = AM.uniform_case(2, 3, N, S, d, zero)
                tag = f"uniform N{N} S{S} d{d} {zero}"
                V = c["V"]
                assert AM.is_bf16(V) and float(V.abs().max()) <= 16, tag
                assert torch.equal(V.sum(2), S * c["m"][:, :, 0]), tag
                assert float(c["m"].abs().max()) <= 8
                assert not torch.equal(V[0], V[1]) or S == 1
                assert float((c["Q"] if zero == "q" else c["K"]).abs().max()) == 0
                if S & (S - 1):
                    continue  # the forward alone (O == m) is exact for any S
                ref = AM.exact_reference(c)
                assert torch.equal(ref["O"], c["m"]), tag
                _check_exactness(c, ref, tag)
                zero_out, live = ("dK", "dQ") if zero == "q" else ("dQ", "dK")
                assert not bool(ref[zero_out].any()), tag
                if S > 1:  # (one key: dP == delta, every gradient but dV is zero)
                    assert int((ref[live] != 0).sum((0, 2, 3)).min()) > 0, f"{tag}: {live} is zero in a head"
                assert int((ref["dV"] != 0).sum((0, 2, 3)).min()) > 0, tag


@pytest.mark.parametrize("shape", AM.SOFT, ids=str)
def test_soft_bounds_hold_for_the_rounding_points(shape):
    """A torch emulation of the kernels' rounding points (P, dS and the outputs rounded to bf16 once each) stays
    inside the soft family's componentwise bounds; no library call."""
    B, H, N, S, d = shape
    c = AM.soft_case(B, H, N, S, d)
    fw = AM.soft_forward_reference(c)
    s = float(AM.scale32(d))
    mx = (c["Q"] @ c["K"].transpose(-1, -2) * s).amax(-1, keepdim=True)
    e = torch.exp(c["Q"] @ c["K"].transpose(-1, -2) * s - mx)
    O = AM.bf16((AM.bf16(e) @ c["V"]) / AM.bf16(e).sum(-1, keepdim=True))
    assert bool(((O - fw["O"]).abs() <= fw["O_bound"] + 2.0 ** -8 * fw["O"].abs()).all())
    bw = AM.soft_backward_reference(c, fw, O)
    P = fw["P"]
    delta = (c["dO"] * O).sum(-1, keepdim=True)
    dS = AM.bf16(P * (c["dO"] @ c["V"].transpose(-1, -2) - delta))
    em = dict(dV=AM.bf16(AM.bf16(P).transpose(-1, -2) @ c["dO"]), dQ=AM.bf16(dS @ c["K"] * s),
              dK=AM.bf16(dS.transpose(-1, -2) @ c["Q"] * s))
    for name in ("dV", "dQ", "dK"):
        err, lim = (em[name] - bw[name]).abs(), bw[name + "_bound"]
        assert bool((err <= lim).all()), f"{name}: worst error / bound {float((err / lim.clamp_min(1e-300)).max())}"


def test_ones_column_lse_bound_admits_the_rounding_point():
    """The lse bound of the d % 16 == 8 forward: the emulated rounding point (row sum of bf16 P) misses the 8 fp32
    ulps of the other head dims, and stays inside the analytic bound in use, -log2(1 - 2^-9) on top of the 8 ulps."""
    ones = [s for s in AM.SOFT if s[4] % 16 == 8]
    assert ones
    for shape in ones:
        c = AM.soft_case(*shape)
        fw = AM.soft_forward_reference(c)
        err = float((AM.emulate_lse_ones(c) - fw["lse"]).abs().max())
        eight = AM.LSE_ULPS * AM.ulp32(fw["lse_scale"])
        assert eight < err <= AM.lse_bound(c["d"], fw["lse_scale"]), (shape, err, eight)
    assert AM.lse_bound(24, 1.0) == 8 * 2.0 ** -23 + AM.LSE_ONES_ROUNDING
    assert AM.lse_bound(64, 1.0) == AM.lse_bound(16, 1.0) == 8 * 2.0 ** -23
    assert 2.81e-3 < AM.LSE_ONES_ROUNDING < 2.0 ** -9 * 1.4427 * (1 + 2.0 ** -9)


def test_uniform_data_tells_a_padding_key_from_a_real_one():
    """The fault the uniform family is for, in torch: a mask that lets one zero-filled padding key through gives
    P = 1 / (S + 1); O then differs from m bitwise wherever m != 0, and lse leaves its 4 ulps."""
    for S in AM.SWEEP_LENS:
        c = AM.uniform_case(2, 3, 17, S, 8, "q")
        wrong = AM.bf16(c["V"].sum(2, keepdim=True) / (S + 1)).expand_as(c["m"])
        live = c["m"] != 0
        assert int(live.sum((0, 2, 3)).min()) > 0 and bool((wrong != c["m"])[live].all()), S
        assert math.log2(S + 1) - math.log2(S) > 100 * 4 * AM.ulp32(max(1.0, math.log2(S)))


@pytest.mark.parametrize("row", [r for r in AM.ROWS if r.entry == AM.FWD], ids=AM.row_id)
def test_selector_data_tells_a_foreign_or_a_dropped_key(row):
    """Two more of the named faults, in torch. A query that reads one key past S meets key 0 of the next batch, which
    carries the code of its own key 0: every query that selects that group ties with it and its O changes. A dropped
    member of the selected group changes O wherever the members' V rows differ."""
    c = _case(row)
    ref = AM.exact_reference(c)
    ext = dict(Q=c["Q"][:1], K=torch.cat([c["K"][0], c["K"][1][:, :1]], 1)[None],
               V=torch.cat([c["V"][0], c["V"][1][:, :1]], 1)[None])
    _, P = AM.exact_p(ext)
    hit = P[0, :, :, -1] > 0
    assert int(hit.sum()) > 0, "no query selects the group of key 0"
    assert bool((AM.bf16(P @ ext["V"])[0] != ref["O"][0]).any(-1)[hit].any())
    P = ref["P"].clone()
    first = (P > 0).double().argmax(-1, keepdim=True)
    P.scatter_(-1, first, 0.0)
    several = (ref["P"] > 0).sum(-1) > 1
    P = P / P.sum(-1, keepdim=True).clamp_min(0.25)
    moved = (AM.bf16(P @ c["V"]) != ref["O"]).any(-1)
    assert float(moved[several].double().mean()) > 0.5


def test_guard_helper_sees_one_changed_element():
    b = AM.Buf(5, 24, torch.bfloat16, "cpu")
    b.window(8, 8).fill_(1.0)
    assert b.outside_untouched([(8, 8)]) and not b.outside_untouched([(0, 8)])
    b.buf[b.front + 16] = 0.0
    assert not b.outside_untouched([(8, 8)])
    assert AM.ulp32(1.0) == 2.0 ** -23 and AM.ulp32(9.5) == 2.0 ** -20
