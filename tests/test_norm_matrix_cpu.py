"""The GroupNorm test matrix cannot fall behind the kernels, its exact data is exact and its bounds have teeth (CPU
only, no library call).

tests/norm_matrix.py ROWS must name every kernel csrc/norm.hip can launch (the list is stated here by hand as well, with
all 22 single-pass instantiations) and hold a row for every launch shape, branch and option listed below; each row's
launches follow from the restated host rules; the exact family's sums are exact in fp32; and on every soft row an fp32
emulation of the kernels' arithmetic in two summation orders stays inside the bounds while each perturbed reference
leaves them."""
import functools

import pytest
import torch

from tests import norm_matrix as NM

PAIRS = ((64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4), (512, 2), (512, 4), (1024, 2), (1024, 4), (1024, 8))
ALL = {f"gn_{d}_pass_kernelILi{nth}ELi{it}EE" for d in ("fwd", "bwd") for nth, it in PAIRS}
ALL |= {"gn_stats_kernel", "gn_apply_kernel", "gn_bwd_reduce_kernel", "gn_bwd_apply_kernel", "gn_bwd_part_kernel",
        "chan_sum_kernel", "gn_rows_sum_grouped_kernel"}
GN = (NM.FWD, NM.STATS, NM.BWD, NM.BWD_ROWS, NM.PART, NM.PART_ROWS)


def test_rows_name_every_kernel():
    assert len(ALL) == 22 + 7 and NM.PASS_SHAPES == PAIRS
    assert NM.kernels_named() == ALL


def test_rows_are_well_formed():
    """The hand-written expectations against the launch rules, restated independently of the rows."""
    assert len({NM.row_id(r) for r in NM.ROWS}) == len(NM.ROWS)
    for r in NM.ROWS:
        assert list(r.launches) == NM.expected_launches(r.entry, r.B, r.P, r.C, r.G, r.opt), NM.row_id(r)
        assert r.C % 8 == 0 and r.C % r.G == 0 and r.silu in (0, 1) and r.B >= 1 and r.P >= 1
        shapes = NM.opt(r, "jobs", ((r.B, r.P, r.C, r.G),))
        for B, P, C, G in shapes:
            # x, dy, the addend, y, dx; the tables; rows (the workspace is sized by the library)
            assert max(B * P * C, B * C * 4, B * C * 2) <= NM.CAP, NM.row_id(r)
        if r.entry in (NM.PART, NM.PART_ROWS):
            assert r.P % NM.opt(r, "rb") == 0
    for B, P, C, G in NM.COUNTER_SHAPES + (NM.COUNTER_ROW,):
        assert NM.pick_pass(B, P, C, G) is not None
    strips = [NM.cdiv(C, NM.pick_pass(B, P, C, G)[0]) for B, P, C, G in NM.COUNTER_SHAPES]
    assert len(set(strips)) == 2, "the counter test alternates two strip counts"


def test_the_restated_rules_at_known_points():
    """The rules themselves, at points worked out by hand from the comments of norm.hip."""
    assert NM.strip_width(96, 3) == 72 and NM.strip_width(64, 16) == 48 and NM.strip_width(128, 64) == 64
    assert NM.strip_width(96, 8) == 56 and NM.strip_width(40, 8) == 24 and NM.strip_width(512, 256) == 256
    assert NM.part_strip_width(384, 12) == 192 and NM.part_strip_width(288, 9) == 72
    assert NM.part_strip_width(160, 5) == 160 and NM.part_strip_width(128, 16) == 64
    assert NM.pick_psplit(2, 3, 255) == 1 and NM.pick_psplit(2, 3, 256) == 2 and NM.pick_psplit(2, 3, 8200) == 32
    assert NM.pick_psplit(2, 256, 8200) == 1 and NM.pick_psplit(600, 2, 8200) == 1
    assert NM.apply_grid(3, 127, 96) == (2, 3, 1) and NM.apply_grid(3, 128, 96) == (2, 3, 2)
    assert NM.pass_shape(1, 3) == (64, 1) and NM.pass_shape(8, 8) == (64, 1) and NM.pass_shape(1024, 8) == (1024, 8)
    assert NM.pass_shape(1025, 8) is None and NM.pass_shape(256, 32) == (1024, 8) and NM.pass_shape(257, 32) is None
    # the 512 -> 256 workgroup target at P >= 1024: 8 x 64 strips of 8 channels, or 8 x 32 of 16
    assert NM.pick_pass(8, 1023, 512, 64)[0] == 8 and NM.pick_pass(8, 1024, 512, 64)[0] == 16
    assert NM.pick_pass(3, 1, 48, 4) == (24, (64, 1)) and NM.pick_pass(3, 1030, 128, 2) is None
    assert NM.chan_segments(3, 225, True) == (3, 225) and NM.chan_segments(3, 225, False) == (10, 68)
    assert NM.chan_segments(1, 63, False) == (1, 63) and NM.chan_segments(3, 3000, False) == (32, 282)
    assert NM.part_psplit(2, 3, 127) == 1 and NM.part_psplit(2, 3, 128) == 2 and NM.part_psplit(2, 600, 4096) == 1


def _single():
    """(row, strip width, NTH, IT, lanes L, rows per pass R, strips) of the single-pass rows."""
    out = []
    for r in NM.ROWS:
        if r.entry in (NM.FWD, NM.BWD) and NM.pick_pass(r.B, r.P, r.C, r.G) is not None:
            cw, (nth, it) = NM.pick_pass(r.B, r.P, r.C, r.G)
            out.append((r, cw, nth, it, cw // 8, nth // (cw // 8), NM.cdiv(r.C, cw)))
    return out


def _need(found, what):
    assert found, f"ROWS has no row for: {what}"


@pytest.mark.parametrize("entry", (NM.FWD, NM.BWD))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_single_pass_pair_is_covered(pair, entry):
    """Per (NTH, IT) and direction: a full slab, a ragged slab and idle tail threads, each on B >= 3, two strips or
    more, two groups per strip or more."""
    mine = [s for s in _single() if (s[2], s[3]) == pair and s[0].entry == entry and s[0].B >= 3 and s[6] >= 2 and
            s[1] // (s[0].C // s[0].G) >= 2]
    _need([s for s in mine if s[0].P == s[3] * s[5]], f"{entry} {pair} full slab (P == IT * R)")
    _need([s for s in mine if s[0].P < s[3] * s[5]], f"{entry} {pair} ragged slab (P < IT * R)")
    _need([s for s in mine if s[2] % s[4]], f"{entry} {pair} idle tail threads (L does not divide NTH)")
    _need({s[0].silu for s in mine} == {0, 1}, f"{entry} {pair} with and without SiLU")


def test_single_pass_branches_are_covered():
    S = _single()
    for entry in (NM.FWD, NM.BWD):
        E = [s for s in S if s[0].entry == entry]
        seg = lambda s: max(1, min(s[5], s[2] // s[1]))  # noqa: E731  small_reduce: segments per channel
        _need([s for s in E if seg(s) == 1], f"{entry}: small_reduce with one segment per channel")
        _need([s for s in E if seg(s) > 1], f"{entry}: small_reduce with several segments")
        _need([s for s in E if s[0].C % s[1]], f"{entry}: a ragged last strip")
        _need([s for s in E if s[0].C == s[0].G], f"{entry}: one channel per group")
        _need([s for s in E if s[0].P == 1], f"{entry}: a single pixel row")
        _need([s for s in E if s[2] % s[4] == 0], f"{entry}: L divides NTH")
        target = lambda s: 256 if s[0].P >= 1024 else 512  # noqa: E731
        u = lambda s: [w for w in range(8, 257, 8) if w % (s[0].C // s[0].G) == 0][0]  # noqa: E731
        _need([s for s in E if s[6] * s[0].B >= target(s) and s[1] > u(s)],
              f"{entry}: the wg >= target branch of pick_pass (a strip wider than the narrowest)")
        _need([s for s in E if s[6] * s[0].B >= 512 and s[2] == 64 and s[1] == 256],
              f"{entry}: 64 threads on 256-channel strips")
    B = [s for s in S if s[0].entry == NM.BWD]
    nthr = lambda s: min(s[2], 256)  # noqa: E731  batch_tail
    nbg = lambda s: max(1, nthr(s) // s[1])  # noqa: E731
    _need([s for s in B if s[3] <= 4], "backward keeping dz (IT <= 4)")
    _need([s for s in B if (s[2], s[3]) == (1024, 8)], "backward re-reading dy (1024 x 8)")
    _need([s for s in B if s[1] > nthr(s) and s[2] == 64 and s[1] >= 72], "batch_tail: strip wider than the workgroup")
    _need([s for s in B if s[1] > nthr(s) and s[0].B > 16], "batch_tail: narrow workgroup, more than 16 batch rows")
    _need([s for s in B if s[1] <= nthr(s) and nbg(s) == 1], "batch_tail: nbg == 1")
    _need([s for s in B if s[1] <= nthr(s) and nbg(s) >= 2], "batch_tail: nbg >= 2")
    _need([s for s in B if s[1] <= nthr(s) and nbg(s) == 1 and s[0].B > 16], "batch_tail: nbg == 1, B > 16")
    _need([s for s in B if s[1] <= nthr(s) and nbg(s) >= 2 and s[0].B > 16 * nbg(s)],
          "batch_tail: nbg >= 2, B > 16 nbg")


def _multi(r):
    """(strip width, strips, pixel splits, apply pixel splits) of a multi-pass row."""
    cw = NM.strip_width(r.C, r.C // r.G)
    nch = NM.cdiv(r.C, cw)
    return cw, nch, NM.pick_psplit(nch, r.B, r.P), NM.apply_grid(r.B, r.P, r.C)[2]


def test_multi_pass_is_covered():
    short_last = lambda r, ps: ps > 1 and r.P - (ps - 1) * NM.cdiv(r.P, ps) < NM.cdiv(r.P, ps)  # noqa: E731
    stats = [r for r in NM.ROWS if r.entry == NM.STATS]
    assert {_multi(r)[2] for r in stats} >= {1, 2, 8, 32}, "sdmi_gn_stats with 1, 2, 8 and 32 pixel splits"
    _need([r for r in stats if _multi(r)[3] == 1], "gn_apply_kernel without pixel splits")
    _need([r for r in stats if _multi(r)[3] > 1], "gn_apply_kernel with pixel splits")
    _need([r for r in stats if r.C % _multi(r)[0]], "gn_stats_kernel with a ragged last strip")
    _need({r.silu for r in stats} == {0, 1}, "sdmi_gn_apply with and without SiLU")
    for entry, first, splits in ((NM.FWD, "gn_stats_kernel", {2, 8}), (NM.BWD, "gn_bwd_reduce_kernel", {2, 8, 32})):
        multi = [r for r in NM.ROWS if r.entry == entry and NM.pick_pass(r.B, r.P, r.C, r.G) is None]
        assert all(r.launches[0][0] == first for r in multi)
        assert {_multi(r)[2] for r in multi} >= splits, f"{entry}: multi-pass with {splits} pixel splits"
        _need([r for r in multi if short_last(r, _multi(r)[2])], f"{entry}: a last pixel range shorter than the others")
        _need({r.silu for r in multi} == {0, 1}, f"{entry}: multi-pass with and without SiLU")
    _need([r for r in stats if short_last(r, _multi(r)[2])], "gn_stats_kernel: a short last pixel range")
    # the exact family compares a single-pass table bitwise with that of sdmi_gn_stats on the same shape
    single = [r for r in NM.ROWS if r.entry == NM.FWD and NM.pick_pass(r.B, r.P, r.C, r.G) is not None]
    assert {_multi(r)[2] for r in single} >= {1, 2, 8, 32}, "single-pass shapes whose sdmi_gn_stats splits 1, 2, 8, 32"
    _need([r for r in NM.ROWS if r.entry == NM.BWD and r.launches[0][0] == "gn_bwd_reduce_kernel" and
           r.C % _multi(r)[0]], "gn_bwd_reduce_kernel with a ragged last strip")


def test_part_rows_are_covered():
    part = [r for r in NM.ROWS if r.entry in (NM.PART, NM.PART_ROWS)]
    width = lambda r: NM.part_strip_width(r.C, r.C // r.G)  # noqa: E731
    lanes = lambda r: min(256 // (width(r) // 2), 4)  # noqa: E731
    ps = lambda r: NM.part_psplit(NM.cdiv(r.C, width(r)), r.B, r.P)  # noqa: E731
    assert {width(r) for r in part if r.entry == NM.PART} >= {64, 128, 192, 256}
    _need([r for r in part if width(r) % 64 and width(r) == r.C], "part: the whole row as one strip")
    _need([r for r in part if width(r) % 64 and width(r) < r.C and width(r) == NM.strip_width(r.C, r.C // r.G)],
          "part: the strip_width fallback")
    assert {lanes(r) for r in part} == {2, 3, 4}, "part_sums with 4, 3 and 2 segment lanes"
    assert {NM.opt(r, "rb") for r in part} == {16, 64}
    _need([r for r in part if ps(r) == 1], "part: one pixel split")
    _need([r for r in part if ps(r) > 1], "part: several pixel splits")
    _need([r for r in part if r.entry == NM.PART_ROWS], "sdmi_gn_bwd_part_rows")
    _need({r.silu for r in part} == {0, 1}, "part with and without SiLU")
    _need([r for r in part if NM.cdiv(r.C, width(r)) >= 2 and width(r) // (r.C // r.G) >= 2],
          "part: 2 strips of 2 groups")


def test_chan_sum_and_deferred_rows_are_covered():
    chan = [r for r in NM.ROWS if r.entry == NM.CHAN]

    def geo(r):
        nb, seg = NM.chan_segments(r.B, r.P, NM.opt(r, "mode") == "bc")
        nch = NM.cdiv(r.C, NM.strip_width(r.C, 8))
        return nb, seg, NM.pick_psplit(nch, nb, seg)
    for mode in ("bc", "seg"):
        mine = [r for r in chan if NM.opt(r, "mode") == mode]
        _need([r for r in mine if geo(r)[2] == 1], f"chan_sum {mode}: one pixel split")
        _need([r for r in mine if geo(r)[2] > 1], f"chan_sum {mode}: several pixel splits")
    _need([r for r in chan if NM.opt(r, "mode") == "seg" and r.B * r.P % geo(r)[1]], "chan_sum: a ragged last segment")
    _need([r for r in chan if NM.opt(r, "mode") == "seg" and geo(r)[0] > 16], "chan_sum: more than 16 segments")
    _need([r for r in chan if NM.opt(r, "per_c2")], "chan_sum: the second output")
    _need([r for r in chan if not NM.opt(r, "per_c2")], "chan_sum: without the second output")
    _need([r for r in chan if NM.opt(r, "c_store") < r.C], "chan_sum: c_store < C")
    _need([r for r in chan if r.C % NM.strip_width(r.C, 8)], "chan_sum: a ragged last strip")
    rows = [r for r in NM.ROWS if r.entry == NM.BWD_ROWS]
    _need([r for r in rows if NM.pick_pass(r.B, r.P, r.C, r.G) is not None], "sdmi_gn_bwd_rows, single pass")
    _need([r for r in rows if NM.pick_pass(r.B, r.P, r.C, r.G) is None], "sdmi_gn_bwd_rows, multi-pass")
    _need([r for r in rows if r.C > 256 and r.C % 256 == 0], "sdmi_gn_rows_sum: two full workgroups")
    _need([r for r in rows if r.C % 256], "sdmi_gn_rows_sum: C no multiple of 256")
    grouped = [r for r in NM.ROWS if r.entry == NM.GROUPED]
    _need(grouped, "sdmi_gn_rows_sum_grouped")
    for r in grouped:
        jobs = NM.opt(r, "jobs")
        assert len(jobs) >= 3 and len({j[2] for j in jobs}) == len(jobs) and all(j[2] % 256 for j in jobs)
        assert jobs[0] == (r.B, r.P, r.C, r.G) and len({j[0] for j in jobs}) > 1
        assert max(j[2] for j in jobs) > 256 > min(j[2] for j in jobs), "a job that ends inside the first workgroup"


def _coverage_checks():
    yield test_rows_name_every_kernel
    for entry in (NM.FWD, NM.BWD):
        for pair in PAIRS:
            yield lambda pair=pair, entry=entry: test_single_pass_pair_is_covered(pair, entry)
    yield test_single_pass_branches_are_covered
    yield test_multi_pass_is_covered
    yield test_part_rows_are_covered
    yield test_chan_sum_and_deferred_rows_are_covered


def _noticed():
    for check in _coverage_checks():
        try:
            check()
        except AssertionError:
            return True
    return False


def test_no_row_and_no_kernel_can_be_deleted(monkeypatch):
    """The coverage tests above have teeth: with any single row taken out of ROWS, or all rows that name one kernel,
    one of them fails (on the test data; the kernels are not touched)."""
    full = list(NM.ROWS)
    assert not _noticed()
    for r in full:
        monkeypatch.setattr(NM, "ROWS", [x for x in full if x is not r])
        assert _noticed(), f"ROWS without {NM.row_id(r)} passes every coverage test"
    for name in sorted(ALL):
        monkeypatch.setattr(NM, "ROWS", [x for x in full if all(n != name for n, _ in x.launches)])
        assert _noticed(), f"ROWS without {name} passes every coverage test"


# ----------------------------------------------------------------------------------------------------------------
# the data
# ----------------------------------------------------------------------------------------------------------------
def _shapes(entries=GN):
    seen = {}
    for r in NM.ROWS:
        for s in (NM.opt(r, "jobs", ((r.B, r.P, r.C, r.G),)) if r.entry in entries + (NM.GROUPED,) else ()):
            seen.setdefault(s, None)
    return list(seen)


@pytest.mark.parametrize("shape", _shapes() + [NM.COUNTER_ROW], ids=str)
def test_exact_family_is_exact(shape):
    B, P, C, G = shape
    c = NM.exact_case(B, P, C, G)
    Cg = C // G
    for name in ("x", "dy", "add", "gamma", "beta"):
        assert NM.is_bf16(c[name]), f"{name} is not exact in bf16"
    assert float(c["x"].abs().max()) <= 8 and float(c["dy"].abs().max()) <= 4 and float(c["add"].abs().max()) <= 4
    assert bool((torch.log2(c["gamma"].abs()) % 1 == 0).all()) and bool(((c["beta"] * 8) % 1 == 0).all())
    # every partial sum a kernel can form, in units of the channel's granularity, stays below 2^24
    x = c["x"]
    gran = torch.where(((x % 1) != 0).any(1), 2.0 ** -7, 1.0)   # [B][C]
    assert bool(((x / gran[:, None]) % 1 == 0).all())
    assert float((x.abs().sum(1) / gran).max()) < 2 ** 24 and float(((x * x).sum(1) / gran ** 2).max()) < 2 ** 24
    assert float(c["dy"].abs().sum((0, 1)).max()) < 2 ** 24
    # the special groups
    assert c["const"] and (c["near"] or P * Cg < 2)
    st, st6 = NM.group_stats(x, G), NM.group_stats(x, G, eps=1e-6)
    for b, g in c["const"]:
        assert float(st["var"][b, g]) == 0.0 and float(st["mean"][b, g]) == 3.0
    for b, g in c["near"]:
        assert 0.0 < float(st["var"][b, g]) <= 1.6e-5
        assert float(st6["rstd"][b, g] / st["rstd"][b, g]) > 1.2, "eps does not decide this group's rstd"
    special = set(c["const"]) | set(c["near"])
    assert len(special) < B * G, "no ordinary group left"
    # the fp32 emulation gives one table in both orders, within 1 ulp of float64, and the exact dbeta
    t1, _ = NM.emulate_forward(c, 0, "seq")
    t2, _ = NM.emulate_forward(c, 0, "pair")
    assert torch.equal(t1, t2)
    bad, _ = NM.check_table(c, t1, st)
    assert bad is None, bad
    for order in ("seq", "pair"):
        em = NM.emulate_backward(c, t1, 0, order, False)
        assert torch.equal(em["dbeta"], c["dy"].sum((0, 1))) and torch.equal(em["S1"], c["dy"].sum(1))


# ----------------------------------------------------------------------------------------------------------------
# the bounds
# ----------------------------------------------------------------------------------------------------------------
def _ratio(err, lim):
    return float((err / lim.clamp_min(1e-300)).max())


def _violates(pert, ref, lim):
    return bool(((pert - ref).abs() > lim).any())


@functools.lru_cache(maxsize=None)
def _measure(shape, silu):
    """Emulated error / (u T) of every backward quantity, the larger of the two orders; and the forward checks."""
    B, P, C, G = shape
    c = NM.soft_case(B, P, C, G)
    st = NM.group_stats(c["x"], G)
    out = dict(dx=0.0, dgamma=0.0, dbeta=0.0, S=0.0, table=0.0, y=0.0)
    for order in ("seq", "pair"):
        tab, y32 = NM.emulate_forward(c, silu, order)
        bad, _ = NM.check_table(c, tab, st)
        assert bad is None, f"{order}: emulated table: {bad}"
        out["table"] = max(out["table"], NM.check_table(c, tab, st, K=1.0)[1])
        ref, lim = NM.y_reference(c, tab, silu)
        out["y"] = max(out["y"], _ratio((NM.bf16(y32) - ref).abs(), lim))
        bw = NM.bwd_reference(c, tab, silu)
        for addend in (False, True):
            em = NM.emulate_backward(c, tab, silu, order, addend)
            ref, _ = NM.dx_reference(c, bw, addend)
            T = bw["T_dx"] + (c["add"].abs() if addend else 0.0)
            out["dx"] = max(out["dx"], _ratio((em["dx"] - ref).abs(), NM.U24 * T))
            assert bool(((NM.bf16(em["dx"]) - ref).abs() <= NM.dx_reference(c, bw, addend)[1]).all())
        out["dgamma"] = max(out["dgamma"], _ratio((em["dgamma"] - bw["dgamma"]).abs(), NM.U24 * bw["T_dgamma"]))
        out["dbeta"] = max(out["dbeta"], _ratio((em["dbeta"] - bw["dbeta"]).abs(), NM.U24 * bw["T_dbeta"]))
        out["S"] = max(out["S"], _ratio((em["S1"] - bw["S1"]).abs(), NM.U24 * bw["T_S1"]),
                       _ratio((em["S2"] - bw["S2"]).abs(), NM.U24 * bw["T_S2"]))
    return out


def _soft_shapes():
    seen = {}
    for r in NM.ROWS:
        if r.entry in GN + (NM.GROUPED,):
            for s in NM.opt(r, "jobs", ((r.B, r.P, r.C, r.G),)):
                seen.setdefault((s, r.silu), None)
    return list(seen)


@pytest.mark.parametrize("shape,silu", _soft_shapes(), ids=str)
def test_soft_bounds_admit_the_rounding_points_and_nothing_else(shape, silu):
    """The fp32 emulation in both summation orders stays at or below every bound on every element (the sums within
    K_SUM / 2: the constant is twice the emulated ratio); every perturbed reference leaves a bound somewhere."""
    B, P, C, G = shape
    m = _measure(shape, silu)
    print(f"{shape} silu {silu}: emulated error / bound: y {m['y']:.3f}; error / (u T): table {m['table']:.3f}, "
          f"dx {m['dx']:.3f}, dgamma {m['dgamma']:.3f}, dbeta {m['dbeta']:.3f}, S1 / S2 {m['S']:.3f}")
    assert m["y"] <= 1.0
    assert max(m["dx"], m["dgamma"], m["dbeta"], m["S"], m["table"]) <= NM.K_SUM / 2
    c = NM.soft_case(B, P, C, G)
    x = c["x"]
    st = NM.group_stats(x, G)
    bm, br = NM.table_bounds(c, st)
    twice, without = torch.ones(P), torch.ones(P)
    twice[P - 1], without[P - 1] = 2.0, 0.0
    for what, pert in (("the last pixel row counted twice", NM.group_stats(x, G, weights=twice)),
                       ("the last pixel row omitted", NM.group_stats(x, G, weights=without)),
                       ("eps = 1e-6", NM.group_stats(x, G, eps=1e-6)),
                       ("n - 1 in the variance", NM.group_stats(x, G, ddof=1))):
        assert _violates(pert["mean"], st["mean"], bm) or _violates(pert["rstd"], st["rstd"], br), \
            f"{what} passes the table bound"
    # a wrong table that slipped through would also show in y, at the issue's own bound
    tab = NM.table_of(st["mean"], st["rstd"], c["gamma"], c["beta"]).float().double()
    ref, lim = NM.y_reference(c, tab, silu)
    for what, w in (("twice", twice), ("omitted", without)):
        p = NM.group_stats(x, G, weights=w)
        pert, _ = NM.y_reference(c, NM.table_of(p["mean"], p["rstd"], c["gamma"], c["beta"]), silu)
        assert _violates(pert, ref, lim), f"y: the last pixel row {what} passes"
    bw = NM.bwd_reference(c, tab, silu)
    for b in {0, B - 1}:
        assert _violates(bw["dgamma"] - bw["S2"][b], bw["dgamma"], NM.sum_bound(bw["T_dgamma"])), "dgamma: a batch row"
        assert _violates(bw["dbeta"] - bw["S1"][b], bw["dbeta"], NM.sum_bound(bw["T_dbeta"])), "dbeta: a batch row"
    dz, dzx = NM.dz_terms(c, tab, silu)   # the last pixel row missing from the backward sums, in every batch row
    assert bool(((dzx[:, -1].abs() > NM.sum_bound(bw["T_S2"])).any(1)).all()), "S2 without a pixel row passes"
    for b, g in c["loud"]:   # also inside the large-mean group, whose |x a| and |s| must not widen the bound
        ch = slice(g * (C // G), (g + 1) * (C // G))
        assert bool((dzx[b, -1, ch].abs() > NM.sum_bound(bw["T_S2"])[b, ch]).any()), "S2 of the large-mean group"
    assert _violates(bw["dgamma"] - dzx[:, -1].sum(0), bw["dgamma"], NM.sum_bound(bw["T_dgamma"])), \
        "dgamma: a pixel row"
    assert _violates(bw["dbeta"] - dz[:, -1].sum(0), bw["dbeta"], NM.sum_bound(bw["T_dbeta"])), "dbeta: a pixel row"
    for addend in (False, True):
        ref, lim = NM.dx_reference(c, bw, addend)
        assert _violates(NM.dx_reference(c, bw, addend, drop_qx=True)[0], ref, lim), "dx without q x passes"
        if silu:
            wrong = NM.dx_reference(c, NM.bwd_reference(c, tab, silu, sigmoid_only=True), addend)[0]
            assert _violates(wrong, ref, lim), "dx with the sigmoid for silu' passes"


def test_the_constant_is_twice_the_emulated_ratio():
    """K_SUM is twice the largest emulated ratio over all soft rows, rounded up: not more than 3 times."""
    worst = max(max(m["dx"], m["dgamma"], m["dbeta"], m["S"], m["table"]) for m in
                (_measure(s, silu) for s, silu in _soft_shapes()))
    print(f"largest emulated error / (u T): {worst:.3f}; K_SUM {NM.K_SUM}")
    assert 2 * worst <= NM.K_SUM <= 3 * worst


@pytest.mark.parametrize("row", [r for r in NM.ROWS if r.entry == NM.CHAN], ids=NM.row_id)
def test_chan_sum_bounds(row):
    c = NM.soft_case(row.B, row.P, row.C, row.G)
    ref = NM.chan_reference(c, row.B, row.P, row.C)
    dy = c["dy"].float()
    for order in ("seq", "pair"):
        bc = NM.sum32(dy, 1, order)
        assert _ratio((bc.double() - ref["per_bc"]).abs(), NM.U24 * ref["T_bc"]) <= NM.K_SUM / 2
        assert _ratio((NM.sum32(bc, 0, order).double() - ref["per_c"]).abs(), NM.U24 * ref["T_c"]) <= NM.K_SUM / 2
        assert not _violates(NM.bf16(bc.double()), ref["per_bc"], NM.sum_bound(ref["T_bc"], True, ref["per_bc"]))
    last = c["dy"][-1, -1]
    assert _violates(ref["per_c"] + last, ref["per_c"], NM.sum_bound(ref["T_c"]))
    assert _violates(ref["per_c"] - last, ref["per_c"], NM.sum_bound(ref["T_c"]))
    wrong = ref["per_bc"].clone()
    wrong[-1] += last
    assert _violates(NM.bf16(wrong), ref["per_bc"], NM.sum_bound(ref["T_bc"], True, ref["per_bc"]))
    e = NM.exact_case(row.B, row.P, row.C, row.G)
    for order in ("seq", "pair"):
        assert torch.equal(NM.sum32(NM.sum32(e["dy"].float(), 1, order), 0, order).double(), e["dy"].sum((0, 1)))


def test_guard_sees_one_changed_element():
    f = NM.Flat(10, "cpu")
    b = NM.Buf(5, 24, torch.bfloat16, "cpu")
    b.col0 = 8
    g = NM.Guard()
    g.add("flat", f, [(0, 4)])
    g.add("buf", b, [("w", 8, 8)])
    f.data[:4] = 1.0
    b.window(8, 8).fill_(2.0)
    assert g.changed() is None
    f.data[4] = 0.0
    assert g.changed() == "flat"
    b.buf[b.front + 16] = 0.0
    assert g.changed() == "flat, buf"
    x = torch.tensor([1.0, 9.5, -0.75], dtype=torch.float64)
    assert NM.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -20, 2.0 ** -24]
