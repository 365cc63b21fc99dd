"""Every GroupNorm and channel-sum kernel and launch shape of csrc/norm.hip (tests/norm_matrix.py ROWS), exact, guarded.

Every row runs on the exact-sum family (silu = 0) and on the soft family (the row's silu), with contiguous operands and
with operands that are column windows (ld = C + 8 .. C + 32, different column offsets) of NaN-filled buffers; the fp32
outputs and the workspace are NaN-guarded too. The recorded launch plan must name the row's kernels and grids. After
every call nothing but the logical output windows and the first sdmi_chan_reduce_workspace bytes of the workspace may
have changed, bit for bit -- inputs included -- and a second identical call must reproduce every output bit.

Exact family: the forward table is one bit pattern per shape (single pass, sdmi_gn_stats at its pixel split -- 1, 2,
8 and 32 splits over the single-pass rows -- and both layouts), mean and rstd within 1 fp32 ulp of float64, a == rstd
gamma; dbeta (inline tail, deferred rows, grouped rows, part path), rows[..][0] and the channel sums are the exact
integers. Both families, every element: the componentwise bounds of tests/norm_matrix.py (y, dx, dx + addend, dgamma,
dbeta, rows), with the kernel's own table once it has passed the table check. Each test prints its worst error / bound.

Also the 2048 counter slots across more launches than slots, and the error returns (nothing launched, nothing written).
Not expressible through the C ABI, hence absent: `rows` together with dgamma (the rows entry points take no dgamma)."""
import ctypes

import pytest
import torch

from tests import norm_matrix as NM

pytestmark = pytest.mark.gpu

LAYOUTS = (NM.CONTIGUOUS, NM.WINDOWS)
FAMILIES = ("exact", "soft")
FORWARD = [r for r in NM.ROWS if r.entry in (NM.FWD, NM.STATS)]
BACKWARD = [r for r in NM.ROWS if r.entry in (NM.BWD, NM.BWD_ROWS, NM.PART, NM.PART_ROWS)]
CHAN = [r for r in NM.ROWS if r.entry == NM.CHAN]
GROUPED = [r for r in NM.ROWS if r.entry == NM.GROUPED]


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    """`call` (a tuple of thunks returning a status) recorded as one plan: every status 0, the launches the row's."""
    def all_of():
        for f in call:
            rc = f()
            if rc:
                return rc
        return 0
    rc, ops = NM.recorded(L, all_of)
    assert rc == 0, f"{tag}: returned {rc}"
    if want is not None:
        assert NM.launches_match(ops, want), f"{tag}: launched {ops}, the matrix says {list(want)}"
    torch.cuda.synchronize()


def _worst(err, lim):
    return float((err / lim.clamp_min(1e-300)).max())


def _within(got, ref, lim, what, tag, seen):
    err = (got - ref).abs()
    assert not bool(torch.isnan(got).any()), f"{tag}: {what} holds NaN"
    w = _worst(err, lim)
    seen[what] = max(seen.get(what, 0.0), w)
    assert bool((err <= lim).all()), f"{tag}: {what} worst error / bound {w:.3f}"


def _silu(row, kind):
    return 0 if kind == "exact" else row.silu


def _report(row, kind, seen):
    print(f"{NM.row_id(row)} {kind}: max(err / bound) " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(seen.items())))


def _table(p, c, st, tag, seen):
    B, P, C, G = p.dims
    tab = p.table.get(B, C, 4)
    bad, worst = NM.check_table(c, tab, st)
    assert bad is None, f"{tag}: table: {bad}"
    seen["table"] = max(seen.get("table", 0.0), worst)
    return tab


def _bits_of(p, names):
    out = []
    for n in names:
        t = p.bufs[n].buf if n in p.bufs else getattr(p, n).buf
        out.append(NM.bits(t).clone())
    return out


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("row", FORWARD, ids=NM.row_id)
def test_forward_rows(row):
    L = _L()
    B, P, C, G = row.B, row.P, row.C, row.G
    single = row.entry == NM.FWD and NM.pick_pass(B, P, C, G) is not None
    for kind in FAMILIES:
        silu, c, seen, tables = _silu(row, kind), NM.case_of(kind, B, P, C, G), {}, []
        st = NM.group_stats(c["x"], G)
        for layout in LAYOUTS:
            tag = f"{NM.row_id(row)} {kind} {layout}"
            p = NM.Problem(c, layout, L)
            call = (lambda: p.fwd(silu, _stream()),) if row.entry == NM.FWD else \
                (lambda: p.stats(_stream()), lambda: p.apply(silu, _stream()))
            g = p.guard({"y", "table", "ws"})
            _run(L, call, row.launches, tag)
            bad = g.changed()
            assert bad is None, f"{tag}: changed outside the outputs: {bad}"
            tab = _table(p, c, st, tag, seen)
            ref, lim = NM.y_reference(c, tab, silu)
            _within(p.out("y"), ref, lim, "y", tag, seen)
            first = _bits_of(p, ("y", "table"))
            _run(L, call, row.launches, tag + " again")
            assert _same_bits(first, _bits_of(p, ("y", "table"))), f"{tag}: a second call gives other bits"
            tables.append(tab)
            if kind == "exact" and single:
                g = p.guard({"table", "ws"})
                _run(L, (lambda: p.stats(_stream()),), None, tag + " stats")
                assert g.changed() is None, f"{tag}: sdmi_gn_stats changed {g.changed()}"
                assert torch.equal(p.table.get(B, C, 4), tab), f"{tag}: sdmi_gn_stats gives another table"
        if kind == "exact":
            assert torch.equal(tables[0], tables[1]), f"{NM.row_id(row)}: the table differs between layouts"
            for b, gi in c["const"]:
                assert float(tables[0][b, gi * (C // G), 2]) == 3.0, "the constant group's mean"
        _report(row, kind, seen)


# (addend, dx aliases dy, dgamma / dbeta given)
VARIANTS = ((False, False, True), (True, False, True), (False, True, True), (False, False, False))
ROWS_VARIANTS = ((False, False, True), (True, True, True))


def _check_backward(row, kind, p, c, bw, addend, sums, tag, seen):
    B, P, C, G = p.dims
    ref, lim = NM.dx_reference(c, bw, addend)
    _within(p.out("dx"), ref, lim, "dx + addend" if addend else "dx", tag, seen)
    rows_entry = row.entry in (NM.BWD_ROWS, NM.PART_ROWS, NM.GROUPED)
    if rows_entry:
        rows = p.rows.get(B, C, 2)
        _within(rows[..., 0], bw["S1"], NM.sum_bound(bw["T_S1"]), "rows S1", tag, seen)
        _within(rows[..., 1], bw["S2"], NM.sum_bound(bw["T_S2"]), "rows S2", tag, seen)
        if kind == "exact":
            assert torch.equal(rows[..., 0], c["dy"].sum(1)), f"{tag}: rows[..][0] is not the exact sum"
    if sums or rows_entry:
        dg, db = p.dgamma.get(C), p.dbeta.get(C)
        _within(dg, bw["dgamma"], NM.sum_bound(bw["T_dgamma"]), "dgamma", tag, seen)
        _within(db, bw["dbeta"], NM.sum_bound(bw["T_dbeta"]), "dbeta", tag, seen)
        if kind == "exact":
            assert torch.equal(db, c["dy"].sum((0, 1))), f"{tag}: dbeta is not the exact integer sum"


@pytest.mark.parametrize("row", BACKWARD, ids=NM.row_id)
def test_backward_rows(row):
    L = _L()
    B, P, C, G = row.B, row.P, row.C, row.G
    rb = NM.opt(row, "rb")
    from_part = row.entry in (NM.PART, NM.PART_ROWS)
    deferred = row.entry in (NM.BWD_ROWS, NM.PART_ROWS)
    for kind in FAMILIES:
        silu, c, seen = _silu(row, kind), NM.case_of(kind, B, P, C, G), {}
        st = NM.group_stats(c["x"], G)
        known = None   # (table, reference, partials): one reference per distinct table
        for layout in LAYOUTS:
            for addend, alias, sums in (ROWS_VARIANTS if deferred else VARIANTS):
                tag = f"{NM.row_id(row)} {kind} {layout} addend={addend} alias={alias} sums={sums}"
                p = NM.Problem(c, layout, L, alias_dx=alias)
                _run(L, (lambda: p.fwd(silu, _stream()),), None, tag + " forward")
                tab = _table(p, c, st, tag, seen)
                if known is None or not torch.equal(known[0], tab):
                    if from_part:
                        part = NM.host_partials(NM.dz_terms(c, tab, silu), rb)
                        known = (tab, NM.bwd_reference_from_partials(c, tab, silu, part), part)
                    else:
                        known = (tab, NM.bwd_reference(c, tab, silu), None)
                bw = known[1]
                pf = NM.Flat(B * (P // rb) * C * 2, "cuda").put(known[2]) if from_part else None
                s = _stream()
                if row.entry == NM.BWD:
                    call = (lambda: p.bwd(silu, s, addend, sums),)
                elif row.entry == NM.BWD_ROWS:
                    call = (lambda: p.bwd_rows(silu, s, addend), lambda: p.rows_sum(s))
                elif row.entry == NM.PART:
                    call = (lambda: p.bwd_part(silu, pf.data, rb, s, addend, sums),)
                else:
                    call = (lambda: p.bwd_part_rows(silu, pf.data, rb, s, addend), lambda: p.rows_sum(s))
                outputs = {"dx", "ws"} | ({"rows", "dgamma", "dbeta"} if deferred else set()) | \
                    ({"dgamma", "dbeta"} if sums else set()) | (set() if from_part else {"table2"})
                g = p.guard(outputs)
                if pf is not None:
                    g.add("partials", pf)
                _run(L, call, row.launches, tag)
                bad = g.changed()
                assert bad is None, f"{tag}: changed outside the outputs: {bad}"
                _check_backward(row, kind, p, c, bw, addend, sums, tag, seen)
                names = ("dx", "dgamma", "dbeta", "rows")
                first = _bits_of(p, names)
                if alias:
                    p.win["dy"].copy_(c["dy"].reshape(B * P, C).to(torch.bfloat16))
                _run(L, call, row.launches, tag + " again")
                assert _same_bits(first, _bits_of(p, names)), f"{tag}: a second call gives other bits"
        _report(row, kind, seen)


@pytest.mark.parametrize("row", CHAN, ids=NM.row_id)
def test_chan_sum_rows(row):
    L = _L()
    B, P, C = row.B, row.P, row.C
    bc, c2, c_store = NM.opt(row, "mode") == "bc", NM.opt(row, "per_c2"), NM.opt(row, "c_store")
    for kind in FAMILIES:
        c, seen = NM.case_of(kind, B, P, C, row.G), {}
        ref = NM.chan_reference(c, B, P, C)
        for layout in LAYOUTS:
            for tail in ((True, False) if bc else (True,)):   # per-(b, c) mode also without the per-channel sums
                tag = f"{NM.row_id(row)} {kind} {layout} per_c={tail}"
                p = NM.Problem(c, layout, L)
                pad, col0 = (0, 0) if layout == NM.CONTIGUOUS else (16, 8)
                per_bc = NM.Buf(B, C + pad, torch.bfloat16, "cuda")
                per_bc.col0 = col0
                win = per_bc.window(col0, C)
                per_c, per_c2 = NM.Flat(C, "cuda"), NM.Flat(C, "cuda")

                def call():
                    return L.sdmi_chan_sum(NM.ptr(p.win["dy"]), p.ld("dy"), B, P, C, NM.ptr(p.ws.data),
                                           NM.ptr(win) if bc else None, win.stride(0),
                                           NM.ptr(per_c.data) if tail else None,
                                           NM.ptr(per_c2.data) if (tail and c2) else None, c_store, _stream())
                g = p.guard({"ws"})
                g.add("per_bc", per_bc, [("w", col0, C)] if bc else [])
                g.add("per_c", per_c, [(0, c_store)] if tail else [])
                g.add("per_c2", per_c2, [(0, c_store)] if (tail and c2) else [])
                _run(L, (call,), row.launches, tag)
                bad = g.changed()
                assert bad is None, f"{tag}: changed outside the outputs: {bad}"
                outs = []
                if bc:
                    got = win.cpu().double()
                    _within(got, ref["per_bc"], NM.sum_bound(ref["T_bc"], True, ref["per_bc"]), "per_bc", tag, seen)
                    outs.append(got)
                    if kind == "exact":
                        assert torch.equal(got, NM.bf16(ref["per_bc"])), f"{tag}: per_bc is not bf16(exact sum)"
                for f in ([per_c] if tail else []) + ([per_c2] if (tail and c2) else []):
                    got = f.get(C)[:c_store]
                    _within(got, ref["per_c"][:c_store], NM.sum_bound(ref["T_c"][:c_store]), "per_c", tag, seen)
                    outs.append(got)
                    if kind == "exact":
                        assert torch.equal(got, ref["per_c"][:c_store]), f"{tag}: per_c is not the exact sum"
                _run(L, (call,), row.launches, tag + " again")
                again = ([win.cpu().double()] if bc else []) + [f.get(C)[:c_store] for f in
                                                                ([per_c] if tail else []) +
                                                                ([per_c2] if (tail and c2) else [])]
                assert all(torch.equal(a, b) for a, b in zip(outs, again)), f"{tag}: a second call gives other bits"
        _report(row, kind, seen)


@pytest.mark.parametrize("row", GROUPED, ids=NM.row_id)
def test_grouped_rows_sum(row):
    """One sdmi_gn_bwd_rows per job, then every job's dgamma / dbeta from one grouped launch: inside the bounds, dbeta
    exact, and bitwise what sdmi_gn_rows_sum gives for the job alone."""
    L = _L()
    jobs = NM.opt(row, "jobs")
    for kind in FAMILIES:
        silu, seen = _silu(row, kind), {}
        for layout in LAYOUTS:
            tag = f"{NM.row_id(row)} {kind} {layout}"
            probs, refs = [], []
            for B, P, C, G in jobs:
                c = NM.case_of(kind, B, P, C, G)
                p = NM.Problem(c, layout, L)
                _run(L, (lambda: p.fwd(silu, _stream()),), None, tag + " forward")
                tab = _table(p, c, NM.group_stats(c["x"], G), tag, seen)
                probs.append(p)
                refs.append(NM.bwd_reference(c, tab, silu))
            arr = (NM.RowsJob * len(jobs))(*[NM.RowsJob(p.rows.data.data_ptr(), p.dgamma.data.data_ptr(),
                                                        p.dbeta.data.data_ptr(), p.dims[0], p.dims[2]) for p in probs])
            guards = [p.guard({"dx", "ws", "table2", "rows", "dgamma", "dbeta"}) for p in probs]
            calls = tuple((lambda p=p: p.bwd_rows(silu, _stream())) for p in probs)
            calls += (lambda: L.sdmi_gn_rows_sum_grouped(ctypes.cast(arr, ctypes.c_void_p), len(jobs), _stream()),)
            _run(L, calls, row.launches, tag)
            for p, g, bw in zip(probs, guards, refs):
                assert g.changed() is None, f"{tag}: job C={p.dims[2]} changed {g.changed()}"
                _check_backward(row, kind, p, p.c, bw, False, True, f"{tag} job C={p.dims[2]}", seen)
                first = _bits_of(p, ("dgamma", "dbeta"))
                p.dgamma.data.fill_(float("nan"))
                p.dbeta.data.fill_(float("nan"))
                _run(L, (lambda: p.rows_sum(_stream()),), None, tag + " alone")
                assert _same_bits(first, _bits_of(p, ("dgamma", "dbeta"))), f"{tag}: grouped differs from single"
        _report(row, kind, seen)


def test_counter_slots_are_rearmed():
    """More launches than the 2048 counter slots: sdmi_gn_bwd with dgamma 2100 times back to back, alternating two
    shapes of 2 and 4 strips, then a checked row. Every slot has come round again; a counter left above zero would
    keep the batch tail from running (dbeta would stay NaN) or run it early."""
    L = _L()
    probs = []
    for shape in NM.COUNTER_SHAPES + (NM.COUNTER_ROW,):
        c = NM.exact_case(*shape)
        p = NM.Problem(c, NM.WINDOWS, L)
        _run(L, (lambda: p.fwd(0, _stream()),), None, f"forward {shape}")
        tab = p.table.get(shape[0], shape[2], 4)
        assert NM.check_table(c, tab)[0] is None
        probs.append((p, c, NM.bwd_reference(c, tab, 0)))
    s = _stream()
    assert 2100 > NM.NSLOTS
    for i in range(2100):
        assert probs[i % 2][0].bwd(0, s) == 0
    torch.cuda.synchronize()
    row = NM.R(NM.BWD, *NM.COUNTER_ROW, 0)
    seen = {}
    for n, (p, c, bw) in enumerate(probs[:2]):
        _check_backward(row, "exact", p, c, bw, False, True, f"after 2100 launches, shape {n}", seen)
    for p, c, bw in probs:   # once more through fresh NaNs: the tail of every strip runs again
        p.dgamma.data.fill_(float("nan"))
        p.dbeta.data.fill_(float("nan"))
        g = p.guard({"dx", "ws", "table2", "dgamma", "dbeta"})
        assert p.bwd(0, s) == 0
        torch.cuda.synchronize()
        assert g.changed() is None
        _check_backward(row, "exact", p, c, bw, False, True, "the checked row after the slots came round", seen)
    print("counter slots: max(err / bound) " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(seen.items())))


def _rejected(L, p, extra, fn, want, tag):
    g = p.guard(set())
    for name, f in extra:
        g.add(name, f)
    rc, ops = NM.recorded(L, fn)
    assert rc == want, f"{tag}: returned {rc}, documented {want}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: a rejected call changed {g.changed()}"


def test_error_returns_launch_nothing():
    """-1 for C % 8 != 0, G <= 0, C % G != 0, a null rows or part, P % rb != 0, B or P <= 0 (chan_sum), no jobs; -3 for
    exactly one of dgamma / dbeta; -5 for a row stride of sdmi_gn_bwd_part that is no multiple of 8; -2 for a group
    wider than 256 channels. Every such call returns before any launch (the recorded plan is empty) and leaves every
    guarded buffer as it was. Every argument list stays inside its buffers even if it were launched."""
    L = _L()
    B, P, C, G = NM.COUNTER_ROW
    c = NM.exact_case(B, P, C, G)
    p = NM.Problem(c, NM.WINDOWS, L)
    _run(L, (lambda: p.fwd(0, _stream()),), None, "forward")
    rb = 13
    part = NM.Flat(B * C * 2, "cuda").put(torch.zeros(B * C * 2))
    extra = [("partials", part)]
    s = _stream()
    x, dy, dx, y, add = (NM.ptr(p.win[n]) for n in ("x", "dy", "dx", "y", "add"))
    ldx, ldy_, lddx, ldy, ldadd = (p.ld(n) for n in ("x", "dy", "dx", "y", "add"))
    ga, be, ws, tab, tab2 = (NM.ptr(f.data) for f in (p.gamma, p.beta, p.ws, p.table, p.table2))
    dg, db, rows, pp = (NM.ptr(f.data) for f in (p.dgamma, p.dbeta, p.rows, part))

    def stats(C=C, G=G):
        return lambda: L.sdmi_gn_stats(x, ldx, B, P, C, G, NM.EPS, ga, be, ws, tab, s)

    def fwd(C=C, G=G):
        return lambda: L.sdmi_gn_fwd(x, ldx, y, ldy, B, P, C, G, NM.EPS, ga, be, 0, ws, tab, s)

    def bwd(C=C, G=G, dg=dg, db=db):
        return lambda: L.sdmi_gn_bwd(x, ldx, dy, ldy_, dx, lddx, tab, ga, B, P, C, G, 0, ws, tab2, dg, db, add,
                                     ldadd, s)

    def bwd_rows(C=C, G=G, rows=rows):
        return lambda: L.sdmi_gn_bwd_rows(x, ldx, dy, ldy_, dx, lddx, tab, ga, B, P, C, G, 0, ws, tab2, rows, add,
                                          ldadd, s)

    def bwd_part(C=C, G=G, dg=dg, db=db, pp=pp, rb=rb, lddx=lddx, ldx=ldx):
        return lambda: L.sdmi_gn_bwd_part(x, ldx, dy, ldy_, dx, lddx, tab, ga, B, P, C, G, 0, pp, rb, ws, dg, db, add,
                                          ldadd, s)

    def part_rows(C=C, G=G, rows=rows, pp=pp, rb=rb):
        return lambda: L.sdmi_gn_bwd_part_rows(x, ldx, dy, ldy_, dx, lddx, tab, ga, B, P, C, G, 0, pp, rb, ws, rows,
                                               add, ldadd, s)
    for name, mk in (("stats", stats), ("fwd", fwd), ("bwd", bwd), ("bwd_rows", bwd_rows), ("bwd_part", bwd_part),
                     ("bwd_part_rows", part_rows)):
        _rejected(L, p, extra, mk(C=C - 4), -1, f"{name}: C % 8 != 0")
        _rejected(L, p, extra, mk(G=0), -1, f"{name}: G = 0")
        _rejected(L, p, extra, mk(G=-4), -1, f"{name}: G < 0")
        _rejected(L, p, extra, mk(G=3), -1, f"{name}: C % G != 0")
    for name, mk in (("bwd", bwd), ("bwd_part", bwd_part)):
        _rejected(L, p, extra, mk(dg=None), -3, f"{name}: dgamma null, dbeta given")
        _rejected(L, p, extra, mk(db=None), -3, f"{name}: dbeta null, dgamma given")
    _rejected(L, p, extra, bwd_rows(rows=None), -1, "bwd_rows: null rows")
    _rejected(L, p, extra, part_rows(rows=None), -1, "bwd_part_rows: null rows")
    for name, mk in (("bwd_part", bwd_part), ("bwd_part_rows", part_rows)):
        _rejected(L, p, extra, mk(rb=4), -1, f"{name}: P % rb != 0")
        _rejected(L, p, extra, mk(rb=0), -1, f"{name}: rb = 0")
        _rejected(L, p, extra, mk(pp=None), -1, f"{name}: null part")
    _rejected(L, p, extra, bwd_part(lddx=lddx + 4), -5, "bwd_part: lddx % 8 != 0")
    _rejected(L, p, extra, bwd_part(ldx=ldx + 4), -5, "bwd_part: ldx % 8 != 0")

    def chan(B=B, P=P, C=C):
        return lambda: L.sdmi_chan_sum(dy, ldy_, B, P, C, ws, None, 0, dg, db, 0, s)
    _rejected(L, p, extra, chan(C=C - 4), -1, "chan_sum: C % 8 != 0")
    _rejected(L, p, extra, chan(B=0), -1, "chan_sum: B = 0")
    _rejected(L, p, extra, chan(P=0), -1, "chan_sum: P = 0")
    job = (NM.RowsJob * 1)(NM.RowsJob(p.rows.data.data_ptr(), p.dgamma.data.data_ptr(), p.dbeta.data.data_ptr(), B, C))
    jp = ctypes.cast(job, ctypes.c_void_p)
    _rejected(L, p, extra, lambda: L.sdmi_gn_rows_sum_grouped(jp, 0, s), -1, "rows_sum_grouped: no jobs")
    _rejected(L, p, extra, lambda: L.sdmi_gn_rows_sum_grouped(None, 1, s), -1, "rows_sum_grouped: null jobs")
    _rejected(L, p, extra, lambda: L.sdmi_gn_rows_sum_grouped(jp, 17, s), -1, "rows_sum_grouped: 17 jobs")
    _rejected(L, p, extra, lambda: L.sdmi_gn_rows_sum(None, B, C, dg, db, s), -1, "rows_sum: null rows")
    # a group wider than 256 channels: no strip of whole groups fits a workgroup (buffers sized for the shape)
    Bw, Pw, Cw, Gw = 3, 4, 512, 1
    w = NM.Problem(NM.exact_case(Bw, Pw, Cw, Gw), NM.WINDOWS, L)
    wpart = NM.Flat(Bw * Cw * 2, "cuda").put(torch.zeros(Bw * Cw * 2))
    a = dict(x=NM.ptr(w.win["x"]), dy=NM.ptr(w.win["dy"]), dx=NM.ptr(w.win["dx"]), y=NM.ptr(w.win["y"]))
    wf = {n: NM.ptr(getattr(w, n).data) for n in ("gamma", "beta", "ws", "table", "table2", "dgamma", "dbeta", "rows")}
    head = (a["x"], w.ld("x"), a["dy"], w.ld("dy"), a["dx"], w.ld("dx"), wf["table"], wf["gamma"], Bw, Pw, Cw, Gw, 0)
    wide = (
        ("stats", lambda: L.sdmi_gn_stats(a["x"], w.ld("x"), Bw, Pw, Cw, Gw, NM.EPS, wf["gamma"], wf["beta"], wf["ws"],
                                          wf["table"], s)),
        ("fwd", lambda: L.sdmi_gn_fwd(a["x"], w.ld("x"), a["y"], w.ld("y"), Bw, Pw, Cw, Gw, NM.EPS, wf["gamma"],
                                      wf["beta"], 0, wf["ws"], wf["table"], s)),
        ("bwd", lambda: L.sdmi_gn_bwd(*head, wf["ws"], wf["table2"], wf["dgamma"], wf["dbeta"], None, 0, s)),
        ("bwd_rows", lambda: L.sdmi_gn_bwd_rows(*head, wf["ws"], wf["table2"], wf["rows"], None, 0, s)),
        ("bwd_part", lambda: L.sdmi_gn_bwd_part(*head, NM.ptr(wpart.data), 4, wf["ws"], wf["dgamma"], wf["dbeta"], None,
                                                0, s)),
    )
    for name, fn in wide:
        _rejected(L, w, [("partials", wpart)], fn, -2, f"{name}: one group of 512 channels")
