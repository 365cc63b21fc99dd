"""Every sampling-step and device-noise kernel of csrc/sampler.hip, and sdmi_add_noise, at every row of
tests/sampler_matrix.py ROWS, exact, guarded.

The recorded launch plan must name the row's kernels and grids. After every call nothing but the declared outputs may
have changed, bit for bit -- inputs, tables, device words a call must not write. Then the statements of
tests/sampler_matrix.py: every step and add_noise output bitwise the numpy.float32 model (a NaN matching a NaN),
sdmi_ddim_prev bitwise sdmi_ddim_prev_dev(_dup), the device words after the decrement / advance launches, t, the text
rows and keep of a draw bitwise from the Philox integers, the noise within K_Z u rad (1 + theta) of float64 on those
integers, sdmi_randn bitwise the noise segment of sdmi_step_draw, sample b's draw the same for every B. A second
identical call gives identical bits. Each noise test prints its worst error / bound.

Also every error return: -1 or -2, nothing launched, nothing written."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sampler_matrix as SM

pytestmark = pytest.mark.gpu
ptr, opt = SM.ptr, SM.opt


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = SM.recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert SM.launches_match(ops, want), f"{tag}: launched {ops[:6]} ({len(ops)}), the matrix says {list(want)[:6]} ({len(want)})"
    torch.cuda.synchronize()


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _same(got, ref, what, tag):
    assert SM.same_bits(got, ref), f"{tag}: {what} differs from its bitwise value in " \
        f"{SM.differing(got, ref) if got.shape == ref.shape else 'shape'} elements"


def _rejected(L, g, fn, tag, code=-1):
    rc, ops = SM.recorded(L, fn)
    assert rc == code, f"{tag}: returned {rc}, documented {code}"
    assert ops == [], f"{tag}: launched {ops}"
    torch.cuda.synchronize()
    assert g.changed() is None, f"{tag}: a rejected call changed {g.changed()}"


def _whole(w):
    return [(0, w.n)]


# ----------------------------------------------------------------------------------------------------------------
# the DDPM step
# ----------------------------------------------------------------------------------------------------------------
TABLE_KEYS = ("betas", "alphas", "abar", "s1m")


def _ddpm_once(L, row, check_launches):
    tag = SM.row_id(row)
    tab, t, x, e, z = SM.ddpm_row_case(row)
    rows, n = x.shape
    alias, dec = opt(row, "alias", 0), opt(row, "dec", 0)
    with_z, with_x0, with_p2 = opt(row, "z", 1), opt(row, "x0", 1), opt(row, "prev2", 0)
    T = {k: SM.dev(getattr(tab, k)) for k in TABLE_KEYS}
    X, E, Z, tw = SM.dev(x), SM.dev(e), SM.dev(z), SM.Words(t)
    P = X if alias else SM.Win(rows * n, "cuda")
    P2, X0 = SM.Win(rows * n, "cuda"), SM.Win(rows * n, "cuda")
    g = SM.Guard()
    for k in TABLE_KEYS:
        g.add(k, T[k])
    g.add("xt", X, _whole(X) if alias else [])
    g.add("eps", E)
    g.add("z", Z)
    g.add("t_dev", tw, [tw.span(0, rows)] if dec else [])
    if not alias:
        g.add("prev", P, _whole(P))
    g.add("prev2", P2, _whole(P2) if with_p2 else [])
    g.add("x0", X0, _whole(X0) if with_x0 else [])
    s = _stream()

    def call():
        rc = 0
        for i in range(rows):
            at = lambda w: ptr(w.data[i * n:])  # noqa: E731
            a = (at(X), at(E), at(Z) if with_z else None, n, ptr(tw.data[i:])) + tuple(ptr(T[k].data) for k in TABLE_KEYS)
            x0p = at(X0) if with_x0 else None
            if with_p2:
                rc |= L.sdmi_ddpm_prev_dup(*a, at(P), at(P2), x0p, dec, s)
            else:
                rc |= L.sdmi_ddpm_prev(*a, at(P), x0p, dec, s)
        return rc

    if check_launches:
        _run(L, call, list(row.launches) * rows, tag)
    else:
        assert call() == 0
        torch.cuda.synchronize()
    _unchanged(g, tag)
    out = dict(prev=SM.host(P, rows, n), t=tw.get())
    if with_p2:
        out["prev2"] = SM.host(P2, rows, n)
    if with_x0:
        out["x0"] = SM.host(X0, rows, n)
    return out


@pytest.mark.parametrize("row", SM.rows_of(SM.DDPM), ids=SM.row_id)
def test_ddpm_rows(row):
    L, tag = _L(), SM.row_id(row)
    tab, t, x, e, z = SM.ddpm_row_case(row)
    prev, x0, _ = SM.ddpm_model(tab, t, x, e, z if opt(row, "z", 1) else None)
    out = _ddpm_once(L, row, True)
    _same(out["prev"], prev, "x_{t-1}", tag)
    if "x0" in out:
        _same(out["x0"], x0, "x0", tag)
    if "prev2" in out:
        _same(out["prev2"], out["prev"], "the second output", tag)
    want_t = [max(int(v) - 1, 0) for v in t] if opt(row, "dec") else [int(v) for v in t]
    assert out["t"] == want_t, f"{tag}: the timestep words are {out['t'][:4]}, expected {want_t[:4]}"
    again = _ddpm_once(L, row, False)
    for k, v in out.items():
        assert again[k] == v if k == "t" else SM.same_bits(again[k], v), f"{tag}: a second identical call gives other {k}"


# ----------------------------------------------------------------------------------------------------------------
# the DDIM step: the host-scalar form and the device-table form on the same pairs
# ----------------------------------------------------------------------------------------------------------------
T_DEV_START = 12345


def _ddim_once(L, row, form, check_launches):
    tag = f"{SM.row_id(row)} {form}"
    abar, ts, tp, eta, x, e, nz = SM.ddim_row_case(row)
    rows, n = x.shape
    sweep, alias, adv = opt(row, "sweep", 0), opt(row, "alias", 0), opt(row, "adv", 0)
    with_nz, with_o2, with_td = opt(row, "noise", 1), opt(row, "out2", 0), opt(row, "tdev", 1)
    dup = with_o2 or opt(row, "dup", 0)
    A, X, E, NZ = SM.dev(abar), SM.dev(x), SM.dev(e), SM.dev(nz)
    O = X if alias else SM.Win(rows * n, "cuda")
    O2 = SM.Win(rows * n, "cuda")
    table_ts, table_tp = (ts, tp) if sweep else (SM.DDIM_TS, SM.DDIM_TP)
    idx0 = list(range(rows)) if sweep else [opt(row, "idx", SM.DDIM_IDX)]
    TS, TP, IDX, TD = SM.Words(table_ts), SM.Words(table_tp), SM.Words(idx0), SM.Words([T_DEV_START])
    dev_form = form == "dev"
    g = SM.Guard()
    for name, w in (("abar", A), ("eps", E), ("noise", NZ), ("ts", TS), ("tp", TP)):
        g.add(name, w)
    g.add("xt", X, _whole(X) if alias else [])
    if not alias:
        g.add("out", O, _whole(O))
    g.add("out2", O2, _whole(O2) if with_o2 and dev_form else [])
    g.add("idx", IDX, [IDX.span(0, rows)] if adv and dev_form else [])
    g.add("t_dev", TD, [TD.span(0)] if adv and dev_form and with_td else [])
    s = _stream()

    def call():
        rc = 0
        for i in range(rows):
            at = lambda w: ptr(w.data[i * n:])  # noqa: E731
            a = (at(X), at(E), at(NZ) if with_nz else None, n)
            if not dev_form:
                rc |= L.sdmi_ddim_prev(*a, float(abar[ts[i]]), float(abar[tp[i]]), eta, at(O), s)
                continue
            a += (ptr(TS.data), ptr(TP.data), ptr(IDX.data[i:]), ptr(TD.data) if with_td else None, ptr(A.data), eta, at(O))
            if dup:
                rc |= L.sdmi_ddim_prev_dev_dup(*a, at(O2) if with_o2 else None, adv, s)
            else:
                rc |= L.sdmi_ddim_prev_dev(*a, adv, s)
        return rc

    want = list(row.launches[1:] if dev_form else row.launches[:1]) * rows
    if check_launches:
        _run(L, call, want, tag)
    else:
        assert call() == 0
        torch.cuda.synchronize()
    _unchanged(g, tag)
    out = dict(out=SM.host(O, rows, n), idx=IDX.get(), t_dev=TD.get()[0])
    if with_o2 and dev_form:
        out["out2"] = SM.host(O2, rows, n)
    return out, idx0


@pytest.mark.parametrize("row", SM.rows_of(SM.DDIM), ids=SM.row_id)
def test_ddim_rows(row):
    L, tag = _L(), SM.row_id(row)
    abar, ts, tp, eta, x, e, nz = SM.ddim_row_case(row)
    sigma, _, c2, inner = SM.ddim_coeffs(abar[ts], abar[tp], eta)
    assert not np.isnan(sigma).any() and not np.isnan(c2).any() and bool((inner >= 0).all()), f"{tag}: a vacuous pair"
    want = SM.ddim_model(abar[ts], abar[tp], eta, x, e, nz if opt(row, "noise", 1) else None)
    host_out, _ = _ddim_once(L, row, "host", True)
    dev_out, idx0 = _ddim_once(L, row, "dev", True)
    _same(host_out["out"], want, "sdmi_ddim_prev", tag)
    _same(dev_out["out"], want, "sdmi_ddim_prev_dev", tag)
    _same(dev_out["out"], host_out["out"], "the device form against the host form", tag)
    if "out2" in dev_out:
        _same(dev_out["out2"], dev_out["out"], "the second output", tag)
    if opt(row, "adv"):
        want_idx = [max(i - 1, 0) for i in idx0]
        moved = idx0[0] > 0 and opt(row, "tdev", 1)
        want_td = SM.DDIM_TS[idx0[0] - 1] if moved else T_DEV_START
    else:
        want_idx, want_td = idx0, T_DEV_START
    assert dev_out["idx"] == want_idx, f"{tag}: the index words are {dev_out['idx'][:4]}, expected {want_idx[:4]}"
    assert dev_out["t_dev"] == want_td, f"{tag}: *t_dev is {dev_out['t_dev']}, expected {want_td}"
    assert host_out["idx"] == idx0 and host_out["t_dev"] == T_DEV_START
    again, _ = _ddim_once(L, row, "dev", False)
    for k, v in dev_out.items():
        assert again[k] == v if k in ("idx", "t_dev") else SM.same_bits(again[k], v), f"{tag}: a second call gives other {k}"


# ----------------------------------------------------------------------------------------------------------------
# the affine step and add_noise
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SM.rows_of(SM.AFF), ids=SM.row_id)
def test_affine_rows(row):
    L, tag = _L(), SM.row_id(row)
    c1, c2, var, x, e, z = SM.affine_row_case(row)
    n, with_z = row.dims[0], opt(row, "z", 1)
    want = SM.affine_model(c1, c2, var, x, e, z if with_z else None)
    first = None
    for trip in range(2):
        X, E, Z, O = SM.dev(x), SM.dev(e), SM.dev(z), SM.Win(n, "cuda")
        g = SM.Guard()
        for name, w in (("x", X), ("eps", E), ("z", Z)):
            g.add(name, w)
        g.add("out", O, _whole(O))
        _run(L, lambda: L.sdmi_affine_step(ptr(X.data), ptr(E.data), ptr(Z.data) if with_z else None, n, float(c1),
                                           float(c2), float(var), ptr(O.data), _stream()), row.launches, tag)
        _unchanged(g, tag)
        got = SM.host(O, 1, n)
        _same(got, want, "the step", tag)
        assert first is None or SM.same_bits(got, first), f"{tag}: a second identical call gives other bits"
        first = got


@pytest.mark.parametrize("row", SM.rows_of(SM.ADDN), ids=SM.row_id)
def test_add_noise_rows(row):
    L, tag = _L(), SM.row_id(row)
    tab, t, x0, eps = SM.addn_row_case(row)
    B, per = row.dims
    want = SM.add_noise_model(tab, t, x0, eps)
    first = None
    for trip in range(2):
        X, E, TW, SA, S1, O = SM.dev(x0), SM.dev(eps), SM.Words(t), SM.dev(tab.sa), SM.dev(tab.s1m), SM.Win(B * per, "cuda")
        g = SM.Guard()
        for name, w in (("x0", X), ("eps", E), ("t", TW), ("sqrt_abar", SA), ("sqrt_one_minus_abar", S1)):
            g.add(name, w)
        g.add("out", O, _whole(O))
        _run(L, lambda: L.sdmi_add_noise(ptr(X.data), ptr(E.data), ptr(TW.data), ptr(SA.data), ptr(S1.data), B, per,
                                         ptr(O.data), _stream()), row.launches, tag)
        _unchanged(g, tag)
        got = SM.host(O, B, per)
        _same(got, want, "x_t", tag)
        assert first is None or SM.same_bits(got, first), f"{tag}: a second identical call gives other bits"
        first = got


# ----------------------------------------------------------------------------------------------------------------
# device noise and the draws of a training step
# ----------------------------------------------------------------------------------------------------------------
def _check_noise(got, seed, off, n, tag):
    z, rad, theta = SM.noise_reference(SM.noise_words(seed, off, SM.cdiv(n, 4)))
    z, lim = z.reshape(-1)[:n], SM.noise_bound(rad, theta).reshape(-1)[:n]
    w = SM.worst_ratio(got.astype(np.float64), z, lim)
    print(f"{tag}: noise max(err / bound) {w:.4f}")
    assert w <= 1.0, f"{tag}: noise worst error / bound {w:.3f}"


def _randn(L, n, seed, off, adv, want=None, tag=""):
    O, OFF = SM.Win(n, "cuda"), SM.Words([off])
    g = SM.Guard()
    g.add("out", O, _whole(O))
    g.add("offset", OFF, [OFF.span(0)] if adv else [])
    call = lambda: L.sdmi_randn(ptr(O.data), n, seed, ptr(OFF.data), adv, _stream())  # noqa: E731
    if want is None:
        assert call() == 0
        torch.cuda.synchronize()
    else:
        _run(L, call, want, tag)
    _unchanged(g, tag)
    return SM.host(O), OFF.get()[0]


@pytest.mark.parametrize("row", SM.rows_of(SM.RANDN), ids=SM.row_id)
def test_randn_rows(row):
    L, tag = _L(), SM.row_id(row)
    n, seed, off, adv = row.dims[0], opt(row, "seed"), opt(row, "off"), opt(row, "adv", 0)
    got, after = _randn(L, n, seed, off, adv, row.launches, tag)
    _check_noise(got, seed, off, n, tag)
    assert after == off + adv, f"{tag}: *offset_dev is {after} after the call, expected {off + adv}"
    again, _ = _randn(L, n, seed, off, adv)
    assert SM.same_bits(again, got), f"{tag}: a second call with the same seed and offset gives other bits"


def test_every_word_of_seed_and_offset_is_live():
    L = _L()
    out = {p: _randn(L, 1025, p[0], p[1], 0)[0] for p in SM.SEED_PAIRS}
    low = out[(7, 1)]
    for p in ((2 ** 32 + 7, 1), (7, 2 ** 32 + 1)):
        assert SM.differing(out[p], low) > 1000, f"{p} draws what its low-word twin (7, 1) draws"
    assert SM.differing(out[(2 ** 32 + 7, 1)], out[(7, 2 ** 32 + 1)]) > 1000


def _draw_once(L, row, check_launches, B=None, seed=SM.DRAW_SEED, off=SM.DRAW_OFF):
    tag = SM.row_id(row)
    n, rowB, re = row.dims
    B = rowB if B is None else B
    T, with_txt, with_keep = opt(row, "T"), opt(row, "txt"), opt(row, "keep")
    pt, pk = SM.draw_probabilities(row, seed, off)
    text, empty = SM.text_case(B, max(re, 4))
    N, TW, TEXT, EMPTY = SM.Win(n, "cuda"), SM.Words([-1] * B), SM.dev(text), SM.dev(empty)
    TXT, KEEP = SM.Win(B * max(re, 4), "cuda"), SM.Win(B, "cuda")
    g = SM.Guard()
    g.add("noise", N, _whole(N))
    g.add("t", TW, [TW.span(0, B)])
    g.add("text", TEXT)
    g.add("empty", EMPTY)
    g.add("txt", TXT, [(0, B * re)] if with_txt else [])
    g.add("keep", KEEP, _whole(KEEP) if with_keep else [])
    p = lambda w: ptr(w.data) if with_txt else None  # noqa: E731
    call = lambda: L.sdmi_step_draw(ptr(N.data), n, ptr(TW.data), B, T, p(TEXT), p(EMPTY), p(TXT), re if with_txt else 0,  # noqa: E731
                                    pt, ptr(KEEP.data) if with_keep else None, pk, seed, off, _stream())
    if check_launches:
        _run(L, call, row.launches, tag)
    else:
        assert call() == 0
        torch.cuda.synchronize()
    _unchanged(g, tag)
    out = dict(noise=SM.host(N), t=TW.get())
    if with_txt:
        out["txt"] = SM.host(TXT)[:B * re].reshape(B, re)
    if with_keep:
        out["keep"] = SM.host(KEEP)
    return out, (text, empty, pt, pk)


@pytest.mark.parametrize("row", SM.rows_of(SM.DRAW), ids=SM.row_id)
def test_draw_rows(row):
    L, tag = _L(), SM.row_id(row)
    n, B, re = row.dims
    out, (text, empty, pt, pk) = _draw_once(L, row, True)
    _check_noise(out["noise"], SM.DRAW_SEED, SM.DRAW_OFF, n, tag)
    t, drop, keep, _, _ = SM.draw_reference(SM.DRAW_SEED, SM.DRAW_OFF, B, opt(row, "T"), pt, pk)
    assert out["t"] == [int(v) for v in t], f"{tag}: t differs from (c0 T) >> 32 (or its upper word is not zero)"
    if "txt" in out:
        _same(out["txt"], np.where(drop[:, None], empty[None, :re], text[:, :re]), "the text rows", tag)
    if "keep" in out:
        _same(out["keep"], keep, "keep", tag)
    alone, _ = _randn(L, n, SM.DRAW_SEED, SM.DRAW_OFF, 0)
    assert SM.same_bits(alone, out["noise"]), f"{tag}: sdmi_randn draws other noise than sdmi_step_draw"
    again, _ = _draw_once(L, row, False)
    for k, v in out.items():
        assert again[k] == v if k == "t" else SM.same_bits(again[k], v), f"{tag}: a second identical call gives other {k}"


def test_a_samples_draw_does_not_depend_on_the_batch():
    L = _L()
    row = [r for r in SM.rows_of(SM.DRAW) if r.dims == (5, 3, 4) and opt(r, "pt") == 0.1][0]
    outs = {B: _draw_once(L, row, False, B=B, seed=7, off=2 ** 32 + 1)[0] for B in (1, 3, 5, 257)}
    big = outs[257]
    for B, o in outs.items():
        assert o["t"] == big["t"][:B], f"B = {B}: t depends on the batch"
        assert SM.same_bits(o["keep"], big["keep"][:B]), f"B = {B}: keep depends on the batch"
        # text_case draws other rows for another B: compare which rows were dropped
        text, empty = SM.text_case(B, 4)
        dropped = [SM.same_bits(o["txt"][b], empty) for b in range(B)]
        _, drop, _, _, _ = SM.draw_reference(7, 2 ** 32 + 1, 257, 1000, *SM.draw_probabilities(row, 7, 2 ** 32 + 1))
        assert dropped == [bool(d) for d in drop[:B]], f"B = {B}: the dropped rows depend on the batch"
        assert SM.same_bits(o["noise"], big["noise"])


# ----------------------------------------------------------------------------------------------------------------
# error returns (only arguments the host code rejects before any launch)
# ----------------------------------------------------------------------------------------------------------------
def test_step_entry_points_reject_without_launching():
    L, s, n = _L(), _stream(), 257
    tab = SM.table("cond")
    x, e, z = SM.step_case(n, 7)
    T = {k: SM.dev(getattr(tab, k)) for k in TABLE_KEYS}
    X, E, Z, O, O2, X0 = SM.dev(x), SM.dev(e), SM.dev(z), SM.Win(n, "cuda"), SM.Win(n, "cuda"), SM.Win(n, "cuda")
    TW, TS, TP, IDX, TD = SM.Words([5]), SM.Words(SM.DDIM_TS), SM.Words(SM.DDIM_TP), SM.Words([3]), SM.Words([T_DEV_START])
    g = SM.Guard()
    for name, w in list(T.items()) + [("x", X), ("e", E), ("z", Z), ("out", O), ("out2", O2), ("x0", X0), ("t", TW),
                                      ("ts", TS), ("tp", TP), ("idx", IDX), ("t_dev", TD)]:
        g.add(name, w)

    def ddpm(dup, **over):
        a = dict(xt=ptr(X.data), eps=ptr(E.data), z=ptr(Z.data), n=n, t_dev=ptr(TW.data), betas=ptr(T["betas"].data),
                 alphas=ptr(T["alphas"].data), abar=ptr(T["abar"].data), s1m=ptr(T["s1m"].data), prev=ptr(O.data))
        if dup:
            a["prev2"] = ptr(O2.data)
        a.update(x0=ptr(X0.data), dec=1)
        a.update(over)
        return (L.sdmi_ddpm_prev_dup if dup else L.sdmi_ddpm_prev)(*a.values(), s)

    for dup in (0, 1):
        for name in ("xt", "eps", "t_dev", "betas", "alphas", "abar", "s1m", "prev"):
            _rejected(L, g, lambda: ddpm(dup, **{name: None}), f"ddpm dup={dup}: {name} null")
        for v in (0, -1):
            _rejected(L, g, lambda: ddpm(dup, n=v), f"ddpm dup={dup}: n = {v}")

    def ddim_dev(dup, **over):
        a = dict(xt=ptr(X.data), eps=ptr(E.data), noise=ptr(Z.data), n=n, ts=ptr(TS.data), tp=ptr(TP.data),
                 idx=ptr(IDX.data), t_dev=ptr(TD.data), abar=ptr(T["abar"].data), eta=0.5, out=ptr(O.data))
        if dup:
            a["out2"] = ptr(O2.data)
        a["adv"] = 1
        a.update(over)
        return (L.sdmi_ddim_prev_dev_dup if dup else L.sdmi_ddim_prev_dev)(*a.values(), s)

    for dup in (0, 1):
        for name in ("xt", "eps", "out", "ts", "tp", "idx", "abar"):
            _rejected(L, g, lambda: ddim_dev(dup, **{name: None}), f"ddim_dev dup={dup}: {name} null")
        for v in (0, -1):
            _rejected(L, g, lambda: ddim_dev(dup, n=v), f"ddim_dev dup={dup}: n = {v}")

    def flat(fn, **over):
        a = dict(x=ptr(X.data), eps=ptr(E.data), z=ptr(Z.data), n=n, a=0.5, b=0.75, c=0.5, out=ptr(O.data))
        a.update(over)
        return fn(*a.values(), s)

    for fn, what in ((L.sdmi_ddim_prev, "ddim"), (L.sdmi_affine_step, "affine")):
        for name in ("x", "eps", "out"):
            _rejected(L, g, lambda: flat(fn, **{name: None}), f"{what}: {name} null")
        for v in (0, -1):
            _rejected(L, g, lambda: flat(fn, n=v), f"{what}: n = {v}")

    SA, TB = SM.dev(tab.sa), SM.Words([0, 999, 500])

    def addn(**over):
        a = dict(x0=ptr(X.data), eps=ptr(E.data), t=ptr(TB.data), sa=ptr(SA.data), s1=ptr(T["s1m"].data), B=3, per=85,
                 out=ptr(O.data))
        a.update(over)
        return L.sdmi_add_noise(*a.values(), s)

    for name in ("x0", "eps", "t", "sa", "s1", "out"):
        _rejected(L, g, lambda: addn(**{name: None}), f"add_noise: {name} null")
    for name in ("B", "per"):
        for v in (0, -1):
            _rejected(L, g, lambda: addn(**{name: v}), f"add_noise: {name} = {v}")


def test_noise_entry_points_reject_without_launching():
    L, s, n, B, re = _L(), _stream(), 64, 3, 8
    text, empty = SM.text_case(B, re)
    N, OFF, TW, TEXT, EMPTY, TXT, KEEP = SM.Win(n, "cuda"), SM.Words([1]), SM.Words([-1] * B), SM.dev(text), \
        SM.dev(empty), SM.Win(B * re, "cuda"), SM.Win(B, "cuda")
    g = SM.Guard()
    for name, w in (("noise", N), ("offset", OFF), ("t", TW), ("text", TEXT), ("empty", EMPTY), ("txt", TXT), ("keep", KEEP)):
        g.add(name, w)
    _rejected(L, g, lambda: L.sdmi_randn(None, n, 7, ptr(OFF.data), 1, s), "randn: out null")
    _rejected(L, g, lambda: L.sdmi_randn(ptr(N.data), n, 7, None, 1, s), "randn: offset_dev null")
    for v in (0, -1):
        _rejected(L, g, lambda: L.sdmi_randn(ptr(N.data), v, 7, ptr(OFF.data), 1, s), f"randn: n = {v}")

    def draw(**over):
        a = dict(noise=ptr(N.data), n=n, t=ptr(TW.data), B=B, T=1000, text=ptr(TEXT.data), empty=ptr(EMPTY.data),
                 txt=ptr(TXT.data), re=re, pt=0.1, keep=ptr(KEEP.data), pk=0.1, seed=7, off=1)
        a.update(over)
        return L.sdmi_step_draw(*a.values(), s)

    for name in ("noise", "t"):
        _rejected(L, g, lambda: draw(**{name: None}), f"step_draw: {name} null")
    for name in ("n", "B", "T"):
        for v in (0, -1):
            _rejected(L, g, lambda: draw(**{name: v}), f"step_draw: {name} = {v}")
    for name in ("text", "empty"):
        _rejected(L, g, lambda: draw(**{name: None}), f"step_draw: {name} null with txt set", code=-2)
    for v in (0, -4, 6):
        _rejected(L, g, lambda: draw(re=v), f"step_draw: row_elems = {v}", code=-2)
    for name, w in (("text", TEXT), ("empty", EMPTY), ("txt", TXT)):
        _rejected(L, g, lambda: draw(**{name: ptr(w.data[1:])}), f"step_draw: {name} 4 bytes off", code=-2)
    # a null noise decides before the text checks
    _rejected(L, g, lambda: draw(noise=None, text=None), "step_draw: noise and text null")
