"""The DiT test matrix cannot fall behind the kernels, its exact data is exact and its bounds have teeth (CPU only, no
library call).

Each row of tests/dit_matrix.py ROWS launches what the restated host rules of csrc/dit.hip give; no row can be removed
without a coverage check failing; the exact family's sums are exact in fp32; on every soft row an fp32 emulation of the
kernels' arithmetic in two summation orders stays within K_SUM / 2 of every bound, K_SUM is at most 3 times the
largest emulated ratio, and each perturbed reference leaves its bound on at least one row of its entry point."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import dit_matrix as DM

CS = {8, 64, 96, 288, 504, 512}
FWD_SHAPES = {(1, 1), (3, 1), (2, 3), (2, 5), (2, 64)}
BWD_N = {1: (1, 1), 2: (2, 1), 6: (2, 3), 4: (4, 1), 12: (4, 3), 8: (8, 1), 24: (8, 3), 7: (1, 7)}   # N: (R, chunks)
FINALIZE_DIMS = {(1, 1, 8), (2, 8, 96), (3, 9, 288), (2, 7, 864)}
PATCH_DIMS = {(1, 1, 1, 1, 1), (2, 4, 8, 8, 2), (2, 3, 4, 6, 2), (3, 4, 6, 4, 1), (1, 2, 8, 12, 4), (2, 5, 6, 10, 2)}
CAPPED = (5, 4, 128, 128, 2)


def test_rows_follow_the_restated_rules():
    assert len({DM.row_id(r) for r in DM.ROWS}) == len(DM.ROWS)
    for r in DM.ROWS:
        assert list(r.launches) == DM.expected_launches(r.entry, r.dims, r.opt), DM.row_id(r)
        if r.entry in (DM.LN_FWD, DM.LN_BWD):
            B, N, C = r.dims
            assert C % 8 == 0 and 8 <= C <= 512
            # the token tensors, the modulation table, the partial rows
            assert max(B * N * (C + 72), B * (3 * C + 32), B * N * (3 * C + 5)) <= DM.CAP
        elif r.entry == DM.FINALIZE:
            B, chunks, W = r.dims
            assert B * chunks * (W + 5) <= DM.CAP
        else:
            B, C, H, W, p = r.dims
            rows, K = DM.patch_dims(*r.dims)
            assert H % p == 0 and W % p == 0 and max(rows * (K + DM.opt(r, "pad")), B * C * H * W) <= DM.CAP
    # grid_for caps only beyond the size cap: no row can reach it
    assert DM.grid_for(DM.CAP) == 8192 and DM.grid_for(DM.CAP - 256) == 8191


def test_the_restated_rules_at_known_points():
    assert [DM.chunk_rows(n) for n in (1, 2, 6, 4, 12, 8, 24, 7, 16, 64, 256)] == [1, 2, 2, 4, 4, 8, 8, 1, 8, 8, 8]
    assert DM.grid_for(1) == 1 and DM.grid_for(256) == 1 and DM.grid_for(257) == 2 and DM.grid_for(2 ** 22) == 8192
    assert DM.expected_launches(DM.LN_FWD, (2, 5, 8), (("f32", 1),)) == [("ln_mod_fwd_kernelILb1EE", 3)]
    assert DM.expected_launches(DM.LN_BWD, (3, 12, 8), (("f32", 0),)) == [("ln_mod_bwd_kernelILb0EE", 9)]
    assert DM.expected_launches(DM.MSE, (5, 4, 128, 128, 2), (("pad", 0),))[0][1] == 1024
    assert DM.expected_launches(DM.MSE, (4, 4, 128, 128, 2), (("pad", 0),))[0][1] == 1024   # 262144 / 256: the edge
    assert DM.expected_launches(DM.MSE, (2, 4, 8, 8, 2), (("pad", 3),)) == [("mse_patch_kernel", 3),
                                                                           ("sum_rows_kernel", 1)]
    assert DM.patch_dims(2, 5, 6, 10, 2) == (30, 20)


# ----------------------------------------------------------------------------------------------------------------
# coverage
# ----------------------------------------------------------------------------------------------------------------
def _need(found, what):
    assert found, f"ROWS has no row for: {what}"


def check_forward_coverage():
    for f in (0, 1):
        mine = [r for r in DM.rows_of(DM.LN_FWD) if DM.opt(r, "f32") == f]
        _need(mine, f"ln_mod_fwd_kernel<{f}>")
        assert all(r.launches[0][0] == DM.fwd_name(f) for r in mine)
        for C in CS:
            _need([r for r in mine if r.dims[2] == C], f"forward, stream {f}, C = {C}")
        for s in FWD_SHAPES:
            _need([r for r in mine if r.dims[:2] == s], f"forward, stream {f}, (B, N) = {s}")
        for res, mod in itertools.product(("none", "v", "gate"), (0, 1)):
            _need([r for r in mine if (DM.opt(r, "res"), DM.opt(r, "mod")) == (res, mod) and
                   (r.dims[0] * r.dims[1]) % 4], f"forward, stream {f}, residual {res}, modulation {mod}, ragged")


def check_backward_coverage():
    rows = DM.rows_of(DM.LN_BWD)
    for f in (0, 1):
        mine = [r for r in rows if DM.opt(r, "f32") == f]
        _need(mine, f"ln_mod_bwd_kernel<{f}>")
        assert all(r.launches[0][0] == DM.bwd_name(f) for r in mine)
        for C in CS:
            _need([r for r in mine if r.dims[2] == C], f"backward, stream {f}, C = {C}")
        for N, (Rr, chunks) in BWD_N.items():
            assert DM.chunk_rows(N) == Rr and N // Rr == chunks
            _need([r for r in mine if r.dims[1] == N], f"backward, stream {f}, N = {N} (R = {Rr}, {chunks} chunks)")
    assert {r.dims[0] for r in rows} >= {1, 2, 3}
    assert {DM.chunk_rows(r.dims[1]) for r in rows} == {1, 2, 4, 8}, "every R"
    assert {r.dims[1] // DM.chunk_rows(r.dims[1]) for r in rows} >= {1, 3, 7}, "one, several, 7 chunks"
    for kind in ("none", "both", "psh", "psc", "neither"):
        _need([r for r in rows if DM.opt(r, "mod") == kind], f"backward with modulation pointers: {kind}")
    for key in ("dres", "gate", "dx16"):
        for val in (0, 1):
            _need([r for r in rows if DM.opt(r, key) == val], f"backward with {key} = {val}")


def check_finalize_coverage():
    rows = DM.rows_of(DM.FINALIZE)
    assert {r.dims for r in rows} >= FINALIZE_DIMS
    chunks = {r.dims[1] for r in rows}
    _need(1 in chunks, "finalize: one chunk")
    _need([k for k in chunks if k > 1 and k % 8 == 0], "finalize: a multiple of 8 chunks")
    _need([k for k in chunks if k > 8 and k % 8], "finalize: a remainder after a full unroll")
    _need([k for k in chunks if 1 < k < 8], "finalize: fewer than 8 chunks")


def check_patch_coverage():
    have = {(r.dims, DM.opt(r, "f32"), DM.opt(r, "pad")) for r in DM.rows_of(DM.TO_NCHW)}
    assert have >= set(itertools.product(PATCH_DIMS, (0, 1), (0, 3))), "tokens_to_nchw: shape x src_f32 x ld"
    have = {(r.dims, DM.opt(r, "pad")) for r in DM.rows_of(DM.TO_TOKENS)}
    assert have >= set(itertools.product(PATCH_DIMS, (0, 3))), "nchw_to_tokens: shape x ld"
    mse = DM.rows_of(DM.MSE)
    assert {(r.dims, DM.opt(r, "pad")) for r in mse} >= set(itertools.product(PATCH_DIMS, (0, 3))), "mse: shape x ld"
    assert {(DM.opt(r, "gs"), DM.opt(r, "grad")) for r in mse} == set(itertools.product(("val", "dev"), (0, 1)))
    for pad in (0, 3):
        assert {DM.opt(r, "gs") for r in mse if DM.opt(r, "pad") == pad} == {"val", "dev"}
        assert {DM.opt(r, "grad") for r in mse if DM.opt(r, "pad") == pad} == {0, 1}

    def elements(r):
        rows, K = DM.patch_dims(*r.dims)
        return rows * (K + DM.opt(r, "pad"))
    _need([r for r in mse if elements(r) > 1024 * 256 and r.launches[0][1] == 1024 and DM.opt(r, "grad")],
          "mse_patch: the capped grid")
    _need([r for r in mse if elements(r) <= 256], "mse_patch: one workgroup")
    for rows in (DM.rows_of(DM.TO_NCHW), DM.rows_of(DM.TO_TOKENS), mse):
        _need([r for r in rows if r.dims[2] < r.dims[3]], "patch: H < W")
        _need([r for r in rows if r.dims[2] > r.dims[3]], "patch: H > W")
        assert {r.dims[4] for r in rows} >= {1, 2, 4}


COVERAGE = (check_forward_coverage, check_backward_coverage, check_finalize_coverage, check_patch_coverage)


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
    """With any single row taken out of ROWS one of the coverage checks fails (on the test data only)."""
    full = list(DM.ROWS)
    assert not _noticed()
    for r in full:
        monkeypatch.setattr(DM, "ROWS", [x for x in full if x is not r])
        assert _noticed(), f"ROWS without {DM.row_id(r)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------
def _ln_shapes():
    return sorted({r.dims for r in DM.rows_of(DM.LN_FWD, DM.LN_BWD)})


@pytest.mark.parametrize("shape", _ln_shapes(), ids=str)
def test_exact_layernorm_family_is_exact(shape):
    B, N, C = shape
    c = DM.ln_case("exact", B, N, C)
    rows = B * N
    for name in ("x", "v", "dy", "dres", "shift", "scale", "gate"):
        assert DM.is_bf16(c[name]), f"{name} is not exact in bf16"
    assert float(c["x"].abs().max()) <= 8 and all(float(c[k].abs().max()) <= 4 for k in ("v", "dy", "dres"))
    for k in ("gate", "scale"):
        assert bool((torch.log2(c[k].abs()) % 1 == 0).all()) and bool((c[k] != -1).all())
    assert bool(((c["shift"] * 8) % 1 == 0).all())
    for res in ("none", "v", "gate"):
        xo = DM.xo_reference(c, res, 1)
        assert torch.equal(xo, DM.xo_unrounded(c, res)) and DM.is_bf16(xo), "x + g v is not exact in bf16"
        assert torch.equal(xo, DM.xo_reference(c, res, 0))
        # sums in units of 2^-7 stay below 2^24, so any order gives the same fp32 bits
        assert float((xo.abs().sum(1) * 128).max()) < 2 ** 24 and bool(((xo * 128) % 1 == 0).all())
        st = DM.row_stats(xo)
        ems = [DM.emulate_forward(c, xo, 1, order) for order in DM.ORDERS]
        assert torch.equal(ems[0]["mean"], ems[1]["mean"])
        bm, br = DM.stats_bounds("exact", C, st)
        for em in ems:
            assert bool(((em["mean"] - st["mean"]).abs() <= bm).all())
            assert bool(((em["rstd"] - st["rstd"]).abs() <= br).all())
        if DM.is_pow2(C):
            assert torch.equal(ems[0]["mean"], st["mean"])
        if c["const"] is not None:
            i = c["const"]
            assert float(st["var"][i]) == 0.0 and float(ems[0]["mean"][i]) == 2.0
            assert torch.equal(ems[0]["y"][i], c["shift"][i // N])
        if c["near"] is not None:
            i = c["near"]
            assert 0.0 < float(st["var"][i]) <= 1.6e-5
            # var <= 1.6e-5: eps = 1e-5 for 1e-6 moves rstd by sqrt(1.7e-5 / 2.6e-5) = 0.81 at the least
            assert float(DM.row_stats(xo, eps=1e-5)["rstd"][i] / st["rstd"][i]) < 0.82, "eps does not decide this rstd"
    assert (c["const"] is None) == (rows < 2) and (c["near"] is None) == (rows < 3)
    ordinary = set(range(rows)) - {c["const"], c["near"]}
    assert ordinary, "no ordinary row left"
    psh, T = DM.chunk_sums(c["dy"], c)
    assert float(T.max()) < 2 ** 24
    for order in DM.ORDERS:
        assert torch.equal(DM.chunk_sum32(c["dy"].float(), N, order).double(), psh)


@pytest.mark.parametrize("row", DM.rows_of(DM.FINALIZE), ids=DM.row_id)
def test_exact_finalize_family_is_exact(row):
    ws = DM.finalize_case("exact", *row.dims)
    ref, T = DM.finalize_reference(ws)
    assert float(T.max()) < 2 ** 24 and bool((ws % 1 == 0).all())
    for order in DM.ORDERS:
        assert torch.equal(DM.emulate_finalize(ws, order), ref)


def _mse_rows():
    seen = {}
    for r in DM.rows_of(DM.MSE):
        seen.setdefault((r.dims, DM.opt(r, "pad")), r)
    return list(seen.values())


@pytest.mark.parametrize("row", _mse_rows(), ids=DM.row_id)
def test_exact_mse_family_is_exact(row):
    c = DM.patch_case("exact", *row.dims)
    m = DM.mse_reference(c, row.dims)
    B, C, H, W, p = row.dims
    assert bool((m["d"] % 1 == 0).all()) and float(m["d"].abs().max()) <= 6
    assert 36.0 * m["d"].numel() < 2 ** 24 and float(m["S"]) % 1 == 0
    want = float(np.float32(float(m["S"])) * (np.float32(1.0) / np.float32(m["n"])))
    for order in DM.ORDERS:
        assert DM.emulate_mse(c, row.dims, DM.opt(row, "pad"), order) == want
    if DM.is_pow2(B * C * H * W):
        assert DM.is_bf16(m["grad"]), "grad is not exact in bf16 although n and gscale are powers of two"


# ----------------------------------------------------------------------------------------------------------------
# the bounds: emulated ratios and perturbed references
# ----------------------------------------------------------------------------------------------------------------
def _ratio(err, lim):
    return float((err / lim.clamp_min(1e-300)).max())


def _violates(pert, ref, lim):
    return bool(((pert - ref).abs() > lim).any())


@functools.lru_cache(maxsize=None)
def _forward(row):
    """Emulated error / (u T) per quantity (the larger of the two orders) and which perturbations leave a bound."""
    B, N, C = row.dims
    f32, res, mod = (DM.opt(row, k) for k in ("f32", "res", "mod"))
    c = DM.ln_case("soft", B, N, C, f32)
    xo = DM.xo_reference(c, res, f32)
    st = DM.row_stats(xo)
    bm, br = DM.stats_bounds("soft", C, st)
    m = dict(mean=0.0, var=0.0, y=0.0)
    for order in DM.ORDERS:
        em = DM.emulate_forward(c, xo, mod, order)
        excess = ((em["mean"] - st["mean"]).abs() - 2.0 ** -23 * st["mean"].abs()).clamp_min(0.0)
        m["mean"] = max(m["mean"], _ratio(excess, DM.U24 * st["eabs"]))
        m["var"] = max(m["var"], _ratio((em["ve"] - (st["var"] + DM.EPS)).abs(), DM.U24 * (st["var"] + DM.EPS)))
        assert not _violates(em["mean"], st["mean"], bm) and not _violates(em["rstd"], st["rstd"], br)
        ref, lim, T = DM.y_reference(c, xo, em["mean"], em["rstd"], mod)
        m["y"] = max(m["y"], _ratio((em["y"] - ref).abs(), DM.U24 * T))
        assert not _violates(DM.bf16(em["y"]), ref, lim)
    caught = {}

    def stats_leave(name, pert):
        caught[name] = _violates(pert["mean"], st["mean"], bm) or _violates(pert["rstd"], st["rstd"], br)
    stats_leave("variance over C - 1", DM.row_stats(xo, ddof=1))
    stats_leave("eps = 1e-5", DM.row_stats(xo, eps=1e-5))
    if C != 512:
        stats_leave("statistics divided by 512", DM.row_stats(xo, div=512))
    mean, rstd = st["mean"].float().double(), st["rstd"].float().double()
    ref, lim, _ = DM.y_reference(c, xo, mean, rstd, mod)
    if mod:
        if B > 1:
            caught["the neighbouring sample's modulation row"] = _violates(
                DM.y_reference(c, xo, mean, rstd, mod, neighbour=True)[0], ref, lim)
        caught["scale in place of 1 + scale"] = _violates(
            DM.y_reference(c, xo, mean, rstd, mod, scale_only=True)[0], ref, lim)
    if res == "gate":
        caught["the gate ignored"] = not torch.equal(DM.xo_reference(c, res, f32, ignore_gate=True), xo)
    if res != "none" and not f32:
        stats_leave("the gated residual not re-rounded", DM.row_stats(DM.xo_unrounded(c, res)))
    return m, caught


@functools.lru_cache(maxsize=None)
def _backward(row):
    B, N, C = row.dims
    f32, mod, dres, gate = (DM.opt(row, k) for k in ("f32", "mod", "dres", "gate"))
    c = DM.ln_case("soft", B, N, C, f32)
    mean, rstd = DM.host_stats(c["x"])
    bw = DM.bwd_reference(c, mean, rstd, mod, dres)
    lim = DM.dx_bound(bw["dx"], bw["T"], f32)
    psh, Tsh = DM.chunk_sums(c["dy"], c)
    psc, Tsc = DM.chunk_sums(c["dy"] * bw["xh"], c)
    m = dict(dx=0.0, psh=0.0, psc=0.0, pg=0.0)
    for order in DM.ORDERS:
        em = DM.emulate_backward(c, mean, rstd, mod, dres, f32, order)
        m["dx"] = max(m["dx"], _ratio((em["dx"] - bw["dx"]).abs(), DM.U24 * bw["T"]))
        assert not _violates(em["stored"], bw["dx"], lim)
        m["psh"] = max(m["psh"], _ratio((em["psh"] - psh).abs(), DM.U24 * Tsh))
        m["psc"] = max(m["psc"], _ratio((em["psc"] - psc).abs(), DM.U24 * Tsc))
        pg, Tg = DM.chunk_sums(em["stored"] * c["v"], c)
        m["pg"] = max(m["pg"], _ratio((em["pg"] - pg).abs(), DM.U24 * Tg))
    caught = {}
    for name, kw in (("s1 dropped", dict(drop_s1=True)), ("s2 dropped", dict(drop_s2=True)),
                     ("s2 over C - 1", dict(s2_ddof=1))):
        caught[name] = _violates(DM.bwd_reference(c, mean, rstd, mod, dres, **kw)["dx"], bw["dx"], lim)
    if dres:
        caught["dres dropped"] = _violates(DM.bwd_reference(c, mean, rstd, mod, dres, drop_dres=True)["dx"],
                                           bw["dx"], lim)
    if mod in ("both", "psc"):
        caught["dscale from dxh"] = _violates(DM.chunk_sums(bw["dxh"] * bw["xh"], c)[0], psc, DM.sum_bound(Tsc))
    twice, without = torch.ones(B * N), torch.ones(B * N)
    twice[B * N - 1], without[0] = 2.0, 0.0
    terms = [("psh", c["dy"], psh, Tsh)] * (mod in ("both", "psh")) + \
        [("psc", c["dy"] * bw["xh"], psc, Tsc)] * (mod in ("both", "psc"))
    if gate:
        stored = bw["dx"] if f32 else DM.bf16(bw["dx"])
        pg, Tg = DM.chunk_sums(stored * c["v"], c)
        terms.append(("pg", stored * c["v"], pg, Tg))
    for what, t, ref, T in terms:
        caught[f"{what}: a token row doubled"] = _violates(DM.chunk_sums(t, c, twice)[0], ref, DM.sum_bound(T))
        caught[f"{what}: a token row omitted"] = _violates(DM.chunk_sums(t, c, without)[0], ref, DM.sum_bound(T))
    return m, caught


@functools.lru_cache(maxsize=None)
def _finalize(row):
    ws = DM.finalize_case("soft", *row.dims)
    ref, T = DM.finalize_reference(ws)
    m = dict(finalize=0.0)
    for order in DM.ORDERS:
        em = DM.emulate_finalize(ws, order)
        m["finalize"] = max(m["finalize"], _ratio((em - ref).abs(), DM.U24 * T))
        assert not _violates(DM.bf16(em), ref, DM.sum_bound(T, ref=ref))
    caught = {"one chunk omitted": _violates(DM.bf16(DM.finalize_reference(ws, skip=row.dims[1] - 1)[0]), ref,
                                             DM.sum_bound(T, ref=ref))}
    return m, caught


@functools.lru_cache(maxsize=None)
def _mse(row):
    c = DM.patch_case("soft", *row.dims)
    B, C, H, W, p = row.dims
    ref = DM.mse_reference(c, row.dims)
    m = dict(loss=0.0)
    for order in DM.ORDERS:
        m["loss"] = max(m["loss"], abs(DM.emulate_mse(c, row.dims, DM.opt(row, "pad"), order) - float(ref["loss"])) /
                        (DM.U24 * float(ref["loss"])))
    # the fp32 gradient before its bf16 rounding: the subtraction, the division and the product, 3 roundoffs of 4
    d32 = c["pred"].float() - DM.tokens_of(c["target"], p).float()
    g32 = (2.0 * d32 / torch.tensor(ref["n"], dtype=torch.float32) * torch.tensor(c["gscale"], dtype=torch.float32))
    assert not _violates(DM.bf16(g32.double()), ref["grad"], DM.grad_bound(ref["grad"]))
    caught = {}
    if DM.patch_dims(*row.dims)[0] != B * C * H * W:
        wrong = DM.mse_reference(c, row.dims, by_tokens=True)
        caught["MSE divided by the token count"] = \
            abs(float(wrong["loss"] - ref["loss"])) > DM.K_SUM * DM.U24 * float(ref["loss"]) and \
            _violates(wrong["grad"], ref["grad"], DM.grad_bound(ref["grad"]))
    return m, caught


def _layout_caught(dims):
    B, C, H, W, p = dims
    img = DM.patch_case("soft", *dims)["img"]
    rows, K = DM.patch_dims(*dims)
    tok = DM.tokens_of(img, p)
    assert torch.equal(tok, img.reshape(-1)[DM.nchw_index(rows, K, C, H, W, p)]), "the two statements of the map differ"
    caught = {}
    swapped = img.reshape(-1)[DM.nchw_index(rows, K, C, W, H, p)]
    if H != W:
        caught["H and W exchanged"] = not torch.equal(swapped, tok)
    else:
        assert torch.equal(swapped, tok), "a swap of H and W is invisible at H = W: such a row proves nothing"
    if p > 1:
        caught["ph and pw exchanged"] = not torch.equal(DM.tokens_of(img, p, swap_taps=True), tok)
    return caught


MEASURES = ((DM.LN_FWD, _forward), (DM.LN_BWD, _backward), (DM.FINALIZE, _finalize), (DM.MSE, _mse))
SOFT_ROWS = [(f, r) for entry, f in MEASURES for r in DM.rows_of(entry)]


@pytest.mark.parametrize("f,row", SOFT_ROWS, ids=lambda v: DM.row_id(v) if isinstance(v, DM.Row) else "")
def test_the_emulation_stays_within_half_the_constant(f, row):
    m, caught = f(row)
    print(f"{DM.row_id(row)}: emulated error / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()) +
          "; leaves its bound: " + ", ".join(k for k, v in caught.items() if v))
    assert max(m.values()) <= DM.K_SUM / 2, m


def test_the_constant_is_twice_the_emulated_ratio():
    worst = {}
    for f, row in SOFT_ROWS:
        for k, v in f(row)[0].items():
            worst[k] = max(worst.get(k, 0.0), v)
    top = max(worst.values())
    print("largest emulated error / (u T): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) +
          f"; K_SUM {DM.K_SUM}")
    assert 2 * top <= DM.K_SUM <= 3 * top


FORWARD_PERTURBATIONS = ("variance over C - 1", "eps = 1e-5", "statistics divided by 512",
                         "the neighbouring sample's modulation row", "scale in place of 1 + scale", "the gate ignored",
                         "the gated residual not re-rounded")
BACKWARD_PERTURBATIONS = ("s1 dropped", "s2 dropped", "s2 over C - 1", "dres dropped", "dscale from dxh") + tuple(
    f"{p}: a token row {how}" for p in ("psh", "psc", "pg") for how in ("doubled", "omitted"))


@pytest.mark.parametrize("entry,f,names", ((DM.LN_FWD, _forward, FORWARD_PERTURBATIONS),
                                           (DM.LN_BWD, _backward, BACKWARD_PERTURBATIONS),
                                           (DM.FINALIZE, _finalize, ("one chunk omitted",)),
                                           (DM.MSE, _mse, ("MSE divided by the token count",))),
                         ids=lambda v: v if isinstance(v, str) else "")
def test_every_perturbed_reference_leaves_its_bound(entry, f, names):
    """On at least one row of its entry point, among the rows on which it applies (modulation given, a gate, dres, the
    partial pointer present, C != 512, more than one sample); the counts are printed."""
    by_name = {}
    for row in DM.rows_of(entry):
        for k, v in f(row)[1].items():
            by_name.setdefault(k, []).append((DM.row_id(row), v))
    assert set(by_name) == set(names)
    for name in names:
        hit = [rid for rid, v in by_name[name] if v]
        print(f"{name}: leaves its bound on {len(hit)} of {len(by_name[name])} rows")
        assert hit, f"{name} passes on every row of {entry}"


def test_a_wrong_index_map_is_seen():
    for entry in (DM.TO_NCHW, DM.TO_TOKENS, DM.MSE):
        seen = {}
        for dims in {r.dims for r in DM.rows_of(entry)} - {CAPPED}:
            for k, v in _layout_caught(dims).items():
                seen[k] = seen.get(k, False) or v
        assert seen == {"H and W exchanged": True, "ph and pw exchanged": True}, (entry, seen)


def test_butterfly_and_chunk_order():
    """The emulation's orders at points worked out by hand: 2^24 + 1 + 1 is 2^24 when the ones come one by one and
    2^24 + 2 when they are added first."""
    big = 2.0 ** 24
    t = torch.zeros(1, 512, dtype=torch.float32)
    t[0, 0], t[0, 1], t[0, 2] = big, 1.0, 1.0            # one lane, in sequence
    assert float(DM.row_sum32(t, "kernel")) == big
    t = torch.zeros(1, 512, dtype=torch.float32)
    t[0, 0], t[0, 8], t[0, 264] = big, 1.0, 1.0          # lanes 0, 1 and 33: (0 + 32), (1 + 33) first
    assert float(DM.row_sum32(t, "kernel")) == big + 2
    v = torch.zeros(8, 1, dtype=torch.float32)
    v[0, 0], v[4, 0], v[1, 0] = big, 1.0, 1.0            # wave 0 takes rows 0 and 4, wave 1 row 1
    assert float(DM.chunk_sum32(v, 8, "kernel")) == big
    v = torch.zeros(8, 1, dtype=torch.float32)
    v[0, 0], v[1, 0], v[5, 0] = big, 1.0, 1.0            # wave 1 adds rows 1 and 5 before the waves meet
    assert float(DM.chunk_sum32(v, 8, "kernel")) == big + 2
