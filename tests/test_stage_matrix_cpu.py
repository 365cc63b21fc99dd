"""The staging / packing / loss / leaf test matrix cannot fall behind the host code, its references are the operations
themselves and its bounds have teeth (CPU only; the library is loaded only for the error returns, which come before any
launch).

Each row of tests/stage_matrix.py ROWS launches what the restated host rules give; the rules hold at known points; no
row can be removed without a named need losing its only cover; the index models and float64 references agree with torch
on the CPU for the same operation; every constant is twice the ratio its fp32 emulation reaches (plus its labelled
library allowance); every perturbed reference leaves its statement."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stage_matrix as M

opt = M.opt


def test_rows_follow_the_restated_rules():
    assert len({M.row_id(r) for r in M.ROWS}) == len(M.ROWS)
    for r in M.ROWS:
        assert r.entry in M.ENTRIES
        assert list(r.launches) == M.expected_launches(r.entry, r.dims, r.opt), M.row_id(r)


def test_the_restated_rules_at_known_points():
    assert [M.grid_for(n) for n in (0, 1, 256, 257, 8192 * 256, 8192 * 256 + 1, 2 ** 40)] == [1, 1, 1, 2, 8192, 8192, 8192]
    assert [M.prep_grid(n) for n in (0, 1, 64, 65, 65536 * 64, 65536 * 64 + 1)] == [1, 1, 1, 2, 65536, 65536]
    assert [M.grid_of(n) for n in (0, 1, 257, 65535 * 8 * 256 + 1)] == [1, 1, 2, 65535 * 8]
    assert [M.mse_blocks(n) for n in (1, 257, 1024 * 256, 1024 * 256 + 1, 8192 * 256)] == [1, 2, 1024, 1024, 1024]
    assert M.mse_workspace() == 4096 and M.CAPPED == 17 * 123377 and M.CAPPED > M.GRID_CAP * M.NT
    lin = M.spec(O=57, I=72, Ipad=72, KH=1, KW=1, layout="nat")
    assert M.pack_rows(lin) == 56 and M.pack_bmap((lin, lin)) == [(0, 0), (0, 56), (1, 0), (1, 56)]
    assert M.pack_rows(M.spec(O=2, I=1010, Ipad=1016, KH=4, KW=4, layout="conv")) == 1 and 16 * (1016 + 8) == M.PACK_LDS
    assert M.pack_path(lin, 0) == "ident" and M.pack_path(M.spec(src_off=4, **dict(lin)), 0) == "onepass"
    assert M.pack_path(M.spec(src_off=4, **dict(lin)), 56) == "perrow"
    assert M.pack_strides(M.spec(O=3, I=5, Ipad=8, KH=3, KW=2, layout="conv", flip=1))[:8] == (30, 6, 2, 1, 2, -1, 1, -1)
    assert M.pack_strides(M.spec(O=3, I=5, Ipad=8, KH=2, KW=2, SKH=4, SKW=4, layout="nat", phase=(1, 0)))[:8] == \
        (80, 1, 20, 5, 1, 2, 0, 2)
    t = M.spec(O=72, I=130, smap=(1, 0), staps=2)
    assert len(M.tpack_bmap((t,))) == 3 * 2 * 2 and M.tpack_bmap((t,))[:3] == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 64, 0)]
    assert M.tpack_dims(t) == (272, 136, 144, 72)
    assert M.expected_launches(M.CW, (1, 8, 8, 16, 18), (("family", "soft"),)) == [(M.K_CW0, 288 * 32), (M.K_CWF, 2)]
    assert M.expected_launches(M.MODB, (3, 5, 65)) == [(M.K_MODB, 6)] and M.expected_launches(M.AMAP, (3, 2, 5, 7, 1)) == \
        [(M.K_AMAP, 15)]
    assert M.cw_split(5) == (1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)] + [(5, 5)] * 27)
    assert M.cw_split(8320)[0] == 260 and M.cw_split(33)[1][16] == (32, 33) and M.cw_split(33)[1][17] == (33, 33)


def test_a_pack_workgroup_of_several_rows_always_fits_the_one_pass_path():
    """With block maps built by the documented rule nrows * taps * (Ipad + 8) <= 8192 whenever nrows > 1, so the per-row
    loop runs only for workgroups of exactly one row: row > 2048, or a tail with O mod rows == 1."""
    for taps in (1, 2, 3, 4, 9, 16, 25):
        for Ipad in range(8, 4200, 8):
            rows = max(1, M.PACK_CHUNK // (taps * Ipad))
            if rows > 1:
                assert rows * taps * (Ipad + 8) <= M.PACK_LDS // 2, (taps, Ipad)
            else:
                assert taps * Ipad > M.PACK_CHUNK // 2
    for r in M.rows_of(M.PACK):
        descs = opt(r, "descs")
        for (j, o), (path, taps) in zip(M.pack_bmap(descs), M.pack_paths(descs)):
            d = dict(descs[j])
            nrows = min(d["O"], o + M.pack_rows(descs[j])) - o
            assert (path == "perrow") == (nrows == 1 and path != "ident"), M.row_id(r)
            assert taps * (d["Ipad"] + 8) <= M.PACK_LDS, "a descriptor outside the documented LDS limit"


# ----------------------------------------------------------------------------------------------------------------
# coverage: every named need has a row, and every row is the only cover of some named need
# ----------------------------------------------------------------------------------------------------------------
def _is(row, entry, dims=None, **o):
    return row.entry == entry and (dims is None or row.dims == tuple(dims)) and dict(row.opt) == o


def _pack_is(r, paths=None, **f):
    """A single-descriptor PACK row whose descriptor holds the fields f and whose workgroups take `paths`."""
    if r.entry != M.PACK or len(opt(r, "descs")) != 1:
        return False
    d = dict(opt(r, "descs")[0])
    return all(d.get(k) == v for k, v in f.items()) and (paths is None or M.pack_paths(opt(r, "descs")) == paths)


def _tp_is(r, **f):
    if r.entry != M.TPACK or len(opt(r, "descs")) != 1:
        return False
    d = dict(opt(r, "descs")[0])
    return all(d.get(k) == v for k, v in f.items())


def _needs():
    need = []
    add = lambda what, pred: need.append((what, pred))  # noqa: E731
    capped = lambda r: r.launches[0][1] == M.GRID_CAP  # noqa: E731
    for f in (0, 1):
        add(f"nhwc_to_nchw src_f32 {f}, ld > C", lambda r, f=f: r.entry == M.N2C and opt(r, "f32") == f and r.dims[3] > r.dims[1] and r.dims[2] > 1 and not capped(r))
        add(f"nhwc_to_nchw src_f32 {f}, ld = C = 8", lambda r, f=f: r.entry == M.N2C and opt(r, "f32") == f and r.dims[3] == r.dims[1] == 8)
    add("nhwc_to_nchw HW = 1", lambda r: r.entry == M.N2C and r.dims[2] == 1 and r.dims[0] > 256)
    add("nhwc_to_nchw past the grid cap", lambda r: r.entry == M.N2C and capped(r) and r.dims[0] * r.dims[1] * r.dims[2] == M.CAPPED)
    add("nchw_to_nhwc C < ld", lambda r: r.entry == M.C2N and r.dims[1] < r.dims[3] and r.dims[2] > 1 and not capped(r))
    add("nchw_to_nhwc C = ld", lambda r: r.entry == M.C2N and r.dims[1] == r.dims[3])
    add("nchw_to_nhwc HW = 1 with many rows", lambda r: r.entry == M.C2N and r.dims[2] == 1 and r.dims[0] > 256)
    add("nchw_to_nhwc past the grid cap", lambda r: r.entry == M.C2N and capped(r) and r.dims[0] * r.dims[2] * r.dims[3] > M.GRID_CAP * M.NT)
    for acc in (0, 1):
        add(f"copy_slice acc {acc}, lds = ldd = C", lambda r, a=acc: r.entry == M.SLICE and opt(r, "acc") == a and r.dims[1] == r.dims[2] == r.dims[3])
        add(f"copy_slice acc {acc}, lds != ldd, C below both", lambda r, a=acc: r.entry == M.SLICE and opt(r, "acc") == a and
            r.dims[2] != r.dims[3] and r.dims[1] < min(r.dims[2:]) and r.dims[0] > 1)
        add(f"copy_slice acc {acc} past the grid cap", lambda r, a=acc: r.entry == M.SLICE and opt(r, "acc") == a and capped(r) and
            r.dims[0] * r.dims[1] // 8 > M.GRID_CAP * M.NT)
    add("copy_slice P = 1", lambda r: r.entry == M.SLICE and r.dims[0] == 1)
    for n in (1, 255, 256, 257, M.CAPPED):
        for b in (0, 1):
            add(f"relu n = {n} bwd {b}", lambda r, n=n, b=b: _is(r, M.RELU, (n,), bwd=b))
    add("resize down in y, up in x", lambda r: r.entry == M.RESIZE and r.dims[1] > r.dims[3] and r.dims[2] < r.dims[4] and r.dims[1] % r.dims[3] and r.dims[4] % r.dims[2])
    add("resize up in y, down in x", lambda r: r.entry == M.RESIZE and r.dims[1] < r.dims[3] and r.dims[2] > r.dims[4] and r.dims[3] % r.dims[1] and r.dims[2] % r.dims[4] and r.dims[0] > 1)
    add("resize down in both, several blocks", lambda r: r.entry == M.RESIZE and r.dims[1] > r.dims[3] and r.dims[2] > r.dims[4] and r.launches[0][1] > 8)
    add("resize identity", lambda r: r.entry == M.RESIZE and r.dims[1:3] == r.dims[3:5])
    add("resize BC = 1", lambda r: r.entry == M.RESIZE and r.dims[0] == 1)
    add("chan_copy whole", lambda r: r.entry == M.CHAN and r.dims[1] == r.dims[3] == r.dims[5] and r.dims[2] > 1)
    add("chan_copy into the middle", lambda r: r.entry == M.CHAN and r.dims[5] > r.dims[1] + r.dims[6] and r.dims[6] > 0 and r.dims[3] == r.dims[1])
    add("chan_copy out of the middle", lambda r: r.entry == M.CHAN and r.dims[3] > r.dims[1] + r.dims[4] and r.dims[4] > 0 and r.dims[5] == r.dims[1])
    add("chan_copy of one element", lambda r: r.entry == M.CHAN and r.dims[:3] == (1, 1, 1))
    add("pack identity fast path, one-row tail", lambda r: _pack_is(r, [("ident", 1)] * 2, O=57, I=72, src_off=None))
    add("pack the same off a 16-byte boundary", lambda r: _pack_is(r, [("onepass", 1), ("perrow", 1)], O=57, I=72, src_off=4))
    add("pack one pass, channel-slow", lambda r: _pack_is(r, [("onepass", 9)], layout="conv", I=4, Ipad=8, flip=None, dst_ld=None))
    add("pack one pass, channel-fast, a partly padded group", lambda r: _pack_is(r, [("onepass", 9)], layout="nat", I=12, Ipad=16))
    add("pack one pass, channel-fast, a wholly padded group", lambda r: _pack_is(r, [("onepass", 9)], layout="nat", I=4, Ipad=16))
    for taps, f in ((1, dict(I=2304)), (4, dict(Ipad=520)), (9, dict(Ipad=256)), (16, dict(Ipad=136)), (3, dict(KH=1, KW=3))):
        add(f"pack per row, {taps} taps", lambda r, t=taps, f=f: _pack_is(r, [("perrow", t)] * 3, O=3, **f))
    add("pack at the LDS limit", lambda r: _pack_is(r, [("perrow", 16)] * 2, Ipad=1016))
    add("pack a one-row tail after full workgroups", lambda r: _pack_is(r, [("onepass", 9)] * 2 + [("perrow", 9)], O=113))
    add("pack flipped taps", lambda r: _pack_is(r, flip=1))
    add("pack a sub-pixel phase", lambda r: _pack_is(r, phase=(1, 0), SKH=4, SKW=4, KH=2, KW=2))
    add("pack into a column slice", lambda r: _pack_is(r, dst_ld=136, col0=16))
    add("pack several descriptors", lambda r: r.entry == M.PACK and len(opt(r, "descs")) > 1)
    add("transpose one full tile", lambda r: _tp_is(r, O=64, I=64))
    add("transpose edge tiles", lambda r: _tp_is(r, O=40, I=72))
    add("transpose 9 reversed taps", lambda r: _tp_is(r, smap=tuple(range(8, -1, -1))))
    add("transpose 4 taps of 16", lambda r: _tp_is(r, staps=16) and len(dict(opt(r, "descs")[0])["smap"]) == 4)
    add("transpose into wider dst_ld and dst_tap", lambda r: _tp_is(r, dst_tap=80, dst_pad=24))
    add("transpose several descriptors", lambda r: r.entry == M.TPACK and len(opt(r, "descs")) > 1)
    add("prep without a mask", lambda r: r.entry == M.PREP and opt(r, "mask") is None and r.dims[2] * r.dims[3] < 100)
    for px in (1, 63, 64, 65):
        add(f"prep {px} pixels", lambda r, px=px: r.entry == M.PREP and r.dims[0] * r.dims[2] * r.dims[3] == px and opt(r, "mask") == "soft" and r.dims[1] + opt(r, "cmo") == r.dims[4] == 8)
    add("prep fp32 mask up-scaled with keep, cpad 16 full", lambda r: r.entry == M.PREP and opt(r, "mask") == "soft" and opt(r, "keep") and opt(r, "MH") == 7 and r.dims[1] + opt(r, "cmo") == r.dims[4] == 16)
    add("prep fp32 mask down-scaled without keep, rest zero", lambda r: r.entry == M.PREP and opt(r, "mask") == "soft" and not opt(r, "keep") and opt(r, "MH") == 48 and r.dims[1] + opt(r, "cmo") < r.dims[4])
    add("prep class map with keep", lambda r: r.entry == M.PREP and opt(r, "mask") == "cmap" and opt(r, "keep") and opt(r, "MH") == 7)
    add("prep class map without keep", lambda r: r.entry == M.PREP and opt(r, "mask") == "cmap" and not opt(r, "keep"))
    add("prep class map down-scaled, cpad 16", lambda r: r.entry == M.PREP and opt(r, "mask") == "cmap" and opt(r, "MH") == 48 and r.dims[4] == 16)
    add("prep past the grid cap", lambda r: r.entry == M.PREP and r.launches[0][1] == M.PREP_CAP and r.dims[2] * r.dims[3] > M.PREP_CAP * M.PREP_NT)
    for fam in ("exact", "soft"):
        for what, dims in (("5 pixels", (1, 1, 5, 2, 3)), ("32 pixels", (1, 4, 8, 2, 3)), ("33 pixels", (1, 3, 11, 2, 3)),
                           ("a chunk of 260", (2, 64, 65, 2, 3)), ("one (o, i)", (2, 8, 8, 1, 1)), ("16 x 18", (2, 16, 16, 16, 18)),
                           ("cmi = 255", (1, 8, 8, 1, 255))):
            add(f"cond_wgrad {fam} {what}", lambda r, fam=fam, dims=dims: r.entry == M.CW and r.dims == dims and opt(r, "family") == fam)
    add("mse a total of 1", lambda r: r.entry == M.MSE and np.prod(r.dims) == 1)
    add("mse a total of 256", lambda r: _is(r, M.MSE, (1, 1, 256, 1)))
    add("mse a total of 257", lambda r: _is(r, M.MSE, (1, 1, 257, 1)))
    for C in (3, 4, 8):
        add(f"mse ld = 8, C = {C}", lambda r, C=C: r.entry == M.MSE and r.dims[3] == 8 and r.dims[1] == C and r.dims[2] < 100 and opt(r, "grad", 1) and (C != 3 or not opt(r, "gdev")))
    add("mse gscale from the device, C < ld", lambda r: r.entry == M.MSE and opt(r, "gdev") and r.dims[1] == 3)
    add("mse without a gradient", lambda r: r.entry == M.MSE and opt(r, "grad") == 0)
    add("mse past its grid cap, ragged", lambda r: r.entry == M.MSE and r.launches[0][1] == M.MSE_CAP and (r.dims[0] * r.dims[2] * r.dims[3]) % (M.MSE_CAP * M.NT))
    add("mse past its grid cap, exact", lambda r: r.entry == M.MSE and r.launches[0][1] == M.MSE_CAP and M.mse_exact(r))
    for dim in (2, 6, 128, 512):
        add(f"time embedding dim {dim}", lambda r, dim=dim: r.entry == M.TEMB and r.dims[1] == dim == r.dims[2] and opt(r, "tstride", 1) and opt(r, "f32", 1))
    add("time embedding ld > dim", lambda r: r.entry == M.TEMB and r.dims[2] > r.dims[1])
    add("time embedding tstride 0, B > 1", lambda r: r.entry == M.TEMB and opt(r, "tstride") == 0 and r.dims[0] > 1)
    add("time embedding B = 1", lambda r: r.entry == M.TEMB and r.dims[0] == 1)
    add("time embedding without out_f32", lambda r: r.entry == M.TEMB and opt(r, "f32") == 0)
    add("silu forward, every bf16", lambda r: _is(r, M.SILU, (65536,), bwd=0))
    for k in range(4):
        add(f"silu backward, dy {M.SILU_DY[k]}", lambda r, k=k: _is(r, M.SILU, (65536,), bwd=1, dy=k))
    for rr in (0, 1):
        for t in (0, 1):
            for a in (0, 1):
                for l in (0, 1):
                    add(f"modulate fwd r {rr} t {t} alpha {a} ls6 {l}", lambda r, o=dict(r=rr, t=t, alpha=a, ls6=l): _is(r, M.MODF, (2, 5, 72), **o))
    add("modulate fwd over several blocks, C off 64", lambda r: r.entry == M.MODF and r.launches[0][1] > 8 and r.dims[2] % 64)
    for n in (1, 3, 4, 5, 37):
        add(f"modulate bwd N = {n}", lambda r, n=n: _is(r, M.MODB, (2, n, 72)))
    for C in (1, 63, 64, 65):
        add(f"modulate bwd C = {C}", lambda r, C=C: r.entry == M.MODB and r.dims[2] == C and opt(r, "ls6"))
    for k in ("dx", "ds", "dt"):
        add(f"modulate bwd without {k}", lambda r, k=k: r.entry == M.MODB and opt(r, "null") == k)
    for S in (1, 77, 255, 256, 257):
        add(f"attention map S = {S}", lambda r, S=S: r.entry == M.AMAP and r.dims[3] == S and r.dims[1] > 1 and r.dims[4] > 1 and not opt(r, "wide") and not opt(r, "big") and (S != 77 or opt(r, "avg")))
    for avg in (0, 1):
        add(f"attention map S = 4096, avg {avg}", lambda r, a=avg: r.entry == M.AMAP and r.dims[3] == 4096 and opt(r, "avg") == a)
        add(f"attention map scores around +-80, avg {avg}", lambda r, a=avg: r.entry == M.AMAP and opt(r, "big") and opt(r, "avg") == a)
    add("attention map H = 1", lambda r: r.entry == M.AMAP and r.dims[1] == 1)
    add("attention map d = 1", lambda r: r.entry == M.AMAP and r.dims[4] == 1)
    add("attention map ldq, ldk wider than H d", lambda r: r.entry == M.AMAP and opt(r, "wide"))
    return need


def _missing(rows, needs):
    return [what for what, pred in needs if not any(pred(r) for r in rows)]


def test_coverage():
    assert _missing(M.ROWS, _needs()) == []


def test_no_row_can_be_removed():
    needs = _needs()
    for r in M.ROWS:
        assert _missing([y for y in M.ROWS if y is not r], needs), f"ROWS without {M.row_id(r)} passes every coverage check"


def test_the_data_families_hold_what_the_statements_need():
    x = M.movement_values(200, 1)
    b = M.bits(x.bfloat16())
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool((M.bits(x) == -2 ** 31).any())
    assert bool(((x != 0) & (x.abs() < 2.0 ** -126)).any()), "no fp32 denormal"
    assert bool(((x.bfloat16().float() != 0) & (x.bfloat16().float().abs() < 2.0 ** -126)).any()), "no bf16 denormal"
    ties = x[(M.bits(x) & 0xFFFF) == 0x8000]
    assert bool(((M.bits(ties) >> 16) & 1 == 0).any()) and bool(((M.bits(ties) >> 16) & 1 == 1).any()), "ties on both sides"
    assert bool((x.bfloat16().float().abs() == float("inf"))[torch.isfinite(x)].any()), "no finite value that rounds to inf"
    assert b.numel() == 200
    # one ulp in a bf16 tie: rounding half away from zero instead of to even differs on the family, and only at its ties
    fin = torch.isfinite(x)
    away = ((M.bits(x[fin]) + 0x8000) >> 16).to(torch.int16)
    tie = (M.bits(x[fin]) & 0xFFFF) == 0x8000
    assert not torch.equal(away, M.bits(x[fin].bfloat16())) and torch.equal(away[~tie], M.bits(x[fin].bfloat16())[~tie])
    for r in M.rows_of(M.SLICE):
        if opt(r, "acc") and r.dims[0] > 1:
            src, dst, after = M.slice_case(r)
            s = src[:, :r.dims[1]].float() + dst[:, :r.dims[1]].float()
            assert bool(((M.bits(s) & 0xFFFF) == 0x8000).any()) and bool((torch.isinf(s) & torch.isfinite(src[:, :r.dims[1]].float())).any())
    for r in M.rows_of(M.PREP):
        if opt(r, "mask") == "cmap":
            cm, cmi = M.prep_case(r)["mask"], opt(r, "cmi")
            assert all(bool((cm == v).any()) for v in (0, 1, cmi, cmi + 1, 255))
        if opt(r, "keep"):
            assert set(M.prep_case(r)["keep"].tolist()) == {0.0, 1.0}
    for r in M.rows_of(M.CW):
        if opt(r, "family") == "exact":
            c = M.cw_case(r)
            assert float(M.cw_terms(r, c).abs().sum(1).max()) < 2 ** 24 and bool((c["mask"].sum(1) <= 1).all())
    for r in M.rows_of(M.TEMB):
        assert {0, 1, 999} <= set(M.temb_t(r).tolist()), M.row_id(r)
    big = [r for r in M.rows_of(M.AMAP) if opt(r, "big")]
    for r in big:
        p, T = M.amap_reference(r, M.amap_case(r))
        q = M.amap_case(r)["q"][:, :, :24].double().view(2, 3, 3, 8).transpose(1, 2)
        k = M.amap_case(r)["k"][:, :, :24].double().view(2, 77, 3, 8).transpose(1, 2)
        sc = (q @ k.transpose(-1, -2)) * M.amap_case(r)["scaling"]
        assert float(sc.max()) > 80 and float(sc.min()) < -80


# ----------------------------------------------------------------------------------------------------------------
# the references are the operations (torch on the CPU)
# ----------------------------------------------------------------------------------------------------------------
def _size_pairs():
    pairs = set()
    for r in M.ROWS:
        if r.entry == M.RESIZE:
            pairs |= {(r.dims[1], r.dims[3]), (r.dims[2], r.dims[4])}
        if r.entry in (M.PREP, M.CW) and (r.entry == M.CW or opt(r, "mask")):
            B, H, W, MH, MW = M._mask_dims(r)
            pairs |= {(MH, H), (MW, W)}
    return sorted(pairs)


def test_the_nearest_index_is_atens():
    assert (7, 10) in _size_pairs() and (48, 32) in _size_pairs() and (9, 20) in _size_pairs()
    for n_in, n_out in _size_pairs() + [(512, 32), (3, 1000), (1000, 3)]:
        assert torch.equal(M.nearest_index(n_in, n_out), M.nearest_index_torch(n_in, n_out)), (n_in, n_out)
    # the perturbed index (rounding instead of the floor) differs wherever the ratio is not an integer
    for n_in, n_out in ((7, 10), (5, 3), (48, 32), (40, 32), (7, 5), (9, 20), (9, 4), (48, 64), (40, 65)):
        assert (n_in, n_out) in _size_pairs()
        if n_in != n_out:
            assert not torch.equal(M.nearest_index(n_in, n_out, rounding=True), M.nearest_index(n_in, n_out)), (n_in, n_out)


def test_movers_against_torch():
    for r in M.rows_of(M.RESIZE):
        x, want = M.resize_case(r)
        ref = F.interpolate(torch.nan_to_num(x, nan=12345.0).unsqueeze(0), size=r.dims[3:]).squeeze(0)
        assert torch.equal(torch.nan_to_num(want, nan=12345.0), ref), M.row_id(r)
        if r.dims[1:3] != r.dims[3:5]:
            assert not M.eq_bits(M.resize_model(x, *r.dims[3:], rounding=True), want)
    for r in M.rows_of(M.CHAN):
        B, C, P, sC, sc0, dC, dc0 = r.dims
        src, dst, after = M.chan_case(r)
        ref = torch.cat([dst[:, :dc0], src[:, sc0:sc0 + C], dst[:, dc0 + C:]], dim=1)
        assert M.eq_bits(after, ref), M.row_id(r)
    for r in M.rows_of(M.N2C, M.C2N):
        if np.prod(r.dims[:3]) > 10 ** 6:
            continue
        B, C, HW, ld = r.dims
        if r.entry == M.N2C:
            src, want = M.n2c_case(r)
            ref = torch.stack([src[(b * HW + p), c].float() for b in range(B) for c in range(C) for p in range(HW)]).view(B, C, HW)
        else:
            src, want = M.c2n_case(r)
            ref = torch.stack([src[b, c, p].bfloat16() if c < C else torch.tensor(0.0).bfloat16() for b in range(B) for p in range(HW) for c in range(ld)]).view(B * HW, ld)
        assert M.eq_bits(want, ref), M.row_id(r)


def test_relu_model_against_torch_and_the_old_kernel():
    x, dy = M.relu_case(257)
    y, ref = M.relu_model(x), torch.relu(x)
    zero = (y == 0) & (ref == 0)
    assert bool((M.bits(y[zero]) == 0).all()), "the model returns +0 for either zero"
    assert bool((M.bits(ref[zero]) != 0).any()), "aten's CPU relu keeps -0: the one sign the model does not follow"
    assert M.eq_bits(y[~zero], ref[~zero]) and bool(torch.isnan(y[torch.isnan(x)]).all())
    g, gref = M.relu_model(x, dy), torch.ops.aten.threshold_backward(dy, x, 0)
    assert M.eq_bits(g, gref) and M.eq_bits(g[torch.isnan(x)], dy[torch.isnan(x)])
    # the kernel before its fix swallowed the NaN in both directions: the statement has teeth
    assert not M.eq_bits(M.relu_model_old(x), y) and not M.eq_bits(M.relu_model_old(x, dy), g)
    keep = ~torch.isnan(x)
    assert M.eq_bits(M.relu_model_old(x)[keep], y[keep]) and M.eq_bits(M.relu_model_old(x, dy)[keep], g[keep])


def test_pack_models_against_plain_loops():
    for r in M.rows_of(M.PACK):
        for j, d in enumerate(opt(r, "descs")):
            dd = dict(d)
            if dd["O"] * dd["I"] > 3000:
                continue
            so, si, skh, skw, kh_off, kh_mul, kw_off, kw_mul, _ = M.pack_strides(d)
            src = M.pack_source(d, j)
            flat, want = src.reshape(-1), M.pack_model(d, src)
            for o in range(0, dd["O"], 3):
                for a in range(dd["KH"]):
                    for b in range(dd["KW"]):
                        for i in range(dd["Ipad"]):
                            v = flat[o * so + i * si + (kh_off + kh_mul * a) * skh + (kw_off + kw_mul * b) * skw].bfloat16() \
                                if i < dd["I"] else torch.tensor(0.0).bfloat16()
                            assert M.eq_bits(want[o, (a * dd["KW"] + b) * dd["Ipad"] + i].view(1), v.view(1)), (M.row_id(r), o, a, b, i)
            # a packer that drops the last row of a chunk, ignores a flip or leaves a pad column differs
            assert not M.eq_bits(M.pack_model(d, src, drop_last_row=True), want)
            if dd.get("flip") or dd.get("phase"):
                assert not M.eq_bits(M.pack_model(d, src, no_flip=True), want)
            if dd["Ipad"] > dd["I"]:
                assert not M.eq_bits(M.pack_model(d, src, pad_garbage=True), want)
    for r in M.rows_of(M.TPACK):
        for j, d in enumerate(opt(r, "descs")):
            dd = dict(d)
            src_ld, src_tap, _, _ = M.tpack_dims(d)
            src = M.tpack_source(d, j)
            want = M.tpack_model(d, src)
            assert want.shape == (dd["I"], len(dd["smap"]), dd["O"])
            for i in range(0, dd["I"], 5):
                for t, sm in enumerate(dd["smap"]):
                    assert M.eq_bits(want[i, t], src[:, sm * src_tap + i]), (M.row_id(r), i, t)
            if tuple(dd["smap"]) != tuple(range(len(dd["smap"]))):
                assert not M.eq_bits(M.tpack_model(d, src, identity_smap=True), want)


def test_staging_references_against_torch():
    for r in M.rows_of(M.PREP):
        B, cx, H, W, cpad = r.dims
        if B * H * W > 10 ** 5:
            continue
        c = M.prep_case(r)
        ref = M.prep_reference(r, c)
        kind, cmi, cmo = opt(r, "mask"), opt(r, "cmi", 0), opt(r, "cmo", 0)
        assert M.eq_bits(ref["exact"][:, :cx], torch.nan_to_num(c["x"], nan=float("nan")).permute(0, 2, 3, 1).reshape(-1, cx).bfloat16())
        keep = (c["keep"] if c["keep"] is not None else torch.ones(B)).view(B, 1, 1, 1)
        if kind == "soft":
            t = F.conv2d(F.interpolate(c["mask"].double(), size=(H, W)), c["w"].double().view(cmo, cmi, 1, 1)) * keep.double()
            assert float((t.permute(0, 2, 3, 1).reshape(-1, cmo) - ref["ref"]).abs().max()) <= 1e-12
            worst = max(M.worst(M.prep_emulate(r, c, v), ref["ref"], M.U24 * ref["T"]) for v in M.VARIANTS)
            assert worst <= M.K_PREP / 2
            bad = M.prep_reference(r, c, rounding=True)
            assert M.worst(M.prep_emulate(r, c, "fused").float().bfloat16(), bad["ref"], M.prep_bound(bad["ref"], bad["T"])) > 10 \
                or (H, W) == (1, 1) or (opt(r, "MH", H), opt(r, "MW", W)) == (H, W)
        elif kind == "cmap":
            oh = F.interpolate(M.one_hot(c["mask"], cmi), size=(H, W))
            t = F.conv2d(oh, c["w"].view(cmo, cmi, 1, 1)) * keep
            assert M.eq_bits(ref["exact"][:, cx:cx + cmo], t.permute(0, 2, 3, 1).reshape(-1, cmo).bfloat16()), M.row_id(r)
            assert not M.eq_bits(M.prep_reference(r, c, clamp=False)["exact"], ref["exact"]), "the clamp of the class has teeth"
        assert bool((M.bits(ref["exact"][:, cx + cmo:].contiguous()) == 0).all())
    for r in M.rows_of(M.CW):
        B, H, W, cmo, cmi = r.dims
        c = M.cw_case(r)
        ref, T = M.cw_reference(r, c)
        w = torch.zeros(cmo, cmi, 1, 1, dtype=torch.float64, requires_grad=True)
        keep = (c["keep"] if c["keep"] is not None else torch.ones(B)).double().view(B, 1, 1, 1)
        y = F.conv2d(F.interpolate(c["mask"].double(), size=(H, W)), w) * keep
        dy = c["dx"][:, M.CW_CX:M.CW_CX + cmo].double().view(B, H, W, cmo).permute(0, 3, 1, 2)
        (y * dy).sum().backward()
        assert float((w.grad.view(-1) - ref).abs().max()) <= 1e-9 * max(1.0, float(T.max())), M.row_id(r)


def test_loss_embedding_and_leaf_references_against_torch():
    for r in M.rows_of(M.MSE):
        B, C, HW, ld = r.dims
        for fam in ("exact", "soft"):
            c = M.mse_case(r, fam)
            p = c["pred"].view(B, HW, ld)[:, :, :C].permute(0, 2, 1).double().clone().requires_grad_(True)
            loss = F.mse_loss(p, c["target"].double())
            loss.backward()
            assert abs(loss.item() - M.mse_reference(r, c)) <= 1e-12 * max(1.0, loss.item())
            g = M.mse_grad_model(r, c).view(B, HW, ld)
            want = (p.grad * c["gscale"]).permute(0, 2, 1)
            assert float(((g[:, :, :C].double() - want).abs() - 0.5 * M.ulp_bf16(want) - 4 * M.U24 * want.abs()).max()) <= 0
            assert bool((M.bits(g[:, :, C:].contiguous()) == 0).all())
            if ld > C:
                assert not M.eq_bits(M.mse_grad_model(r, c, n_pad=True), M.mse_grad_model(r, c))
    for r in M.rows_of(M.TEMB):
        t, dim = M.temb_t(r), r.dims[1]
        ref, a = M.temb_reference(t, dim)
        factor = 10000 ** ((torch.arange(start=0, end=dim // 2, dtype=torch.float32) / (dim // 2)))
        e = t[:, None].repeat(1, dim // 2) / factor
        e = torch.cat([torch.sin(e), torch.cos(e)], dim=-1)
        assert M.worst(e, ref, M.temb_bound(a)) <= 1.0, M.row_id(r)
        if opt(r, "t") == M.TGOLD:
            assert M.worst(M.golden_temb()[f"emb{dim}"], ref, M.temb_bound(a)) <= 1.0
    x = M.silu_x()
    ref, T = M.silu_reference(x)
    xf = x.float()
    tf = F.silu(xf)
    ok = ~torch.isnan(ref)
    assert float(((tf.double() - ref).abs() / (ref.abs() + 1e-300))[ok & torch.isfinite(ref) & ~M.silu_carved(x) & (ref.abs() > 1e-37)].max()) < 1e-5
    carved = M.silu_carved(x)
    assert int(carved.sum()) > 15000 and bool((M.bits(tf[carved]) == -2 ** 31).all()), "torch's fp32 silu gives -0 on every carved input"
    assert float(ref[carved].abs().max()) < 2.0e-37 and float(F.silu(torch.tensor(-88.5))) < -3e-37
    for dy in M.SILU_DY:
        xg = xf.clone().requires_grad_(True)
        F.silu(xg).backward(torch.full_like(xf, dy))
        assert bool((xg.grad[carved] == 0).all()), "torch's fp32 silu backward gives a zero on every carved input"
        rb, Tb = M.silu_reference(x, dy)
        xd = xf.double().clone().requires_grad_(True)
        F.silu(xd).backward(torch.full_like(xd, dy))
        fin = torch.isfinite(rb) & torch.isfinite(xd.grad)
        assert float(((xd.grad - rb).abs() - 1e-12 * Tb)[fin].max()) <= 0
    for r in M.rows_of(M.MODF):
        B, N, C = r.dims
        c = M.mod_case(r, "soft")
        y, _ = M.modf_reference(r, c)
        s, t = c["s"][:, :C].double().unsqueeze(1), c["t"][:, :C].double().unsqueeze(1)
        want = c["x"].double() * (c["alpha"] + s) + (t if opt(r, "t", 1) else 0) + (c["r"].double() if opt(r, "r", 1) else 0)
        assert float((want - y).abs().max()) <= 1e-12
    for r in M.rows_of(M.MODB):
        B, N, C = r.dims
        c = M.mod_case(r, "soft")
        ref = M.modb_reference(r, c)
        x, s, t = (v.double().clone().requires_grad_(True) for v in (c["x"], c["s"][:, :C], c["s"][:, :C] * 0))
        (x * (c["alpha"] + s.unsqueeze(1)) + t.unsqueeze(1)).backward(c["dy"].double())
        assert float((s.grad - ref["ds"]).abs().max()) <= 1e-12 and float((t.grad - ref["dt"]).abs().max()) <= 1e-12
        assert float((x.grad - ref["dx"].double()).abs().max()) <= 4 * M.U24 * float(x.grad.abs().max())
    for r in M.rows_of(M.AMAP):
        B, H, N, S, d = r.dims
        c = M.amap_case(r)
        p, T = M.amap_reference(r, c)
        qh = c["q"][:, :, :H * d].double().reshape(B, N, H, d).transpose(1, 2)
        kh = c["k"][:, :, :H * d].double().reshape(B, S, H, d).transpose(1, 2)
        want = torch.softmax(qh @ kh.transpose(-2, -1) * c["scaling"], dim=-1)
        assert float((want - p).abs().max()) <= 1e-12
        assert float((M.amap_out(r, p) - (want.mean(dim=1) if opt(r, "avg") else want)).abs().max()) <= 1e-14


# ----------------------------------------------------------------------------------------------------------------
# the constants are measured, and every perturbed reference leaves its statement
# ----------------------------------------------------------------------------------------------------------------
def _constant(name, ratio):
    K0 = M.KS[name] - M.ALLOW[name]
    assert abs(ratio - M.EMULATED[name]) <= 0.02 * max(1.0, ratio), f"{name}: emulated ratio {ratio}, the module says {M.EMULATED[name]}"
    assert ratio <= K0 / 2 and 2 * ratio <= K0 <= 3 * ratio, f"{name}: K - allowance = {K0} against an emulated ratio of {ratio}"


def test_prep_and_cond_wgrad_constants():
    worst = 0.0
    for r in M.rows_of(M.PREP):
        if opt(r, "mask") == "soft":
            c = M.prep_case(r)
            ref = M.prep_reference(r, c)
            worst = max([worst] + [M.worst(M.prep_emulate(r, c, v), ref["ref"], M.U24 * ref["T"]) for v in M.VARIANTS])
    _constant("prep", worst)
    worst = 0.0
    for r in M.rows_of(M.CW):
        c = M.cw_case(r)
        ref, T = M.cw_reference(r, c)
        total = r.dims[0] * r.dims[1] * r.dims[2]
        chunk, ranges = M.cw_split(total)
        lim = M.K_CW * M.U24 * T
        for v in M.VARIANTS:
            e = M.cw_emulate(r, c, v)
            if opt(r, "family") == "exact":
                assert torch.equal(e, ref), f"{M.row_id(r)}: the exact family is not exact in the kernel's order ({v})"
            else:
                worst = max(worst, M.worst(e, ref, M.U24 * T))
        # perturbed: one pixel, lane, wave, split dropped (of those that hold a nonzero term)
        term = M.cw_terms(r, c)
        p = int(term.abs().sum(0).argmax())
        z = p // chunk
        lane, wave = (p - z * chunk) % M.NT, ((p - z * chunk) % M.NT) // 64
        for drop in (("pixel", p), ("lane", lane), ("wave", wave), ("split", z)):
            e = M.cw_emulate(r, c, "fused", drop)
            if opt(r, "family") == "exact":
                assert not torch.equal(e, ref), (M.row_id(r), drop)
            elif total >= 32:
                assert M.worst(e, ref, lim) > 100, (M.row_id(r), drop)
        w = torch.ones(total, dtype=torch.float64)
        w[p] = 2.0
        assert not torch.equal(M.cw_reference(r, c, weights=w)[0], ref), "a pixel counted twice"
        _, _, _, MH, MW = M._mask_dims(r)
        if (MH, MW) != r.dims[1:3]:
            bad, _ = M.cw_reference(r, c, rounding=True)
            assert M.worst(M.cw_emulate(r, c, "fused"), bad, lim) > 100, "rounding instead of the floor in the nearest index"
    _constant("cw", worst)


def test_mse_constant_and_exact_family():
    worst = 0.0
    for r in M.rows_of(M.MSE):
        c = M.mse_case(r, "soft")
        ref = M.mse_reference(r, c)
        for v in M.VARIANTS:
            worst = max(worst, abs(M.mse_emulate(r, c, v) - ref) / (M.U24 * ref))
        ce = M.mse_case(r, "exact")
        if M.mse_exact(r):
            assert all(M.mse_emulate(r, ce, v) == M.mse_reference(r, ce) for v in M.VARIANTS), M.row_id(r)
        lim = M.K_MSE * M.U24 * ref
        if np.prod(r.dims[:3]) > 1:
            assert abs(M.mse_emulate(r, c, "fused", ("item", 0)) - ref) > lim or np.prod(r.dims[:3]) > 10 ** 4
            if M.mse_exact(r):
                assert M.mse_emulate(r, ce, "fused", ("item", 0)) != M.mse_reference(r, ce) or float(ce["pred"].abs().sum()) == 0
        if M.mse_blocks(r.dims[0] * r.dims[2] * r.dims[3]) > 1:
            assert abs(M.mse_emulate(r, c, "fused", ("block", 1)) - ref) > 100 * lim
        if r.dims[3] > r.dims[1]:
            assert abs(M.mse_emulate(r, c, "fused") - M.mse_reference(r, c, n_pad=True)) > 1000 * lim, "n off by the pad columns"
    _constant("mse", worst)


def test_time_embedding_constants():
    wa = ws = 0.0
    for r in M.rows_of(M.TEMB):
        t, dim = M.temb_t(r), r.dims[1]
        ref, a = M.temb_reference(t, dim)
        a32, e32 = M.temb_emulate(t, dim)
        wa = max(wa, M.worst(a32, a, M.U24 * a.abs()))
        h = dim // 2
        ws = max(ws, float((e32 - torch.cat([torch.sin(a32[:, :h]), torch.cos(a32[:, :h])], 1)).abs().max() / M.U24))
        assert M.worst(e32, ref, M.temb_bound(a, M.K_TA - M.ALLOW["ta"], M.K_TS - M.ALLOW["ts"])) <= 0.5
        assert M.worst(e32, M.temb_reference(t, dim, swap=True)[0], M.temb_bound(a)) > 1000, "sin and cos swapped"
        if dim > 2:
            assert M.worst(e32, M.temb_reference(t, dim, half_is_dim=True)[0], M.temb_bound(a)) > 1000, "half replaced by dim"
    _constant("ta", wa)
    _constant("ts", ws)


def test_silu_constants():
    x = M.silu_x()
    carved = M.silu_carved(x)
    ref, T = M.silu_reference(x)
    keep = ~carved & ~torch.isnan(ref)
    e = M.silu_emulate(x)
    _constant("silu", M.worst(e[keep], ref[keep], M.U24 * T[keep]))
    out = e.float().bfloat16()
    assert M.worst(out[keep], ref[keep], M.silu_bound(ref[keep], T[keep], M.K_S)) <= 1.0
    # a result one bf16 ulp off sits at the edge of the bound or outside: the half ulp is all the slack there is
    moved = (M.bits(out) + 1).view(torch.bfloat16)
    big = keep & (ref.abs() > 2.0 ** -100) & torch.isfinite(ref) & (ref.abs() < 1e30)
    r1 = ((moved[big].double() - ref[big]).abs() / M.silu_bound(ref[big], T[big], M.K_S))
    assert float(r1.min()) > 0.99 and float((r1 > 1).double().mean()) > 0.99
    worst = 0.0
    for dy in M.SILU_DY:
        ref, T = M.silu_reference(x, dy)
        keep = ~carved & ~torch.isnan(ref)
        for v in M.VARIANTS:
            worst = max(worst, M.worst(M.silu_emulate(x, dy, v)[keep], ref[keep], M.U24 * T[keep]))
        # the derivative's zero (x near -1.278) is inside the data and covered by T
        assert float(T[keep].min()) >= 0 and bool((ref[keep].abs() <= T[keep] * (1 + 1e-12)).all())
    _constant("silub", worst)
    assert M.ALLOW["silub"] == 4 * (1 + 17.5) and float(torch.sigmoid(torch.tensor(17.5)).float()) == 1.0


def test_modulate_constants_and_exact_family():
    wf = ws = wt = 0.0
    for r in M.rows_of(M.MODF):
        c = M.mod_case(r, "soft")
        y, T = M.modf_reference(r, c)
        wf = max([wf] + [M.worst(M.modf_emulate(r, c, v), y, M.U24 * T) for v in M.VARIANTS])
        ce = M.mod_case(r, "exact")
        assert all(torch.equal(M.modf_emulate(r, ce, v), M.modf_reference(r, ce)[0]) for v in M.VARIANTS)
    for r in M.rows_of(M.MODB):
        c = M.mod_case(r, "soft")
        ref = M.modb_reference(r, c)
        for v in M.VARIANTS:
            s, t = M.modb_emulate(r, c, v)
            ws, wt = max(ws, M.worst(s, ref["ds"], M.U24 * ref["Ts"])), max(wt, M.worst(t, ref["dt"], M.U24 * ref["Tt"]))
        ce = M.mod_case(r, "exact")
        re_ = M.modb_reference(r, ce)
        for v in M.VARIANTS:
            s, t = M.modb_emulate(r, ce, v)
            assert torch.equal(s, re_["ds"]) and torch.equal(t, re_["dt"])
        s, t = M.modb_emulate(r, c, "fused")
        bad = M.modb_reference(r, c, drop_row=r.dims[1] - 1)
        assert M.worst(t, bad["dt"], M.K_MT * M.U24 * bad["Tt"] + 1e-300) > 100, "one row lane's last row dropped"
    _constant("modf", wf)
    _constant("mods", ws)
    _constant("modt", wt)


def test_attention_map_constants():
    wa = wr = 0.0
    for r in M.rows_of(M.AMAP):
        B, H, N, S, d = r.dims
        c = M.amap_case(r)
        p, T = M.amap_reference(r, c)
        for v in M.VARIANTS:
            out, ph = M.amap_emulate(r, c, v)
            wa = max(wa, M.worst(out, M.amap_out(r, p), M.U24 * M.amap_out(r, T) + M.UNDERFLOW))
            wr = max(wr, float((ph.sum(-1) - 1).abs().max() / M.U24))
        out, _ = M.amap_emulate(r, c, "fused")
        lim = M.amap_bound(M.amap_out(r, T))
        if opt(r, "avg") and H > 1:
            assert M.worst(out, M.amap_out(r, p, heads=H - 1), lim) > 1000, "the average over H - 1 heads"
        if opt(r, "big"):
            bad, _ = M.amap_reference(r, c, no_max=True)
            assert not bool(torch.isfinite(bad).all()), "the softmax without its maximum overflows fp32 on these scores"
        for fam, want in (("equal", 1.0 / S), ("peak", None)):
            ce = M.amap_case(r, fam)
            pe, _ = M.amap_reference(r, ce)
            oe, _ = M.amap_emulate(M.Row(r.entry, r.dims, r.launches, tuple(kv for kv in r.opt if kv[0] != "avg")), ce, "fused")
            if fam == "equal":
                assert bool((oe == float(np.float32(1.0) / np.float32(S))).all())
            else:
                assert bool((oe[..., 0] == 1).all()) and bool((oe[..., 1:] == 0).all()) and (S == 1 or float(pe[..., 1:].max()) < 1e-80)
    _constant("amap", wa)
    _constant("arow", wr)


# ----------------------------------------------------------------------------------------------------------------
# error returns that come before any launch (no pointer below is ever dereferenced)
# ----------------------------------------------------------------------------------------------------------------
def _cases(base, nullable=()):
    """Every argument of `base` in turn null (pointers, value 1) or 0 and -1 (sizes)."""
    out = [dict(base)]
    for k, v in base.items():
        if k in nullable:
            out.append(dict(base, **{k: 0}))
        elif not isinstance(v, bool):
            out += [dict(base, **{k: 0}), dict(base, **{k: -1})]
    return out


def test_entry_points_refuse_bad_arguments_before_a_launch():
    from sdmi import _lib
    L = _lib.lib()
    host = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(host) + 15) // 16 * 16
    P = lambda on: p if on else None  # noqa: E731
    refused, accepted = collections.Counter(), collections.Counter()

    def check(entry, fn, a):
        want = M.status(entry, a)
        if want == 0:
            accepted[entry] += 1                # a valid call would launch: not made here, but counted below
            return
        refused[entry] += 1
        assert fn(a) == want == -1, (entry, a)

    ptrs = lambda *ks: {k: 1 for k in ks}  # noqa: E731
    for a in _cases(dict(ptrs("src", "dst"), ld=8, B=2, C=3, HW=5), ("src", "dst")) + [dict(ptrs("src", "dst"), ld=2, B=2, C=3, HW=5)]:
        check(M.N2C, lambda a: L.sdmi_nhwc_to_nchw(P(a["src"]), 1, a["ld"], a["B"], a["C"], a["HW"], P(a["dst"]), None), a)
        check(M.C2N, lambda a: L.sdmi_nchw_to_nhwc_bf16(P(a["src"]), a["B"], a["C"], a["HW"], P(a["dst"]), a["ld"], None), a)
    for a in _cases(dict(ptrs("src", "dst"), lds=16, ldd=24, P=3, C=8), ("src", "dst")) + \
            [dict(ptrs("src", "dst"), lds=16, ldd=24, P=3, C=c) for c in (4, 32)] + [dict(ptrs("src", "dst"), lds=12, ldd=24, P=3, C=8)]:
        check(M.SLICE, lambda a: L.sdmi_copy_slice(P(a["src"]), a["lds"], P(a["dst"]), a["ldd"], a["P"], a["C"], 0, None), a)
    for a in _cases(dict(ptrs("x", "y"), n=16), ("x", "y")):
        check(M.SILU, lambda a: L.sdmi_silu(P(a["x"]), None, P(a["y"]), a["n"], None), a)
        if a["n"] != 0:
            check(M.RELU, lambda a: L.sdmi_relu(P(a["x"]), None, P(a["y"]), a["n"], None), a)
    assert L.sdmi_relu(p, None, p, 0, None) == 0
    for a in _cases(dict(ptrs("pred", "target", "ws", "loss"), ld=8, B=2, C=3, HW=5), ("pred", "target", "ws", "loss")) + \
            [dict(ptrs("pred", "target", "ws", "loss"), ld=2, B=2, C=3, HW=5)]:
        check(M.MSE, lambda a: L.sdmi_mse(P(a["pred"]), a["ld"], P(a["target"]), a["B"], a["C"], a["HW"], 1.0, None, None,
                                          P(a["ws"]), P(a["loss"]), None), a)
    for a in _cases(dict(ptrs("t", "out"), tstride=1, B=2, dim=6, ld=8), ("t", "out")) + \
            [dict(ptrs("t", "out"), tstride=1, B=2, dim=d, ld=8) for d in (5, 7, 10)]:
        if a["tstride"] == 0:
            continue
        check(M.TEMB, lambda a: L.sdmi_time_embedding(P(a["t"]), a["tstride"], a["B"], a["dim"], P(a["out"]), a["ld"], None, None), a)
    base = dict(ptrs("x", "out", "mask", "wcond"), cmap=False, B=2, cx=4, H=5, W=3, cmi=3, MH=7, MW=5, cmo=4, cpad=8)
    extra = [dict(base, cpad=12), dict(base, cpad=24), dict(base, cmo=5), dict(base, cx=9, mask=0)]
    for cmap in (False, True):
        for a in _cases(base, ("x", "out", "wcond", "mask")) + extra + ([dict(base, cmi=256)] if cmap else []):
            a = dict(a, cmap=cmap)
            fn = L.sdmi_prep_input_cmap if cmap else L.sdmi_prep_input
            check(M.PREP, lambda a: fn(P(a["x"]), a["B"], a["cx"], a["H"], a["W"], P(a["mask"]), a["cmi"], a["MH"], a["MW"],
                                       P(a["wcond"]), a["cmo"], P(a["out"]), a["cpad"], None, None), a)
    base = dict(ptrs("dxin", "mask", "dw"), ld=16, cx=3, B=2, H=5, W=3, cmi=3, MH=7, MW=5, cmo=4)
    for fn in (L.sdmi_cond_wgrad, L.sdmi_cond_wgrad_cmap):
        for a in _cases(base, ("dxin", "mask", "dw")) + [dict(base, cmo=17, ld=32), dict(base, cmi=256), dict(base, ld=6)]:
            if a["cx"] == 0:
                continue
            check(M.CW, lambda a: fn(P(a["dxin"]), a["ld"], a["cx"], a["B"], a["H"], a["W"], P(a["mask"]), a["cmi"], a["MH"],
                                     a["MW"], a["cmo"], P(a["dw"]), None, None), a)
    for a in _cases(dict({"in": 1, "out": 1}, BC=2, IH=3, IW=4, OH=5, OW=6), ("in", "out")):
        check(M.RESIZE, lambda a: L.sdmi_resize_nearest(P(a["in"]), a["BC"], a["IH"], a["IW"], P(a["out"]), a["OH"], a["OW"], None), a)
    base = dict(ptrs("src", "dst"), src_c=4, src_c0=1, dst_c=5, dst_c0=2, B=2, C=3, P=7)
    for a in _cases(base, ("src", "dst")) + [dict(base, src_c0=2), dict(base, dst_c0=3)]:
        if a["src_c0"] == 0 or a["dst_c0"] == 0:
            continue
        check(M.CHAN, lambda a: L.sdmi_chan_copy(P(a["src"]), a["src_c"], a["src_c0"], P(a["dst"]), a["dst_c"], a["dst_c0"],
                                                 a["B"], a["C"], a["P"], None), a)
    for a in _cases(dict(ptrs("x", "s", "y"), ls=8, B=2, N=3, C=8), ("x", "s", "y")) + [dict(ptrs("x", "s", "y"), ls=7, B=2, N=3, C=8)]:
        check(M.MODF, lambda a: L.sdmi_modulate_fwd(P(a["x"]), None, P(a["s"]), None, a["ls"], 1.0, P(a["y"]), a["B"], a["N"], a["C"], None), a)
    for a in _cases(dict(ptrs("x", "dy", "s"), ls=8, B=2, N=3, C=8), ("x", "dy", "s")) + [dict(ptrs("x", "dy", "s"), ls=7, B=2, N=3, C=8)]:
        check(M.MODB, lambda a: L.sdmi_modulate_bwd(P(a["x"]), P(a["dy"]), P(a["s"]), a["ls"], 1.0, p, p, p, a["B"], a["N"], a["C"], None), a)
    base = dict(ptrs("q", "k", "out"), ldq=16, ldk=16, B=2, H=2, N=3, S=5, d=8)
    for a in _cases(base, ("q", "k", "out")) + [dict(base, S=4097), dict(base, ldq=15), dict(base, ldk=15), dict(base, N=65535 * 32 + 1)]:
        check(M.AMAP, lambda a: L.sdmi_attn_map(P(a["q"]), a["ldq"], P(a["k"]), a["ldk"], a["B"], a["H"], a["N"], a["S"], a["d"],
                                                1.0, 1, P(a["out"]), None), a)
    assert M.status(M.AMAP, dict(base, S=4096)) == 0 and M.status(M.AMAP, dict(base, S=4097)) == -1
    # how many cases each entry point must refuse, and the only ones status() may accept: the unmodified base call of
    # each form (and, for the staging, the base call without a mask) -- a status() that wrongly accepts shows up here
    assert dict(refused) == {M.N2C: 11, M.C2N: 11, M.SLICE: 13, M.SILU: 4, M.RELU: 3, M.MSE: 13, M.TEMB: 12, M.PREP: 51,
                             M.CW: 46, M.RESIZE: 12, M.CHAN: 16, M.MODF: 12, M.MODB: 12, M.AMAP: 21}
    assert dict(accepted) == {M.N2C: 1, M.C2N: 1, M.SLICE: 1, M.SILU: 1, M.RELU: 1, M.MSE: 1, M.TEMB: 1, M.PREP: 4, M.CW: 2,
                              M.RESIZE: 1, M.CHAN: 1, M.MODF: 1, M.MODB: 1, M.AMAP: 1}
