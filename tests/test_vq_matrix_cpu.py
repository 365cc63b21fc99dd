"""The VQ test matrix cannot fall behind the kernels, its exact data is exact and its bounds have teeth (CPU only, no
library call).

Each row of tests/vq_matrix.py ROWS launches what the restated host rules of csrc/vqvae.hip give; no row can be
removed without a coverage check failing; every exact case has a tied minimum on each kind of seam its slice rule has,
integer d^2, and a Python emulation of the slice / half / wave merge returns the first minimum; every soft row meets the
1 % condition from the reference alone; the fp32 emulations stay within K / 2 of every bound, K is at most 3 times
the largest emulated ratio, and each perturbed reference leaves its bound or its bitwise statement."""
import functools

import pytest
import torch

from tests import vq_matrix as VM


def _P(r):
    return r.dims[0] * (r.dims[1] if r.entry != VM.POINT else r.dims[2])


def test_rows_follow_the_restated_rules():
    assert len({VM.row_id(r) for r in VM.ROWS}) == len(VM.ROWS)
    for r in VM.ROWS:
        assert list(r.launches) == VM.expected_launches(r.entry, r.dims, r.opt), VM.row_id(r)
        if r.entry == VM.QUANT:
            B, HW, C, K = r.dims
            assert VM.quant_workspace(B * HW) == 4 * r.launches[0][1] and 1 <= C <= VM.MAXC
            assert VM.opt(r, "ldz") >= C
        elif r.entry == VM.BWD:
            B, HW, C, K = r.dims
            assert all(ld >= C for ld in VM.opt(r, "ld")) and 1 <= C <= VM.MAXC
            assert r.launches[0][1] * VM.BWD_PART * 4 <= VM.bwd_workspace()
        else:
            B, C, HW, cout, ld = r.dims
            assert ld >= cout


def test_the_restated_rules_at_known_points():
    assert VM.bwd_workspace() == 294912 and VM.quant_workspace(32) == 4 and VM.quant_workspace(33) == 8
    assert VM.slices(37)[0] == (0, 2, 3) and VM.slices(37)[12] == (36, 37, 37) and VM.slices(37)[13] == (39, 37, 37)
    assert VM.slices(16385)[0] == (0, 513, 1025) and VM.slices(16385)[15] == (15375, 15888, 16385)
    assert VM.slices(1) == [(0, 1, 1)] + [(w, 1, 1) for w in range(1, 16)]
    assert VM.slices(16)[3] == (3, 4, 4)
    assert VM.expected_launches(VM.QUANT, (8, 1024, 4, 8192)) == [("vq_quantize_kernelILb1EE", 256),
                                                                  ("vq_loss_kernel", 1)]
    assert VM.expected_launches(VM.QUANT, (1, 1, 4, 16385))[0] == ("vq_quantize_kernelILb0EE", 1)
    assert [VM.bwd_blocks(p) for p in (1, 256, 257, 131072, 131073)] == [1, 1, 2, 512, 512]
    assert VM.expected_launches(VM.BWD, (1, 1, 4, 65))[2] == ("vq_codebook_grad_kernel", 2)
    assert VM.expected_launches(VM.POINT, (1, 4, 2 ** 17, 4, 16))[0][1] == 8192
    assert VM.expected_launches(VM.POINT, (1, 4, 2 ** 17 - 1, 4, 16))[0][1] == 8192
    assert VM.expected_launches(VM.POINT, (1, 4, 2 ** 17 - 16, 4, 16))[0][1] == 8191


# ----------------------------------------------------------------------------------------------------------------
# coverage
# ----------------------------------------------------------------------------------------------------------------
def _need(found, what):
    assert found, f"ROWS has no row for: {what}"


def _per(K):
    return VM.cdiv(K, VM.VQ_WAVES)


def _ragged(K):
    live = [s for s in VM.slices(K) if s[0] < K]
    return 0 < live[-1][2] - live[-1][0] < _per(K)


def check_quant_coverage():
    rows = VM.rows_of(VM.QUANT)
    for en in (0, 1):
        _need([r for r in rows if r.launches[0][0] == VM.quant_name(en)], f"vq_quantize_kernel<{en}>")
    _need([r for r in rows if r.dims[3] == 1], "K = 1")
    _need([r for r in rows if 1 < r.dims[3] < 16], "1 < K < 16: whole waves without a slice")
    _need([r for r in rows if _per(r.dims[3]) % 2 and _per(r.dims[3]) > 1], "an odd per: unequal halves")
    _need([r for r in rows if _per(r.dims[3]) == 1 and _P(r) % 32 == 0], "per = 1 on exactly full workgroups")
    _need([r for r in rows if _ragged(r.dims[3])], "a ragged last slice")
    _need([r for r in rows if any(s[0] > r.dims[3] for s in VM.slices(r.dims[3]))], "waves with w0 > K")
    for C in (1, 3, 4, 5, 8):
        _need([r for r in rows if r.dims[2] == C], f"quantize C = {C}")
    for conv in ("none", "w", "wb"):
        _need([r for r in rows if VM.opt(r, "conv") == conv], f"quantize conv {conv}")
    for xq in (0, 1):
        _need([r for r in rows if VM.opt(r, "xq") == xq], f"quantize xq {xq}")
    _need([r for r in rows if VM.opt(r, "ldz") == r.dims[2]], "ldz == C")
    _need([r for r in rows if _P(r) % 32], "a tail workgroup")
    _need([r for r in rows if r.dims[0] > 1 and r.dims[1] % 32], "a workgroup that straddles images")
    _need([r for r in rows if r.launches[0][1] > 256], "more than 256 loss partials")
    _need([r for r in rows if r.dims[3] == 8192], "the bench codebook")
    _need([r for r in rows if r.dims[3] == VM.EN_MAX], "the largest LDS table")


def check_bwd_coverage():
    rows = VM.rows_of(VM.BWD)
    _need([r for r in rows if _P(r) < 64], "backward: fewer pixels than a wave")
    _need([r for r in rows if r.dims[0] > 1 and _P(r) <= 256], "backward: one workgroup holding two images")
    _need([r for r in rows if r.dims[2] == 3 and VM.opt(r, "ld")[2] >= 16], "backward: C = 3 and the wide pad")
    _need([r for r in rows if _P(r) % 256 == 1 and _P(r) > 256], "backward: a last workgroup with one pixel")
    _need([r for r in rows if VM.opt(r, "ld") == (r.dims[2],) * 3], "backward: every stride equal to C")
    _need([r for r in rows if r.dims[2] > 4], "the sxb branch")
    _need([r for r in rows if _P(r) > VM.CB_ROUND], "more than one round")
    _need([r for r in rows if _P(r) > VM.CB_ROUND and _P(r) % 4], "padding inside an int4")
    _need([r for r in rows if r.dims[3] > 64 and r.dims[3] % 64], "several codebook workgroups, the last ragged")
    _need([r for r in rows if VM.opt(r, "add")], "dzq_add")
    _need([r for r in rows if VM.opt(r, "lw")], "loss_w")
    _need([r for r in rows if not VM.opt(r, "lw")], "loss_w absent")
    for null in ("none", "post", "pre"):
        _need([r for r in rows if VM.opt(r, "null") == null], f"null pattern {null}")
    _need([r for r in rows if _P(r) > VM.BWD_CAP * VM.BWD_NT and r.launches[0][1] == VM.BWD_CAP], "the 512 cap")


def check_point_coverage():
    rows = VM.rows_of(VM.POINT)
    _need([r for r in rows if r.launches[0][1] == 1], "pointwise: one workgroup")
    _need([r for r in rows if not VM.opt(r, "bias")], "pointwise: no bias")
    _need([r for r in rows if r.dims[4] == r.dims[3]], "pointwise: ld == cout")
    _need([r for r in rows if r.dims[3] != r.dims[1]], "pointwise: cout != C")
    _need([r for r in rows if r.dims[0] > 1 and r.dims[4] >= 2 * r.dims[3] and VM.opt(r, "bias")],
          "pointwise: several images, a bias and a pad at least as wide as cout")
    _need([r for r in rows if _P(r) * r.dims[4] > 2 ** 21 and r.launches[0][1] == VM.POINT_CAP], "the 8192 cap")


COVERAGE = (check_quant_coverage, check_bwd_coverage, check_point_coverage)


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
    full = list(VM.ROWS)
    assert not _noticed()
    for r in full:
        monkeypatch.setattr(VM, "ROWS", [x for x in full if x is not r])
        assert _noticed(), f"ROWS without {VM.row_id(r)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------
def _qcase(kind, r):
    return VM.quant_case(kind, *r.dims, VM.opt(r, "conv"))


@pytest.mark.parametrize("row", VM.rows_of(VM.QUANT), ids=VM.row_id)
def test_exact_quantize_family(row):
    B, HW, C, K = row.dims
    c = _qcase("exact", row)
    x, e = VM.conv_chain(c["z"], c["w"], c["b"]), c["codebook"]
    assert torch.equal(x, c["x"]), "the fma chain does not return the planted x"
    for t in (c["z"], x, e) + ((c["w"],) if c["w"] is not None else ()) + ((c["b"],) if c["b"] is not None else ()):
        assert bool((t % 1 == 0).all())
    assert float(x.abs().max()) <= 4 and float(e.abs().max()) <= 4
    if c["w"] is not None:
        assert set(c["w"].reshape(-1).tolist()) <= {-1.0, 0.0, 1.0, 2.0}
    d2 = VM.dist2(x, e)
    assert bool((d2 % 1 == 0).all()) and float(VM.dist_scale(x, e).max()) < 2 ** 22
    vals = torch.unique(d2)
    assert bool((torch.sqrt(vals.float()).diff() > 0).all()), "two d^2 collapse under sqrtf"
    for order in VM.ORDERS:
        assert torch.equal(VM.emulate_d2(x, e, order), d2)
    first = d2.argmin(1)
    d = torch.sqrt(d2.float())
    assert torch.equal(VM.search(d, K), first), "the emulated merge does not return the first minimum"
    kinds = VM.tie_kinds(d2, K)
    for kind, seams in c["seams"].items():
        for s in seams:
            assert torch.equal(e[s], e[s - 1])
        if seams:
            assert kinds[kind] >= 1, f"no tied minimum on a seam of kind {kind}: {kinds}"
    print(f"{VM.row_id(row)}: pixels with a tied first minimum {kinds}, seams {c['seams']}")
    if kinds["halves"]:
        assert not torch.equal(VM.search(d, K, half_le=True), first)
    if kinds["waves"]:
        assert not torch.equal(VM.search(d, K, wave_le=True), first)
    if K > 1:
        assert sum(kinds.values()) >= 1
        assert not torch.equal(VM.next_tied(d2), first), "the next tied index passes for the first"
    # a third of the pixels at distance 0, and midpoints whenever the codebook has two different codes
    assert int((d2.min(1)[0] == 0).sum()) >= VM.cdiv(B * HW, 3)
    loss, S = VM.loss_reference(x, e, first)
    assert float(S) % 1 == 0 and float(S) < 2 ** 24
    assert torch.equal(VM.zq_reference(x, e, first), e[first])
    want = VM.exact_loss(S, B * HW * C)
    for order in VM.ORDERS:
        assert VM.emulate_loss(x, e, first, order) == want


def _bcase(kind, r, dist):
    return VM.bwd_case(kind, *r.dims, dist, VM.opt(r, "add"), VM.opt(r, "lw"))


def _bwd_terms(c, ref):
    """name -> ([P][Q] fp32 products, float64 ref [Q], T [Q])."""
    dzin, dx = c["dzin"].float(), ref["dx"].float()
    mk = lambda a, b: (a[:, :, None] * b[:, None, :]).reshape(a.shape[0], -1)  # noqa: E731
    return dict(dw_post=(mk(dzin, c["zq"].float()), ref["dw_post"].reshape(-1), ref["T_dw_post"].reshape(-1)),
                db_post=(dzin, ref["db_post"], ref["T_db_post"]),
                dw_pre=(mk(dx, c["z_enc"].float()), ref["dw_pre"].reshape(-1), ref["T_dw_pre"].reshape(-1)),
                db_pre=(dx, ref["db_pre"], ref["T_db_pre"]))


_BWD_SHAPES = sorted({(r.dims, VM.opt(r, "add"), VM.opt(r, "lw")) for r in VM.rows_of(VM.BWD)})


def _brow(shape):
    return [r for r in VM.rows_of(VM.BWD) if (r.dims, VM.opt(r, "add"), VM.opt(r, "lw")) == shape][0]


@pytest.mark.parametrize("shape", _BWD_SHAPES, ids=str)
def test_exact_backward_family(shape):
    row = _brow(shape)
    B, HW, C, K = row.dims
    n = B * HW * C
    for dist in VM.DISTS:
        c = _bcase("exact", row, dist)
        for name in ("dzin", "zq", "xq", "z_enc", "w_post", "w_pre", "codebook"):
            assert bool((c[name] % 1 == 0).all()) and float(c[name].abs().max()) <= 4
        assert VM.is_bf16(c["dzin"]) and float(torch.tensor(n).float()) == n
        ref = VM.bwd_reference(c)
        for g in (ref["g"], ref["gcb"]):
            assert torch.log2(torch.tensor(abs(g))) % 1 == 0, "a gradient scale is not a power of two"
        assert VM.exact_margin(c) < 2 ** 24
        for order in VM.ORDERS:
            for name, (terms, want, _) in _bwd_terms(c, ref).items():
                assert torch.equal(VM.emulate_bwd_sum(terms, order), want), (dist, name, order)
            used, got = VM.emulate_demb(c, ref["gcb"], order)
            assert torch.equal(got, ref["demb"][used]), (dist, "demb", order)
        unused = ref["count"] == 0
        assert bool((ref["demb"][unused] == 0).all())
        if dist == "collapsed":
            assert float(ref["count"].max()) == B * HW
        if dist == "sparse" and K > 3:
            assert int(unused.sum()) >= K - 3
        # 1 ulp of bf16 in dz_enc is seen by the bitwise statement
        bumped = (ref["dz"].to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double()
        assert not torch.equal(bumped, ref["dz"])


@pytest.mark.parametrize("row", VM.rows_of(VM.POINT), ids=VM.row_id)
def test_exact_pointwise_family(row):
    B, C, HW, cout, ld = row.dims
    c = VM.point_case("exact", B, C, HW, cout, VM.opt(row, "bias"))
    ref = VM.conv_chain(c["z"], c["w"], c["b"])
    want = c["z"] @ c["w"].T + (c["b"] if c["b"] is not None else 0.0)
    assert torch.equal(ref, want) and VM.is_bf16(ref)
    if c["b"] is not None:
        assert not torch.equal(VM.point_reference(c, drop_bias=True), VM.point_reference(c))


# ----------------------------------------------------------------------------------------------------------------
# the soft family: the 1 % condition, emulated ratios, perturbed references
# ----------------------------------------------------------------------------------------------------------------
def _ratio(err, lim):
    return float((err / lim.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def _quant(row):
    B, HW, C, K = row.dims
    c = _qcase("soft", row)
    x, e = VM.conv_chain(c["z"], c["w"], c["b"]), c["codebook"]
    d64, T = VM.dist2(x, e), VM.dist_scale(x, e)
    adm, best = VM.admissible(x, e)
    multi = int((adm.sum(1) > 1).sum())
    m = dict(d2=0.0, loss=0.0)
    loss, S = VM.loss_reference(x, e, best)
    for order in VM.ORDERS:
        d32 = VM.emulate_d2(x, e, order)
        m["d2"] = max(m["d2"], _ratio((d32 - d64).abs(), VM.U24 * T))
        got = VM.search(torch.sqrt(d32.clamp_min(0.0).float()), K)
        assert bool(adm[torch.arange(B * HW), got].all()), "the emulated search returns an inadmissible code"
        m["loss"] = max(m["loss"], abs(VM.emulate_loss(x, e, best, order) - float(loss)) / (VM.U24 * float(loss)))
    w = torch.ones(B * HW, dtype=torch.float64)
    w[int(((e[best] - x) ** 2).sum(1).argmax())] = 0.0
    caught = {"loss: a pixel dropped": abs(float(VM.loss_reference(x, e, best, w)[0] - loss)) >
              VM.K_S * VM.U24 * float(loss)}
    return m, caught, multi


@functools.lru_cache(maxsize=None)
def _bwd(shape):
    row = _brow(shape)
    P = _P(row)
    m, caught = {}, {}
    for dist in VM.DISTS:
        c = _bcase("soft", row, dist)
        ref = VM.bwd_reference(c)
        for order in VM.ORDERS:
            for name, (terms, want, T) in _bwd_terms(c, ref).items():
                m[name] = max(m.get(name, 0.0), _ratio((VM.emulate_bwd_sum(terms, order) - want).abs(), VM.U24 * T))
            used, got = VM.emulate_demb(c, ref["gcb"], order)
            excess = ((got - ref["demb"][used]).abs() - 2 * VM.U24 * ref["demb"][used].abs()).clamp_min(0.0)
            m["demb"] = max(m.get("demb", 0.0), _ratio(excess, VM.U24 * ref["T_demb"][used]))
        drop = torch.ones(P)
        drop[P - 1] = 0.0
        pert = VM.bwd_reference(c, weights=drop)
        for name in ("dw_post", "db_post", "dw_pre", "db_pre"):
            key = f"{name}: a pixel dropped"
            caught[key] = caught.get(key, False) or bool(((pert[name] - ref[name]).abs() >
                                                          VM.sum_bound(ref["T_" + name])).any())
        twice = torch.ones(P)
        twice[:min(P, VM.CB_ROUND)] = 2.0
        pert = VM.bwd_reference(c, demb_weights=twice)
        caught["demb: a round counted twice"] = caught.get("demb: a round counted twice", False) or bool(
            ((pert["demb"] - ref["demb"]).abs() > VM.demb_bound(ref["demb"], ref["T_demb"])).any())
    return m, caught


@pytest.mark.parametrize("row", VM.rows_of(VM.QUANT), ids=VM.row_id)
def test_soft_quantize_rows(row):
    m, caught, multi = _quant(row)
    print(f"{VM.row_id(row)}: emulated error / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()) +
          f"; pixels with more than one admissible code: {multi} of {_P(row)}")
    assert multi <= 0.01 * _P(row), "the 1 % condition fails: the index test would be vacuous"
    assert m["d2"] <= VM.K_D / 2 and m["loss"] <= VM.K_S / 2, m
    assert caught["loss: a pixel dropped"]


@pytest.mark.parametrize("shape", _BWD_SHAPES, ids=str)
def test_soft_backward_rows(shape):
    m, caught = _bwd(shape)
    print(f"{shape}: emulated error / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()) +
          "; leaves its bound: " + ", ".join(k for k, v in caught.items() if v))
    assert max(m.values()) <= VM.K_S / 2, m
    assert all(caught.values()), caught


def test_the_constants_are_twice_the_emulated_ratios():
    worst = {}
    for row in VM.rows_of(VM.QUANT):
        for k, v in _quant(row)[0].items():
            worst[k] = max(worst.get(k, 0.0), v)
    for shape in _BWD_SHAPES:
        for k, v in _bwd(shape)[0].items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest emulated error / (u T): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) +
          f"; K_D {VM.K_D}, K_S {VM.K_S}")
    top_s = max(v for k, v in worst.items() if k != "d2")
    assert 2 * worst["d2"] <= VM.K_D <= 3 * worst["d2"]
    assert 2 * top_s <= VM.K_S <= 3 * top_s


def test_search_and_sum_orders_at_known_points():
    """The emulations at points worked out by hand."""
    d = torch.tensor([[3.0, 1.0, 1.0, 2.0, 1.0] + [5.0] * 32])       # K = 37: per 3, wave 0 = {0, 1 | 2}, wave 1 = {3, 4 | 5}
    assert int(VM.search(d, 37)) == 1
    assert int(VM.search(d, 37, half_le=True)) == 2 and int(VM.search(d, 37, wave_le=True)) == 4
    assert VM.tie_kinds(d.double(), 37) == dict(within=0, halves=1, waves=1)
    assert int(VM.next_tied(d.double())) == 2
    big = 2.0 ** 24
    t = torch.zeros(600, 1)
    t[0, 0], t[1, 0], t[33, 0] = big, 1.0, 1.0            # lanes 0, 1 and 33 of wave 0: (1 + 33) meet before lane 0
    assert float(VM.emulate_bwd_sum(t, "kernel")) == big + 2
    t = torch.zeros(600, 1)
    t[0, 0], t[64, 0], t[300, 0] = big, 1.0, 1.0          # wave 0, wave 1 and the second workgroup, one by one
    assert float(VM.emulate_bwd_sum(t, "kernel")) == big
