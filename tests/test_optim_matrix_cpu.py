"""The optimizer test matrix cannot fall behind the kernels, its exact data is exact and its bounds have teeth (CPU
only, no library call).

Each row of tests/optim_matrix.py ROWS launches what the restated host rules of csrc/optim.hip give; no row, state
case or flag case can be removed without a coverage check failing; the hand-written expectations of the state cases
agree with the numpy.float32 model; the exact families are exact (an fp32 evaluation with separate rounding and one
with fused multiply-adds give the bits of float64); the fp32 emulations stay within K / 2 of every bound and every K
is between 2 and 3 times the largest emulated ratio; each perturbed reference leaves its statement; and the difference
between Adam on the fp32 complements (the ABI) and on torch's double complements is the computed complement_gap, which
five steps of torch's CPU Adam confirm."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import optim_matrix as OM


def test_rows_follow_the_restated_rules():
    assert len({OM.row_id(r) for r in OM.ROWS}) == len(OM.ROWS)
    for r in OM.ROWS:
        assert list(r.launches) == OM.expected_launches(r.entry, r.dims, r.opt), OM.row_id(r)
        if r.entry in (OM.SUMSQ, OM.WIDEN, OM.CLIP):
            assert 4 * r.launches[0][1] <= OM.optim_workspace_for(r.dims[0])
            assert OM.clip_status(r.dims[0], 4 * r.launches[0][1]) == 0
            assert OM.clip_status(r.dims[0], 4 * r.launches[0][1] - 4) == -3


def test_the_restated_rules_at_known_points():
    assert OM.optim_workspace() == 8192 and OM.optim_workspace_for(1) == 8192
    assert OM.optim_workspace_for(2048 * 2 ** 17) == 8192 and OM.optim_workspace_for(2048 * 2 ** 17 + 1) == 8196
    assert [OM.norm_blocks(n) for n in (1, 2 ** 17, 2 ** 17 + 1, 3 * 2 ** 17)] == [1, 1, 2, 3]
    assert OM.clip_status(2 ** 17 + 1, 4) == -3 and OM.clip_status(2 ** 17 + 1, 8) == 0
    assert OM.clip_status(2048 * 2 ** 17 + 1, OM.optim_workspace()) == -3
    assert [OM.adam_grid(n, 4) for n in (1, 1024, 1027, 1028, 4 * 8192 * 256, 4 * 8192 * 256 + 1027)] == \
        [1, 1, 1, 2, 8192, 8192]
    assert [OM.adam_grid(n, 1) for n in (1, 256, 257, 8192 * 256 + 259)] == [1, 1, 2, 8192]
    assert [OM.cast_grid(n) for n in (3, 1024, 1028, 4 * 8192 * 256 + 1027)] == [1, 1, 2, 8192]
    assert OM.adam_vec(None) == 4 and OM.adam_vec("pb8") == 4 and OM.adam_vec("pb") == 1
    assert all(OM.adam_vec(k) == 1 for k in OM.FP32_OPERANDS)
    assert OM.adam_vec("ema", ema=0) == 4 and OM.adam_vec("pb", pb=0) == 4 and OM.adam_vec("ema", pb=0) == 1


# ----------------------------------------------------------------------------------------------------------------
# coverage: every named branch has a row, and every row is the only one covering some named branch
# ----------------------------------------------------------------------------------------------------------------
BLOCK_SIZES = (1, 3, 4, 5, 4099, 32764, 32768, 32772, 131071, 131072, 131073, 2 * 131072 + 5, 3 * 131072)
TAILS = (1, 3, 4, 5, 1023, 1025, 1026, 1027)


def _o(r):
    return dict(r.opt)


def _plain(r, **o):
    """The row's options are exactly `o`."""
    return _o(r) == o


def _row_needs():
    need = []
    for n in BLOCK_SIZES:
        need.append((f"sumsq at e = {n}", lambda r, n=n: r.entry == OM.SUMSQ and r.dims == (n,)))
        need.append((f"widen with partials at e = {n}", lambda r, n=n: r.entry == OM.WIDEN and r.dims == (n,) and
                     OM.opt(r, "partial") == 1))
    need.append(("widen without partials: a float4 and a tail in one block",
                 lambda r: r.entry == OM.WIDEN and not OM.opt(r, "partial") and 4 < r.dims[0] < OM.NORM_BLK and
                 r.dims[0] % 4))
    need.append(("widen without partials across blocks",
                 lambda r: r.entry == OM.WIDEN and not OM.opt(r, "partial") and r.dims[0] > OM.NORM_BLK))
    need.append(("clip on one block", lambda r: r.entry == OM.CLIP and r.dims[0] <= OM.NORM_BLK))
    need.append(("clip on a ragged last block", lambda r: r.entry == OM.CLIP and r.dims[0] > OM.NORM_BLK and
                 r.dims[0] % OM.NORM_BLK))
    need.append(("clip on full blocks", lambda r: r.entry == OM.CLIP and r.dims[0] > OM.NORM_BLK and
                 r.dims[0] % OM.NORM_BLK == 0))
    for k in (1, 255, 256, 257, 2048, 2049):
        need.append((f"finalize on {k} partials", lambda r, k=k: r.entry == OM.FIN and r.dims == (k,)))
    for n in TAILS:
        need.append((f"adam<4> at n = {n}", lambda r, n=n: r.entry == OM.ADAM and r.dims == (n,) and _plain(r)))
        need.append((f"cast at n = {n}", lambda r, n=n: r.entry == OM.CAST and r.dims == (n,)))
        if n != 1027:
            need.append((f"adam<1> at n = {n}", lambda r, n=n: r.entry == OM.ADAM and r.dims == (n,) and
                         _plain(r, off="g")))
    need.append(("adam<4> on more than two workgroups", lambda r: r.entry == OM.ADAM and r.launches[0] == (OM.adam_name(4), 3)))
    need.append(("cast on more than two workgroups", lambda r: r.entry == OM.CAST and r.launches[0][1] == 3))
    for off in OM.FP32_OPERANDS + ("pb", "pb8"):
        need.append((f"adam with {off} off its boundary", lambda r, off=off: r.entry == OM.ADAM and
                     r.dims == (1027,) and {k: v for k, v in r.opt if k not in ("lr", "decay")} == dict(off=off)))
    for off in (None, "g"):
        base = dict(off=off) if off else {}
        for absent in (dict(ema=0), dict(pb=0), dict(ema=0, pb=0)):
            need.append((f"adam off={off} with {absent}", lambda r, o=dict(base, **absent): r.entry == OM.ADAM and
                         _plain(r, **o)))
        need.append((f"adam off={off} skipped", lambda r, o=dict(base, skip=1): r.entry == OM.ADAM and _plain(r, **o)))
        need.append((f"adam off={off} on the capped grid", lambda r, off=off: r.entry == OM.ADAM and
                     OM.opt(r, "big") and OM.opt(r, "off") == off and r.launches[0][1] == OM.GRID_CAP and
                     r.dims[0] > OM.GRID_CAP * OM.NT * OM.adam_vec(off)))
    need.append(("a misaligned absent ema", lambda r: r.entry == OM.ADAM and _plain(r, off="ema", ema=0)))
    need.append(("a misaligned absent params_bf16", lambda r: r.entry == OM.ADAM and _plain(r, off="pb", pb=0)))
    for step in (2, 1000, 2 ** 20 + 1):
        need.append((f"adam<4> at step {step}", lambda r, s=step: r.entry == OM.ADAM and OM.opt(r, "step") == s and
                     not OM.opt(r, "off")))
    need.append(("adam<1> at a later step", lambda r: r.entry == OM.ADAM and OM.opt(r, "step", 1) > 1 and
                 OM.opt(r, "off") == "g"))
    need.append(("cast on the capped grid", lambda r: r.entry == OM.CAST and r.launches[0][1] == OM.GRID_CAP and
                 r.dims[0] > 4 * OM.GRID_CAP * OM.NT))
    need.append(("lr 1e-5 and decay 0.9999", lambda r: OM.opt(r, "lr") == 1e-5 and OM.opt(r, "decay") == 0.9999))
    return need


def _classify(x):
    return "nan" if math.isnan(x) else "+inf" if x == OM.INF else "-inf" if x == -OM.INF else "zero" if x == 0 else "finite"


def _state_needs():
    t = OM.case_trace
    has = lambda c, f: c["parts"] is not None and any(f(x) for x in c["parts"])  # noqa: E731
    clean = lambda c: not t(c)["loss_bad"] and not t(c)["norm_bad"]  # noqa: E731
    return [
        ("mode 0 ignores a non-finite loss and a raised flag", lambda c: c["mode"] == 0 and math.isnan(c["loss"]) and
         c["flag"] != 0 and clean(c)),
        ("mode 1 ignores the flag", lambda c: c["mode"] == 1 and c["flag"] != 0 and clean(c)),
        ("mode 1 NaN loss, finite norm", lambda c: c["mode"] == 1 and math.isnan(c["loss"]) and not t(c)["norm_bad"]),
        ("mode 1 inf loss", lambda c: c["mode"] == 1 and math.isinf(c["loss"])),
        ("mode 2 ignores the loss word", lambda c: c["mode"] == 2 and math.isnan(c["loss"]) and clean(c)),
        ("mode 2 raised flag", lambda c: c["mode"] == 2 and t(c)["loss_bad"]),
        ("inf partial, mode 0, scaler on", lambda c: has(c, math.isinf) and c["mode"] == 0 and c["gi"] > 0 and
         c["maxn"] != OM.INF),
        ("NaN partial alone", lambda c: has(c, math.isnan) and not t(c)["loss_bad"]),
        ("squares that overflow fp32", lambda c: c["grads"] is not None and t(c)["norm_bad"] and
         all(math.isfinite(x) for x in c["grads"])),
        ("non-finite norm and non-finite loss", lambda c: t(c)["norm_bad"] and t(c)["loss_bad"]),
        ("a partial sum beyond fp32 with a finite norm", lambda c: c["parts"] is not None and
         not t(c)["norm_bad"] and sum(c["parts"]) > OM.MAXF),
        ("growth_interval 0, clean", lambda c: c["gi"] == 0 and clean(c) and c["maxn"] != OM.INF),
        ("growth_interval <= 0, non-finite norm", lambda c: c["gi"] <= 0 and t(c)["norm_bad"]),
        ("growth_interval negative", lambda c: c["gi"] < 0),
        ("growth_interval 1", lambda c: c["gi"] == 1 and t(c)["grew"]),
        ("growth_interval 3 at tracker 1", lambda c: c["gi"] == 3 and c["tr"] == 1 and clean(c) and not t(c)["grew"]),
        ("growth_interval 3 at tracker 2", lambda c: c["gi"] == 3 and c["tr"] == 2 and t(c)["grew"]),
        ("coef below 1 at grad_div 1", lambda c: t(c)["below1"] and c["div"] == 1 and t(c)["norm"] < 1e10),
        ("coef clamped", lambda c: clean(c) and not t(c)["below1"] and c["maxn"] != OM.INF),
        ("norm 0", lambda c: t(c)["norm"] == 0),
        ("max_norm inf as the VQVAE trainer calls", lambda c: c["maxn"] == OM.INF and clean(c) and c["div"] == 2 and
         c["gi"] == 0),
        ("max_norm inf over norm inf", lambda c: c["maxn"] == OM.INF and t(c)["raw_nan"]),
        ("grad_div 2 with a scaler", lambda c: c["div"] == 2 and c["gi"] > 0),
        ("grad_div 3", lambda c: c["div"] == 3),
        ("the scale backs off", lambda c: t(c)["backed"]),
    ]


def _flag_needs():
    return [(f"loss flag mode {m} on {k}", lambda f, m=m, k=k: f[0] == m and _classify(f[1]) == k)
            for m, k in ((0, "zero"), (0, "finite"), (0, "+inf"), (0, "-inf"), (0, "nan"), (1, "zero"), (1, "finite"),
                         (1, "+inf"), (1, "nan"))]


TABLES = (("ROWS", _row_needs, OM.row_id), ("STATE_CASES", _state_needs, lambda c: c["name"]),
          ("FLAG_CASES", _flag_needs, str))


def _missing(items, needs):
    return [what for what, pred in needs if not any(pred(x) for x in items)]


@pytest.mark.parametrize("table", TABLES, ids=lambda t: t[0])
def test_coverage(table):
    name, needs, _ = table
    assert _missing(getattr(OM, name), needs()) == []


@pytest.mark.parametrize("table", TABLES, ids=lambda t: t[0])
def test_no_row_can_be_removed(table):
    name, needs, ident = table
    full, needs = list(getattr(OM, name)), needs()
    for x in full:
        assert _missing([y for y in full if y is not x], needs), f"{name} without {ident(x)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# the state machine: the hand-written expectations agree with the model
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OM.STATE_CASES, ids=lambda c: c["name"])
def test_state_cases_are_what_the_model_gives(case):
    tr = OM.case_trace(case)
    st = tr["after"]
    assert (int(st[5]), float(st[2]), float(st[3]), float(st[4])) == case["want"], (st, case["want"])
    assert (np.isnan(st[6]) and math.isnan(case["loss"])) or float(st[6]) == case["loss"]
    assert float(st[7]) == case["flag"]
    assert bool(st[5]) == (tr["loss_bad"] or tr["norm_bad"])


def test_state_model_at_known_points():
    norm, inv = OM.norm_model(25.0, 8.0, 1.0)
    assert float(norm) == 0.625 and float(inv) == 0.125
    st = OM.finalize_model(norm, [0, 0, 8, 0, 5, 0, 1.5, 0], 1.0, 3, 0, 1.0)
    assert float(st[1]) == 0.125 and float(st[0]) == 0.625
    st = OM.finalize_model(np.float32(5.0), [0, 0, 1, 0, 5, 0, 1.5, 0], 1.0, 3, 0, 1.0)
    assert float(st[1]) == float(np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6)))
    assert float(OM.norm_model(2.0 ** 129, 1.0, 1.0)[0]) == float(np.float32(2.0 ** 64.5))
    assert float(OM.case_partials(dict(grads=(2.0 ** 64,) * 5, parts=None))[0]) == OM.INF


# ----------------------------------------------------------------------------------------------------------------
# the exact families
# ----------------------------------------------------------------------------------------------------------------
_NORM_SIZES = sorted({r.dims[0] for r in OM.rows_of(OM.SUMSQ, OM.WIDEN, OM.CLIP)})


@pytest.mark.parametrize("n", _NORM_SIZES)
def test_exact_norm_family(n):
    g = OM.norm_case("exact", n)
    assert bool((g % 1 == 0).all()) and bool((g != 0).all()) and float(g.abs().max()) <= 3
    assert torch.equal(OM.bf16(g), g)
    ref = OM.block_sums(g)
    assert float(ref.max()) < 2 ** 24
    for variant in OM.VARIANTS:
        assert torch.equal(OM.emulate_blocks(g, variant), ref), variant
    drops = [("float4", 0), ("float4", n // 8), ("float4", n // 4 - 1)] if n >= 4 else []
    drops += [("tail", 0), ("tail", n % 4 - 1)] if n % 4 else []
    drops += [("wave", w) for w in range(16) if (min(n, OM.NORM_BLK) // 4 > 64 * w or (w == 0 and n < 4))]
    drops += [("block", b) for b in range(OM.norm_blocks(n))]
    for d in drops:
        assert not torch.equal(OM.emulate_blocks(g, "separate", drop=d), ref), f"{d} dropped goes unnoticed"
    s = OM.NORM_STATE["exact"]
    norm, inv = OM.norm_model(float(ref.sum()), s["scale"], s["div"])
    assert math.log2(float(inv)) % 1 == 0 and abs(float(norm) - math.sqrt(float(ref.sum())) * float(inv)) <= \
        OM.U24 * float(norm)


def _adam_rows():
    seen, out = set(), []
    for r in OM.rows_of(OM.ADAM):
        key = (r.dims[0], OM.opt(r, "step", 1), OM.opt(r, "lr", 1e-3), OM.opt(r, "decay", 0.99))
        if key not in seen and not OM.opt(r, "big"):
            seen.add(key)
            out.append(r)
    return out


@pytest.mark.parametrize("row", _adam_rows(), ids=OM.row_id)
def test_exact_adam_family(row):
    c = OM.row_case("exact", row)
    n = c["n"]
    for k in "pgmve":
        assert torch.equal(c[k].float().double().nan_to_num(7.0), c[k].nan_to_num(7.0)), f"{k} is not fp32"
    assert bool((c["g"] != 0).all())
    ref = OM.adam_reference(c)
    ema64, _, ema_bits = OM.ema_reference(c, ref["p"])
    closed = OM.adam_closed_form(c)
    want = dict(m=ref["m"], v=ref["v"], p=ref["p"], e=ema64)
    for k, w in want.items():
        assert OM.same_bits(w.float(), closed[k]), f"{k}: the closed form is not the float64 value"
        assert torch.equal(w.float().double().nan_to_num(7.0, 8.0, 9.0), w.nan_to_num(7.0, 8.0, 9.0)), f"{k} not exact"
    assert OM.same_bits(ema_bits.float(), closed["e"])
    for variant in OM.VARIANTS:
        emu = OM.emulate_adam(c, variant)
        for k, w in want.items():
            assert OM.same_bits(emu[k].float(), w.float()), f"{k}: the {variant} fp32 evaluation is not exact"
    # the update is p - lr sign(g), and the stored parameters hold every planted target once n allows
    fin = torch.isfinite(c["p"])
    assert torch.equal(ref["p"][fin], (c["p"] - c["lr"] * torch.sign(c["g"]))[fin])
    if n >= 7 * len(OM.TARGETS):
        for tgt in OM.TARGETS:
            assert bool((ref["p"] == tgt).any()), f"target {tgt} is not planted"
        assert bool(torch.isnan(ref["p"]).any()) and bool((ref["p"] == OM.INF).any()) and bool((ref["p"] == -OM.INF).any())
        assert bool((OM.bits(ref["p"].float()) == 0).any()), "no +0 among the stored parameters"
    if c["step"] > 1:   # a step word read as 0 would make both bias corrections 0
        assert OM.bias_terms(c) == (c["lr"], 1.0) and OM.bias_terms(dict(c, step=0))[0] == OM.INF


def test_targets_are_the_bf16_edge_cases():
    t = torch.tensor(OM.CAST_SPECIALS, dtype=torch.float64)
    b = OM.bf16(t)
    up, down = 1 + 2.0 ** -7, 1.0
    assert float(b[0]) == down and float(b[1]) == 1 + 2.0 ** -6 and float(b[2]) == -down      # ties: to the even below / above
    assert float(OM.bf16(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -23]))) == up                    # just past the tie
    assert float(OM.bf16(torch.tensor([1 + 2.0 ** -8 - 2.0 ** -24]))) == down                  # just short of it
    assert float(b[3]) == 2.0                                                                  # into the next binade
    assert float(OM.bf16(torch.tensor([OM.MAXF]))) == OM.INF
    x = OM.cast_case("exact", 1027)
    for s in OM.CAST_SPECIALS:
        assert bool(torch.isnan(x).any()) if math.isnan(s) else bool(((x == s) & (torch.signbit(x) == (math.copysign(1, s) < 0))).any()), s
    # 1 ulp of bf16 in a tie is seen by the bitwise statement
    ref = x.float().to(torch.bfloat16)
    bumped = (OM.bits(ref) + 1).view(torch.bfloat16)
    tie = (x == OM.TARGETS[0]).nonzero()[0]
    assert not OM.same_bits(bumped[tie], ref[tie])


# ----------------------------------------------------------------------------------------------------------------
# the soft families: emulated ratios, the constants, perturbed references
# ----------------------------------------------------------------------------------------------------------------
def _ratio(err, lim):
    return float((err / lim.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def _norm_ratio(n, wire):
    g = OM.norm_case("soft", n, wire)
    ref = OM.block_sums(g)
    return max(_ratio((OM.emulate_blocks(g, v) - ref).abs(), OM.U24 * ref) for v in OM.VARIANTS)


@functools.lru_cache(maxsize=None)
def _adam_ratio(row):
    c = OM.row_case("soft", row)
    ref = OM.adam_reference(c)
    out = {}
    for variant in OM.VARIANTS:
        emu = OM.emulate_adam(c, variant)
        for k in "mvp":
            out[k] = max(out.get(k, 0.0), _ratio((emu[k] - ref[k]).abs(), OM.U24 * ref["T_" + k]))
        e64, T_e, e_bits = OM.ema_reference(c, emu["p"])
        assert torch.equal(e_bits, emu["e"])
        out["ema"] = max(out.get("ema", 0.0), _ratio((emu["e"] - e64).abs(), OM.U24 * T_e))
    return out


@pytest.mark.parametrize("n", _NORM_SIZES)
def test_soft_norm_rows(n):
    r = max(_norm_ratio(n, False), _norm_ratio(n, True))
    print(f"n = {n}: emulated partial error / (u T) {r:.3f}")
    assert r <= OM.K_N / 2
    for wire in (False, True):
        g = OM.norm_case("soft", n, wire)
        ref = OM.block_sums(g)
        w = torch.ones(n, dtype=torch.float64)
        w[int(g.abs().argmax())] = 0.0
        assert bool(((OM.block_sums(g, w) - ref).abs() > OM.K_N * OM.U24 * ref).any()), "an element dropped stays inside"


@pytest.mark.parametrize("row", _adam_rows(), ids=OM.row_id)
def test_soft_adam_rows(row):
    m = _adam_ratio(row)
    print(f"{OM.row_id(row)}: emulated error / (u T): " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()))
    assert m["m"] <= OM.K_M / 2 and m["v"] <= OM.K_V / 2 and m["p"] <= OM.K_P / 2 and m["ema"] <= OM.K_E / 2, m


def test_the_constants_are_twice_the_emulated_ratios():
    worst = dict(partial=max(max(_norm_ratio(n, False), _norm_ratio(n, True)) for n in _NORM_SIZES))
    for row in _adam_rows():
        for k, v in _adam_ratio(row).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest emulated error / (u T): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, K in (("partial", OM.K_N), ("m", OM.K_M), ("v", OM.K_V), ("p", OM.K_P), ("ema", OM.K_E)):
        assert 2 * worst[k] <= K <= 3 * worst[k], (k, worst[k], K)


def _leaves(c, ref, pert, key, K):
    return bool(((pert[key] - ref[key]).abs() > K * OM.U24 * ref["T_" + key]).any())


@pytest.mark.parametrize("step", (1, 2, 1000))
def test_perturbed_adam_references_leave_their_statements(step):
    row = [r for r in _adam_rows() if OM.opt(r, "step", 1) == step and r.dims == (1027,)][0]
    c = OM.row_case("soft", row)
    ref = OM.adam_reference(c)
    assert _leaves(c, ref, OM.adam_reference(c, comp2=OM.complement_torch(0.999)), "v", OM.K_V), "torch's 1 - b2"
    assert _leaves(c, ref, OM.adam_reference(c, step_off=1), "p", OM.K_P), "step + 1"
    assert _leaves(c, ref, OM.adam_reference(c, no_sqrt=True), "p", OM.K_P), "bc2 without its square root"
    assert _leaves(c, ref, OM.adam_reference(c, eps_inside=True), "p", OM.K_P), "eps inside the square root"
    _, _, want = OM.ema_reference(c, ref["p"].float().double())
    _, _, pert = OM.ema_reference(c, ref["p"].float().double(), alpha=OM.complement32(c["decay"]))
    assert not torch.equal(want, pert), "the EMA with 1 - decay formed in fp32"


@pytest.mark.parametrize("k", (257, 2048, 2049))
def test_a_partial_beyond_index_255_dropped_is_seen(k):
    for kind in OM.FAMILIES:
        parts = OM.finalize_parts(kind, k)
        assert OM.bf16(parts).shape == parts.shape and float(parts.min()) >= 1
        full = OM.norm_model(OM.partials_sum(parts), 8.0, 1.0)[0]
        for upto in (256, k - 1):
            assert OM.norm_model(OM.partials_sum(parts, upto), 8.0, 1.0)[0] != full
        # the double sum of these partials is exact in any order
        assert float(parts.flip(0).sum()) == OM.partials_sum(parts) == float(parts.view(-1, 1).sum())


# ----------------------------------------------------------------------------------------------------------------
# the definitional difference from torch.optim.Adam fed Python doubles
# ----------------------------------------------------------------------------------------------------------------
def test_the_difference_from_torch_is_the_complement_gap():
    gap2, gap1 = OM.complement_gap(0.999), OM.complement_gap(0.9)
    print(f"complement gap: v {gap2:.4e}, m {gap1:.4e}")
    assert OM.complement32(OM._f(0.999)) != OM.complement_torch(0.999)
    c = dict(OM.adam_case("soft", 1027))
    c["v"], c["m"] = torch.zeros_like(c["v"]), torch.zeros_like(c["m"])
    ours = OM.adam_reference(c)
    theirs = OM.adam_reference(c, comp2=OM.complement_torch(0.999), comp1=OM.complement_torch(0.9))
    rel_v = ((theirs["v"] - ours["v"]).abs() / theirs["v"]).max()
    rel_m = ((theirs["m"] - ours["m"]).abs() / theirs["m"].abs()).max()
    # (the models multiply by float(1 - b); the gap is relative to 1 - b itself, 2^-24 apart at most)
    assert abs(float(rel_v) - gap2) <= 1e-7 * gap2 + OM.U24 * gap2 and abs(float(rel_m) - gap1) <= OM.U24
    assert 40 * OM.U24 < gap2 < 2.0 ** -16 and gap1 < 8 * OM.U24     # far above rounding on v, at its level on m


def test_five_steps_of_torch_adam_take_the_double_complements():
    n, steps = 1000, 5
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(steps)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-3)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    v_torch = opt.state[p]["exp_avg_sq"].double()
    b2 = OM._f(0.999)
    models = {}
    for name, c2 in (("abi", OM.complement32(b2)), ("torch", OM.complement_torch(0.999))):
        v = torch.zeros(n, dtype=torch.float64)
        for g in grads:
            v = v * b2 + c2 * g.double() * g.double()
        models[name] = float(((v_torch - v).abs() / v).max())
    gap = OM.complement_gap(0.999)
    print(f"torch's exp_avg_sq after {steps} steps: {models['torch']:.3e} from the double-complement model, "
          f"{models['abi']:.3e} from the ABI's; complement gap {gap:.3e}")
    assert models["torch"] <= 16 * OM.U24 and abs(models["abi"] - gap) <= 16 * OM.U24
