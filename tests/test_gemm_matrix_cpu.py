"""The tuned table cannot outrun the GEMM tests (CPU only).

Every entry of sdmi/tuned_gemm.json reduces to a class (a_mode, b_mode, variant, splits > 1, second source, column
permute, conv kernel, stride); each class -- and the grouped weight-gradient mainloop -- must have a row in
tests/gemm_matrix.py, which tests/test_gemm_variants_gpu.py runs exactly. A tuning run that introduces a new (mode,
variant) pair fails here until a GPU case exists. Also the matrix's own well-formedness, and a self-check of the exact
data's precondition and float64 references that calls no library code."""
import json
import os
import re

import pytest
import torch

from tests import gemm_matrix as GM

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stablediffusion-pytorch_amd", "sdmi",
                     "tuned_gemm.json")
KEY = re.compile(r"a(\d)b(\d) m(\d+) n(\d+) k(\d+) g(\d+)x(\d+)s(\d+) i(\d+)c(\d+) x(\d)p(\d)$")


def _classes():
    out = {}
    for key, e in json.load(open(TABLE)).items():
        m = KEY.match(key)
        assert m, f"unparsable key {key!r}"
        a, b, _, _, _, kh, kw, s, _, _, x, p = map(int, m.groups())
        splits, variant = (e[0], e[1]) if isinstance(e, list) else (e, 0)
        out.setdefault((a, b, variant, splits > 1, x, p, kh, kw, s), key)
    return out


def test_every_tuned_class_has_a_matrix_row():
    covered = GM.covered_classes()
    missing = {c: k for c, k in _classes().items() if c not in covered}
    assert not missing, f"tuned-table classes without a row in tests/gemm_matrix.py (class: first key): {missing}"


def test_grouped_weight_gradient_mainloop_has_a_row():
    from sdmi import kernels
    for split in (False, True):
        assert (GM.A_COL, GM.B_KN, kernels.GROUPED_VARIANT, split, 0, 0, 0, 0, 0) in GM.covered_classes()


def test_matrix_is_well_formed():
    assert len({(r.a, r.b, r.req, r.var, r.tile_n, tuple(sorted(r.extras.items()))) for r in GM.ROWS}) == len(GM.ROWS)
    for r in GM.ROWS:
        assert 0 <= r.req <= 11 and r.var in GM.GEOM and r.tile_n in (64, 128, 192, 256, 384), r
        assert (r.a, r.b) in ((0, 0), (0, 1), (1, 0), (2, 1), (2, 2)), r
        assert ("convs" in r.extras) == (r.a == GM.A_CONV or r.b == GM.B_KNCONV), r
        for c in r.extras.get("convs", ()):
            assert c in (GM.CONVS if r.a == GM.A_CONV else GM.WCONVS), r
        if "rule" in r.extras:
            assert r.extras["rule"] in GM.FALLBACK_RULES and r.var != r.req, r
        elif r.req >= 2:
            assert r.var == r.req, r  # a row that does not name a fallback rule runs what it requests
    # shape limits of the exact data: nothing beyond M = 255, K = 4160; N = 768 but for the one 3 x 384 conv-B case
    for v in GM.GEOM:
        assert all(k <= GM.K_MAX for k in GM.ks_for(v))
    assert max(n for r in GM.ROWS for n in r.extras.get("N", ())) <= 768
    GM.assert_exact_k(GM.K_MAX)
    # three requested slices really run, unevenly, at every row's long K; a 4-tile K runs two
    assert GM.launched_slices(3, GM.K_LONG) == 3 and GM.K_LONG % 192 and GM.launched_slices(3, 200) == 2
    assert GM.launched_slices(3, 264) == 3 and GM.launched_slices(3, 8) == 1 and GM.launched_slices(1, 264) == 1


@pytest.mark.parametrize("rule", GM.FALLBACK_RULES)
def test_every_fallback_rule_has_a_row(rule):
    hit = [r for r in GM.ROWS if r.extras.get("rule") == rule]
    assert hit, rule
    want = {"v4_needs_n_256_or_384": {2}, "64row_needs_kcontiguous": {2}, "v3_with_reductions": {2},
            "gsum_group_not_multiple_of_8": {0}, "gsum_more_than_40_groups": {0}, "conv_k_split_not_multiple_of_64": {0}}[rule]
    assert {r.var for r in hit} == want


def test_required_instantiations_are_rows():
    have = {(r.a, r.b, r.var, r.tile_n) for r in GM.ROWS}
    for a in (0, 1):
        assert {(a, 0, 4, 256), (a, 0, 4, 384), (a, 0, 7, 64), (a, 0, 8, 128), (a, 0, 9, 128), (a, 0, 10, 128)} <= have
    for a, b in ((0, 0), (0, 1), (1, 0)):
        assert {(a, b, 3, 128), (a, b, 5, 128), (a, b, 6, 128)} <= have


def test_exact_data_and_references_self_check():
    """The exactness argument on the CPU, with no library call: integer operands are exact in bf16, the int64 product
    is exact in fp32 in a scrambled summation order, the exactness precondition rejects a too-long K, and the float64
    conv references agree with an im2col matmul of the same integers."""
    A, B = GM.int_operands()
    assert torch.equal(A.to(torch.bfloat16).long(), A) and A.min() == -3 and A.max() == 3
    m, n, k = 37, 24, GM.K_MAX
    ref = GM.int_ref(m, n, k)
    assert int(ref.abs().max()) < 2 ** 24
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(0))
    acc = torch.zeros(m, n, dtype=torch.float32)
    for ch in perm.split(64):  # fp32 accumulation, k in a shuffled order, 64 at a time
        acc = acc + A[:m, ch].float() @ B[ch, :n].float()
    assert torch.equal(acc, ref.float())
    with pytest.raises(AssertionError):
        GM.assert_exact_k(2 ** 24 // 9 + 1)
    # conv A reference: F.conv2d == im2col matmul
    for name in ("3x3c8", "4x4s2", "x2c64"):
        c = GM.conv_case(name)
        q = c["q"]
        x = c["x"].view(q["B"], q["H"], q["W"], q["cin"]).permute(0, 3, 1, 2)
        cols = torch.nn.functional.unfold(x, q["k"], padding=q["p"], stride=q["s"])  # [B][cin * k * k][pixels]
        cols = cols.view(q["B"], q["cin"], q["k"] * q["k"], -1).permute(0, 3, 2, 1).reshape(c["ref"].shape[0], -1)
        if c["x2"] is not None:
            cols = torch.cat([cols, c["x2"]], 1)
        assert torch.equal(cols @ c["wpk"].t(), c["ref"]), name
    # conv B reference: conv2d_weight == dy^T @ im2col(x), and the permuted layouts are permutations of it
    w = GM.wconv_case("g4x8", 16)
    q = w["q"]
    x = w["x"].view(q["B"], q["H"], q["W"], q["cin"]).permute(0, 3, 1, 2)
    cols = torch.nn.functional.unfold(x, 3, padding=1).view(q["B"], q["cin"], 9, -1).permute(0, 3, 2, 1).reshape(w["K"], -1)
    assert torch.equal(w["dy"].t() @ cols, w["ref"].reshape(16, -1))
    for p in (1, 2):
        assert sorted(GM.permuted(w["ref"], p, q["cin"]).flatten().tolist()) == sorted(w["ref"].flatten().tolist())
    assert torch.equal(GM.permuted(w["ref"], 1, 8)[:, 9 * 3 + 4], w["ref"][:, 4, 3])
    assert torch.equal(GM.permuted(w["ref"], 2, 8)[:, 8 * 4 + 3], w["ref"][:, 4, 3])
    # the random-value bound is the fp32 dot-product bound and bf16 rounding stays inside the bf16 term
    ref, bound = GM.rand_ref(16, 16, 136)
    assert bool((bound > 0).all())
    assert bool(((ref.to(torch.bfloat16).double() - ref).abs() <= GM.rand_bound(ref, bound, torch.bfloat16)).all())
    # guard helper: untouched outside, and a single changed guard element is seen
    g = GM.Guarded(5, 6, 9, torch.bfloat16, "cpu", offset=1)
    g.view.fill_(1.0)
    assert g.outside_untouched()
    g.buf[g._window[0] + 6] = 0.0
    assert not g.outside_untouched()
