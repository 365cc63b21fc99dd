"""The declared test matrix of sdmi_gemm (csrc/gemm.hip and the gemm_* sources it launches) and the helpers its exact
tests share.

ROWS is data: one row per kernel instantiation, `(a_mode, b_mode, requested variant, expected variant, expected
tile_n, extras)`. The expected variant and column tile are written by hand from the rules stated in the comments of
pick_variant / pick_tbn and the variant table (csrc/gemm_variants.h) -- they are the independent statement of what should run, never computed by calling the
library -- and tests/test_gemm_variants_gpu.py asserts after every launch that the library's own log agrees.
tests/test_gemm_matrix_cpu.py asserts that every (mode, variant, split, second source, permute, conv kernel) class of
sdmi/tuned_gemm.json has a row here.

Exact data: operands are integers in [-3, 3] (exact in bf16); with K * 9 < 2^24 every partial sum is an integer below
2^24, so the fp32 accumulator is exact in any summation order, split count or k-group order. An fp32 C then equals the
int64 matmul, a bf16 C equals its round-to-nearest-even (f2bf, csrc/common.h).

Guards: every operand and output is a view into a larger buffer filled with a NaN bit pattern (front pad, row stride
wider than the row, rows past the end). An unmasked read past a logical edge poisons the output; a store outside the
m_store x n_store window changes guard bits. Everything stays inside the allocations."""
import collections
import functools

import torch
import torch.nn.functional as F

A_ROW, A_CONV, A_COL = 0, 1, 2
B_NK, B_KN, B_KNCONV = 0, 1, 2

Row = collections.namedtuple("Row", "a b req var tile_n extras")

# variant -> (row tile TBM, staged depth KBK, ring STAGES), from the mainloop list of include/sdmi.h (variant_hint);
# 0 is the register-staged double buffer, 11 runs two k-groups of 2 stages each
GEOM = {0: (128, 64, 2), 2: (128, 64, 2), 3: (128, 64, 3), 4: (128, 32, 4), 5: (128, 32, 3), 6: (128, 64, 4),
        7: (64, 64, 6), 8: (64, 64, 6), 9: (64, 64, 3), 10: (64, 64, 2), 11: (128, 64, 2)}

K_LONG = 1032   # every row: sums far beyond what bf16 or a narrow accumulator holds
K_MAX = 4160    # once per mode (the rows marked kmax): the largest K the exactness argument admits with margin


def ks_for(var):
    """K in {shorter than one stage, exactly one trip round the ring, a wrap with a ragged tail, long}; variant 11
    also one k-tile (the second k-group idles) and an odd k-tile count."""
    _, kbk, st = GEOM[var]
    ks = [8, kbk * st, kbk * (st + 1) + 8, K_LONG]
    if var == 11:
        ks += [64, 320]
    return ks


def wrap_k(var):
    _, kbk, st = GEOM[var]
    return kbk * (st + 1) + 8


def logged_splits(hint, k):
    """What sdmi_gemm_plan reports (and the launch log records) for a splits_hint: clamped to at least one 64-deep
    k-tile per slice (include/sdmi.h)."""
    if hint <= 1 or k <= 64:
        return 1
    if k <= 128:
        return min(hint, 2)
    return hint  # hint <= 3 in these tests


def launched_slices(hint, k):
    """The slices a launch really runs: the launcher shares the 64-deep k-tiles out evenly, ceil(tiles / planned) per
    slice, and drops the slices left empty -- 4 k-tiles planned as 3 slices run as 2 + 2. Stated here from the
    launcher's comment so that the tests can insist on K whose three slices are real (and uneven)."""
    tiles = (k + 63) // 64
    per = -(-tiles // logged_splits(hint, k))
    return -(-tiles // per)


# implicit-conv A cases (a1b0): B, H, W, cin, kernel, stride, pad, second-source channels. 12 x 20 at B = 3 is M = 720
# (ragged against 64 and 128); 6 x 7 gives M = 126.
CONVS = {
    "3x3c8": dict(B=3, H=12, W=20, cin=8, k=3, s=1, p=1),     # taps straddle k-tiles
    "3x3c64": dict(B=3, H=6, W=7, cin=64, k=3, s=1, p=1),     # incremental-tap fast path
    "3x3c128": dict(B=2, H=6, W=7, cin=128, k=3, s=1, p=1),   # K = 1152
    "4x4s2": dict(B=3, H=12, W=20, cin=16, k=4, s=2, p=1),
    "1x1": dict(B=3, H=6, W=7, cin=72, k=1, s=1, p=0),
    "2x2s1": dict(B=3, H=6, W=7, cin=32, k=2, s=1, p=1),
    "2x2s2": dict(B=3, H=12, W=20, cin=16, k=2, s=2, p=0),
    "x2c64": dict(B=3, H=6, W=7, cin=64, k=3, s=1, p=1, cin2=64),  # K-concatenated second source, DMA-eligible
    "x2c8": dict(B=3, H=6, W=7, cin=8, k=3, s=1, p=1, cin2=16),    # k_split = 72: register staging
}
DMA_CONVS = ("3x3c8", "3x3c64", "3x3c128", "4x4s2", "1x1", "2x2s1", "2x2s2", "x2c64")
FEW_CONVS = ("3x3c8", "3x3c64", "x2c64")

# implicit-conv B cases (a2b2, weight gradients): output grid (= input grid for 3x3 s1 p1). 8 x 8, 4 x 4 and 4 x 8 are
# the three fast-gather classes (4 x 8 differs between 64- and 32-deep stages), 12 x 20 the general gather.
WCONVS = {
    "g8x8": dict(B=3, H=8, W=8, cin=16, k=3, s=1, p=1),
    "g4x4": dict(B=5, H=4, W=4, cin=16, k=3, s=1, p=1),
    "g4x8": dict(B=3, H=4, W=8, cin=16, k=3, s=1, p=1),
    "g12x20": dict(B=3, H=12, W=20, cin=16, k=3, s=1, p=1),
    "g12x20k": dict(B=5, H=12, W=20, cin=16, k=3, s=1, p=1),   # K = 1200
    "g6x7": dict(B=3, H=6, W=7, cin=16, k=3, s=1, p=1),        # 42 pixels per sample: not a multiple of 8
    "k4s2": dict(B=3, H=12, W=20, cin=16, k=4, s=2, p=1),      # N = 256
    "k4s2c24": dict(B=3, H=12, W=20, cin=24, k=4, s=2, p=1),   # N = 384
    "k2s2": dict(B=3, H=12, W=20, cin=16, k=2, s=2, p=0),      # N = 64
    "k3c128": dict(B=3, H=4, W=4, cin=128, k=3, s=1, p=1),     # N = 1152 = 3 x 384 (the one case wider than 768)
}
W_GRIDS = ("g8x8", "g4x4", "g4x8", "g12x20", "k4s2", "k2s2")


def R(a, b, req, var, tile_n, **extras):
    return Row(a, b, req, var, tile_n, extras)


def _linear_rows(a, b):
    """Row-major / col-major A with a plain B. tile 64 and 192 and the 64-row tiles exist only for [n][k] B with
    K-contiguous A."""
    nk = b == B_NK and a != A_COL
    rows = [
        R(a, b, 0, 2, 128, N=(232,)),            # no request: the DMA ring
        R(a, b, 1, 0, 128, N=(168,), kmax=True),
        R(a, b, 2, 2, 128, N=(232, 384) if nk else (168, 384), kmax=True),
        R(a, b, 3, 3, 128, N=(168,)),
        R(a, b, 4, 4, 256, N=(256,)),
        R(a, b, 4, 4, 384, N=(384, 768)),
        R(a, b, 4, 2, 128, N=(232,), rule="v4_needs_n_256_or_384"),
        R(a, b, 5, 5, 128, N=(168,)),
        R(a, b, 6, 6, 128, N=(168,)),
        R(a, b, 11, 11, 128, N=(168,)),
    ]
    if nk:
        rows += [
            R(a, b, 2, 2, 64, N=(40, 64, 168)),  # N <= 64, or a last 128-tile at most half used
            R(a, b, 5, 5, 192, N=(384,)),
            R(a, b, 7, 7, 64, N=(104, 40, 64)),
            R(a, b, 8, 8, 128, N=(168,)),
            R(a, b, 9, 9, 128, N=(168,)),
            R(a, b, 10, 10, 128, N=(168,)),
        ]
    else:
        rows += [R(a, b, v, 2, 128, N=(168,), rule="64row_needs_kcontiguous") for v in (7, 8, 9, 10)]
    return rows


ROWS = []
ROWS += _linear_rows(A_ROW, B_NK)
ROWS += _linear_rows(A_ROW, B_KN)
ROWS += _linear_rows(A_COL, B_KN)
# col-major A with reduction outputs: sum (VALU row sums), gsum (synthesised columns, group % 8 == 0), gsum_odd
for _v, _e in ((1, 0), (2, 2), (5, 5), (6, 6), (11, 11)):
    ROWS.append(R(A_COL, B_KN, _v, _e, 128, N=(168,), red="sum"))
    ROWS.append(R(A_COL, B_KN, _v, _e, 128, N=(168,), red="gsum"))
ROWS += [
    R(A_COL, B_KN, 4, 4, 256, N=(256,), red="sum"),
    R(A_COL, B_KN, 4, 4, 384, N=(384,), red="gsum"),
    R(A_COL, B_KN, 3, 2, 128, N=(168,), red="sum", rule="v3_with_reductions"),
    R(A_COL, B_KN, 3, 2, 128, N=(168,), red="gsum", rule="v3_with_reductions"),
    R(A_COL, B_KN, 8, 2, 128, N=(168,), red="sum", rule="64row_needs_kcontiguous"),
    R(A_COL, B_KN, 2, 0, 128, N=(168,), red="gsum_odd", rule="gsum_group_not_multiple_of_8"),
    R(A_COL, B_KN, 3, 0, 128, N=(168,), red="gsum_odd", rule="gsum_group_not_multiple_of_8"),
    R(A_COL, B_KN, 11, 0, 128, N=(168,), red="gsum_odd", rule="gsum_group_not_multiple_of_8"),
    # the DMA kernels form at most 48 reduction columns (8 + groups): 129 groups of 8 go to register staging
    R(A_COL, B_KN, 2, 0, 128, N=(168,), red="gsum_many", rule="gsum_more_than_40_groups"),
    R(A_COL, B_KN, 11, 0, 128, N=(168,), red="gsum_many", rule="gsum_more_than_40_groups"),
]
# implicit-conv A
ROWS += [
    R(A_CONV, B_NK, 0, 2, 128, N=(232,), convs=FEW_CONVS),
    R(A_CONV, B_NK, 1, 0, 128, N=(168,), convs=DMA_CONVS + ("x2c8",)),
    R(A_CONV, B_NK, 2, 2, 128, N=(232,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 2, 2, 64, N=(40, 64, 168), convs=FEW_CONVS),
    R(A_CONV, B_NK, 3, 3, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 4, 4, 256, N=(256,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 4, 4, 384, N=(384, 768), convs=FEW_CONVS),
    R(A_CONV, B_NK, 4, 2, 128, N=(232,), convs=FEW_CONVS, rule="v4_needs_n_256_or_384"),
    R(A_CONV, B_NK, 5, 5, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 5, 5, 192, N=(384,), convs=FEW_CONVS),
    R(A_CONV, B_NK, 6, 6, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 7, 7, 64, N=(104, 40, 64), convs=DMA_CONVS),
    R(A_CONV, B_NK, 8, 8, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 9, 9, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 10, 10, 128, N=(168,), convs=DMA_CONVS),
    R(A_CONV, B_NK, 11, 11, 128, N=(168,), convs=DMA_CONVS),
]
ROWS += [R(A_CONV, B_NK, v, 0, 128, N=(168,), convs=("x2c8",), rule="conv_k_split_not_multiple_of_64")
         for v in (2, 5, 7, 9, 11)]
# col-major A with implicit-conv B (conv weight gradients); 64- and 32-deep stages both run every grid
ROWS += [
    R(A_COL, B_KNCONV, 0, 2, 128, convs=("g8x8", "g12x20")),
    R(A_COL, B_KNCONV, 1, 0, 128, convs=W_GRIDS),
    R(A_COL, B_KNCONV, 2, 2, 128, convs=W_GRIDS + ("g12x20k",)),
    R(A_COL, B_KNCONV, 3, 3, 128, convs=W_GRIDS),
    R(A_COL, B_KNCONV, 4, 4, 256, convs=("k4s2",)),
    R(A_COL, B_KNCONV, 4, 4, 384, convs=("k4s2c24", "k3c128")),
    R(A_COL, B_KNCONV, 4, 2, 128, convs=("g8x8", "g4x8"), rule="v4_needs_n_256_or_384"),
    R(A_COL, B_KNCONV, 5, 5, 128, convs=W_GRIDS),
    R(A_COL, B_KNCONV, 6, 6, 128, convs=W_GRIDS),
    R(A_COL, B_KNCONV, 11, 11, 128, convs=W_GRIDS),
    R(A_COL, B_KNCONV, 9, 2, 128, convs=("g8x8", "g12x20"), rule="64row_needs_kcontiguous"),
]
for _v, _e in ((1, 0), (2, 2), (5, 5), (6, 6), (11, 11)):
    ROWS.append(R(A_COL, B_KNCONV, _v, _e, 128, convs=("g8x8", "g4x4", "g12x20"), red="sum"))
    ROWS.append(R(A_COL, B_KNCONV, _v, _e, 128, convs=("g8x8", "g4x4", "g12x20"), red="gsum"))
ROWS += [
    R(A_COL, B_KNCONV, 4, 4, 256, convs=("k4s2",), red="sum"),   # (its 6 x 10 grid is no multiple of 8: no gsum)
    R(A_COL, B_KNCONV, 3, 2, 128, convs=("g8x8",), red="gsum", rule="v3_with_reductions"),
    R(A_COL, B_KNCONV, 2, 0, 128, convs=("g6x7",), red="gsum_odd", rule="gsum_group_not_multiple_of_8"),
]

FALLBACK_RULES = ("v4_needs_n_256_or_384", "64row_needs_kcontiguous", "v3_with_reductions",
                  "gsum_group_not_multiple_of_8", "gsum_more_than_40_groups", "conv_k_split_not_multiple_of_64")
# 3 requested slices: K = 8 / 64 / 128 have fewer k-tiles than the hint; the launcher re-derives the slice count
# (launched_slices), so a 4-tile K (200, 256) runs 2 + 2 while the log still says 3; three real, uneven slices run at
# every row's K_LONG (17 tiles: 6 + 6 + 5) and at the wrap K of the deeper rings (264: 2 + 2 + 1; 328: 2 + 2 + 2)
SPLIT_HINTS = (1, 3)
PERMS = (0, 1, 2)      # a2b2 rows run every column permute


def row_id(r):
    x = r.extras
    tag = x.get("red") or ""
    tag += ("-" + x["rule"]) if "rule" in x else ""
    if "convs" in x and len(x["convs"]) <= 2:
        tag += "-" + "+".join(x["convs"])
    return f"a{r.a}b{r.b}-req{r.req}-v{r.var}-t{r.tile_n}{('-' + tag.strip('-')) if tag else ''}"


def rows(a, b, **want):
    return [r for r in ROWS if (r.a, r.b) == (a, b) and all((k in r.extras) == v for k, v in want.items())]


def covered_classes():
    """The (a_mode, b_mode, requested variant, split, second source, permute, kh, kw, stride) classes the GPU tests
    launch: every row runs unsplit and split, every a2b2 row every permute, every conv row its listed cases."""
    out = set()
    for r in ROWS:
        if "red" in r.extras:
            continue  # the table's keys do not tell reductions apart; plain rows carry the coverage claim
        for sp in (False, True):
            if r.a == A_CONV:
                for c in r.extras["convs"]:
                    q = CONVS[c]
                    out.add((r.a, r.b, r.req, sp, int("cin2" in q), 0, q["k"], q["k"], q["s"]))
            elif r.b == B_KNCONV:
                for c in r.extras["convs"]:
                    q = WCONVS[c]
                    for p in PERMS:
                        out.add((r.a, r.b, r.req, sp, 0, p, q["k"], q["k"], q["s"]))
            else:
                out.add((r.a, r.b, r.req, sp, 0, 0, 0, 0, 0))
    return out


# ----------------------------------------------------------------------------------------------------------------
# exact data and references (CPU, no library call)
# ----------------------------------------------------------------------------------------------------------------
def assert_exact_k(k):
    assert k * 9 < 2 ** 24, f"K = {k}: partial sums of [-3, 3] products may exceed 2^24, fp32 is no longer exact"


def ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def int_operands():
    """One A [255][4160] and B [4160][1152] for every linear case (sliced), so references are shared."""
    return ints((255, K_MAX), 1), ints((K_MAX, 1152), 2)


@functools.lru_cache(maxsize=None)
def int_ref(m, n, k):
    assert_exact_k(k)
    a, b = int_operands()
    return a[:m, :k] @ b[:k, :n]


@functools.lru_cache(maxsize=None)
def rand_operands():
    g = torch.Generator().manual_seed(3)
    return (torch.randn(255, 1152, generator=g).to(torch.bfloat16), torch.randn(1152, 1152, generator=g).to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def rand_ref(m, n, k):
    """float64 product of the bf16-rounded operands and the elementwise fp32 dot-product bound 2 K 2^-24 (|A| @ |B|)."""
    a, b = rand_operands()
    a, b = a[:m, :k].double(), b[:k, :n].double()
    return a @ b, 2.0 * k * 2.0 ** -24 * (a.abs() @ b.abs())


def rand_bound(ref, bound, c_dtype):
    """+ half a bf16 ulp (2^-8 relative) when C is bf16. Derived, not measured."""
    return bound + (2.0 ** -8 * ref.abs() if c_dtype == torch.bfloat16 else 0.0)


def out_hw(q):
    return (q["H"] + 2 * q["p"] - q["k"]) // q["s"] + 1, (q["W"] + 2 * q["p"] - q["k"]) // q["s"] + 1


@functools.lru_cache(maxsize=None)
def conv_case(name, rand=False):
    """Implicit-conv A case: x [B, cin, H, W], w [768, cin, k, k] (+ x2, w2) and the float64 F.conv2d reference
    [pixels, 768] (sliced per N); rand: randn rounded to bf16 and the elementwise bound instead of integers."""
    q = CONVS[name]
    cin2 = q.get("cin2", 0)
    kd = q["k"] * q["k"] * q["cin"] + cin2
    assert_exact_k(kd)
    if rand:
        g = torch.Generator().manual_seed(11)
        mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()  # noqa: E731
    else:
        g = torch.Generator().manual_seed(12)
        mk = lambda *s: torch.randint(-3, 4, s, generator=g).double()  # noqa: E731
    x, w = mk(q["B"], q["cin"], q["H"], q["W"]), mk(768, q["cin"], q["k"], q["k"])
    ref = F.conv2d(x, w, stride=q["s"], padding=q["p"])
    bound = F.conv2d(x.abs(), w.abs(), stride=q["s"], padding=q["p"])
    x2 = w2 = None
    if cin2:
        x2, w2 = mk(q["B"], cin2, q["H"], q["W"]), mk(768, cin2, 1, 1)
        ref = ref + F.conv2d(x2, w2)
        bound = bound + F.conv2d(x2.abs(), w2.abs())
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])  # noqa: E731
    wpk = w.permute(0, 2, 3, 1).reshape(768, -1)
    if cin2:
        wpk = torch.cat([wpk, w2.reshape(768, cin2)], 1)
    return dict(q=q, K=kd, x=flat(x), x2=flat(x2) if cin2 else None, wpk=wpk, ref=flat(ref),
                bound=2.0 * kd * 2.0 ** -24 * flat(bound))


@functools.lru_cache(maxsize=None)
def wconv_case(name, m, rand=False):
    """Implicit-conv B case: dy [pixels, m], x [pixels, cin]; reference dW [m][tap][cin] by
    torch.nn.grad.conv2d_weight in float64 on the same integers, and the exact sums of dy; rand: randn rounded to bf16
    and the elementwise bound."""
    q = WCONVS[name]
    oh, ow = out_hw(q)
    kd = q["B"] * oh * ow
    assert_exact_k(kd)
    if rand:
        g = torch.Generator().manual_seed(23)
        dy = torch.randn(kd, m, generator=g).to(torch.bfloat16).double()
        x = torch.randn(q["B"] * q["H"] * q["W"], q["cin"], generator=g).to(torch.bfloat16).double()
    else:
        dy = ints((kd, m), 21).double()
        x = ints((q["B"] * q["H"] * q["W"], q["cin"]), 22).double()

    def wgrad(x_, dy_):
        xn = x_.view(q["B"], q["H"], q["W"], q["cin"]).permute(0, 3, 1, 2)
        dyn = dy_.view(q["B"], oh, ow, m).permute(0, 3, 1, 2)
        dw = torch.nn.grad.conv2d_weight(xn, (m, q["cin"], q["k"], q["k"]), dyn, stride=q["s"], padding=q["p"])
        return dw.permute(0, 2, 3, 1).reshape(m, q["k"] * q["k"], q["cin"])

    return dict(q=q, K=kd, oh=oh, ow=ow, dy=dy, x=x, ref=wgrad(x, dy),
                bound=2.0 * kd * 2.0 ** -24 * wgrad(x.abs(), dy.abs()))


def permuted(ref3, perm, cvalid):
    """[m][tap][cin] -> the stored layout: perm 0 plain (tap, c), 1 torch (c, tap), 2 tap-major (tap, c), the last
    two only for c < cvalid."""
    m = ref3.shape[0]
    if perm == 0:
        return ref3.reshape(m, -1)
    r = ref3[:, :, :cvalid]
    return (r.permute(0, 2, 1) if perm == 1 else r).reshape(m, -1)


def to_c(ref, c_dtype):
    """What an exact kernel stores: the fp32 value (exact for these integers), rounded to nearest even for bf16."""
    return ref.to(torch.float32).to(c_dtype)


# ----------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ----------------------------------------------------------------------------------------------------------------
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


class Guarded:
    """A [rows][cols] view (row stride ld, `offset` elements past a 16-byte boundary) into a NaN-filled buffer with a
    front pad and `tail` whole rows after the view."""

    def __init__(self, rows, cols, ld, dtype, device, tail=8, offset=0, front=64):
        assert ld >= cols
        self.buf = torch.full((front + offset + (rows + tail) * ld,), float("nan"), dtype=dtype, device=device)
        self.view = self.buf[front + offset:].as_strided((rows, cols), (ld, 1))
        self.ld = ld
        self._window = (front + offset, rows, cols, ld)

    def outside_untouched(self):
        """Everything but the view still holds the fill pattern, bit for bit."""
        z = self.buf.clone()
        off, rows, cols, ld = self._window
        z[off:].as_strided((rows, cols), (ld, 1)).fill_(float("nan"))
        return torch.equal(z.view(_BITS[z.dtype]), torch.full_like(z, float("nan")).view(_BITS[z.dtype]))


def place(t, ld, device, dtype=torch.bfloat16, tail=136, offset=0):
    """A CPU [rows][cols] tensor as a guarded device view: NaN in the ld - cols columns past each row, in the front
    pad and in `tail` rows past the end (a whole tile of them, so a masked-off lane's address is still inside)."""
    g = Guarded(t.shape[0], t.shape[1], ld, dtype, device, tail=tail, offset=offset)
    g.view.copy_(t.to(dtype))
    return g


class NanEmpty:
    """Stands in for the torch module inside sdmi.kernels: torch.empty (the split-K workspace and the GroupNorm
    partials) comes back NaN-filled, so a slab element read before it was written poisons the output."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **kw):
        return torch.full(a[0] if len(a) == 1 and not isinstance(a[0], int) else a, float("nan"), **kw)


RAN = set()  # (a_mode, b_mode, variant, tile_n, split) instantiations launched in this process


def force(monkeypatch, kernels, splits, variant):
    """[splits, variant] for every shape (as tests/test_gemm_reduce_gpu.py), a fresh launch log, NaN workspaces."""
    monkeypatch.setattr(kernels, "TUNED", {"__all__": [splits, variant]})
    monkeypatch.setattr(kernels, "gemm_key", lambda d: "__all__")
    monkeypatch.setattr(kernels, "GEMM_LOG", [])
    monkeypatch.setattr(kernels, "torch", NanEmpty())


def check_log(kernels, var, tile_n, splits, tag, entry=-1):
    e = kernels.GEMM_LOG[entry]
    got = (e["variant"], e["tile_n"], e["splits"])
    assert got == (var, tile_n, splits), f"{tag}: launched (variant, tile_n, splits) = {got}, the matrix says " \
                                         f"{(var, tile_n, splits)}"
    RAN.add((e["a"], e["b"], var, tile_n, splits > 1))


def run_linear(kernels, L, a_mode, b_mode, m, n, k, A, B, c_dtype, device, *, ldc=None, c_offset=0, m_store=0,
               n_store=0, c_cols=None, **epi):
    """One guarded launch of a plain-operand mode. A [m][k], B [k][n]: CPU tensors. Returns the Guarded C."""
    if a_mode == A_ROW:
        ag, lda, am = place(A, k + 8, device), k + 8, L.A_ROWMAJOR
    else:
        ag, lda, am = place(A.t(), m + 8, device), m + 8, L.A_COLMAJOR
    if b_mode == B_NK:
        bg, ldb, bm = place(B.t(), k + 8, device), k + 8, L.B_NK
    else:
        bg, ldb, bm = place(B, n + 8, device), n + 8, L.B_KN
    cols = c_cols or n_store or n
    ldc = ldc or cols + 8
    c = Guarded(m_store or m, cols, ldc, c_dtype, device, offset=c_offset)
    kernels.gemm(m, n, k, ag.view, am, lda, bg.view, bm, ldb, c.view, ldc, m_store=m_store, n_store=n_store, **epi)
    c.keep = (ag, bg)  # a captured descriptor (kernels.GEMM_CAPTURE) stays launchable while the caller holds c
    return c
