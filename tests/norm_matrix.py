"""The declared test matrix of the GroupNorm and channel-sum kernels (csrc/norm.hip) and the helpers its exact tests
share.

ROWS is data: one row per launch shape, `(entry point, B, P, C, G, silu, expected launches, options)`. The expected
launches -- a fragment of the mangled kernel name with its template arguments, and the product of the grid -- are
written by hand. The host rules of norm.hip that decide which kernels run and on what grid (strip_width,
part_strip_width, pick_psplit, apply_grid, pass_shape / pick_pass with the 256 / 512 workgroup target, the segment
split of sdmi_chan_sum and the pixel-split rule of gn_bwd_part_impl) are restated below, also by hand;
tests/test_norm_matrix_cpu.py checks rows against rules and that the rows cover every kernel, every (NTH, IT) pair and
every branch listed there, tests/test_norm_exact_gpu.py that the library launches what the rows say. Every tensor of
every row has at most 2^21 elements (the workspace, which the library sizes, excepted).

Entry points of a row: FWD sdmi_gn_fwd; STATS sdmi_gn_stats followed by sdmi_gn_apply; BWD sdmi_gn_bwd; BWD_ROWS
sdmi_gn_bwd_rows followed by sdmi_gn_rows_sum; PART sdmi_gn_bwd_part; PART_ROWS sdmi_gn_bwd_part_rows followed by
sdmi_gn_rows_sum; CHAN sdmi_chan_sum; GROUPED one sdmi_gn_bwd_rows per job, then one sdmi_gn_rows_sum_grouped.

Not reachable below the size cap, hence without a row: gn_bwd_reduce_kernel with one pixel split (pick_pass rejects a
shape only from P = 257 on, where pick_psplit splits unless strips * B >= 512, i.e. 33 M elements) and
gn_bwd_apply_kernel without pixel splits (same reason; the shared apply_grid rule runs unsplit under gn_apply_kernel).

Data, two families (all inputs exact in bf16; the references are float64 on the CPU, from the bf16 inputs):

  exact  silu = 0. x integers in [-8, 8], dy and the addend integers in [-4, 4], gamma a signed power of two, beta a
         multiple of 1/8. Every per-channel sum of x, x^2 and dy and every batch sum is an integer below 2^24: exact in
         fp32 in any summation order, so the forward table is one bit pattern whatever kernel and pixel split produced
         it, and dbeta is the exact integer. Per batch row one group is constant (x = 3: variance exactly 0, rstd =
         1 / sqrt(eps)) and one is nearly constant (x in {1, 1 + 2^-7}: variance <= 1.6e-5, so eps = 1e-5 decides its
         rstd). Sums of (1 + 2^-7)^2 = 1 + 2^-6 + 2^-14 stay exact only while the count is below 1008, so rows with
         P > 1000 use {0, 2^-7} for that group (same variance, sums exact at any count).
  soft   x = bf16(2 randn + 0.5), dy = bf16(randn), as tests/test_kernels_gpu.py. Per batch row one group has a large
         mean (100 + randn: the cancelling terms s = beta - mean a and q x + o) and one is quiet (2^-6 randn: variance
         2.4e-4, which makes eps visible in the table at the table's bound).

Rounding points of the kernels and the bounds derived from them (u = 2^-24, the fp32 unit roundoff; K = K_SUM):

  table  s1 = sum x and s2 = sum x^2 per channel in fp32 (x^2 is exact: 16 significant bits), merged per group, divided
         and subtracted in fp64, mean and rstd rounded to fp32 once. Exact family: mean and rstd within 1 fp32 ulp of
         float64, a == rstd gamma bitwise. Soft family: |mean - ref| <= 2^-23 |ref| + K u E|x|; the variance moves by
         dvar <= K u (E x^2 + 2 |mean| E|x|) and rstd by rstd (2^-23 + dvar / (2 (var + eps))) (E over the group).
         Both: |a - rstd gamma| <= 2^-23 |a| and |s - (beta - mean a)| <= 2^-23 (|beta| + |mean a|), on the kernel's own
         mean, rstd and a (each one or two fp32 roundings).
  y      bf16(act(fma(x, a, s))): |y - ref| <= 2^-8 |ref| + 2^-20 (|x a| + |s|), ref = act(x a + s) in float64 on the
         kernel's own table. 2^-8 is the bf16 unit roundoff (twice the half-ulp of round-to-nearest); the second term
         is 8 fp32 roundoffs of the two cancelling terms (2^-20 = 16 u), which also covers the raw exp2 / rcp of silu_f.
  sums   S1 = sum_p dz, S2 = sum_p dz xhat per (b, c), dz = dy [silu'(z)], z = fma(x, a, s), xhat = (x - mean) rstd,
         all in fp32. z is one fma on the table the reference uses, so it carries one roundoff, u |z|. An element of dz
         is uncertain by u W, W = |dz| + silu |dy| / 4. The first part is the roundoff of the products. The second is
         absolute, for the places where silu' passes through 0 (z = -1.28) and |dz| says nothing: there the roundoff of
         z moves silu' by |silu''| u |z| <= u / 2, and the raw exp2 / rcp move the sigmoid s by a few u s (1 - s),
         which silu' = s (1 + z (1 - s)) passes on with |1 + z - 2 z s| <= 1 + |z|: together below 2 u |dy|, which is
         K u |dy| / 4 at K = 8. Without it two-pixel rows (P = 2) whose dz both fall near that zero have no scale. A sum
         of n such terms in any order is uncertain by a multiple of u sum W: |S1 - ref| <= K u sum_p W, |S2 - ref| <=
         K u sum_p W |xhat|, |dbeta - ref| <= K u sum_b sum_p W, |dgamma - ref| <= K u sum_b sum_p W |xhat|.
  dx     bf16(add + fma(a, dz, fma(q, x, o))), q = -rstd^2 Bc / n, o = rstd^2 mean Bc / n - rstd A / n, A = sum_c gamma
         S1, Bc = sum_c gamma S2 over the group. With |A|' = sum_c |gamma| sum_p W and |Bc|' likewise (W |xhat|):
         |dx - ref| <= 2^-8 |ref| + K u (|add| + |a| W + rstd^2 |Bc|' (|x| + |mean|) / n + rstd |A|' / n).
  chan   per_c = sum dy in fp32: K u sum |dy|; per_bc adds the bf16 rounding 2^-8 |ref|.

K_SUM: tests/test_norm_matrix_cpu.py runs an fp32 emulation of this arithmetic in two summation orders (sequential in
runs of 256, and pairwise, over pixels, channels and batch rows) on every soft row and measures max |fp32 value -
float64 ref| / (u T), T the sum of absolute values above. The emulation forms z and dx with the kernel's fmas (product
and sum in float64, rounded once); the accumulating fmas of the reductions are modelled as a rounded product that is
then added, one rounding more per term than the kernel, so the model is the coarser of the two. The larger of the two
orders reached 2.32 (dx), 2.12 (dgamma), 1.36 (dbeta), 3.99 (S1 / S2, on a row without SiLU: a term dz xhat carries
three roundoffs, of x - mean, of the product with rstd and of the product with dz, before the sum adds its own) and
1.24 (table, against 2^-23 |ref| + u E|x| and its counterpart for rstd); the largest over all rows and quantities is
3.99. The GPU's reduction tree is a third order and the raw rcp adds an ulp, so the constant is twice that: 8. The CPU
test asserts that the emulation stays within K_SUM / 2 of every bound, that K_SUM is no more than 3 times the largest
emulated ratio, and that the perturbed references (a pixel row doubled or omitted, eps = 1e-6, n - 1 in the variance,
a batch row missing from dgamma / dbeta, q x dropped, the sigmoid for silu') leave the bounds.

Guards: every operand and output is a column window of a buffer filled with a NaN bit pattern (front pad, pad columns,
rows past the end); the fp32 outputs and the workspace sit between NaN pads too. An unmasked read poisons the output; a
store outside the logical windows, into an input, or past the first sdmi_chan_reduce_workspace bytes changes guard
bits."""
import collections
import ctypes
import functools

import numpy as np
import torch

from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401  (shared with the attention tests)

FWD, STATS, BWD, BWD_ROWS, PART, PART_ROWS, CHAN, GROUPED = ("fwd", "stats", "bwd", "bwd_rows", "part", "part_rows",
                                                             "chan", "grouped")
Row = collections.namedtuple("Row", "entry B P C G silu launches opt")
EPS = float(np.float32(1e-5))
U24 = 2.0 ** -24
K_SUM = 8.0
SILU_ABS = 0.25   # the absolute part of the uncertainty of dy silu'(z), in units of |dy| (docstring: sums)
CAP = 2 ** 21


def R(entry, B, P, C, G, silu, *launches, **opt):
    return Row(entry, B, P, C, G, silu, launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/norm.hip, restated
# ----------------------------------------------------------------------------------------------------------------
NT = 256            # threads of every kernel but the single-pass ones
SLOT_CTRS = 2048
BATCH_CTR = 1024
PS_MAX = 32
NSLOTS = 2048
APPLY_CW = 64
PASS_SHAPES = ((64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4), (512, 2), (512, 4), (1024, 2), (1024, 4),
               (1024, 8))


def cdiv(a, b):
    return -(-a // b)


def strip_width(C, unit):
    """Whole groups, a multiple of 8 channels, at least 64 channels when C allows, at most SLOT_CTRS strips."""
    cw = unit
    while cw % 8 or (cw < 64 and cw * 2 <= C):
        cw += unit
    while cdiv(C, cw) > SLOT_CTRS:
        cw += unit
    return cw


def part_strip_width(C, unit):
    """Whole groups and a multiple of 64 channels, else the whole row; strip_width where that exceeds 256."""
    cw = unit
    while cw % 64 and cw < C:
        cw += unit
    if cw > C or cw > NT:
        cw = strip_width(C, unit)
    return cw


def pick_psplit(nch, nb, rows_per_b):
    """Pixel splits per (strip, batch row): up to 512 workgroups of at least 128 pixels, at most 32."""
    if nch * nb > BATCH_CTR:
        return 1
    ps = 1
    while nch * nb * ps < 512 and rows_per_b // (ps * 2) >= 128 and ps < PS_MAX:
        ps *= 2
    return ps


def apply_grid(B, P, C):
    """C / 64 strips x B x pixel splits: up to 2048 workgroups of at least 64 pixels."""
    strips = cdiv(C, APPLY_CW)
    ps = 1
    while strips * B * ps < 2048 and P // (ps * 2) >= 64:
        ps *= 2
    return strips, B, ps


def pass_shape(P, L):
    """The first pair with at most 4 pixel rows per thread that holds P rows at L lanes per row, else at most 8."""
    for lim in (4, 8):
        for nth, it in PASS_SHAPES:
            if it <= lim and P <= it * (nth // L):
                return nth, it
    return None


def pick_pass(B, P, C, G):
    """(strip width, (NTH, IT)) of the single-pass launch, or None: the widest strip of whole groups (8-channel lanes,
    at most 256 channels) that still gives `target` workgroups, else the strip with the most workgroups (the
    narrowest)."""
    Cg = C // G
    target = 256 if P >= 1024 else 512
    u = Cg
    while u % 8:
        u += Cg
    good = most = None
    most_wg = 0
    cw = u
    while cw <= NT and cw - u < C:
        sh = pass_shape(P, cw // 8)
        if sh is not None:
            wg = cdiv(C, cw) * B
            if wg >= target:
                good = (cw, sh)
            if wg > most_wg:
                most, most_wg = (cw, sh), wg
        cw += u
    best = good if good is not None else most
    if best is None or cdiv(C, best[0]) > BATCH_CTR:
        return None
    return best


def chan_segments(B, P, per_bc):
    """(virtual batch rows, pixel rows of each) of sdmi_chan_sum: the batch rows, or without per_bc up to 32
    contiguous segments of at least 64 of the B * P rows."""
    if per_bc:
        return B, P
    total = B * P
    nb = min(max(total // 64, 1), 32)
    seg = cdiv(total, nb)
    return cdiv(total, seg), seg


def part_psplit(nch, B, P):
    """gn_bwd_part_impl: up to 1024 workgroups while every pixel split keeps 64 pixels."""
    ps = 1
    while nch * B * ps < 1024 and P // (ps * 2) >= 64:
        ps *= 2
    return ps


def pass_name(bwd, nth, it):
    return f"gn_{'bwd' if bwd else 'fwd'}_pass_kernelILi{nth}ELi{it}EE"


def _multi(B, P, C, G, first, second):
    cw = strip_width(C, C // G)
    nch = cdiv(C, cw)
    g = apply_grid(B, P, C)
    return [(first, nch * B * pick_psplit(nch, B, P)), (second, g[0] * g[1] * g[2])]


def _rows_sum(jobs):
    return ("gn_rows_sum_grouped_kernel", cdiv(max(C for _, C in jobs), NT) * len(jobs))


def expected_launches(entry, B, P, C, G, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    o = dict(options)
    if entry == STATS:
        return _multi(B, P, C, G, "gn_stats_kernel", "gn_apply_kernel")
    if entry in (FWD, BWD, BWD_ROWS):
        pc = pick_pass(B, P, C, G)
        if pc is not None:
            out = [(pass_name(entry != FWD, *pc[1]), cdiv(C, pc[0]) * B)]
        elif entry == FWD:
            out = _multi(B, P, C, G, "gn_stats_kernel", "gn_apply_kernel")
        else:
            out = _multi(B, P, C, G, "gn_bwd_reduce_kernel", "gn_bwd_apply_kernel")
        return out + ([_rows_sum([(B, C)])] if entry == BWD_ROWS else [])
    if entry in (PART, PART_ROWS):
        nch = cdiv(C, part_strip_width(C, C // G))
        out = [("gn_bwd_part_kernel", nch * B * part_psplit(nch, B, P))]
        return out + ([_rows_sum([(B, C)])] if entry == PART_ROWS else [])
    if entry == CHAN:
        nb, seg = chan_segments(B, P, o["mode"] == "bc")
        nch = cdiv(C, strip_width(C, 8))
        return [("chan_sum_kernel", nch * nb * pick_psplit(nch, nb, seg))]
    assert entry == GROUPED
    out = []
    for jb, jp, jc, jg in o["jobs"]:
        out += expected_launches(BWD, jb, jp, jc, jg)
    return out + [_rows_sum([(jb, jc) for jb, _, jc, _ in o["jobs"]])]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
# Single-pass shapes (B, P, C, G, silu, NTH, IT, workgroups), run by sdmi_gn_fwd and by sdmi_gn_bwd. Per (NTH, IT) the
# smallest shape with B = 3, two strips of two groups, whose slab is full (P == IT * R, R = NTH / L rows per pass of
# L = strip / 8 lanes) and the smallest whose slab is ragged (P < IT * R); in all of them L does not divide NTH (idle
# tail threads). Strips of 184 .. 232 channels on 64 threads run the one-thread-per-channel batch tail and one
# small_reduce segment per channel; the 24-channel strips run several segments and nbg = 10 batch-tail groups; the
# 184 .. 232-channel strips on 256 threads and more run nbg = 1.
PASS = [
    (3, 1, 48, 4, 0, 64, 1, 6),   # one pixel row; the full 64 x 1 slabs are the 256- and 240-channel strips below
    (3, 4, 368, 4, 1, 64, 2, 6), (3, 13, 80, 4, 0, 64, 2, 6),
    (3, 8, 368, 4, 1, 64, 4, 6), (3, 5, 368, 4, 0, 64, 4, 6),
    # (the ragged 256 x 1 slab on B = 20: its batch tail runs nbg = 1 over more than 16 batch rows)
    (3, 9, 432, 4, 1, 256, 1, 6), (20, 9, 368, 4, 0, 256, 1, 40),
    (3, 16, 464, 4, 1, 256, 2, 6), (3, 86, 48, 4, 0, 256, 2, 6),
    (3, 32, 464, 4, 1, 256, 4, 6), (3, 17, 464, 4, 0, 256, 4, 6),
    (3, 34, 464, 4, 1, 512, 2, 6), (3, 33, 464, 4, 0, 512, 2, 6),
    (3, 72, 432, 4, 1, 512, 4, 6), (3, 37, 432, 4, 0, 512, 4, 6),
    (3, 74, 432, 4, 1, 1024, 2, 6), (3, 73, 432, 4, 0, 1024, 2, 6),
    (3, 148, 432, 4, 1, 1024, 4, 6), (3, 81, 400, 4, 0, 1024, 4, 6),
    (3, 296, 432, 4, 1, 1024, 8, 6), (3, 149, 432, 4, 0, 1024, 8, 6),
    # the wg >= target branch of pick_pass: 512 workgroups of 64 threads on 256-channel strips (L divides NTH, no idle
    # threads; B > 16: the batch tail of a narrow workgroup runs ordered_sum<16> over more than one batch)
    (256, 2, 512, 32, 1, 64, 1, 512),
    # the same branch with a ragged last strip: 240 + 144 channels of 384
    (260, 2, 384, 32, 0, 64, 1, 520),
    # one channel per group
    (3, 5, 32, 32, 1, 64, 1, 12),
]
ROWS = [R(FWD, B, P, C, G, s, (pass_name(False, nth, it), wg)) for B, P, C, G, s, nth, it, wg in PASS]
ROWS += [R(BWD, B, P, C, G, s, (pass_name(True, nth, it), wg)) for B, P, C, G, s, nth, it, wg in PASS]
# forward only: single-pass shapes on which sdmi_gn_stats takes 8 and 32 pixel splits (8-channel strips of one group;
# P = 8192 is the most a single pass holds), so the exact family compares the single-pass table with those bitwise
ROWS += [R(FWD, 3, 1030, 16, 2, 0, (pass_name(False, 512, 4), 6)),
         R(FWD, 3, 8192, 16, 2, 1, (pass_name(False, 1024, 8), 6))]
# backward only: the batch tail with nbg = 2 threads per channel and B > 32 (one 128-channel group per strip)
ROWS += [R(BWD, 33, 20, 256, 2, 1, (pass_name(True, 256, 2), 66))]
# Multi-pass: strips of strip_width channels x B x pixel splits, then the elementwise pass on 64-channel strips x B x
# its own pixel splits. sdmi_gn_stats always runs it: 72 + 24 channels of 96 with one split and an unsplit apply; 2
# splits of 151 + 150 pixels; 8 splits of 129 (the last 127); 32 splits of 257 (the last 233) on 48 + 16 channels of 64.
ROWS += [
    R(STATS, 3, 5, 96, 32, 1, ("gn_stats_kernel", 6), ("gn_apply_kernel", 6)),
    R(STATS, 3, 301, 512, 2, 0, ("gn_stats_kernel", 12), ("gn_apply_kernel", 96)),
    R(STATS, 3, 1030, 128, 2, 1, ("gn_stats_kernel", 48), ("gn_apply_kernel", 96)),
    R(STATS, 3, 8200, 64, 4, 0, ("gn_stats_kernel", 192), ("gn_apply_kernel", 384)),
    # shapes pick_pass rejects: a 256-channel group with more than 256 pixels, a 64-channel group with more than 1024
    R(FWD, 3, 301, 512, 2, 1, ("gn_stats_kernel", 12), ("gn_apply_kernel", 96)),
    R(FWD, 3, 1030, 128, 2, 0, ("gn_stats_kernel", 48), ("gn_apply_kernel", 96)),
    R(BWD, 3, 301, 512, 2, 1, ("gn_bwd_reduce_kernel", 12), ("gn_bwd_apply_kernel", 96)),
    R(BWD, 3, 1030, 128, 2, 0, ("gn_bwd_reduce_kernel", 48), ("gn_bwd_apply_kernel", 96)),
    R(BWD, 3, 8200, 64, 4, 1, ("gn_bwd_reduce_kernel", 192), ("gn_bwd_apply_kernel", 384)),
]
# dgamma / dbeta deferred: the single-pass and the multi-pass form publish rows, sdmi_gn_rows_sum adds them
ROWS += [
    R(BWD_ROWS, 3, 13, 80, 4, 1, (pass_name(True, 64, 2), 6), ("gn_rows_sum_grouped_kernel", 1)),
    R(BWD_ROWS, 3, 301, 512, 2, 0, ("gn_bwd_reduce_kernel", 12), ("gn_bwd_apply_kernel", 96),
      ("gn_rows_sum_grouped_kernel", 2)),
]
# sdmi_gn_bwd_part on host-made segment partials: strips of 64 (4 segment lanes), 128 (4), 192 (2), 256 (2) channels,
# the whole row of 160 (3 lanes) and the strip_width fallback (72 of 288: 4 lanes); rb = 16 and 64; 1 and 2 pixel splits
ROWS += [
    R(PART, 3, 64, 128, 8, 1, ("gn_bwd_part_kernel", 6), rb=16),
    R(PART, 3, 192, 256, 2, 0, ("gn_bwd_part_kernel", 12), rb=64),
    R(PART, 3, 64, 384, 32, 1, ("gn_bwd_part_kernel", 6), rb=64),
    R(PART, 3, 128, 512, 2, 0, ("gn_bwd_part_kernel", 12), rb=16),
    R(PART, 3, 64, 160, 32, 1, ("gn_bwd_part_kernel", 3), rb=16),
    R(PART, 3, 192, 288, 32, 0, ("gn_bwd_part_kernel", 24), rb=64),
    R(PART_ROWS, 3, 64, 384, 32, 0, ("gn_bwd_part_kernel", 6), ("gn_rows_sum_grouped_kernel", 2), rb=16),
]
# sdmi_chan_sum (G unused): 56 + 40 channels of 96 per batch row, and in 10 segments of 68 rows (the last 63) with the
# second output and 88 stored channels; 24 + 16 channels of 40 with 4 pixel splits per batch row, and in 32 segments of
# 282 rows (the last 258) with 2 pixel splits
ROWS += [
    R(CHAN, 3, 225, 96, 1, 0, ("chan_sum_kernel", 6), mode="bc", per_c2=1, c_store=96),
    R(CHAN, 3, 225, 96, 1, 0, ("chan_sum_kernel", 20), mode="seg", per_c2=1, c_store=88),
    R(CHAN, 3, 600, 40, 1, 0, ("chan_sum_kernel", 24), mode="bc", per_c2=0, c_store=32),
    R(CHAN, 3, 3000, 40, 1, 0, ("chan_sum_kernel", 128), mode="seg", per_c2=0, c_store=40),
]
# three deferred backwards of different C (none a multiple of 256), summed by one grouped launch of 2 x 3 workgroups
ROWS += [
    R(GROUPED, 3, 1, 48, 4, 0, (pass_name(True, 64, 1), 6), (pass_name(True, 256, 1), 40), (pass_name(True, 64, 1), 12),
      ("gn_rows_sum_grouped_kernel", 6), jobs=((3, 1, 48, 4), (20, 9, 368, 4), (3, 5, 32, 32))),
]

# the counter-slot test alternates these two single-pass shapes (2 strips; 4 strips) and then checks this row
COUNTER_SHAPES = ((3, 1, 48, 4), (3, 5, 32, 32))
COUNTER_ROW = (3, 13, 80, 4)


def row_id(r):
    extra = "".join(f"-{k}{v}" for k, v in r.opt if k != "jobs")
    return f"{r.entry}-B{r.B}-P{r.P}-C{r.C}-G{r.G}-silu{r.silu}{extra}"


def kernels_named():
    return {name for r in ROWS for name, _ in r.launches}


# ----------------------------------------------------------------------------------------------------------------
# data (CPU, no library call): float64 tensors [B][P][C] holding bf16-representable values
# ----------------------------------------------------------------------------------------------------------------
def special_groups(b, G):
    """(first, second) special group of batch row b (None: this row has none): with three groups or more every batch
    row has both, with fewer they alternate between batch rows so that ordinary groups remain."""
    if G >= 3:
        return b % G, (b + 1) % G
    return (0, None) if b % 2 == 0 else (None, G - 1)


@functools.lru_cache(maxsize=8)
def exact_case(B, P, C, G, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    Cg = C // G
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()  # noqa: E731
    x, dy, add = ri(-8, 8, B, P, C), ri(-4, 4, B, P, C), ri(-4, 4, B, P, C)
    base = 1.0 if P <= 1000 else 0.0
    const, near = [], []
    for b in range(B):
        gc, gn = special_groups(b, G)
        if gc is not None:
            x[b, :, gc * Cg:(gc + 1) * Cg] = 3.0
            const.append((b, gc))
        if gn is not None and P * Cg >= 2:
            bits = ri(0, 1, P, Cg)
            bits.view(-1)[0], bits.view(-1)[-1] = 0.0, 1.0
            x[b, :, gn * Cg:(gn + 1) * Cg] = base + 2.0 ** -7 * bits
            near.append((b, gn))
    gamma = torch.randint(0, 2, (C,), generator=gen).double().mul(2).sub(1) * 2.0 ** ri(-2, 2, C)
    beta = ri(-16, 16, C) / 8
    return dict(kind="exact", B=B, P=P, C=C, G=G, x=x, dy=dy, add=add, gamma=gamma, beta=beta, const=const, near=near)


@functools.lru_cache(maxsize=8)
def soft_case(B, P, C, G, seed=0):
    gen = torch.Generator().manual_seed(2000 + seed)
    Cg = C // G
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    x = rn(B, P, C) * 2 + 0.5
    loud, quiet = [], []
    for b in range(B):
        gl, gq = special_groups(b, G)
        if gl is not None:
            x[b, :, gl * Cg:(gl + 1) * Cg] = 100.0 + rn(P, Cg)
            loud.append((b, gl))
        if gq is not None:
            x[b, :, gq * Cg:(gq + 1) * Cg] = 2.0 ** -6 * rn(P, Cg)
            quiet.append((b, gq))
    gamma = (rn(C) * 0.1 + 1).float().double()
    beta = (rn(C) * 0.1).float().double()
    return dict(kind="soft", B=B, P=P, C=C, G=G, x=bf16(x), dy=bf16(rn(B, P, C)), add=bf16(rn(B, P, C)), gamma=gamma,
                beta=beta, loud=loud, quiet=quiet)


def case_of(kind, B, P, C, G):
    return (exact_case if kind == "exact" else soft_case)(B, P, C, G)


# ----------------------------------------------------------------------------------------------------------------
# references (float64) and bounds
# ----------------------------------------------------------------------------------------------------------------
def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).double()


def is_bf16(x):
    return bool(torch.equal(bf16(x), x))


def ulp32(x):
    """The fp32 unit in the last place at |x|, elementwise (float64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def per_channel(t, C):
    """[B][G] -> [B][C]."""
    return t.repeat_interleave(C // t.shape[1], dim=1)


def group_stats(x, G, eps=EPS, weights=None, ddof=0):
    """mean, var, rstd [B][G] in float64 and the group averages E|x|, E x^2; `weights` [P] counts pixel rows (2: a
    row counted twice, 0: omitted; n stays P * Cg, as a kernel that miscounts rows would have it), `ddof` = 1 divides
    the variance by n - 1."""
    B, P, C = x.shape
    w = torch.ones(P, dtype=torch.float64) if weights is None else weights.double()
    xg = x.view(B, P, G, C // G)
    n = float(P * (C // G))
    s = lambda t: (t * w[None, :, None, None]).sum((1, 3))  # noqa: E731
    mean = s(xg) / n
    var = (s(xg * xg) / n - mean * mean).clamp_min(0.0)
    if ddof:
        var = var * n / (n - ddof)
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), eabs=s(xg.abs()) / n, ex2=s(xg * xg) / n)


def table_of(mean, rstd, gamma, beta):
    """[B][C][4] = {a, s, mean, rstd} from [B][G] statistics."""
    C = gamma.shape[0]
    m, r = per_channel(mean, C), per_channel(rstd, C)
    a = r * gamma
    return torch.stack([a, beta - m * a, m, r], -1)


def table_bounds(c, st, K=None):
    """Allowed |mean - ref| and |rstd - ref| [B][G] (docstring: table); K = K_SUM unless the caller measures."""
    if c["kind"] == "exact":
        return ulp32(st["mean"]), ulp32(st["rstd"])
    K = K_SUM if K is None else K
    bm = 2.0 ** -23 * st["mean"].abs() + K * U24 * st["eabs"]
    dvar = K * U24 * (st["ex2"] + 2 * st["mean"].abs() * st["eabs"])
    return bm, st["rstd"] * (2.0 ** -23 + dvar / (2 * (st["var"] + EPS)))


def check_table(c, tab, st=None, K=None):
    """None, or what is wrong with a table [B][C][4] (float64 copy of the fp32 values); also the worst error / bound."""
    st = st or group_stats(c["x"], c["G"])
    G, C = c["G"], c["C"]
    bm, br = table_bounds(c, st, K)
    a, s, m, r = tab.unbind(-1)
    Cg = C // G
    for name, col in (("mean", m), ("rstd", r)):
        if not bool((col.view(-1, G, Cg) == col.view(-1, G, Cg)[..., :1]).all()):
            return f"{name} differs within a group", float("inf")
    worst = 0.0
    for name, got, ref, lim in (("mean", m[:, ::Cg], st["mean"], bm), ("rstd", r[:, ::Cg], st["rstd"], br)):
        err = (got - ref).abs()
        worst = max(worst, float((err / lim).max()))
        if not bool((err <= lim).all()):
            return f"{name} off by {float((err / lim).max()):.3g} bounds", worst
    ea, la = (a - r * c["gamma"]).abs(), 2.0 ** -23 * a.abs()
    if c["kind"] == "exact":
        la = torch.zeros_like(la)
    es, ls = (s - (c["beta"] - m * a)).abs(), 2.0 ** -23 * (c["beta"].abs() + (m * a).abs())
    if not bool((ea <= la).all()):
        return "a is not rstd * gamma", worst
    if not bool((es <= ls).all()):
        return f"s off by {float((es / ls.clamp_min(1e-300)).max()):.3g} bounds", worst
    return None, worst


def act(z, silu):
    return z * torch.sigmoid(z) if silu else z


def act_grad(z, silu):
    if not silu:
        return torch.ones_like(z)
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def y_reference(c, tab, silu):
    """ref = act(x a + s) on the given table and the allowed |y - ref| (docstring: y)."""
    a, s = tab[..., 0][:, None], tab[..., 1][:, None]
    ref = act(c["x"] * a + s, silu)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -20 * ((c["x"] * a).abs() + s.abs())


def bwd_reference(c, tab, silu, sigmoid_only=False):
    """The backward in float64 on the given table [B][C][4]: S1, S2 [B][C], dgamma, dbeta [C], the parts of dx (without
    the addend), and the sums of absolute values T_* that scale the bounds (docstring: sums, dx)."""
    x, dy, gamma = c["x"], c["dy"], c["gamma"]
    B, P, C = x.shape
    G, Cg = c["G"], C // c["G"]
    a, s, m, r = (tab[..., i][:, None] for i in range(4))
    z = x * a + s
    gp = torch.sigmoid(z) if (silu and sigmoid_only) else act_grad(z, silu)
    dz = dy * gp
    W = dz.abs() + (SILU_ABS * dy.abs() if silu else 0.0)
    xh = (x - m) * r
    S1, S2 = dz.sum(1), (dz * xh).sum(1)
    T1, T2 = W.sum(1), (W * xh.abs()).sum(1)
    grp = lambda t: per_channel(t.view(B, G, Cg).sum(-1), C)  # noqa: E731
    A, Bc = grp(gamma * S1), grp(gamma * S2)
    TA, TB = grp(gamma.abs() * T1), grp(gamma.abs() * T2)
    n = float(P * Cg)
    rs, mu = tab[..., 3], tab[..., 2]
    q = -rs * rs * Bc / n
    o = rs * rs * mu * Bc / n - rs * A / n
    adz, qx = a * dz, q[:, None] * x
    T_dx = a.abs() * W + (rs * rs * TB / n)[:, None] * (x.abs() + mu.abs()[:, None]) + (rs * TA / n)[:, None]
    return dict(S1=S1, S2=S2, T_S1=T1, T_S2=T2, dgamma=S2.sum(0), dbeta=S1.sum(0), T_dgamma=T2.sum(0),
                T_dbeta=T1.sum(0), adz=adz, qx=qx, o=o[:, None].expand_as(x), T_dx=T_dx)


def dx_reference(c, bw, addend, drop_qx=False):
    """dx and the allowed |dx - ref|."""
    ref = bw["adz"] + bw["o"] + (0.0 if drop_qx else bw["qx"])
    T = bw["T_dx"]
    if addend:
        ref, T = ref + c["add"], T + c["add"].abs()
    return ref, 2.0 ** -8 * ref.abs() + K_SUM * U24 * T


def sum_bound(T, bf16_out=False, ref=None):
    return K_SUM * U24 * T + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)


def host_partials(bw_terms, rb):
    """part[b][seg][c] = {sum dz, sum dz xhat} over each rb pixel rows, float64 rounded to fp32: [B][P / rb][C][2]."""
    dz, dzx = bw_terms
    B, P, C = dz.shape
    f = lambda t: t.view(B, P // rb, rb, C).sum(2)  # noqa: E731
    return torch.stack([f(dz), f(dzx)], -1).float()


def dz_terms(c, tab, silu):
    """dz and dz xhat [B][P][C] in float64 on the given table."""
    a, s, m, r = (tab[..., i][:, None] for i in range(4))
    dz = c["dy"] * act_grad(c["x"] * a + s, silu)
    return dz, dz * (c["x"] - m) * r


def bwd_reference_from_partials(c, tab, silu, part):
    """bwd_reference with S1, S2 replaced by the float64 sums of the fp32 partials the kernel is given."""
    bw = bwd_reference(c, tab, silu)
    B, P, C = c["x"].shape
    G, Cg = c["G"], C // c["G"]
    S = part.double().sum(1)
    S1, S2 = S[..., 0], S[..., 1]
    grp = lambda t: per_channel(t.view(B, G, Cg).sum(-1), C)  # noqa: E731
    A, Bc = grp(c["gamma"] * S1), grp(c["gamma"] * S2)
    n = float(P * Cg)
    rs, mu = tab[..., 3], tab[..., 2]
    q = -rs * rs * Bc / n
    o = rs * rs * mu * Bc / n - rs * A / n
    bw.update(S1=S1, S2=S2, dgamma=S2.sum(0), dbeta=S1.sum(0), qx=q[:, None] * c["x"], o=o[:, None].expand_as(c["x"]))
    return bw


def chan_reference(c, B, P, C):
    dy = c["dy"]
    per_bc = dy.sum(1)
    return dict(per_bc=per_bc, per_c=per_bc.sum(0), T_bc=dy.abs().sum(1), T_c=dy.abs().sum((0, 1)))


# ----------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' arithmetic in a chosen summation order (CPU, torch)
# ----------------------------------------------------------------------------------------------------------------
SEQ_RUN = 256


def sum32(t, dim, order):
    """fp32 sum along dim: 'seq' adds the terms one by one in index order, in runs of at most 256 terms whose sums are
    added the same way (no thread of norm.hip adds a longer chain: a single-pass thread adds its <= 8 rows and then
    <= 256 / L row partials, a reduction thread its pixel split's rows / R, then R <= 256 partials and <= 32 splits);
    'pair' adds halves recursively."""
    t = t.movedim(dim, 0).contiguous()
    assert t.dtype == torch.float32
    if order == "seq":
        while t.shape[0] > 1:
            runs = []
            for i0 in range(0, t.shape[0], SEQ_RUN):
                acc = t[i0]
                for i in range(i0 + 1, min(i0 + SEQ_RUN, t.shape[0])):
                    acc = acc + t[i]
                runs.append(acc)
            t = torch.stack(runs)
        return t[0]
    while t.shape[0] > 1:
        h = t.shape[0] // 2
        t = torch.cat([t[:h] + t[h:2 * h], t[2 * h:]])
    return t[0]


def fma32(a, b, c):
    """fmaf: the product and the sum in float64 (exact for fp32 operands up to the last of 106 bits), rounded once."""
    return (a.double() * b.double() + c.double()).float()


def emulate_forward(c, silu, order):
    """The forward with the kernels' rounding points: fp32 channel sums in `order`, the fp64 group merge, mean and rstd
    rounded to fp32, a and s in fp32, y = act(fma(x, a, s)) in fp32 (before its bf16 rounding)."""
    B, P, C = c["x"].shape
    G, Cg = c["G"], C // c["G"]
    x = c["x"].float()
    s1, s2 = sum32(x, 1, order), sum32(x * x, 1, order)
    n = float(P * Cg)
    m1, m2 = s1.double().view(B, G, Cg).sum(-1), s2.double().view(B, G, Cg).sum(-1)
    mu = m1 / n
    var = (m2 / n - mu * mu).clamp_min(0.0)
    mean, rstd = per_channel(mu.float(), C), per_channel((1.0 / torch.sqrt(var + EPS)).float(), C)
    a = rstd * c["gamma"].float()
    s = c["beta"].float() - mean * a
    tab = torch.stack([a, s, mean, rstd], -1)
    z = fma32(x, a[:, None], s[:, None])
    return tab.double(), (z * torch.sigmoid(z) if silu else z).double()


def emulate_backward(c, tab, silu, order, addend):
    """The backward in fp32 on the fp32 table `tab`, every sum in `order`; dx before its bf16 rounding. z and dx are
    formed with the kernel's fmas. The accumulating fmas of the reductions (v = fma(dz, xhat, v)) are modelled as a
    rounded product that is then added: one rounding more per term than the kernel, so the model is the coarser."""
    B, P, C = c["x"].shape
    G, Cg = c["G"], C // c["G"]
    x, dy, gamma = c["x"].float(), c["dy"].float(), c["gamma"].float()
    a, s, m, r = (tab[..., i].float()[:, None] for i in range(4))
    if silu:
        z = fma32(x, a, s)
        sg = torch.sigmoid(z)
        dz = dy * (sg * (1 + z * (1 - sg)))
    else:
        dz = dy
    S1, S2 = sum32(dz, 1, order), sum32(dz * ((x - m) * r), 1, order)
    grp = lambda t: per_channel(sum32(t.view(B, G, Cg), 2, order), C)  # noqa: E731
    A, Bc = grp(gamma * S1), grp(gamma * S2)
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(P) * Cg, dtype=torch.float32)
    rs, mu = tab[..., 3].float(), tab[..., 2].float()
    q = -rs * rs * Bc * inv_n
    o = rs * rs * mu * Bc * inv_n - rs * A * inv_n
    dx = fma32(a, dz, fma32(q[:, None], x, o[:, None]))
    if addend:
        dx = c["add"].float() + dx
    return dict(S1=S1.double(), S2=S2.double(), dgamma=sum32(S2, 0, order).double(), dbeta=sum32(S1, 0, order).double(),
                dx=dx.double())


# ----------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ----------------------------------------------------------------------------------------------------------------
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
CONTIGUOUS, WINDOWS = "contiguous", "windows"
# (extra row stride, first column) of the operands as windows of wider buffers: every stride and offset differs
_WINDOW = dict(x=(8, 0), dy=(16, 8), add=(24, 16), y=(24, 8), dx=(32, 24))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Flat:
    """n fp32 elements between a 64-element front pad and a 256-element tail, all NaN; `data` is the logical window."""

    def __init__(self, n, device, front=64, tail=256):
        self.buf = torch.full((front + n + tail,), float("nan"), dtype=torch.float32, device=device)
        self.n, self.front = n, front
        self.data = self.buf[front:front + n]

    def put(self, values):
        self.data.copy_(values.reshape(-1).to(torch.float32))
        return self

    def get(self, *shape):
        return self.data.cpu().double().view(*shape)


def bits(t):
    return t.view(_BITS[t.dtype])


class Guard:
    """Snapshots of buffers taken before a call; afterwards only the declared regions may differ, bit for bit."""

    def __init__(self):
        self.items = []

    def add(self, name, buf, writable=()):
        """writable: flat (start, stop) ranges, or for a Buf (col0, cols) windows given as ('w', col0, cols)."""
        self.items.append((name, buf, buf.buf.clone(), tuple(writable)))

    def changed(self):
        bad = []
        for name, buf, snap, writable in self.items:
            now = buf.buf.clone()
            for w in writable:
                for t in (now, snap):
                    if w[0] == "w":
                        t[buf.front + w[1]:].as_strided((buf.rows, w[2]), (buf.ld, 1)).zero_()
                    else:
                        t[buf.front + w[0]:buf.front + w[1]].zero_()
            if not torch.equal(bits(now), bits(snap)):
                bad.append(name)
        return ", ".join(bad) or None


class Problem:
    """One case on the device in one layout: x, dy, addend, y, dx as [B * P][C] windows (contiguous: ld = C; windows:
    ld = C + 8 .. C + 32 at column offsets 0 .. 24 of NaN-filled buffers), gamma, beta, table, table2, dgamma, dbeta,
    rows and the workspace as guarded fp32 buffers."""

    def __init__(self, c, layout, L, device="cuda", alias_dx=False):
        B, P, C = c["x"].shape
        self.c, self.dims, self.L = c, (B, P, C, c["G"]), L
        self.bufs, self.win = {}, {}
        for name in ("x", "dy", "add", "y", "dx"):
            pad, col0 = (0, 0) if layout == CONTIGUOUS else _WINDOW[name]
            if name == "dx" and alias_dx:
                self.bufs[name], self.win[name] = self.bufs["dy"], self.win["dy"]
                continue
            b = Buf(B * P, C + pad, torch.bfloat16, device)
            self.bufs[name], self.win[name] = b, b.window(col0, C)
            b.col0 = col0
            if name in c:
                self.win[name].copy_(c[name].reshape(B * P, C).to(torch.bfloat16))
        self.alias_dx = alias_dx
        self.gamma, self.beta = Flat(C, device).put(c["gamma"]), Flat(C, device).put(c["beta"])
        self.table, self.table2 = Flat(B * C * 4, device), Flat(B * C * 4, device)
        self.dgamma, self.dbeta, self.rows = Flat(C, device), Flat(C, device), Flat(B * C * 2, device)
        self.ws_need = L.sdmi_chan_reduce_workspace(B, P, C)
        assert self.ws_need % 4 == 0
        self.ws = Flat(self.ws_need // 4, device, tail=4096)

    def ld(self, name):
        return self.win[name].stride(0)

    def guard(self, outputs):
        """A Guard over every buffer; `outputs` names those a call may write (their logical windows only)."""
        g = Guard()
        C = self.dims[2]
        seen = set()
        for name in ("x", "dy", "add", "y", "dx"):
            b = self.bufs[name]
            if id(b) in seen:
                continue
            seen.add(id(b))
            out = name in outputs or (name == "dy" and self.alias_dx and "dx" in outputs)
            g.add(name, b, [("w", b.col0, C)] if out else [])
        for name in ("gamma", "beta", "table", "table2", "dgamma", "dbeta", "rows"):
            f = getattr(self, name)
            g.add(name, f, [(0, f.n)] if name in outputs else [])
        g.add("workspace", self.ws, [(0, self.ws.n)] if "ws" in outputs else [])
        return g

    def out(self, name):
        B, P, C, _ = self.dims
        return self.win[name].cpu().double().view(B, P, C)

    # ---- the entry points
    def stats(self, stream):
        B, P, C, G = self.dims
        return self.L.sdmi_gn_stats(ptr(self.win["x"]), self.ld("x"), B, P, C, G, EPS, ptr(self.gamma.data),
                                    ptr(self.beta.data), ptr(self.ws.data), ptr(self.table.data), stream)

    def apply(self, silu, stream):
        B, P, C, G = self.dims
        return self.L.sdmi_gn_apply(ptr(self.win["x"]), self.ld("x"), ptr(self.win["y"]), self.ld("y"),
                                    ptr(self.table.data), B, P, C, silu, stream)

    def fwd(self, silu, stream):
        B, P, C, G = self.dims
        return self.L.sdmi_gn_fwd(ptr(self.win["x"]), self.ld("x"), ptr(self.win["y"]), self.ld("y"), B, P, C, G, EPS,
                                  ptr(self.gamma.data), ptr(self.beta.data), silu, ptr(self.ws.data),
                                  ptr(self.table.data), stream)

    def _bwd_head(self, silu):
        B, P, C, G = self.dims
        return (ptr(self.win["x"]), self.ld("x"), ptr(self.win["dy"]), self.ld("dy"), ptr(self.win["dx"]),
                self.ld("dx"), ptr(self.table.data), ptr(self.gamma.data), B, P, C, G, silu)

    def _add(self, addend):
        return (ptr(self.win["add"]), self.ld("add")) if addend else (None, 0)

    def bwd(self, silu, stream, addend=False, sums=True):
        dg, db = (ptr(self.dgamma.data), ptr(self.dbeta.data)) if sums else (None, None)
        return self.L.sdmi_gn_bwd(*self._bwd_head(silu), ptr(self.ws.data), ptr(self.table2.data), dg, db,
                                  *self._add(addend), stream)

    def bwd_rows(self, silu, stream, addend=False):
        return self.L.sdmi_gn_bwd_rows(*self._bwd_head(silu), ptr(self.ws.data), ptr(self.table2.data),
                                       ptr(self.rows.data), *self._add(addend), stream)

    def bwd_part(self, silu, part, rb, stream, addend=False, sums=True):
        dg, db = (ptr(self.dgamma.data), ptr(self.dbeta.data)) if sums else (None, None)
        return self.L.sdmi_gn_bwd_part(*self._bwd_head(silu), ptr(part), rb, ptr(self.ws.data), dg, db,
                                       *self._add(addend), stream)

    def bwd_part_rows(self, silu, part, rb, stream, addend=False):
        return self.L.sdmi_gn_bwd_part_rows(*self._bwd_head(silu), ptr(part), rb, ptr(self.ws.data),
                                            ptr(self.rows.data), *self._add(addend), stream)

    def rows_sum(self, stream):
        B, P, C, G = self.dims
        return self.L.sdmi_gn_rows_sum(ptr(self.rows.data), B, C, ptr(self.dgamma.data), ptr(self.dbeta.data), stream)


class RowsJob(ctypes.Structure):
    """sdmi_gn_rows_job of include/sdmi.h."""
    _fields_ = [("rows", ctypes.c_void_p), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p),
                ("B", ctypes.c_int), ("C", ctypes.c_int)]
