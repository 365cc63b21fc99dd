"""The declared test matrix of the staging, packing, loss and leaf kernels -- csrc/misc.hip (every kernel but add_noise,
which tests/sampler_matrix.py covers) and csrc/leafops.hip -- and the helpers its exact tests share.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`. The expected launches -- a
fragment of the mangled kernel name, with its template argument where there is one, and the grid -- are written by
hand. The host rules of both sources are restated below, also by hand. misc.hip: NT = 256; grid_for = max(1,
min(ceil(work / 256), 8192)) with work = B C HW (sdmi_nhwc_to_nchw), B HW ld (sdmi_nchw_to_nhwc_bf16), P C / 8
(sdmi_copy_slice), n (sdmi_relu, sdmi_silu), B dim / 2 (sdmi_time_embedding); prep_grid = max(1, min(ceil(B H W / 64),
65536)); sdmi_mse launches min(grid_for(B HW ld), 1024) workgroups (its workspace is 1024 floats) and then
sum_partials_kernel <<<1>>>; sdmi_cond_wgrad(_cmap) launches a (cmo cmi, 32) grid and then a finisher of ceil(cmo cmi /
256) workgroups; sdmi_pack_weights and sdmi_pack_transpose launch nblocks workgroups and nothing for nblocks <= 0. The
pack work split: max(1, sdmi_pack_chunk() / (KH KW Ipad)) rows per workgroup (chunk = 4096), one int2 (descriptor, first
row) each, KH KW (Ipad + 8) <= 16384; pack_path restates which of the kernel's three paths a workgroup takes (identity:
Ipad = I, unit channel stride, no dst_ld, identity taps, contiguous rows, row % 8 = 0, 16-byte aligned source; one pass:
more than one row and nrows taps (Ipad + 8) <= 16384; else per row, with the tap switch 1 / 4 / 9 / 16 / other). With
block maps built by that rule a workgroup of several rows always fits the one-pass path (nrows taps (Ipad + 8) <= 8192),
so the per-row loop runs only for one-row workgroups: row > 2048 or a tail with O mod rows = 1; the CPU test asserts it
and rows cover both. The transpose split: one int4 (descriptor, first i, first o, tap) per 64 x 64 tile per tap.
leafops.hip: grid_of = max(1, min(ceil(work / 256), 65535 * 8)); sdmi_modulate_bwd launches (ceil(C / 64), B);
sdmi_attn_map (N, B). status() restates every -1 return (a null required pointer, a non-positive size, a row stride
below its columns, cpad not 8 or 16, cmo outside 1..16, cmi outside 1..255, C / lds / ldd of a slice off 8, an odd dim,
S > 4096); tests/test_stage_matrix_cpu.py calls the library with each and expects what status() says, before any launch.
tests/test_stage_matrix_cpu.py checks rows against rules and that no row can be removed;
tests/test_stage_exact_gpu.py that the library launches what the rows say.

Entry points and dims: N2C sdmi_nhwc_to_nchw (B, C, HW, ld) with f32; C2N sdmi_nchw_to_nhwc_bf16 (B, C, HW, ld); SLICE
sdmi_copy_slice (P, C, lds, ldd) with acc; RELU sdmi_relu (n) with bwd; RESIZE sdmi_resize_nearest (BC, IH, IW, OH, OW);
CHAN sdmi_chan_copy (B, C, P, src_c, src_c0, dst_c, dst_c0); PACK sdmi_pack_weights, TPACK sdmi_pack_transpose with
descs (the descriptors as data: O, I, Ipad, KH, KW, layout conv = [O][I][SKH][SKW] / nat = [O][SKH][SKW][I], flip, phase,
dst_ld / col0, src_off in bytes; O, I, smap, staps = the taps of the source, dst_tap, dst_pad); PREP
sdmi_prep_input(_cmap) (B, cx, H, W, cpad) with mask (none / soft: fp32 in [0, 1] / cmap: uint8 classes), cmi, cmo, MH,
MW, keep; CW sdmi_cond_wgrad and, in the exact family, sdmi_cond_wgrad_cmap on the same mask (B, H, W, cmo, cmi) with
family, MH, MW, keep (ld = 24, cx = 3); MSE sdmi_mse (B, C, HW, ld) with gdev, grad; TEMB sdmi_time_embedding (B, dim,
ld) with t, tstride, f32; SILU sdmi_silu (65536: every bf16 bit pattern) with bwd, dy; MODF / MODB
sdmi_modulate_fwd / _bwd (B, N, C) with r, t, alpha, ls6, null; AMAP sdmi_attn_map (B, H, N, S, d) with avg, wide, big.
Shapes are the smallest at which each kernel can still go wrong; the capped-grid rows (8192 * 256 + 257 items and the
like, at most 67 MB) reach the second turn of each grid-stride loop. The leaf grid cap (134 M items) is out of reach at
any sane size and is not tested; nor is B > 65535 on the y grid of modulate_bwd and attn_map.

Value family of the movers (movement_values): 24-bit integers times 2^-20 with, at every fifth element, the CAST targets
of tests/optim_matrix.py (bf16 ties on both sides, a value that rounds up into the next binade, +-0, +-inf, the largest
finite value -- it rounds to inf --, NaN) and fp32 and bf16 denormals (2^-149, 2^-134 and 3 * 2^-134: ties at the bottom
of the bf16 range). A NaN matches any NaN; everything else compares by bits, -0 included.

Statements (u = 2^-24; T the sum of absolute terms; references are float64 on the stored inputs).

  movers   sdmi_nhwc_to_nchw, sdmi_nchw_to_nhwc_bf16 (pad columns +0), sdmi_copy_slice (accumulate: bitwise
           bf16(fp32(a) + fp32(b)), one add and RNE; sums that tie, overflow, cancel; columns past C untouched),
           sdmi_resize_nearest (F.interpolate), sdmi_chan_copy (torch.cat), sdmi_pack_weights, sdmi_pack_transpose:
           bitwise a torch index model on the CPU, which the CPU test checks against torch's own op or a plain loop.
  relu     bitwise y = x <= 0 ? +0 : x and dx = x <= 0 ? +0 : dy: a NaN x gives NaN forward and passes dy backward
           (torch.relu and aten's threshold_backward on the CPU). Both zeros give +0; aten's CPU kernel returns -0 for
           -0, an accident of its vectorised max, and that sign is not followed. A kernel that
           computes v > 0 ? v : 0 returns 0 for a NaN in both directions (relu_model_old: the CPU test shows it leaves
           the statement at the NaN elements and nowhere else).
  prep     x converted bitwise, columns past cx + cmo +0. Class map: bitwise bf16(w[o][min(cls, cmi) - 1] * keep[b]),
           +0 for class 0 (so a negative weight under keep = 0 is -0). fp32 mask: |out - ref| <= ulp_bf16(ref) / 2 +
           K_PREP u T, ref = sum_i w[o][i] m[..] keep[b] on the nearest-resized mask (index model = F.interpolate).
  wgrad    exact family (dxin integers in [-8, 8], one-hot mask, keep in {0, 1}: every partial sum an integer below
           2^24 in any order): dw bitwise, one-hot form = class-map form bitwise; soft: |dw - ref| <= K_CW u T. Nine
           calls in a row wrap the eight partial-sum slots, each with its own data.
  mse      gradient bitwise numpy.float32 bf16(2 d / n gscale) (d one rounded subtraction; the division is the
           correctly rounded one of plain hipcc -O3), pad columns +0; |loss - ref| <= K_MSE u loss; exact family
           (pred - target small integers, n a power of two) loss bitwise. The workspace is a guarded window of exactly
           sdmi_mse_workspace() bytes of which only the first `blocks` floats may change.
  temb     |out_f32 - ref| <= u (K_TA |a| + K_TS), a = t / 10000^(j / half) with the exponent the fp32 quotient (the
           reference forms it in fp32), everything after in float64; the first term is the error of the fp32 angle. The
           bf16 output is bitwise RNE of the kernel's own out_f32, and the same bits without out_f32. The reference
           program's own fp32 values (tests/golden/time_embedding.safetensors) satisfy the same bound (ratio 0.163);
           the kernel differs from them by at most 6.06e-5 (at t = 999, where u K_TA |a| = 4.8e-4): a measurement.
  silu     every bf16 x. Forward |y - silu64(x)| <= ulp_bf16 / 2 + K_S u |silu64(x)|; backward, for dy in SILU_DY,
           |dx - ref| <= ulp_bf16 / 2 + K_SB u T, T = |dy| s (1 + |x| (1 - s)). NaN in, NaN out; -inf forward and +-inf
           backward give NaN (inf * 0), as the float64 formula and torch do. For x <= -89 the fp32 evaluation of
           1 + 2^(-x log2 e) overflows: the kernel and torch's own fp32 F.silu both return -0 (backward: a zero); the
           float64 value there is below 2.0e-37. The statement for those inputs is "-0, bitwise" (backward: "a zero"),
           and the CPU test asserts that torch fp32 gives exactly that on every such input, so the carve-out is the
           reference's, not the kernel's.
  modulate forward |y - ref| <= K_MF u T, T = |x| (|alpha| + |s|) + |t| + |r|; dx bitwise one rounded product of dy and
           the fp32 alpha + s; |ds - ref| <= K_MS u T, |dt - ref| <= K_MT u T; all bitwise on the exact family (small
           integers and powers of two).
  attn map per head p_j = softmax_j(q.k_j scaling): |out - ref| <= K_A u T + 2^-126, T_j = p_j (1 + A_j + sum_k p_k
           A_k), A_j = d sum_e |q_e k_je| |scaling| + |sc_j| + |sc_j - max|: the d fused terms of the dot product and the
           scaling (first two terms of A_j), the subtraction of the maximum (third; the maximum's own error cancels: the
           softmax is shift invariant), then expf, the S-term sum of non-negative terms, the reciprocal, the product and
           the head average, each a relative error of p_j or of the normaliser (the p-weighted mean of the A_k); 2^-126
           is the fp32 underflow threshold (a term below it may be flushed). The head average is the mean of the heads'
           bounds. Every row of a per-head map sums to 1 within K_AROW u (the sum's and the reciprocal's roundings only:
           the error of expf does not enter). Exact families: every score equal gives fl(1 / S), one score 200 above the
           rest gives {1, 0}, bitwise (the average too for H in 1, 2, 4).

Constants are measured, not chosen: tests/test_stage_matrix_cpu.py runs an fp32 emulation of each kernel in its own
order (prep: i ascending from 0; wgrad: per thread its pixels p0 + tid, + 256, .., the 64-lane butterfly, the four waves
in order, the 32 splits in order; mse: the grid-stride terms of each thread, butterfly, waves, then sum_partials the
same way and the product by fl(1 / n); modulate_bwd: row lane l its rows l, l + 4, .., then ((l0 + l1) + l2) + l3;
attn_map: the fmaf chain, scaling, maximum, the 16 keys of a thread in order, butterfly, waves, 1 / sum, the heads in
order, fl(1 / H)), once with every product rounded separately and once with the contractions -ffp-contract=fast
permits, on every soft row, and measures max |fp32 - float64| / (u T). The larger ratio per statement is EMULATED; K is
twice it, rounded up, because the GPU's own contraction choices are a third variant: prep 2.09 -> 5, wgrad 2.02 -> 5,
mse 0.82 -> 2, angle 1.57 -> 4, sin / cos 0.50 -> 1, silu 57.5 -> 115 (the rounding of -x log2 e, |x| up to 88.5, is
the whole of it), silu backward 56.6 -> 114, modulate 2.38 -> 5, ds 2.53 -> 6, dt 1.76 -> 4, attn map 0.94 -> 2, its row
sums 2.64 -> 6. The device math library's own error cannot be measured here; it is the ALLOWANCE tests/sampler_matrix.py
already uses, added to K and NOT a measurement: 2 ulp (4 u relative) per powf, sinf, cosf, expf call, 1 ulp (2 u) each
for the raw v_exp_f32 and v_rcp_f32 behind the SiLU (csrc/common.h). K_TA = 4 + 4 (powf), K_TS = 1 + 4 (sinf / cosf),
K_S = 115 + 4 (2 u (1 - s) from the exponential, 2 u from the reciprocal), K_A = 2 + 8 (4 u on the term and 4 u on the
normaliser). SiLU backward: an error eps s of s moves s (1 + x (1 - s)) by eps s (1 + x (1 - 2 s)), at most (1 + |x|)
times T's share, and beyond x = 17.5 fp32 s is exactly 1 (the reciprocal of 1), so 4 u (1 + 17.5): K_SB = 114 + 74.
The CPU test asserts that the emulations stay within (K - allowance) / 2, that 2 ratio <= K - allowance <= 3 ratio,
and that each perturbed reference leaves its statement: one pixel, lane, wave or split dropped or a pixel counted
twice (wgrad), an item or a block dropped (mse), a row dropped (modulate), the floor of the nearest index replaced by
rounding, the clamp of the class removed, n off by the pad columns, sin and cos swapped, half replaced by dim, round
half away instead of RNE on the family's ties (and one bf16 ulp on the SiLU: at the edge of its bound or outside), the
softmax without its maximum (overflows fp32 on the +-80 rows), the average over H - 1 heads, a packer that drops the
last row of a chunk, ignores the flip or leaves a pad column, a transpose with the identity tap map, a ReLU
that swallows the NaN.

Measured on an MI355X, max(err / bound) over all rows: cond_wgrad 0.403, mse loss 0.408 (the exact
family where n is no power of two: 0.147), time embedding 0.243, modulate
forward 0.475, ds 0.385, dt 0.440, attention map 0.109, its row sums 0.446. The three bf16 statements read 1.000 (prep
mask columns), 1.000 (silu forward) and 0.997 (silu backward): an fp32 value next to a bf16 tie is off its float64
value by all but nothing of the half ulp, which is then the whole bound; that is the format, not the kernel. What is
left of the error beyond the half ulp, as a share of the fp32 part K u T, is at most 0.089 (prep), 0.013
(silu forward) and 0.007 (silu backward). Bitwise on every row: the movers, converters, packers (the
misaligned source against the fast path too), ReLU, the class-map staging, x and the zero columns of every staging row,
dw of the exact family in both forms and of nine calls in a row, the MSE gradient and the exact family's loss (capped
grid included), the bf16 time embedding against its own fp32 output and without out_f32, dx of the modulation and its
exact family, the equal and peak families of the attention map, every bit of a second call; and no guard changed.
Rows that pin more than rounding. relu-*: the NaN (above). silu-65536-bwd0 and its four backward rows pin x = -88.5,
-88 and -87.5, where 1 + 2^(-x log2 e) exceeds 2^126 but silu is still a normal number (-3.25e-37 at -88.5, -8.76e-37 at
-87.5; torch fp32 returns them): v_rcp_f32 flushes a subnormal result, so x * v_rcp_f32(sum) is -0 there, err / bound
441 forward and 439 backward. sdmi_silu takes the reciprocal of 2^-64 times the sum where it exceeds 2^64 and scales
the product back (silu_wide_f in csrc/common.h); those three inputs are the only ones of the 65536, forward and for
each dy, at which that differs in a bit from silu_f, which the fused GroupNorm and GEMM epilogues keep. The error
returns of status() hold for every entry point of both sources, sdmi_mse with B C HW = 0 included, and no caller in
sdmi/ passes what is refused.

Guards: every operand and output -- descriptor arrays, block maps, class maps and timesteps included -- is a window of
a NaN-filled buffer; after a call only the declared outputs may have changed, bit for bit (for a column slice, only its
columns). A second identical call repeats every bit. No element is excluded from any statement."""
import collections
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.optim_matrix import (CAST_SPECIALS, Buf, Flat, Guard, Win, bf16, bits, butterfly32, cdiv,  # noqa: F401
                                fma32, launches_match, ptr, recorded, same_bits, seq32, sum32, ulp32)

N2C, C2N, SLICE, RELU, RESIZE, CHAN = "nhwc_to_nchw", "nchw_to_nhwc", "copy_slice", "relu", "resize", "chan_copy"
PACK, TPACK, PREP, CW, MSE, TEMB, SILU = "pack", "tpack", "prep", "cond_wgrad", "mse", "time_embedding", "silu"
MODF, MODB, AMAP = "modulate_fwd", "modulate_bwd", "attn_map"
ENTRIES = (N2C, C2N, SLICE, RELU, RESIZE, CHAN, PACK, TPACK, PREP, CW, MSE, TEMB, SILU, MODF, MODB, AMAP)
Row = collections.namedtuple("Row", "entry dims launches opt")
f32 = np.float32
U24 = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("separate", "fused")

# constants: (emulated ratio, library allowance, K); the docstring says how each was obtained
EMULATED = dict(prep=2.09, cw=2.02, mse=0.82, ta=1.57, ts=0.50, silu=57.5, silub=56.6, modf=2.38, mods=2.53, modt=1.76,
                amap=0.94, arow=2.64)
ALLOW = dict(prep=0.0, cw=0.0, mse=0.0, ta=4.0, ts=4.0, silu=4.0, silub=74.0, modf=0.0, mods=0.0, modt=0.0, amap=8.0,
             arow=0.0)
K_PREP, K_CW, K_MSE, K_TA, K_TS, K_S, K_SB, K_MF, K_MS, K_MT, K_A, K_AROW = 5.0, 5.0, 2.0, 8.0, 5.0, 119.0, 188.0, 5.0, \
    6.0, 4.0, 10.0, 6.0
KS = dict(prep=K_PREP, cw=K_CW, mse=K_MSE, ta=K_TA, ts=K_TS, silu=K_S, silub=K_SB, modf=K_MF, mods=K_MS, modt=K_MT,
          amap=K_A, arow=K_AROW)


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


def spec(**kw):
    """A descriptor of a PACK / TPACK row as hashable data."""
    return tuple(sorted(kw.items()))


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/misc.hip and csrc/leafops.hip, restated
# ----------------------------------------------------------------------------------------------------------------
NT = 256
GRID_CAP = 8192
PREP_NT, PREP_CAP = 64, 65536
MSE_CAP = 1024
CW_SPLITS, CW_SLOTS = 32, 8
LEAF_CAP = 65535 * 8
PACK_CHUNK = 4096
PACK_LDS = 16384
AMAP_SMAX = 4096
K_N2C, K_C2N, K_SLICE, K_RELU = "19nhwc_to_nchw_kernel", "24nchw_to_nhwc_bf16_kernel", "17copy_slice_kernel", \
    "11relu_kernel"
K_RESIZE, K_CHAN, K_PACK, K_TPACK = "21resize_nearest_kernel", "16chan_copy_kernel", "11pack_kernel", \
    "21pack_transpose_kernel"
K_PREP0, K_PREP1 = "prep_input_kernelILb0EE", "prep_input_kernelILb1EE"
K_CW0, K_CW1, K_CWF = "cond_wgrad_kernelILb0EE", "cond_wgrad_kernelILb1EE", "24cond_wgrad_finish_kernel"
K_MSEK, K_SUMP, K_TEMB, K_SILU = "10mse_kernel", "19sum_partials_kernel", "21time_embedding_kernel", "11silu_kernel"
K_MODF, K_MODB, K_AMAP = "19modulate_fwd_kernel", "19modulate_bwd_kernel", "15attn_map_kernel"


def grid_for(work):
    return max(1, min(cdiv(work, NT), GRID_CAP))


def prep_grid(work):
    return max(1, min(cdiv(work, PREP_NT), PREP_CAP))


def grid_of(work):
    return max(1, min(cdiv(work, NT), LEAF_CAP))


def mse_blocks(total):
    return min(grid_for(total), MSE_CAP)


def mse_workspace():
    return MSE_CAP * 4


def pack_rows(d):
    """Destination rows per workgroup of a pack descriptor."""
    d = dict(d)
    return max(1, PACK_CHUNK // (d["KH"] * d["KW"] * d["Ipad"]))


def pack_bmap(descs):
    """One (descriptor, first row) per workgroup, by the documented rule."""
    return [(j, o) for j, d in enumerate(descs) for o in range(0, dict(d)["O"], pack_rows(d))]


def pack_strides(d):
    """(so, si, skh, skw, kh_off, kh_mul, kw_off, kw_mul, source shape) of a descriptor spec. Layout `conv` is torch's
    [O][I][SKH][SKW] (channel-slow), `nat` the GEMM-natural [O][SKH][SKW][I] (channel-fast; a linear is 1 x 1)."""
    d = dict(d)
    I, O, KH, KW = d["I"], d["O"], d["KH"], d["KW"]
    SKH, SKW = d.get("SKH", KH), d.get("SKW", KW)
    if d["layout"] == "conv":
        so, si, skh, skw, shape = I * SKH * SKW, SKH * SKW, SKW, 1, (O, I, SKH, SKW)
    else:
        assert d["layout"] == "nat"
        so, si, skh, skw, shape = SKH * SKW * I, 1, SKW * I, I, (O, SKH, SKW, I)
    if d.get("flip"):
        taps = (KH - 1, -1, KW - 1, -1)
    elif d.get("phase") is not None:
        taps = (d["phase"][0], 2, d["phase"][1], 2)
    else:
        taps = (0, 1, 0, 1)
    return (so, si, skh, skw) + taps + (shape,)


def pack_path(d, o0):
    """The path pack_kernel takes for the workgroup that starts at row o0: ident / onepass / perrow."""
    so, si, skh, skw, kh_off, kh_mul, kw_off, kw_mul, _ = pack_strides(d)
    d = dict(d)
    taps, I, Ipad, KH, KW = d["KH"] * d["KW"], d["I"], d["Ipad"], d["KH"], d["KW"]
    row = taps * Ipad
    ident = Ipad == I and si == 1 and d.get("dst_ld", 0) == 0 and (kh_off, kh_mul, kw_off, kw_mul) == (0, 1, 0, 1) and \
        (KW == 1 or skw == I) and (KH == 1 or skh == KW * I) and so == row and row % 8 == 0 and \
        d.get("src_off", 0) % 16 == 0
    if ident:
        return "ident"
    nrows = min(d["O"], o0 + pack_rows(d.items())) - o0
    return "onepass" if nrows > 1 and nrows * taps * (Ipad + 8) <= PACK_LDS else "perrow"


def pack_paths(descs):
    return [(pack_path(descs[j], o), dict(descs[j])["KH"] * dict(descs[j])["KW"]) for j, o in pack_bmap(descs)]


def tpack_bmap(descs):
    """One (descriptor, first i, first o, tap) per 64 x 64 tile per tap."""
    return [(j, i, o, t) for j, d in enumerate(descs) for i in range(0, dict(d)["I"], 64)
            for o in range(0, dict(d)["O"], 64) for t in range(len(dict(d)["smap"]))]


def pad8(n):
    return cdiv(n, 8) * 8


def status(entry, a):
    """The status an entry point returns before any launch (0: it launches) for the arguments `a` (a dict by the
    names of include/sdmi.h; pointers are 1 (present) / 0 (null))."""
    pos = lambda *ks: all(a[k] > 0 for k in ks)  # noqa: E731
    if entry in (N2C, C2N):
        return 0 if a["src"] and a["dst"] and pos("B", "C", "HW") and a["ld"] >= a["C"] else -1
    if entry == SLICE:
        ok = a["src"] and a["dst"] and pos("P", "C") and a["lds"] >= a["C"] and a["ldd"] >= a["C"]
        return 0 if ok and not (a["C"] % 8 or a["lds"] % 8 or a["ldd"] % 8) else -1
    if entry == RELU:
        return 0 if a["x"] and a["y"] and a["n"] >= 0 else -1
    if entry == SILU:
        return 0 if a["x"] and a["y"] and a["n"] > 0 else -1
    if entry == MSE:
        return 0 if a["pred"] and a["target"] and a["ws"] and a["loss"] and pos("B", "C", "HW") and a["ld"] >= a["C"] else -1
    if entry == TEMB:
        ok = a["t"] and a["out"] and pos("B", "dim") and a["dim"] % 2 == 0 and a["ld"] >= a["dim"] and a["tstride"] >= 0
        return 0 if ok else -1
    if entry == PREP:
        if not (a["x"] and a["out"] and pos("B", "cx", "H", "W", "cpad")):
            return -1
        if a["mask"] and not (a["wcond"] and pos("MH", "MW", "cmo") and (a["cmap"] or a["cmi"] > 0)):
            return -1
        if a["cpad"] % 8 or a["cx"] + (a["cmo"] if a["mask"] else 0) > a["cpad"] or a["cpad"] > 16:
            return -1
        return -1 if a["cmap"] and not 1 <= a["cmi"] <= 255 else 0
    if entry == CW:
        ok = a["dxin"] and a["mask"] and a["dw"] and pos("B", "H", "W", "MH", "MW") and a["cx"] >= 0 and \
            a["ld"] >= a["cx"] + a["cmo"]
        return 0 if ok and 1 <= a["cmo"] <= 16 and 1 <= a["cmi"] <= 255 else -1
    if entry == RESIZE:
        return 0 if a["in"] and a["out"] and pos("BC", "IH", "IW", "OH", "OW") else -1
    if entry == CHAN:
        ok = a["src"] and a["dst"] and pos("B", "C", "P") and a["src_c0"] >= 0 and a["dst_c0"] >= 0 and \
            a["src_c0"] + a["C"] <= a["src_c"] and a["dst_c0"] + a["C"] <= a["dst_c"]
        return 0 if ok else -1
    if entry == MODF:
        return 0 if a["x"] and a["s"] and a["y"] and pos("B", "N", "C") and a["ls"] >= a["C"] else -1
    if entry == MODB:
        return 0 if a["x"] and a["dy"] and a["s"] and pos("B", "N", "C") and a["ls"] >= a["C"] else -1
    assert entry == AMAP
    ok = a["q"] and a["k"] and a["out"] and pos("B", "H", "N", "S", "d") and a["S"] <= AMAP_SMAX and \
        a["ldq"] >= a["H"] * a["d"] and a["ldk"] >= a["H"] * a["d"] and a["N"] <= 65535 * 32
    return 0 if ok else -1


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS). CW: the launches of the
    one-hot form, then (exact family) those of the class-map form."""
    o = dict(options)
    if entry == N2C:
        B, C, HW, ld = dims
        return [(K_N2C, grid_for(B * C * HW))]
    if entry == C2N:
        B, C, HW, ld = dims
        return [(K_C2N, grid_for(B * HW * ld))]
    if entry == SLICE:
        P, C, lds, ldd = dims
        return [(K_SLICE, grid_for(P * C // 8))]
    if entry == RELU:
        return [(K_RELU, grid_for(dims[0]))]
    if entry == SILU:
        return [(K_SILU, grid_for(dims[0]))]
    if entry == RESIZE:
        BC, IH, IW, OH, OW = dims
        return [(K_RESIZE, grid_of(BC * OH * OW))]
    if entry == CHAN:
        B, C, P = dims[:3]
        return [(K_CHAN, grid_of(B * C * P))]
    if entry == PACK:
        return [(K_PACK, len(pack_bmap(o["descs"])))]
    if entry == TPACK:
        return [(K_TPACK, len(tpack_bmap(o["descs"])))]
    if entry == PREP:
        B, cx, H, W, cpad = dims
        return [(K_PREP1 if o.get("mask") == "cmap" else K_PREP0, prep_grid(B * H * W))]
    if entry == CW:
        B, H, W, cmo, cmi = dims
        one = lambda k: [(k, cmo * cmi * CW_SPLITS), (K_CWF, cdiv(cmo * cmi, NT))]  # noqa: E731
        return one(K_CW0) + (one(K_CW1) if o.get("family", "exact") == "exact" else [])
    if entry == MSE:
        B, C, HW, ld = dims
        return [(K_MSEK, mse_blocks(B * HW * ld)), (K_SUMP, 1)]
    if entry == TEMB:
        B, dim, ld = dims
        return [(K_TEMB, grid_for(B * dim // 2))]
    if entry == MODF:
        B, N, C = dims
        return [(K_MODF, grid_of(B * N * C))]
    if entry == MODB:
        B, N, C = dims
        return [(K_MODB, cdiv(C, 64) * B)]
    assert entry == AMAP
    B, H, N, S, d = dims
    return [(K_AMAP, N * B)]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
CAPPED = 8192 * 256 + 257          # = 17 * 123377: one row past one trip of the capped grid of misc.hip
ROWS = [
    # bf16 and fp32 sources, ld > C and ld = C = 8, HW = 1 (the class / text use), the capped grid
    R(N2C, (2, 3, 35, 8), (K_N2C, 1), f32=1), R(N2C, (2, 3, 35, 8), (K_N2C, 1), f32=0),
    R(N2C, (3, 8, 11, 8), (K_N2C, 2), f32=1), R(N2C, (3, 8, 11, 8), (K_N2C, 2), f32=0),
    R(N2C, (300, 5, 1, 16), (K_N2C, 6), f32=0), R(N2C, (1, 17, 123377, 24), (K_N2C, 8192), f32=0),
    # C < ld (pad columns written +0), C = ld, HW = 1 with many rows, the capped grid
    R(C2N, (2, 3, 35, 8), (K_C2N, 3)), R(C2N, (3, 8, 11, 8), (K_C2N, 2)), R(C2N, (300, 5, 1, 16), (K_C2N, 19)),
    R(C2N, (1, 17, 87392, 24), (K_C2N, 8192)),
    # plain / accumulate; lds != ldd; C < min(lds, ldd); P = 1; the capped grid
    R(SLICE, (37, 16, 16, 16), (K_SLICE, 1), acc=0), R(SLICE, (37, 16, 16, 16), (K_SLICE, 1), acc=1),
    R(SLICE, (37, 8, 24, 40), (K_SLICE, 1), acc=0), R(SLICE, (37, 8, 24, 40), (K_SLICE, 1), acc=1),
    R(SLICE, (1, 8, 8, 16), (K_SLICE, 1), acc=1), R(SLICE, (131087, 128, 136, 128), (K_SLICE, 8192), acc=1),
    R(SLICE, (131087, 128, 128, 136), (K_SLICE, 8192), acc=0),
]
ROWS += [R(RELU, (n,), (K_RELU, g), bwd=b) for n, g in ((1, 1), (255, 1), (256, 1), (257, 2), (CAPPED, 8192))
         for b in (0, 1)]
ROWS += [
    # non-integer ratios down and up in each axis, identity, one plane
    R(RESIZE, (6, 7, 9, 5, 20), (K_RESIZE, 3)), R(RESIZE, (6, 7, 9, 10, 4), (K_RESIZE, 1)),
    R(RESIZE, (6, 48, 40, 32, 32), (K_RESIZE, 24)), R(RESIZE, (5, 7, 9, 7, 9), (K_RESIZE, 2)),
    R(RESIZE, (1, 3, 5, 7, 2), (K_RESIZE, 1)),
    # (B, C, P, src_c, src_c0, dst_c, dst_c0): whole tensors, into the middle of a wider one, out of the middle
    R(CHAN, (3, 4, 35, 4, 0, 4, 0), (K_CHAN, 2)), R(CHAN, (3, 4, 35, 4, 0, 11, 5), (K_CHAN, 2)),
    R(CHAN, (3, 4, 35, 11, 5, 4, 0), (K_CHAN, 2)), R(CHAN, (1, 1, 1, 3, 1, 3, 1), (K_CHAN, 1)),
]
_LIN = spec(O=57, I=72, Ipad=72, KH=1, KW=1, layout="nat")
_C33 = dict(I=4, Ipad=8, KH=3, KW=3, layout="conv")
ROWS += [
    # the identity fast path (56 rows and a one-row tail) and the same descriptor off a 16-byte source boundary
    R(PACK, (), (K_PACK, 2), descs=(_LIN,)), R(PACK, (), (K_PACK, 2), descs=(spec(src_off=4, **dict(_LIN)),)),
    # one pass: channel-slow; channel-fast with a partly and with a wholly padded group of 8
    R(PACK, (), (K_PACK, 1), descs=(spec(O=10, **_C33),)),
    R(PACK, (), (K_PACK, 1), descs=(spec(O=5, I=12, Ipad=16, KH=3, KW=3, layout="nat"),)),
    R(PACK, (), (K_PACK, 1), descs=(spec(O=5, I=4, Ipad=16, KH=3, KW=3, layout="nat"),)),
    # the per-row path at each arm of the tap switch
    R(PACK, (), (K_PACK, 3), descs=(spec(O=3, I=2304, Ipad=2304, KH=1, KW=1, layout="nat", src_off=4),)),
    R(PACK, (), (K_PACK, 3), descs=(spec(O=3, I=513, Ipad=520, KH=2, KW=2, layout="conv"),)),
    R(PACK, (), (K_PACK, 3), descs=(spec(O=3, I=250, Ipad=256, KH=3, KW=3, layout="conv"),)),
    R(PACK, (), (K_PACK, 3), descs=(spec(O=3, I=130, Ipad=136, KH=4, KW=4, layout="conv"),)),
    R(PACK, (), (K_PACK, 3), descs=(spec(O=3, I=685, Ipad=688, KH=1, KW=3, layout="conv"),)),
    # the documented LDS limit exactly: 16 * (1016 + 8) = 16384
    R(PACK, (), (K_PACK, 2), descs=(spec(O=2, I=1010, Ipad=1016, KH=4, KW=4, layout="conv"),)),
    # a one-row tail workgroup after two full ones: O = 56 * 2 + 1
    R(PACK, (), (K_PACK, 3), descs=(spec(O=113, **_C33),)),
    # a spatial flip, a sub-pixel phase (2 x 2 taps of a 4 x 4 source), a column slice of a wider matrix
    R(PACK, (), (K_PACK, 1), descs=(spec(O=10, flip=1, **_C33),)),
    R(PACK, (), (K_PACK, 1), descs=(spec(O=6, I=8, Ipad=8, KH=2, KW=2, SKH=4, SKW=4, phase=(1, 0), layout="conv"),)),
    R(PACK, (), (K_PACK, 1), descs=(spec(O=10, dst_ld=136, col0=16, **_C33),)),
    # two descriptors in one launch
    R(PACK, (), (K_PACK, 4), descs=(_LIN, spec(O=10, flip=1, **_C33), spec(O=1, I=8, Ipad=8, KH=1, KW=1, layout="nat"))),
]
_REV9 = tuple(range(8, -1, -1))
ROWS += [
    # one full tile; edge tiles in both directions; 9 taps reversed; 4 of 16; wider dst_ld and dst_tap; two descriptors
    R(TPACK, (), (K_TPACK, 1), descs=(spec(O=64, I=64, smap=(0,), staps=1),)),
    R(TPACK, (), (K_TPACK, 2), descs=(spec(O=40, I=72, smap=(0,), staps=1),)),
    R(TPACK, (), (K_TPACK, 9), descs=(spec(O=16, I=24, smap=_REV9, staps=9),)),
    R(TPACK, (), (K_TPACK, 4), descs=(spec(O=8, I=16, smap=(5, 7, 13, 15), staps=16),)),
    R(TPACK, (), (K_TPACK, 8), descs=(spec(O=72, I=40, smap=(3, 2, 1, 0), staps=4, dst_tap=80, dst_pad=24),)),
    R(TPACK, (), (K_TPACK, 11), descs=(spec(O=40, I=72, smap=(0,), staps=1), spec(O=16, I=24, smap=_REV9, staps=9))),
]
_SOFT = dict(mask="soft", cmi=3, cmo=4)
ROWS += [
    # (B, cx, H, W, cpad). No mask; 1, 63, 64, 65 pixels with cx + cmo = cpad = 8
    R(PREP, (2, 3, 5, 7, 8), (K_PREP0, 2)),
    R(PREP, (1, 4, 1, 1, 8), (K_PREP0, 1), **_SOFT), R(PREP, (1, 4, 7, 9, 8), (K_PREP0, 1), **_SOFT),
    R(PREP, (1, 4, 8, 8, 8), (K_PREP0, 1), **_SOFT), R(PREP, (1, 4, 5, 13, 8), (K_PREP0, 2), **_SOFT),
    # non-integer mask ratios up and down; cx + cmo = cpad = 16 with keep; cx + cmo < cpad without
    R(PREP, (2, 4, 10, 3, 16), (K_PREP0, 1), mask="soft", cmi=18, cmo=12, MH=7, MW=5, keep=1),
    R(PREP, (3, 3, 32, 32, 8), (K_PREP0, 48), mask="soft", cmi=5, cmo=2, MH=48, MW=40),
    # the class map: classes 0, 1, cmi and above cmi, with and without keep, both ratios
    R(PREP, (2, 4, 10, 3, 8), (K_PREP1, 1), mask="cmap", cmi=18, cmo=4, MH=7, MW=5, keep=1),
    R(PREP, (2, 4, 10, 3, 8), (K_PREP1, 1), mask="cmap", cmi=18, cmo=4, MH=7, MW=5),
    R(PREP, (3, 3, 32, 32, 16), (K_PREP1, 48), mask="cmap", cmi=5, cmo=12, MH=48, MW=40, keep=1),
    # one row past 65536 * 64 pixels
    R(PREP, (1, 1, 2048, 2049, 8), (K_PREP0, 65536)),
]


def _cw(cmo, cmi, both=True):
    one = lambda k: ((k, cmo * cmi * 32), (K_CWF, 1 if cmo * cmi <= 256 else 2))  # noqa: E731
    return one(K_CW0) + (one(K_CW1) if both else ())


for _fam in ("exact", "soft"):
    _b = _fam == "exact"
    ROWS += [
        # (B, H, W, cmo, cmi). 5 pixels (27 empty splits), 32, 33, a split's chunk of 260, one (o, i), 16 x 18, cmi = 255
        R(CW, (1, 1, 5, 2, 3), *_cw(2, 3, _b), family=_fam), R(CW, (1, 4, 8, 2, 3), *_cw(2, 3, _b), family=_fam),
        R(CW, (1, 3, 11, 2, 3), *_cw(2, 3, _b), family=_fam, keep=1),
        R(CW, (2, 64, 65, 2, 3), *_cw(2, 3, _b), family=_fam, MH=48, MW=40, keep=1),
        R(CW, (2, 8, 8, 1, 1), *_cw(1, 1, _b), family=_fam), R(CW, (2, 16, 16, 16, 18), *_cw(16, 18, _b), family=_fam, keep=1),
        R(CW, (1, 8, 8, 1, 255), *_cw(1, 255, _b), family=_fam),
    ]
ROWS += [
    # (B, C, HW, ld). A total of 1, 256, 257; ld = 8 with C of 3, 4, 8; gscale by value / from the device; no gradient
    R(MSE, (1, 1, 1, 1), (K_MSEK, 1), (K_SUMP, 1)), R(MSE, (1, 1, 256, 1), (K_MSEK, 1), (K_SUMP, 1)),
    R(MSE, (1, 1, 257, 1), (K_MSEK, 2), (K_SUMP, 1)), R(MSE, (2, 3, 33, 8), (K_MSEK, 3), (K_SUMP, 1)),
    R(MSE, (2, 4, 32, 8), (K_MSEK, 2), (K_SUMP, 1), gdev=1), R(MSE, (2, 8, 32, 8), (K_MSEK, 2), (K_SUMP, 1)),
    R(MSE, (2, 3, 33, 8), (K_MSEK, 3), (K_SUMP, 1), gdev=1), R(MSE, (2, 3, 33, 8), (K_MSEK, 3), (K_SUMP, 1), grad=0),
    # above 1024 * 256 items: the capped grid and the whole workspace; ragged (8 items) and two whole trips (exact)
    R(MSE, (1, 3, 32769, 8), (K_MSEK, 1024), (K_SUMP, 1)), R(MSE, (1, 4, 65536, 8), (K_MSEK, 1024), (K_SUMP, 1)),
]
T3, T5, TGOLD = (0, 1, 999), (0, 1, 999, 500, 37), "golden"
ROWS += [
    # (B, dim, ld)
    R(TEMB, (3, 2, 2), (K_TEMB, 1), t=T3), R(TEMB, (3, 6, 6), (K_TEMB, 1), t=T3),
    R(TEMB, (8, 128, 128), (K_TEMB, 2), t=TGOLD), R(TEMB, (8, 512, 512), (K_TEMB, 8), t=TGOLD),
    R(TEMB, (5, 128, 136), (K_TEMB, 2), t=T5), R(TEMB, (5, 6, 6), (K_TEMB, 1), t=T3, tstride=0),
    R(TEMB, (1, 128, 128), (K_TEMB, 1), t=T3, tstride=0), R(TEMB, (3, 128, 128), (K_TEMB, 1), t=T3, f32=0),
]
ROWS += [R(SILU, (65536,), (K_SILU, 256), bwd=0)] + [R(SILU, (65536,), (K_SILU, 256), bwd=1, dy=k) for k in range(4)]
# (B, N, C): every combination of r, t, alpha and the row stride of s and t
ROWS += [R(MODF, (2, 5, 72), (K_MODF, 3), r=r, t=t, alpha=a, ls6=l) for r in (0, 1) for t in (0, 1) for a in (0, 1)
         for l in (0, 1)]
ROWS += [R(MODF, (3, 37, 65), (K_MODF, 29), r=1, t=1, alpha=1, ls6=1)]
ROWS += [R(MODB, (2, n, 72), (K_MODB, 4)) for n in (1, 3, 4, 5, 37)]
ROWS += [R(MODB, (2, 5, c), (K_MODB, 2 * g), ls6=1) for c, g in ((1, 1), (63, 1), (64, 1), (65, 2))]
ROWS += [R(MODB, (2, 5, 72), (K_MODB, 4), null=k) for k in ("dx", "ds", "dt")]
ROWS += [
    # (B, H, N, S, d)
    R(AMAP, (2, 3, 2, 1, 8), (K_AMAP, 4), avg=1), R(AMAP, (2, 3, 3, 77, 8), (K_AMAP, 6), avg=1),
    R(AMAP, (1, 2, 2, 255, 8), (K_AMAP, 2), avg=0), R(AMAP, (1, 2, 2, 256, 8), (K_AMAP, 2), avg=0),
    R(AMAP, (1, 2, 2, 257, 8), (K_AMAP, 2), avg=1), R(AMAP, (1, 2, 2, 4096, 8), (K_AMAP, 2), avg=0),
    R(AMAP, (1, 2, 1, 4096, 8), (K_AMAP, 1), avg=1),
    R(AMAP, (2, 1, 3, 77, 8), (K_AMAP, 6), avg=1), R(AMAP, (2, 3, 3, 77, 1), (K_AMAP, 6), avg=0),
    R(AMAP, (2, 3, 3, 77, 8), (K_AMAP, 6), avg=0, wide=1), R(AMAP, (2, 3, 3, 77, 8), (K_AMAP, 6), avg=0, big=1),
    R(AMAP, (2, 3, 3, 77, 8), (K_AMAP, 6), avg=1, big=1),
]


def _s(v):
    if isinstance(v, tuple):
        return "(" + ",".join(_s(x) for x in v) + ")"
    return str(v).replace("'", "")


def row_id(r):
    o = "".join(f"-{k}{_s(v)}" for k, v in r.opt)
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + o


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


# ----------------------------------------------------------------------------------------------------------------
# value families
# ----------------------------------------------------------------------------------------------------------------
DENORMALS = (2.0 ** -149, -(2.0 ** -140), 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -127, -(2.0 ** -133 + 2.0 ** -142))
SPECIALS = CAST_SPECIALS + DENORMALS


def movement_values(n, *key):
    """n fp32 values: 24-bit integers times 2^-20, with SPECIALS planted at i % 5 == 0 (bf16 ties on both sides, a
    value that rounds up into the next binade, +-0, +-inf, the largest finite value, NaN, fp32 and bf16 denormals)."""
    x = torch.randint(-2 ** 23, 2 ** 23, (n,), generator=_gen(31, n, *key)).double() * 2.0 ** -20
    i = torch.arange(n)
    sel = i % 5 == 0
    x[sel] = torch.tensor(SPECIALS, dtype=torch.float64)[(i[sel] // 5 + (sum(key) if key else 0)) % len(SPECIALS)]
    return x.float()


def eq_bits(a, b):
    """Tensors of one dtype (fp32 / bf16) equal bit for bit, a NaN matching any NaN."""
    return same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1))


def n_diff(a, b):
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((na != nb) | (~na & ~nb & (bits(a) != bits(b)))).sum())


def ulp_bf16(x):
    """The bf16 unit in the last place at |x| (float64 tensor), denormals included."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def worst(got, ref, lim):
    """max(err / bound) over float64 tensors; a NaN must meet a NaN, an inf the same inf; an error where the bound is
    zero counts as infinite."""
    got, ref, lim = got.double().reshape(-1), ref.double().reshape(-1), lim.double().reshape(-1)
    special = ~torch.isfinite(ref)
    ok_special = (torch.isnan(ref) & torch.isnan(got)) | (torch.isinf(ref) & (got == ref))
    if bool((special & ~ok_special).any()) or bool((~special & ~torch.isfinite(got)).any()):
        return INF
    err = (got - ref).abs()[~special]
    lim = lim[~special]
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / lim.clamp_min(1e-300))
    r = torch.where((lim <= 0) & (err > 0), torch.full_like(err, INF), r)
    return float(r.max())


def excess(got, ref, half, fine):
    """max((err - half) / fine) over the finite references: the share of the fp32 part K u T of a bf16 statement that is
    in use once the half ulp of the output rounding is taken off (negative: the half ulp alone covers every error)."""
    got, ref, half, fine = (t.double().reshape(-1) for t in (got, ref, half, fine))
    ok = torch.isfinite(ref) & torch.isfinite(got) & (fine > 0)
    return float((((got - ref).abs() - half) / fine.clamp_min(1e-300))[ok].max()) if bool(ok.any()) else 0.0


# ----------------------------------------------------------------------------------------------------------------
# layout converters, slice copy, ReLU, resize, channel copy: index models
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def n2c_case(r):
    """src [B * HW][ld] (fp32, or its bf16 image) and the (B, C, HW) fp32 result."""
    B, C, HW, ld = r.dims
    src = movement_values(B * HW * ld, 1).view(B * HW, ld)
    if not opt(r, "f32"):
        src = src.bfloat16()
    return src, src.view(B, HW, ld)[:, :, :C].permute(0, 2, 1).float().contiguous()


@functools.lru_cache(maxsize=2)
def c2n_case(r):
    """src (B, C, HW) fp32 and the [B * HW][ld] bf16 result, pad columns +0."""
    B, C, HW, ld = r.dims
    src = movement_values(B * C * HW, 2).view(B, C, HW)
    out = torch.zeros(B, HW, ld, dtype=torch.bfloat16)
    out[:, :, :C] = src.permute(0, 2, 1).bfloat16()
    return src, out.view(B * HW, ld)


SUM_PAIRS = ((1.0, 2.0 ** -8), (1 + 2.0 ** -7, 2.0 ** -8), (3.3895313892515355e38, 3.3895313892515355e38),
             (-3.3895313892515355e38, -2.0 ** 120), (1.0, -1.0), (-0.0, -0.0), (INF, -INF), (2.0 ** -133, 2.0 ** -133))


@functools.lru_cache(maxsize=2)
def slice_case(r):
    """src [P][lds], dst before [P][ldd] (bf16) and dst after: columns < C copied or accumulated (one fp32 add, RNE),
    the rest untouched. SUM_PAIRS are planted: sums that tie down and up, overflow to inf, cancel, -0 + -0, inf - inf,
    denormals."""
    P, C, lds, ldd = r.dims
    src = movement_values(P * lds, 3).view(P, lds).bfloat16()
    dst = movement_values(P * ldd, 4).view(P, ldd).bfloat16()
    for k, (a, b) in enumerate(SUM_PAIRS):
        if k < C:
            src[0, k], dst[0, k] = a, b
            src[P - 1, C - 1 - k], dst[P - 1, C - 1 - k] = b, a
    after = dst.clone()
    after[:, :C] = (src[:, :C].float() + dst[:, :C].float()).bfloat16() if opt(r, "acc") else src[:, :C]
    return src, dst, after


def relu_model(x, dy=None):
    """y = x <= 0 ? +0 : x (a NaN stays; -0 and every negative give +0); with dy: x <= 0 ? +0 : dy (a NaN x passes
    dy). aten's CPU relu returns -0 for -0, an accident of its vectorised max; that sign is not followed."""
    return torch.where(x <= 0, torch.zeros_like(x), x if dy is None else dy)


def relu_model_old(x, dy=None):
    """The kernel before its fix (v > 0 ? v : 0): a NaN gives 0 in both directions."""
    return torch.where(x > 0, x if dy is None else dy, torch.zeros_like(x))


@functools.lru_cache(maxsize=2)
def relu_case(n):
    x, dy = movement_values(n, 5), movement_values(n, 6)
    if n > 30:
        dy = torch.roll(dy, 7)       # every special of x meets a generic dy and the reverse
    return x, dy


def nearest_index(n_in, n_out, rounding=False):
    """aten's nearest source index: min(floor(dst * (float)in / out), in - 1), in fp32. rounding: a perturbed one."""
    scale = f32(n_in) / f32(n_out)
    v = np.arange(n_out, dtype=f32) * scale
    v = np.rint(v) if rounding else np.floor(v)
    return torch.from_numpy(np.minimum(v.astype(np.int64), n_in - 1))


def nearest_index_torch(n_in, n_out):
    """The same index read off F.interpolate (mode 'nearest') on the CPU."""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1)).view(-1).long()


def resize_model(x, OH, OW, rounding=False):
    iy, ix = nearest_index(x.shape[-2], OH, rounding), nearest_index(x.shape[-1], OW, rounding)
    return x[..., iy, :][..., ix].contiguous()


@functools.lru_cache(maxsize=2)
def resize_case(r):
    BC, IH, IW, OH, OW = r.dims
    x = movement_values(BC * IH * IW, 7).view(BC, IH, IW)
    return x, resize_model(x, OH, OW)


@functools.lru_cache(maxsize=2)
def chan_case(r):
    """src (B, sC, P), dst before (B, dC, P), dst after."""
    B, C, P, sC, sc0, dC, dc0 = r.dims
    src, dst = movement_values(B * sC * P, 8).view(B, sC, P), movement_values(B * dC * P, 9).view(B, dC, P)
    after = dst.clone()
    after[:, dc0:dc0 + C] = src[:, sc0:sc0 + C]
    return src, dst, after


# ----------------------------------------------------------------------------------------------------------------
# weight packing
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def pack_source(d, j=0):
    shape = pack_strides(d)[-1]
    n = int(np.prod(shape))
    return movement_values(n, 10 + j).view(shape)


def pack_model(d, src, drop_last_row=False, no_flip=False, pad_garbage=False):
    """dst [O][KH * KW * Ipad] bf16 of a descriptor spec, by numpy-style indexing. The keywords are perturbed models."""
    _, _, _, _, kh_off, kh_mul, kw_off, kw_mul, _ = pack_strides(d)
    d = dict(d)
    O, I, Ipad, KH, KW = d["O"], d["I"], d["Ipad"], d["KH"], d["KW"]
    w = src if d["layout"] == "conv" else src.permute(0, 3, 1, 2)          # [O][I][SKH][SKW]
    if no_flip:
        kh_off, kh_mul, kw_off, kw_mul = 0, 1, 0, 1
    khs, kws = kh_off + kh_mul * torch.arange(KH), kw_off + kw_mul * torch.arange(KW)
    sel = w[:, :, khs][:, :, :, kws].permute(0, 2, 3, 1)                   # [O][KH][KW][I]
    out = torch.zeros(O, KH, KW, Ipad, dtype=torch.bfloat16)
    if pad_garbage:
        out += 1
    out[..., :I] = sel.bfloat16()
    out = out.reshape(O, KH * KW * Ipad)
    if drop_last_row:
        j, o0 = pack_bmap((tuple(d.items()),))[-1]
        out[min(O, o0 + pack_rows(d.items())) - 1] = 0
    return out


def tpack_dims(d):
    """(src_ld, src_tap, dst_ld, dst_tap) of a transpose spec: the source is [O][staps * pad8(I)], the destination
    [I][taps * dst_tap + dst_pad]."""
    d = dict(d)
    src_tap = pad8(d["I"])
    dst_tap = d.get("dst_tap", d["O"])
    return d["staps"] * src_tap, src_tap, len(d["smap"]) * dst_tap + d.get("dst_pad", 0), dst_tap


@functools.lru_cache(maxsize=16)
def tpack_source(d, j=0):
    src_ld = tpack_dims(d)[0]
    return movement_values(dict(d)["O"] * src_ld, 20 + j).view(dict(d)["O"], src_ld).bfloat16()


def tpack_model(d, src, identity_smap=False):
    """[I][taps][O] bf16: dst[i][t][o] = src[o][smap[t]][i]."""
    dd = dict(d)
    O, I = dd["O"], dd["I"]
    _, src_tap, _, _ = tpack_dims(d)
    smap = list(range(len(dd["smap"]))) if identity_smap else list(dd["smap"])
    v = src.view(O, dd["staps"], src_tap)[:, smap, :I]                     # [O][taps][I]
    return v.permute(2, 1, 0).contiguous()


# ----------------------------------------------------------------------------------------------------------------
# input staging and the conditioning weight gradient
# ----------------------------------------------------------------------------------------------------------------
def _mask_dims(r):
    if r.entry == PREP:
        B, cx, H, W, cpad = r.dims
    else:
        B, H, W = r.dims[:3]
    return B, H, W, opt(r, "MH", H), opt(r, "MW", W)


def keep_of(r, B):
    """keep[b] in {0, 1}, both present from B = 2 on (B = 1: 1)."""
    return torch.tensor([float((b + 1) % 2) for b in range(B)]) if opt(r, "keep") else None


@functools.lru_cache(maxsize=2)
def prep_case(r):
    """x (B, cx, H, W), mask ((B, cmi, MH, MW) fp32 in [0, 1], or (B, MH, MW) uint8 with classes 0, 1, cmi, cmi + 1 and
    255 among them), w (cmo, cmi), keep."""
    B, cx, H, W, cpad = r.dims
    _, _, _, MH, MW = _mask_dims(r)
    g = _gen(40, B, H, W, cx)
    x = movement_values(B * cx * H * W, 11).view(B, cx, H, W)
    kind, cmi, cmo = opt(r, "mask"), opt(r, "cmi", 0), opt(r, "cmo", 0)
    mask = w = None
    if kind == "soft":
        mask = torch.rand(B, cmi, MH, MW, generator=g)
        w = torch.randn(cmo, cmi, generator=g)
    elif kind == "cmap":
        mask = torch.randint(0, cmi + 2, (B, MH, MW), generator=g).to(torch.uint8)
        flat = mask.view(-1)
        flat[:5] = torch.tensor([0, 1, cmi, cmi + 1, 255], dtype=torch.uint8)
        w = torch.randn(cmo, cmi, generator=g)
        w[0, 0] = -abs(w[0, 0])          # a negative weight times keep = 0 is -0
    return dict(x=x, mask=mask, w=w, keep=keep_of(r, B))


def resized(mask, H, W, rounding=False):
    iy, ix = nearest_index(mask.shape[-2], H, rounding), nearest_index(mask.shape[-1], W, rounding)
    return mask[..., iy, :][..., ix]


def one_hot(cmap, cmi, clamp=True):
    """The reference's one-hot of a class map (celeb_dataset.py:164-175): clamp(0, cmi), one_hot(cmi + 1), background
    dropped. clamp = False (a perturbed one): classes above cmi select nothing."""
    c = cmap.long()
    c = c.clamp(0, cmi) if clamp else torch.where(c > cmi, torch.zeros_like(c), c)
    return F.one_hot(c, cmi + 1).movedim(-1, 1)[:, 1:].float().contiguous()


def prep_reference(r, c, rounding=False, clamp=True):
    """(exact [B * H * W][cpad] bf16 or None per column, float64 reference, T): columns < cx and >= cx + cmo (and the
    class-map columns) are bitwise in `exact`; the mask columns of the fp32 form are ref / T. Returns a dict."""
    B, cx, H, W, cpad = r.dims
    kind, cmi, cmo = opt(r, "mask"), opt(r, "cmi", 0), opt(r, "cmo", 0)
    exact = torch.zeros(B, H, W, cpad, dtype=torch.bfloat16)
    exact[..., :cx] = c["x"].permute(0, 2, 3, 1).bfloat16()
    out = dict(exact=exact.view(B * H * W, cpad), ref=None, T=None)
    keep = c["keep"] if c["keep"] is not None else torch.ones(B)
    if kind == "cmap":
        m = resized(one_hot(c["mask"], cmi, clamp), H, W)                                # [B][cmi][H][W], one 1 at most
        idx = m.argmax(1)
        val = torch.where(m.sum(1) > 0, c["w"].t()[idx].permute(3, 0, 1, 2), torch.zeros(()))     # [cmo][B][H][W]
        if c["keep"] is not None:
            val = val * keep.view(1, B, 1, 1)
        exact[..., cx:cx + cmo] = val.permute(1, 2, 3, 0).bfloat16()
    elif kind == "soft":
        m = resized(c["mask"], H, W, rounding).double()
        terms = c["w"].double().view(1, cmo, cmi, 1, 1) * m.view(B, 1, cmi, H, W) * keep.double().view(B, 1, 1, 1, 1)
        out["ref"] = terms.sum(2).permute(0, 2, 3, 1).reshape(B * H * W, cmo)
        out["T"] = terms.abs().sum(2).permute(0, 2, 3, 1).reshape(B * H * W, cmo)
    return out


def prep_emulate(r, c, variant):
    """The mask columns in fp32 in the kernel's order (i ascending from 0.f), before the bf16 rounding."""
    B, cx, H, W, cpad = r.dims
    cmi, cmo = opt(r, "cmi"), opt(r, "cmo")
    m = resized(c["mask"], H, W)
    acc = torch.zeros(B, cmo, H, W)
    for i in range(cmi):
        wi, mi = c["w"][:, i].view(1, cmo, 1, 1), m[:, i].view(B, 1, H, W)
        acc = fma32(wi.expand_as(acc), mi.expand_as(acc), acc) if variant == "fused" else acc + wi * mi
    if c["keep"] is not None:
        acc = acc * c["keep"].view(B, 1, 1, 1)
    return acc.permute(0, 2, 3, 1).reshape(B * H * W, cmo).double()


def prep_bound(ref, T, K=None):
    return 0.5 * ulp_bf16(ref) + (K_PREP if K is None else K) * U24 * T


CW_LD, CW_CX = 24, 3


@functools.lru_cache(maxsize=2)
def cw_case(r, seed=0):
    """dxin [B * H * W][ld] bf16 (ld = 24, cx = 3: the gradient columns sit in the middle), the class map / fp32 mask,
    keep. exact: integers in [-8, 8] against a one-hot mask; soft: randn against a mask in [0, 1]."""
    B, H, W, cmo, cmi = r.dims
    _, _, _, MH, MW = _mask_dims(r)
    g = _gen(50, B, H, W, cmo, cmi, seed)
    exact = opt(r, "family") == "exact"
    P = B * H * W
    dx = movement_values(P * CW_LD, 12).view(P, CW_LD).bfloat16()
    if exact:
        dx[:, CW_CX:CW_CX + cmo] = torch.randint(-8, 9, (P, cmo), generator=g).bfloat16()
        cmap = torch.randint(0, cmi + 2, (B, MH, MW), generator=g).to(torch.uint8)
        mask = one_hot(cmap, cmi)
    else:
        dx[:, CW_CX:CW_CX + cmo] = torch.randn(P, cmo, generator=g).bfloat16()
        cmap, mask = None, torch.rand(B, cmi, MH, MW, generator=g)
    return dict(dx=dx, cmap=cmap, mask=mask, keep=keep_of(r, B))


def cw_terms(r, c, rounding=False):
    """[cmo * cmi][B * H * W] float64 terms dxin[p][cx + o] * mask_resized[b][i][p] * keep[b]."""
    B, H, W, cmo, cmi = r.dims
    m = resized(c["mask"], H, W, rounding).double()
    if c["keep"] is not None:
        m = m * c["keep"].double().view(B, 1, 1, 1)
    m = m.permute(1, 0, 2, 3).reshape(cmi, B * H * W)
    d = c["dx"][:, CW_CX:CW_CX + cmo].double().t()                         # [cmo][P]
    return (d.view(cmo, 1, -1) * m.view(1, cmi, -1)).reshape(cmo * cmi, -1)


def cw_reference(r, c, weights=None, rounding=False):
    """(dw [cmo * cmi] float64, T). weights [P]: counts pixels (0: dropped), a perturbed reference."""
    t = cw_terms(r, c, rounding)
    tw = t if weights is None else t * weights
    return tw.sum(1), t.abs().sum(1)


def cw_split(total):
    """(chunk, [(p0, p1)] per split): the pixel ranges of the 32 splits."""
    chunk = cdiv(total, CW_SPLITS)
    return chunk, [(min(total, z * chunk), min(total, (z + 1) * chunk)) for z in range(CW_SPLITS)]


def cw_emulate(r, c, variant, drop=None):
    """dw in fp32 in the kernels' order: per thread its pixels p0 + tid, + 256, .., the 64-lane butterfly, the four waves
    in order, the 32 splits in order. drop: ('pixel', p) / ('lane', l) / ('wave', w) / ('split', z) leaves that out."""
    B, H, W, cmo, cmi = r.dims
    total = B * H * W
    m = resized(c["mask"], H, W)
    if c["keep"] is not None:
        m = m * c["keep"].view(B, 1, 1, 1)                                 # fl(mv * keep): exact for keep in {0, 1}
    m = m.permute(1, 0, 2, 3).reshape(1, cmi, total).expand(cmo, cmi, total).reshape(cmo * cmi, total)
    d = c["dx"][:, CW_CX:CW_CX + cmo].float().t().reshape(cmo, 1, total).expand(cmo, cmi, total).reshape(cmo * cmi, total)
    if drop is not None and drop[0] == "pixel":
        d = d.clone()
        d[:, drop[1]] = 0.0
    chunk, ranges = cw_split(total)
    steps = max(1, cdiv(chunk, NT))
    dd, mm = torch.zeros(cmo * cmi, CW_SPLITS, steps * NT), torch.zeros(cmo * cmi, CW_SPLITS, steps * NT)
    for z, (p0, p1) in enumerate(ranges):
        dd[:, z, :p1 - p0], mm[:, z, :p1 - p0] = d[:, p0:p1], m[:, p0:p1]
    dd, mm = dd.view(-1, CW_SPLITS, steps, NT), mm.view(-1, CW_SPLITS, steps, NT)
    acc = torch.zeros(cmo * cmi, CW_SPLITS, NT)
    for s in range(steps):
        acc = fma32(dd[:, :, s], mm[:, :, s], acc) if variant == "fused" else acc + dd[:, :, s] * mm[:, :, s]
    if drop is not None and drop[0] == "lane":
        acc[:, :, drop[1]] = 0.0
    waves = butterfly32(acc.view(-1, CW_SPLITS, NT // 64, 64))
    if drop is not None and drop[0] == "wave":
        waves[:, :, drop[1]] = 0.0
    parts = seq32(waves, 2)
    if drop is not None and drop[0] == "split":
        parts[:, drop[1]] = 0.0
    return seq32(parts, 1).double()


# ----------------------------------------------------------------------------------------------------------------
# MSE
# ----------------------------------------------------------------------------------------------------------------
MSE_GSCALE = {"exact": 0.5, "soft": 1000.0 / 3}


@functools.lru_cache(maxsize=2)
def mse_case(r, family):
    """pred [B * HW][ld] fp32 (pad columns hold the movement family: they must not be read into the loss), target
    (B, C, HW). exact: pred - target small integers; soft: randn."""
    B, C, HW, ld = r.dims
    g = _gen(60, B, C, HW, ld, family == "exact")
    pred = movement_values(B * HW * ld, 13).view(B, HW, ld)
    if family == "exact":
        tgt = torch.randint(-4, 5, (B, C, HW), generator=g).float()
        pred[:, :, :C] = tgt.permute(0, 2, 1) + torch.randint(-3, 4, (B, HW, C), generator=g).float()
    else:
        tgt = torch.randn(B, C, HW, generator=g)
        pred[:, :, :C] = torch.randn(B, HW, C, generator=g)
    return dict(pred=pred.view(B * HW, ld), target=tgt, gscale=float(f32(MSE_GSCALE[family])))


def mse_exact(r):
    """n = B * C * HW is a power of two: the exact family's loss is then exact in any order."""
    n = r.dims[0] * r.dims[1] * r.dims[2]
    return n & (n - 1) == 0


def mse_reference(r, c, n_pad=False, weights=None):
    """float64 loss on the stored fp32 inputs. n_pad (a perturbed one): n counts the pad columns."""
    B, C, HW, ld = r.dims
    d = c["pred"].view(B, HW, ld)[:, :, :C].double() - c["target"].permute(0, 2, 1).double()
    n = B * HW * (ld if n_pad else C)
    sq = d * d if weights is None else d * d * weights
    return float(sq.sum() / n)


def mse_grad_model(r, c, n_pad=False):
    """[B * HW][ld] bf16: bf16(2 * d / n * gscale) in numpy.float32 (d one rounded subtraction, the product by 2 exact,
    a correctly rounded division, one rounded product), pad columns +0."""
    B, C, HW, ld = r.dims
    p, t = c["pred"].view(B, HW, ld)[:, :, :C].numpy(), c["target"].permute(0, 2, 1).numpy()
    n = f32(B * HW * (ld if n_pad else C))
    with np.errstate(all="ignore"):
        g = f32(2.0) * (p - t) / n * f32(c["gscale"])
    assert g.dtype == f32
    out = torch.zeros(B, HW, ld, dtype=torch.bfloat16)
    out[:, :, :C] = torch.from_numpy(g).bfloat16()
    return out.view(B * HW, ld)


def mse_emulate(r, c, variant, drop=None):
    """The loss in fp32 in the kernels' order: block k's thread j adds items k * 256 + j, + blocks * 256, ..; butterfly;
    waves; then sum_partials: thread j adds partials j, j + 256, ..; butterfly; waves; times fl(1 / n).
    drop: ('item', i) / ('block', k)."""
    B, C, HW, ld = r.dims
    total = B * HW * ld
    blocks = mse_blocks(total)
    d = torch.zeros(B, HW, ld)
    d[:, :, :C] = c["pred"].view(B, HW, ld)[:, :, :C] - c["target"].permute(0, 2, 1)
    d = d.view(-1)
    if drop is not None and drop[0] == "item":
        d = d.clone()
        d[torch.nonzero(d)[drop[1]]] = 0.0
    trips = cdiv(total, blocks * NT)
    dd = torch.zeros(trips * blocks * NT)
    dd[:total] = d
    dd = dd.view(trips, blocks, NT)
    acc = torch.zeros(blocks, NT)
    for s in range(trips):
        acc = fma32(dd[s], dd[s], acc) if variant == "fused" else acc + dd[s] * dd[s]
    parts = seq32(butterfly32(acc.view(blocks, NT // 64, 64)), 1)
    if drop is not None and drop[0] == "block":
        parts[drop[1]] = 0.0
    t2 = cdiv(blocks, NT)
    pp = torch.zeros(t2 * NT)
    pp[:blocks] = parts
    s = seq32(butterfly32(seq32(pp.view(t2, NT), 0).view(NT // 64, 64)), 0)
    scale = torch.tensor(1.0) / torch.tensor(float(B * C * HW))
    return float((s * scale).double())


# ----------------------------------------------------------------------------------------------------------------
# time embedding
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def golden_temb():
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, "time_embedding.safetensors"))


def temb_t(r):
    """The int64 timesteps the call reads (one for tstride = 0)."""
    t = opt(r, "t")
    return golden_temb()["t"].clone() if t == TGOLD else torch.tensor(t, dtype=torch.int64)


def temb_reference(t, dim, swap=False, half_is_dim=False):
    """blocks.py:5-24 in float64: (emb [len(t)][dim], the angle a [len(t)][dim]). The exponent j / half is the fp32
    quotient (the reference forms it in fp32: that is the definition); everything after it is float64."""
    half = dim // 2
    e = (torch.arange(half, dtype=torch.float32) / (dim if half_is_dim else half)).double()
    a = t.double().view(-1, 1) / (10000.0 ** e).view(1, -1)
    s, c = torch.sin(a), torch.cos(a)
    return (torch.cat([c, s], 1) if swap else torch.cat([s, c], 1)), torch.cat([a, a], 1)


def temb_emulate(t, dim):
    """(a32, emb32) as float64: the fp32 angle with powf as the rounded float64 power and a correctly rounded division,
    sinf / cosf as the rounded float64 function of that fp32 angle."""
    half = dim // 2
    e = (torch.arange(half, dtype=torch.float32) / half).double()
    f = (10000.0 ** e).float()
    a = (t.float().view(-1, 1) / f.view(1, -1))
    ad = a.double()
    return torch.cat([ad, ad], 1), torch.cat([torch.sin(ad).float(), torch.cos(ad).float()], 1).double()


def temb_bound(a, KA=None, KSC=None):
    return U24 * ((K_TA if KA is None else KA) * a.abs() + (K_TS if KSC is None else KSC))


# ----------------------------------------------------------------------------------------------------------------
# SiLU: every bf16 bit pattern
# ----------------------------------------------------------------------------------------------------------------
SILU_DY = (1.0, -1.5, 1.9921875, 2.0 ** 100)            # 1.9921875 = 2 - 2^-7: a full bf16 mantissa
SILU_CARVE = -89.0


@functools.lru_cache(maxsize=1)
def silu_x():
    """All 65536 bf16 values in bit order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def silu_reference(x, dy=None):
    """float64 (ref, T). Forward: x sigmoid(x), T = |ref|. Backward: dy s (1 + x (1 - s)), T = |dy| s (1 + |x| (1 - s)).
    -inf gives NaN forward (-inf * 0) and +-inf give NaN backward (inf * 0), as torch's own formulas do."""
    xd = x.double()
    s = torch.sigmoid(xd)
    if dy is None:
        ref = xd * s
        return ref, ref.abs()
    oms = torch.sigmoid(-xd)                                # 1 - s without cancellation
    ref = dy * (s * (1 + xd * oms))
    return ref, abs(dy) * s * (1 + xd.abs() * oms)


def silu_emulate(x, dy=None, variant="separate"):
    """silu_f / silu_grad_f in fp32 before the bf16 rounding: exp2 and the reciprocal as the rounded float64 value."""
    xf = x.float()
    arg = -xf * torch.tensor(1.4426950408889634, dtype=torch.float32)
    E = torch.exp2(arg.double()).float()
    s = (1.0 / (1.0 + E).double()).float()
    if dy is None:
        return (xf * s).double()
    dyf = torch.tensor(dy, dtype=torch.float32)
    if variant == "fused":
        g = s * fma32(xf, 1.0 - s, torch.ones_like(s))
    else:
        g = s * (1.0 + xf * (1.0 - s))
    return (dyf * g).double()


def silu_carved(x):
    """The inputs whose fp32 evaluation overflows 1 + 2^(-x log2 e): x <= -89 (-inf excluded: it gives NaN)."""
    xf = x.float()
    return (xf <= SILU_CARVE) & torch.isfinite(xf)


def silu_bound(ref, T, K):
    return 0.5 * ulp_bf16(ref) + K * U24 * T


# ----------------------------------------------------------------------------------------------------------------
# adaLN modulation
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def mod_case(r, family):
    """x, dy, r (B, N, C), the table (B, ls) holding s at columns [s0, s0 + C) and t at [t0, t0 + C), alpha. exact: small
    integers and powers of two."""
    B, N, C = r.dims
    ls = 6 * C if opt(r, "ls6") else C
    g = _gen(70, B, N, C, family == "exact")
    if family == "exact":
        mk = lambda *s: torch.randint(-4, 5, s, generator=g).float()  # noqa: E731
        x, dy, rr = mk(B, N, C), mk(B, N, C), mk(B, N, C)
        s = 2.0 ** torch.randint(-2, 3, (B, ls), generator=g).float() * (torch.randint(0, 2, (B, ls), generator=g) * 2 - 1)
        t = mk(B, ls)
    else:
        mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        x, dy, rr, s, t = mk(B, N, C), mk(B, N, C), mk(B, N, C), mk(B, ls), mk(B, ls)
    return dict(x=x, dy=dy, r=rr, s=s, t=t, ls=ls, alpha=float(opt(r, "alpha", 1)))


def modf_reference(r, c):
    B, N, C = r.dims
    x, s, t, rr = c["x"].double(), c["s"][:, :C].double().view(B, 1, C), c["t"][:, :C].double().view(B, 1, C), c["r"].double()
    y, T = x * (c["alpha"] + s), x.abs() * (abs(c["alpha"]) + s.abs())
    if opt(r, "t", 1):
        y, T = y + t, T + t.abs()
    if opt(r, "r", 1):
        y, T = y + rr, T + rr.abs()
    return y, T


def modf_emulate(r, c, variant):
    B, N, C = r.dims
    m = torch.tensor(c["alpha"], dtype=torch.float32) + c["s"][:, :C].view(B, 1, C)
    t = c["t"][:, :C].view(B, 1, C).expand(B, N, C)
    if opt(r, "t", 1):
        v = fma32(c["x"], m.expand(B, N, C), t) if variant == "fused" else c["x"] * m + t
    else:
        v = c["x"] * m
    if opt(r, "r", 1):
        v = v + c["r"]
    return v.double()


def modb_reference(r, c, drop_row=None):
    """dx bitwise (fp32), ds / dt float64 with their T. drop_row: a perturbed one without that n."""
    B, N, C = r.dims
    m = torch.tensor(c["alpha"], dtype=torch.float32) + c["s"][:, :C].view(B, 1, C)
    dy, x = c["dy"].double(), c["x"].double()
    if drop_row is not None:
        dy = dy.clone()
        dy[:, drop_row] = 0
    return dict(dx=c["dy"] * m, ds=(dy * x).sum(1), Ts=(dy * x).abs().sum(1), dt=dy.sum(1), Tt=dy.abs().sum(1))


def modb_emulate(r, c, variant):
    """ds / dt in fp32: row lane l adds rows l, l + 4, .. (ds by fmaf), then ((l0 + l1) + l2) + l3."""
    B, N, C = r.dims
    steps = cdiv(N, 4)
    dy, x = torch.zeros(B, steps * 4, C), torch.zeros(B, steps * 4, C)
    dy[:, :N], x[:, :N] = c["dy"], c["x"]
    dy, x = dy.view(B, steps, 4, C), x.view(B, steps, 4, C)
    a_s, a_t = torch.zeros(B, 4, C), torch.zeros(B, 4, C)
    for k in range(steps):
        a_s = fma32(dy[:, k], x[:, k], a_s) if variant == "fused" else a_s + dy[:, k] * x[:, k]
        a_t = a_t + dy[:, k]
    return seq32(a_s, 1).double(), seq32(a_t, 1).double()


# ----------------------------------------------------------------------------------------------------------------
# attention map
# ----------------------------------------------------------------------------------------------------------------
UNDERFLOW = 2.0 ** -126


@functools.lru_cache(maxsize=2)
def amap_case(r, family="soft"):
    """q (B, N, ldq), k (B, S, ldk) fp32 and the scaling. big: scores around +-80. Exact families: `equal` (q = 0: every
    score 0) and `peak` (key n % S scores 200, the rest 0)."""
    B, H, N, S, d = r.dims
    ld = H * d + (8 if opt(r, "wide") else 0)
    g = _gen(80, B, H, N, S, d)
    q, k = movement_values(B * N * ld, 14).view(B, N, ld), movement_values(B * S * (ld + (4 if opt(r, "wide") else 0)), 15)
    k = k.view(B, S, -1)
    scaling = float(f32(d ** -0.5))
    if family == "soft":
        amp = (40.0 / (scaling * d ** 0.5)) ** 0.5 if opt(r, "big") else 1.0     # scores of standard deviation 40
        q[:, :, :H * d] = torch.randn(B, N, H * d, generator=g) * amp
        k[:, :, :H * d] = torch.randn(B, S, H * d, generator=g) * amp
    elif family == "equal":
        q[:, :, :H * d] = 0.0
        k[:, :, :H * d] = torch.randn(B, S, H * d, generator=g)
    else:
        assert family == "peak"
        scaling = 1.0
        q[:, :, :H * d] = 0.0
        k[:, :, :H * d] = 0.0
        q[:, :, 0:H * d:d] = 1.0
        k[:, 0, 0:H * d:d] = 200.0
    return dict(q=q, k=k, scaling=scaling)


def amap_reference(r, c, no_max=False, heads=None):
    """float64 softmax(q k^T scaling): (p per head (B, H, N, S), T per head). no_max and heads are perturbed ones (the
    softmax of fp32-range exponentials without the maximum; the average over `heads` heads)."""
    B, H, N, S, d = r.dims
    q = c["q"][:, :, :H * d].double().view(B, N, H, d).transpose(1, 2)
    k = c["k"][:, :, :H * d].double().view(B, S, H, d).transpose(1, 2)
    prod = q.unsqueeze(3) * k.unsqueeze(2)                                  # [B][H][N][S][d]
    sc = prod.sum(-1) * c["scaling"]
    A = d * prod.abs().sum(-1) * abs(c["scaling"]) + sc.abs()
    M = sc.max(-1, keepdim=True).values
    if no_max:
        e = torch.exp(sc.float().double()).float().double()
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(sc, -1)
    A = A + (sc - M).abs()
    T = p * (1 + A + (p * A).sum(-1, keepdim=True))
    return p, T


def amap_out(r, p, heads=None):
    """The output layout of a per-head quantity: its head average (B, N, S) or itself (B, H, N, S)."""
    if opt(r, "avg"):
        return p.sum(1) / (p.shape[1] if heads is None else heads)
    return p


def amap_bound(T, K=None):
    return (K_A if K is None else K) * U24 * T + UNDERFLOW


def amap_emulate(r, c, variant):
    """The kernel in fp32: fmaf dot products (e ascending), times scaling, the maximum, expf as the rounded float64
    function, thread tid adds keys tid, tid + 256, .., the butterfly, the waves, 1 / sum, the products, the heads in
    order, times fl(1 / H). Returns (output as float64, per-head rows as float64)."""
    B, H, N, S, d = r.dims
    q = c["q"][:, :, :H * d].view(B, N, H, d).transpose(1, 2)
    k = c["k"][:, :, :H * d].view(B, S, H, d).transpose(1, 2)
    dot = torch.zeros(B, H, N, S)
    for e in range(d):
        dot = fma32(q[..., e].unsqueeze(3).expand(B, H, N, S), k[..., e].unsqueeze(2).expand(B, H, N, S), dot)
    sc = dot * torch.tensor(c["scaling"], dtype=torch.float32)
    M = sc.max(-1, keepdim=True).values
    ex = torch.exp((sc - M).double()).float()
    per = cdiv(S, NT)
    pad = torch.zeros(B, H, N, per * NT)
    pad[..., :S] = ex
    lanes = seq32(pad.view(B, H, N, per, NT), 3)
    tot = seq32(butterfly32(lanes.view(B, H, N, NT // 64, 64)), 3)
    inv = (1.0 / tot).unsqueeze(-1)
    p = ex * inv
    if not opt(r, "avg"):
        return p.double(), p.double()
    acc = torch.zeros(B, N, S)
    for h in range(H):
        acc = fma32(ex[:, h], inv[:, h].expand(B, N, S), acc) if variant == "fused" else acc + p[:, h]
    return (acc * (torch.tensor(1.0) / torch.tensor(float(H)))).double(), p.double()


# ----------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ----------------------------------------------------------------------------------------------------------------
def dev(t, device="cuda", off=0):
    """A CPU tensor (fp32 or bf16) as a guarded flat window on the device."""
    return Win(t.numel(), device, t.dtype, off=off).put(t.contiguous())


def dev_buf(t, ld, col0=0, device="cuda"):
    """A CPU [rows][cols] tensor as the (col0, cols) window of a NaN-filled [rows][ld] buffer: (Buf, window)."""
    b = Buf(t.shape[0], ld, t.dtype, device)
    w = b.window(col0, t.shape[1])
    w.copy_(t)
    return b, w


def host(w, *shape):
    a = w.data.cpu()
    return a.view(*shape) if shape else a


class Bytes:
    """A byte string (descriptor arrays, block maps, class maps, int64 timesteps) inside a NaN-filled fp32 buffer."""

    def __init__(self, raw, device="cuda"):
        raw = bytes(raw)
        self.nbytes = len(raw)
        self.win = Win(cdiv(len(raw), 4), device)
        self.buf, self.front = self.win.buf, self.win.front
        self.data = self.win.data.view(torch.uint8)[:len(raw)]
        self.data.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
