"""The declared test matrix of the optimizer-step kernels (csrc/optim.hip) and the helpers its exact tests share.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`. The expected launches -- a
fragment of the mangled kernel name with its template argument, and the grid -- are written by hand. The host rules of
optim.hip are restated below, also by hand: NORM_BLK = 2^17 gradients per norm block, one 1024-thread workgroup per
block, nb = ceil(n / NORM_BLK); sdmi_optim_workspace() = 2048 * 4 and sdmi_optim_workspace_for(n) = 4 max(nb, 2048)
bytes; sdmi_clip_unscale_ws returns -3 iff 4 nb > ws_bytes; the Adam grid is min(8192, max(1, ceil((n / VEC) / 256)))
with VEC = 4 iff params, grads, m, v and ema are 16-B aligned and params_bf16 is 8-B aligned (a null ema or
params_bf16 counts as aligned), else VEC = 1; the cast grid is min(8192, max(1, ceil((n / 4) / 256)));
sdmi_clip_finalize and sdmi_loss_flag launch a single workgroup; no entry point of this file issues a second,
decrement-style launch. STATE_CASES and FLAG_CASES are data too: one case per branch of norm_finalize_kernel and
loss_flag_kernel, each with its expected skip / scale / tracker / step words written by hand.
tests/test_optim_matrix_cpu.py checks rows against rules and that no row or case can be removed;
tests/test_optim_exact_gpu.py that the library launches what the rows say.

Entry points and dims: SUMSQ sdmi_sumsq_blocks (n); WIDEN sdmi_widen_bf16_sumsq (n) with partial (present / null);
CLIP sdmi_clip_unscale_ws (n); FIN sdmi_clip_finalize (number of partials) on hand-made partial arrays; ADAM
sdmi_adam_ema_bf16 (n) -- sdmi_adam_ema where pb = 0 -- with off (the operand that starts 4 bytes into its buffer: p,
g, m, v, ema; pb: params_bf16 2 bytes in; pb8: params_bf16 8 bytes in, which keeps VEC = 4), ema, pb (the optional
operands present), skip, step, lr, decay; CAST sdmi_cast_bf16 (n).

The definition the tests pin is that of the C ABI: Adam on the float betas as passed. 1 - b is the exact fp32
complement (1.f - 0.999f = 0.0009999871, not float(1 - 0.999) = 0.001), bc = 1 - (double)b ^ step, step_size =
float32(lr / bc1), bc2s = float32(sqrt(bc2)), the gradient is g state[1], the EMA is one rounded product and one fused
add with the ema_alpha passed. torch.optim.Adam fed Python doubles differs from this on v by
|(1.f - b2) - float(1 - b2)| / (1 - b2) relative (1.29e-5 for 0.999; complement_gap computes it) and on m by the same
expression in b1 (2.2e-7 for 0.9): a definitional difference, not rounding.

Data, two families. References are float64 on the CPU, computed from the stored fp32 inputs.

  exact  Norm: every gradient is a nonzero integer in [-3, 3], so a block's sum of squares is an integer below 2^24 in
         any order and under any contraction, and any float4, tail element, wave or block dropped or counted twice
         changes it; the scale and grad_div are powers of two: the partials are the integers and state[0] is bitwise
         float32(sqrt(float64 S)) * inv. Adam at step 1: b1 = 0.5, b2 = 0.75, eps = 0, m = v = 0, lr = 2^-10, g and
         state[1] signed powers of two: m = gi / 2, v = gi^2 / 4, and the update is exactly p - lr sign(g). Adam at
         steps 2, 1000, 2^20 + 1: b1 = b2 = 0 over non-trivial power-of-two m and v: m = gi, v = gi^2, both bias
         corrections are 1 (a step word read as 0 would make them 0). p = target + lr sign(g), so the stored parameter
         is the target: bf16 ties whose even neighbour is below and above, a value that rounds up into the next
         binade, +0, generic powers of two; p = +-inf and NaN stay what they are. EMA: decay = alpha = 0.5 on
         multiples of 2^-8. Cast: the same targets plus -0, +-inf, +-the largest finite value, NaN.
  soft   Norm: randn * 10^U(-3, 1) * 65536. Adam: per element a magnitude s = 10^U(-5, 1); g state[1] = s randn,
         m = 0.1 s randn, v = 0.01 s^2 (randn^2 + 0.1) (so eps decides some denominators), p and ema randn, state[1] =
         fl(0.73 / 65536), torch's default betas and eps, lr 1e-3 and 1e-5, decay 0.99 and 0.9999.

Statements and bounds (u = 2^-24; T the sum of absolute terms of the output):

  wire    the widened gradients are the exact fp32 image of the bf16 wire, bitwise.
  partial |partial - ref| <= K_N u T, T = the block's sum of squares; exact family bitwise. A block gives the same
          partial whichever entry point summed it (sdmi_clip_unscale_ws whole, sdmi_sumsq_blocks on block-aligned
          pieces, sdmi_widen_bf16_sumsq on the bf16 image), bitwise, and so the same state[0].
  norm    state[0]: |norm - ref| <= (K_N / 2 + 4) u ref (the square root halves the sum's error; then the rounding of
          the root to fp32, of scale * grad_div, of its reciprocal and of the product). On hand-made partials (the
          double sum of at most 2049 fp32 values of one magnitude is exact in any order) bitwise.
  state   words [1] .. [5] bitwise a numpy.float32 model of the state machine evaluated on the kernel's own state[0];
          [6], [7] untouched. state[1] is bitwise too: the build is plain hipcc -O3, whose fp32 division is the
          correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence (read in the disassembly of
          norm_finalize_kernel and adam_ema_kernel; sqrtf likewise carries its fma correction), so no ulp is allowed.
  m, v    |m - ref| <= K_M u T_m, T_m = |m| + (1 - b1) (|gi| + |m|); |v - ref| <= K_V u T_v, T_v = b2 v + (1 - b2) gi^2.
  p       |p - ref| <= K_P u T_p, T_p = |p| + step_size / denom (T_m + 1.5 |m'|): the update inherits the error of m'
          and half the relative error of v' (all of v's terms are positive), and adds its own roundings.
  ema     bitwise fma32(alpha, p, fl(ema decay)) on the kernel's own p, both families (mul_ieee and an explicit
          fmaf in the source); also |ema - ref| <= K_E u (|ema decay| + |alpha p|) against float64 on that p.
  image   params_bf16 and the cast output are bitwise RNE of the fp32 value stored (a NaN stays a NaN).
  skip    a skipped step leaves p, m, v, ema and params_bf16 untouched; a second call repeats every bit.

K is measured, not chosen: tests/test_optim_matrix_cpu.py runs an fp32 emulation in the kernel's order (block sum: per
thread its float4s in order -- the 8-wide unrolled body adds in the same order as its remainder loop --, the scalar
tail, the 64-lane butterfly, the 16 waves in order; Adam: the expression as written) once with every product rounded
separately and once with the contractions a compiler may make (fma chains in sq4 and the tail; gi - m, the lerp, the
second moment and the update as fmas), on every soft row, and measures max |fp32 - float64| / (u T). The larger of the
two variants reached: partial 2.31, m 2.37, v 2.63, p 0.99, ema 1.89. The GPU's contraction choices are a third
variant, so a constant is twice the largest ratio of its kind, rounded up: K_N = 5, K_M = 5, K_V = 6, K_P = 2, K_E = 4.
The CPU test asserts that the emulations stay within K / 2, that 2 ratio <= K <= 3 ratio, and that each perturbed
reference (1 - b2 replaced by torch's float(1 - 0.999), the step off by one, bc2 without its square root, eps inside
the square root, the EMA with 1 - decay formed in fp32, one float4 / tail element / wave / block dropped from a sum,
a partial beyond index 255 dropped in the finalize, 1 ulp in a bf16 tie) leaves its statement.

Measured on an MI355X, max(err / bound) over all rows, exact family / soft family: partial 0 / 0.463, norm 0.105 /
0.224 (the exact family's state[0] is also bitwise float32(sqrt(S)) * inv; 0.105 is that value against the float64
norm), m 0 / 0.308, v 0 / 0.367, p 0 / 0.493, ema 0 / 0.472. Bitwise in both families: the wire, params_bf16 and the
cast image, the EMA on the kernel's own p, the same partial from all three entry points, state words [0] .. [5] of
every finalize row and state case against the model, untouched operands on a skipped step, every bit of a second call;
in the exact family also the partials, m, v and p (capped grids included). On a first step the GPU's v lies 3.2 u from
the ABI's float64 model and 1.2730e-5 .. 1.3091e-5 from the model with torch's complements (complement gap 1.2922e-5):
the gap is what the old rtol = 4e-5 of tests/test_gradscaler_gpu.py was absorbing, and it explains all of it but about
1e-6. No row found a defect in the kernels of optim.hip. Reading the host code found one: sdmi_adam_ema and
sdmi_adam_ema_bf16 checked none of their arguments; they now return -1 for a null params, grads, m, v or state and for
n < 0, and 0 without a launch for n == 0, and the error-return test covers it.

Guards: every operand and output is a window of a NaN-filled buffer; state and the workspace sit between NaN pads.
After a call only the declared outputs may have changed, bit for bit: that covers the inputs, the workspace past nb
floats, an absent ema or params_bf16 and the state words a branch must not write. No case is excluded from any
statement."""
import collections
import functools

import numpy as np
import torch

from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401  (shared with the attention tests)
from tests.dit_matrix import butterfly32, seq32
from tests.norm_matrix import Flat, Guard, bf16, bits, cdiv, fma32, ptr, sum32, ulp32  # noqa: F401

SUMSQ, WIDEN, CLIP, FIN, ADAM, CAST = "sumsq", "widen", "clip", "finalize", "adam", "cast"
Row = collections.namedtuple("Row", "entry dims launches opt")
U24 = 2.0 ** -24
K_N, K_M, K_V, K_P, K_E = 5.0, 5.0, 6.0, 2.0, 4.0
NORM_ROUNDINGS = 4.0      # docstring: norm
FAMILIES = ("exact", "soft")
VARIANTS = ("separate", "fused")
f32 = np.float32


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/optim.hip, restated
# ----------------------------------------------------------------------------------------------------------------
NORM_BLK = 2 ** 17
NTN, NT = 1024, 256
NORM_BLOCKS = 2048
GRID_CAP = 8192
FP32_OPERANDS = ("p", "g", "m", "v", "ema")


def norm_blocks(n):
    return cdiv(n, NORM_BLK) if n > 0 else 0


def optim_workspace():
    return NORM_BLOCKS * 4


def optim_workspace_for(n):
    return 4 * max(norm_blocks(n), NORM_BLOCKS)


def clip_status(n, ws_bytes):
    return -3 if 4 * norm_blocks(n) > ws_bytes else 0


def byte_offsets(off):
    """The byte offset of every Adam operand from a 16-B boundary for a row's `off` option."""
    o = dict.fromkeys(FP32_OPERANDS + ("pb",), 0)
    if off in FP32_OPERANDS:
        o[off] = 4
    elif off == "pb":
        o["pb"] = 2
    elif off == "pb8":
        o["pb"] = 8
    else:
        assert off is None
    return o


def adam_vec(off, ema=1, pb=1):
    o = byte_offsets(off)
    if not ema:
        o["ema"] = 0
    if not pb:
        o["pb"] = 0
    return 4 if all(o[k] % 16 == 0 for k in FP32_OPERANDS) and o["pb"] % 8 == 0 else 1


def adam_grid(n, vec):
    return min(GRID_CAP, max(1, cdiv(n // vec, NT)))


def cast_grid(n):
    return min(GRID_CAP, max(1, cdiv(n // 4, NT)))


def adam_name(vec):
    return f"adam_ema_kernelILi{vec}EE"


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    o = dict(options)
    n = dims[0]
    if entry == SUMSQ:
        return [("sumsq_block_kernel", norm_blocks(n))]
    if entry == WIDEN:
        return [("widen_sumsq_kernel", norm_blocks(n))]
    if entry == CLIP:
        return [("sumsq_block_kernel", norm_blocks(n)), ("norm_finalize_kernel", 1)]
    if entry == FIN:
        return [("norm_finalize_kernel", 1)]
    if entry == CAST:
        return [("cast_bf16_kernel", cast_grid(n))]
    assert entry == ADAM
    vec = adam_vec(o.get("off"), o.get("ema", 1), o.get("pb", 1))
    return [(adam_name(vec), adam_grid(n, vec))]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
_S, _W, _F = "sumsq_block_kernel", "widen_sumsq_kernel", ("norm_finalize_kernel", 1)
# one block: 1, 3 (tail only), 4 (one float4), 5 (a float4 and a tail element), 4099 (threads 1024 .. without a float4),
# 32764 / 32768 / 32772 (around e4 = 8192: every thread runs exactly one unrolled pass), 131071 (the last tail), 131072
ROWS = [
    R(SUMSQ, (1,), (_S, 1)), R(SUMSQ, (3,), (_S, 1)), R(SUMSQ, (4,), (_S, 1)), R(SUMSQ, (5,), (_S, 1)),
    R(SUMSQ, (4099,), (_S, 1)), R(SUMSQ, (32764,), (_S, 1)), R(SUMSQ, (32768,), (_S, 1)), R(SUMSQ, (32772,), (_S, 1)),
    R(SUMSQ, (131071,), (_S, 1)), R(SUMSQ, (131072,), (_S, 1)),
    # several blocks: a second block of one element, a third of five, three full ones
    R(SUMSQ, (131073,), (_S, 2)), R(SUMSQ, (262149,), (_S, 3)), R(SUMSQ, (393216,), (_S, 3)),
]
ROWS += [
    R(WIDEN, (1,), (_W, 1), partial=1), R(WIDEN, (3,), (_W, 1), partial=1), R(WIDEN, (4,), (_W, 1), partial=1),
    R(WIDEN, (5,), (_W, 1), partial=1), R(WIDEN, (4099,), (_W, 1), partial=1), R(WIDEN, (32764,), (_W, 1), partial=1),
    R(WIDEN, (32768,), (_W, 1), partial=1), R(WIDEN, (32772,), (_W, 1), partial=1),
    R(WIDEN, (131071,), (_W, 1), partial=1), R(WIDEN, (131072,), (_W, 1), partial=1),
    R(WIDEN, (131073,), (_W, 2), partial=1), R(WIDEN, (262149,), (_W, 3), partial=1),
    R(WIDEN, (393216,), (_W, 3), partial=1),
    # no partial: the widening alone, with a tail and across blocks
    R(WIDEN, (5,), (_W, 1), partial=0), R(WIDEN, (262149,), (_W, 3), partial=0),
]
# the whole-buffer call: one block, a ragged third block, three full blocks (compared with the pieces above)
ROWS += [
    R(CLIP, (4099,), (_S, 1), _F), R(CLIP, (262149,), (_S, 3), _F), R(CLIP, (393216,), (_S, 3), _F),
]
# the finalize on hand-made partials: fewer than, exactly and more than its 256 threads; 2048 (the fixed workspace) + 1
ROWS += [R(FIN, (k,), _F) for k in (1, 255, 256, 257, 2048, 2049)]
_A4, _A1 = "adam_ema_kernelILi4EE", "adam_ema_kernelILi1EE"
ROWS += [
    # VEC = 4, every optional operand: tail only, one float4, float4 + tail, a full block minus one, tails of 1, 2, 3
    R(ADAM, (1,), (_A4, 1)), R(ADAM, (3,), (_A4, 1)), R(ADAM, (4,), (_A4, 1)), R(ADAM, (5,), (_A4, 1)),
    R(ADAM, (1023,), (_A4, 1)), R(ADAM, (1025,), (_A4, 1)), R(ADAM, (1026,), (_A4, 1)), R(ADAM, (1027,), (_A4, 1)),
    # three workgroups, the last with one float4, and a tail in block 0
    R(ADAM, (2055,), (_A4, 3), lr=1e-5, decay=0.9999),
    # params_bf16 on an 8-byte boundary keeps VEC = 4
    R(ADAM, (1027,), (_A4, 1), off="pb8"),
    # VEC = 1 forced by each operand in turn (1027 elements: five workgroups, the last with three)
    R(ADAM, (1027,), (_A1, 5), off="p"), R(ADAM, (1027,), (_A1, 5), off="g"), R(ADAM, (1027,), (_A1, 5), off="m"),
    R(ADAM, (1027,), (_A1, 5), off="v"), R(ADAM, (1027,), (_A1, 5), off="ema", lr=1e-5, decay=0.9999),
    R(ADAM, (1027,), (_A1, 5), off="pb"),
    # VEC = 1 at the small sizes
    R(ADAM, (1,), (_A1, 1), off="g"), R(ADAM, (3,), (_A1, 1), off="g"), R(ADAM, (4,), (_A1, 1), off="g"),
    R(ADAM, (5,), (_A1, 1), off="g"), R(ADAM, (1023,), (_A1, 4), off="g"), R(ADAM, (1025,), (_A1, 5), off="g"),
    R(ADAM, (1026,), (_A1, 5), off="g"),
    # the optional operands absent (pb = 0 runs sdmi_adam_ema)
    R(ADAM, (1027,), (_A4, 1), ema=0), R(ADAM, (1027,), (_A4, 1), pb=0), R(ADAM, (1027,), (_A4, 1), ema=0, pb=0),
    R(ADAM, (1027,), (_A1, 5), off="g", ema=0), R(ADAM, (1027,), (_A1, 5), off="g", pb=0),
    R(ADAM, (1027,), (_A1, 5), off="g", ema=0, pb=0),
    # an absent operand's alignment does not count
    R(ADAM, (1027,), (_A4, 1), off="ema", ema=0), R(ADAM, (1027,), (_A4, 1), off="pb", pb=0),
    # a skipped step
    R(ADAM, (1027,), (_A4, 1), skip=1), R(ADAM, (1027,), (_A1, 5), off="g", skip=1),
    # the step counter
    R(ADAM, (1027,), (_A4, 1), step=2), R(ADAM, (1027,), (_A4, 1), step=1000),
    R(ADAM, (1027,), (_A4, 1), step=2 ** 20 + 1, lr=1e-5), R(ADAM, (1027,), (_A1, 5), off="g", step=1000),
    # the capped grids and their grid-stride loops (exact family only): 259 elements and 1027 past one full trip
    R(ADAM, (8192 * 256 + 259,), (_A1, 8192), off="g", big=1),
    R(ADAM, (4 * 8192 * 256 + 1027,), (_A4, 8192), big=1),
]
_C = "cast_bf16_kernel"
ROWS += [
    R(CAST, (1,), (_C, 1)), R(CAST, (3,), (_C, 1)), R(CAST, (4,), (_C, 1)), R(CAST, (5,), (_C, 1)),
    R(CAST, (1023,), (_C, 1)), R(CAST, (1025,), (_C, 1)), R(CAST, (1026,), (_C, 1)), R(CAST, (1027,), (_C, 1)),
    R(CAST, (2055,), (_C, 3)), R(CAST, (4 * 8192 * 256 + 1027,), (_C, 8192), big=1),
]

# Every branch of norm_finalize_kernel on hand-made partials (`parts`; `grads`: through sdmi_clip_unscale_ws instead).
# want = (skip, scale, tracker, step) after the call, written by hand. Defaults: scale 8, div 1, maxn 1, mode 0,
# loss 1.5, flag 0, gi 3, tr 0, step 5; parts (9, 16) give S = 25, sqrt 5, norm 5 / 8.
INF, NAN = float("inf"), float("nan")


def S(name, want, **kw):
    c = dict(name=name, parts=(9.0, 16.0), grads=None, scale=8.0, div=1.0, maxn=1.0, mode=0, loss=1.5, flag=0.0, gi=3,
             tr=0.0, step=5.0, want=want)
    assert set(kw) <= set(c)
    c.update(kw)
    return c


STATE_CASES = [
    # mode 0 ignores a non-finite loss and a raised flag; the clip coefficient is clamped at 1
    S("mode0-ignores-loss-and-flag", (0, 8.0, 1.0, 6.0), loss=NAN, flag=1.0),
    # mode 1: finite loss (the flag is ignored), tracker 1 of 3; NaN and inf losses skip without a scaler update
    S("mode1-finite-tracker1", (0, 8.0, 2.0, 6.0), mode=1, flag=1.0, tr=1.0),
    S("mode1-nan-loss", (1, 8.0, 1.0, 5.0), mode=1, loss=NAN, tr=1.0),
    S("mode1-inf-loss", (1, 8.0, 2.0, 5.0), mode=1, loss=INF, tr=2.0),
    # mode 2: the flag decides, the loss word is ignored; tracker 2 of 3 grows the scale
    S("mode2-flag0-tracker2-grows", (0, 16.0, 0.0, 6.0), mode=2, loss=NAN, tr=2.0),
    S("mode2-flag-raised", (1, 8.0, 2.0, 5.0), mode=2, flag=2.0, tr=2.0),
    # a non-finite norm backs the scale off and resets the tracker: from an inf, from a NaN, from squares that overflow
    S("inf-partial", (1, 4.0, 0.0, 5.0), parts=(INF, 1.0), tr=2.0),
    S("nan-partial-mode1", (1, 4.0, 0.0, 5.0), parts=(NAN, 1.0), mode=1, tr=1.0),
    S("squares-overflow-fp32", (1, 4.0, 0.0, 5.0), parts=None, grads=(2.0 ** 64,) * 5, tr=2.0),
    # both at once: the loss decides first, no scaler update
    S("nan-partial-and-nan-loss", (1, 8.0, 2.0, 5.0), parts=(NAN, 1.0), mode=1, loss=NAN, tr=2.0),
    # partials whose sum overflows fp32 stay finite in the double accumulation: norm 2^64.5, coef below 1
    S("partial-sum-beyond-fp32", (0, 1.0, 1.0, 6.0), parts=(2.0 ** 127,) * 4, scale=1.0),
    # no loss scaler
    S("growth0-clean", (0, 8.0, 2.0, 6.0), gi=0, tr=2.0),
    S("growth0-bad", (1, 8.0, 2.0, 5.0), gi=0, tr=2.0, parts=(INF, 1.0)),
    S("growth-negative-clean", (0, 8.0, 0.0, 6.0), gi=-1),
    S("growth1", (0, 16.0, 0.0, 6.0), gi=1),
    # the coefficient: below 1, norm 0, max_norm inf (with grad_div 2 and no scaler: the VQVAE trainer's call)
    S("coef-below-1", (0, 1.0, 1.0, 6.0), scale=1.0),
    S("norm-0", (0, 8.0, 1.0, 6.0), parts=(0.0, 0.0)),
    S("max-norm-inf", (0, 1.0, 0.0, 6.0), scale=1.0, maxn=INF, gi=0, div=2.0),
    S("max-norm-inf-norm-inf", (1, 4.0, 0.0, 5.0), parts=(INF, 1.0), maxn=INF),
    # grad_div 2 and 3 (3: the reciprocal of 24 is rounded)
    S("div2", (0, 8.0, 1.0, 6.0), div=2.0),
    S("div3-coef-below-1", (0, 8.0, 1.0, 6.0), div=3.0, maxn=0.125),
]

# sdmi_loss_flag: (mode, *src, the expected *dst)
FLAG_CASES = [(0, 0.0, 0.0), (0, 1.5, 0.0), (0, INF, 1.0), (0, -INF, 1.0), (0, NAN, 1.0),
              (1, 0.0, 0.0), (1, 1.5, 1.0), (1, INF, 1.0), (1, NAN, 1.0)]


def row_id(r):
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{v}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# norm: data, references, emulation
# ----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


NORM_STATE = dict(exact=dict(scale=16.0, div=2.0, maxn=1.0), soft=dict(scale=65536.0, div=1.0, maxn=1.0))


@functools.lru_cache(maxsize=8)
def norm_case(kind, n, wire=False):
    """n gradients as float64 copies of fp32 values (`wire`: of bf16 values)."""
    gen = _gen(1 if kind == "exact" else 2, n)
    if kind == "exact":
        mag = torch.randint(1, 4, (n,), generator=gen).double()
        return mag * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    g = g * 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4 - 3) * 65536.0
    return bf16(g) if wire else g.float().double()


def block_sums(g, weights=None):
    """The float64 sum of squares of every NORM_BLK block; `weights` counts elements (0: dropped)."""
    sq = g * g if weights is None else g * g * weights
    nb = norm_blocks(g.numel())
    pad = torch.zeros(nb * NORM_BLK, dtype=torch.float64)
    pad[:g.numel()] = sq
    return pad.view(nb, NORM_BLK).sum(1)


def emulate_blocks(g, variant, drop=None):
    """The partial of every block in fp32 in the kernel's order. drop: ('float4', i) / ('tail', j) / ('wave', w) /
    ('block', b) leaves that piece out (the perturbations of the CPU test)."""
    g = g.float()
    out = []
    for b, b0 in enumerate(range(0, g.numel(), NORM_BLK)):
        blk = g[b0:b0 + NORM_BLK]
        e = blk.numel()
        e4 = e // 4
        v = blk[:e4 * 4].view(e4, 4)
        x, y, z, w = v.unbind(1)
        if variant == "fused":
            s = fma32(w, w, fma32(z, z, fma32(y, y, x * x)))
        else:
            s = ((x * x + y * y) + z * z) + w * w
        if drop is not None and drop[0] == "float4" and e4:
            s = s.clone()
            s[drop[1] % e4] = 0.0
        steps = max(cdiv(e4, NTN), 1)
        lanes = torch.zeros(steps * NTN, dtype=torch.float32)
        lanes[:e4] = s
        acc = seq32(lanes.view(steps, NTN), 0)
        t = blk[e4 * 4:]
        if drop is not None and drop[0] == "tail" and t.numel():
            t = t.clone()
            t[drop[1] % t.numel()] = 0.0
        k = t.numel()
        acc[:k] = fma32(t, t, acc[:k]) if variant == "fused" else acc[:k] + t * t
        waves = butterfly32(acc.view(NTN // 64, 64))
        if drop is not None and drop[0] == "wave":
            waves = waves.clone()
            waves[drop[1]] = 0.0
        p = seq32(waves, 0)
        out.append(p * 0.0 if drop is not None and drop == ("block", b) else p)
    return torch.stack(out).double()


def partials_sum(parts, upto=None):
    """The double sum the finalize forms of fp32 partials (`upto`: a perturbed one that stops there)."""
    p = torch.as_tensor(parts, dtype=torch.float64)
    return float(p[:upto].sum())


def norm_model(S, scale, div):
    """float32(sqrt(float64 S)) * (1.f / (scale * grad_div)) with numpy.float32 roundings: (norm, inv)."""
    with np.errstate(all="ignore"):
        inv = f32(1.0) / (f32(scale) * f32(div))
        return f32(np.sqrt(np.float64(S))) * inv, inv


def norm_bound(ref, K=None):
    return ((K_N if K is None else K) / 2 + NORM_ROUNDINGS) * U24 * abs(ref)


def finalize_model(norm, state, maxn, gi, mode, div):
    """norm_finalize_kernel's thread 0 after the sum, in numpy.float32, on a given state[0]: the eight words after."""
    st = np.array(state, dtype=f32)
    with np.errstate(all="ignore"):
        scale = st[2]
        inv = f32(1.0) / (scale * f32(div))
        st[0] = norm
        loss_bad = (not np.isfinite(st[6])) if mode == 1 else bool(st[7] != 0) if mode == 2 else False
        bad = (not np.isfinite(norm)) or loss_bad
        st[5] = f32(1.0 if bad else 0.0)
        coef = f32(maxn) / (f32(norm) + f32(1e-6))
        coef = coef if coef < f32(1.0) else f32(1.0)
        st[1] = coef * inv
        if gi <= 0:
            if not bad:
                st[4] = st[4] + f32(1.0)
        elif not loss_bad:
            if bad:
                st[2] = scale * f32(0.5)
                st[3] = f32(0.0)
            else:
                tr = st[3] + f32(1.0)
                if int(tr) >= gi:
                    st[2] = scale * f32(2.0)
                    tr = f32(0.0)
                st[3] = tr
                st[4] = st[4] + f32(1.0)
    return st


def state_words(c):
    """The eight state words a state case starts from."""
    return np.array([NAN, NAN, c["scale"], c["tr"], c["step"], NAN, c["loss"], c["flag"]], dtype=f32)


def case_partials(c):
    """The fp32 partials of a state case (from `grads`: what the block sum leaves, squares rounded to fp32)."""
    if c["grads"] is not None:
        with np.errstate(all="ignore"):
            g = np.array(c["grads"], dtype=f32)
            return np.array([np.sum(g * g, dtype=f32)], dtype=f32)
    return np.array(c["parts"], dtype=f32)


def case_trace(c):
    """The branches a state case takes, by the model: a dict of flags for the coverage checks."""
    parts = case_partials(c)
    norm, _ = norm_model(float(np.sum(parts.astype(np.float64))), c["scale"], c["div"])
    st = finalize_model(norm, state_words(c), c["maxn"], c["gi"], c["mode"], c["div"])
    loss_bad = (c["mode"] == 1 and not np.isfinite(c["loss"])) or (c["mode"] == 2 and c["flag"] != 0)
    with np.errstate(all="ignore"):
        raw = f32(c["maxn"]) / (norm + f32(1e-6))
    return dict(norm=float(norm), after=st, loss_bad=bool(loss_bad), norm_bad=not np.isfinite(norm),
                grew=bool(st[2] > c["scale"]), backed=bool(st[2] < c["scale"]), below1=bool(raw < 1),
                raw_nan=bool(np.isnan(raw)))


def finalize_parts(kind, k):
    """k hand-made partials of one magnitude: integers (exact) or fp32 values in [1, 9) (soft)."""
    gen = _gen(3 if kind == "exact" else 4, k)
    if kind == "exact":
        return torch.randint(1, 1000, (k,), generator=gen).double()
    return (1.0 + 8.0 * torch.rand(k, generator=gen, dtype=torch.float64)).float().double()


# ----------------------------------------------------------------------------------------------------------------
# Adam: data, references, emulation
# ----------------------------------------------------------------------------------------------------------------
LR_EXACT = 2.0 ** -10
TARGETS = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2 - 2.0 ** -9, 0.0, -(1 + 3 * 2.0 ** -8))
P_SPECIALS = (INF, -INF, NAN)
MAXF = float(np.finfo(np.float32).max)
CAST_SPECIALS = TARGETS + (-0.0, INF, -INF, MAXF, -MAXF, NAN, 2.0 ** -126, 2.0 ** -133, 1 + 2.0 ** -8 + 2.0 ** -23,
                           1 + 2.0 ** -8 - 2.0 ** -24)


def _f(x):
    return float(f32(x))


def _pow2(gen, n, lo, hi, signed=True):
    v = 2.0 ** torch.randint(lo, hi + 1, (n,), generator=gen).double()
    return v * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1) if signed else v


def _plant(t, values, phase):
    """t[i] = values[(i // 7) % len] where i % 7 == phase (every value appears once n reaches 7 len)."""
    i = torch.arange(t.numel())
    sel = i % 7 == phase
    t[sel] = torch.tensor(values, dtype=torch.float64)[(i[sel] // 7) % len(values)]
    return t


@functools.lru_cache(maxsize=4)
def adam_case(kind, n, step=1, lr=1e-3, decay=0.99):
    """p, g, m, v, e (float64 copies of fp32 values) and the scalars, every one the fp32 value the ABI receives."""
    gen = _gen(5 if kind == "exact" else 6, n, step)
    if kind == "exact":
        gs = 2.0 ** -4
        g = _pow2(gen, n, -3, 3)
        target = _plant(_pow2(gen, n, -4, 4), TARGETS, 3)
        p = _plant(target + LR_EXACT * torch.sign(g), P_SPECIALS, 5)
        e = torch.randint(-1024, 1025, (n,), generator=gen).double() / 256
        if step == 1:
            m, v, b1, b2 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), 0.5, 0.75
        else:
            m, v, b1, b2 = _pow2(gen, n, -6, 0), _pow2(gen, n, -6, 0, signed=False), 0.0, 0.0
        return dict(kind=kind, n=n, p=p, g=g, m=m, v=v, e=e, gs=gs, step=step, lr=LR_EXACT, b1=b1, b2=b2, eps=0.0,
                    decay=0.5, alpha=0.5)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)  # noqa: E731
    s = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 5)
    gs = _f(0.73 / 65536)
    c = dict(kind=kind, n=n, p=rn(), g=s * rn() / gs, m=0.1 * s * rn(), v=0.01 * s * s * (rn() ** 2 + 0.1), e=rn())
    c = {k: (t.float().double() if isinstance(t, torch.Tensor) else t) for k, t in c.items()}
    c.update(gs=gs, step=step, lr=_f(lr), b1=_f(0.9), b2=_f(0.999), eps=_f(1e-8), decay=_f(decay), alpha=_f(1 - decay))
    return c


def row_case(kind, r):
    return adam_case(kind, r.dims[0], opt(r, "step", 1), opt(r, "lr", 1e-3), opt(r, "decay", 0.99))


def complement32(b):
    """1.f - b: the exact fp32 complement the kernel forms."""
    return float(f32(1.0) - f32(b))


def complement_torch(b_double):
    """float(1 - b) from the Python double: what torch.optim.Adam multiplies by."""
    return _f(1.0 - b_double)


def complement_gap(b_double):
    """|(1.f - b) - float(1 - b_double)| / (1 - b_double): the relative difference between the two definitions."""
    return abs(complement32(_f(b_double)) - complement_torch(b_double)) / (1.0 - b_double)


def bias_terms(c, step_off=0, no_sqrt=False):
    """(step_size, bc2s) as float64 copies of the fp32 values the kernel forms in double."""
    step = c["step"] + step_off
    bc1, bc2 = 1.0 - c["b1"] ** step, 1.0 - c["b2"] ** step
    with np.errstate(all="ignore"):
        return float(f32(np.float64(c["lr"]) / np.float64(bc1))), float(f32(bc2 if no_sqrt else np.sqrt(bc2)))


def adam_reference(c, comp2=None, comp1=None, step_off=0, no_sqrt=False, eps_inside=False):
    """The step in float64 as the ABI defines it, with the sums of absolute terms that scale the bounds. The keyword
    arguments are the perturbed references of the CPU test."""
    c1 = complement32(c["b1"]) if comp1 is None else comp1
    c2 = complement32(c["b2"]) if comp2 is None else comp2
    step_size, bc2s = bias_terms(c, step_off, no_sqrt)
    gi = c["g"] * c["gs"]
    m = c["m"] + c1 * (gi - c["m"])
    v = c["v"] * c["b2"] + c2 * gi * gi
    denom = torch.sqrt(v + c["eps"]) / bc2s if eps_inside else torch.sqrt(v) / bc2s + c["eps"]
    p = c["p"] - step_size * (m / denom)
    T_m = c["m"].abs() + c1 * (gi.abs() + c["m"].abs())
    T_v = c["v"].abs() * c["b2"] + c2 * gi * gi
    T_p = c["p"].abs() + step_size / denom * (T_m + 1.5 * m.abs())
    return dict(m=m, v=v, p=p, T_m=T_m, T_v=T_v, T_p=T_p)


def ema_reference(c, p, alpha=None):
    """(float64 ema on the given p, T_e, the bitwise value fma32(alpha, p, fl(e decay)))."""
    a = c["alpha"] if alpha is None else alpha
    prod = c["e"].float() * torch.tensor(c["decay"], dtype=torch.float32)
    exact = fma32(torch.tensor(a, dtype=torch.float32), p.float(), prod).double()
    return c["e"] * c["decay"] + a * p, (c["e"] * c["decay"]).abs() + (a * p).abs(), exact


def adam_closed_form(c):
    """The exact family in plain fp32 without a float64 pass: m, v, p, e."""
    assert c["kind"] == "exact"
    g, p, e = c["g"].float(), c["p"].float(), c["e"].float()
    gi = g * c["gs"]
    m, v = (gi * 0.5, gi * gi * 0.25) if c["step"] == 1 else (gi, gi * gi)
    pn = p - c["lr"] * torch.sign(g)
    return dict(m=m, v=v, p=pn, e=(pn + e) * 0.5)


def emulate_adam(c, variant):
    """adam_one in fp32 as written, every product rounded separately or with the contractions a compiler may make."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    g, m, v, p = (c[k].float() for k in "gmvp")
    gs, b2 = t(c["gs"]), t(c["b2"])
    c1, c2 = t(1.0) - t(c["b1"]), t(1.0) - t(c["b2"])
    ss, bc2s = (t(x) for x in bias_terms(c))
    gi = g * gs
    if variant == "fused":
        mi = fma32(c1, fma32(g, gs, -m), m)
        vi = fma32(c2 * gi, gi, v * b2)
    else:
        mi = m + c1 * (gi - m)
        vi = v * b2 + c2 * gi * gi
    q = mi / (torch.sqrt(vi) / bc2s + t(c["eps"]))
    pn = fma32(-ss, q, p) if variant == "fused" else p - ss * q
    en = fma32(t(c["alpha"]), pn, c["e"].float() * t(c["decay"]))
    return dict(m=mi.double(), v=vi.double(), p=pn.double(), e=en.double())


@functools.lru_cache(maxsize=4)
def cast_case(kind, n):
    gen = _gen(7 if kind == "exact" else 8, n)
    if kind == "soft":
        return torch.randn(n, generator=gen, dtype=torch.float64).float().double()
    x = torch.randint(-2 ** 23, 2 ** 23, (n,), generator=gen).double() * 2.0 ** -20
    return _plant(x, CAST_SPECIALS, 0)


def same_bits(a, b):
    """Equal bit for bit, a NaN matching any NaN (fp32 or bf16 tensors on the CPU)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and \
        torch.equal(bits(a.contiguous())[~na], bits(b.contiguous())[~nb])


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
class Win(Flat):
    """n elements of `dtype` starting `off` elements past the 64-element front pad of a NaN-filled buffer."""

    def __init__(self, n, device, dtype=torch.float32, off=0, front=64, tail=256):
        self.buf = torch.full((front + off + n + tail,), NAN, dtype=dtype, device=device)
        self.n, self.front = n, front + off
        self.data = self.buf[self.front:self.front + n]

    def put(self, values):
        self.data.copy_(values.reshape(-1).to(self.buf.dtype))
        return self


class NormProblem:
    """Gradients (fp32, and their bf16 wire), the widened copy, the workspace and state of one norm case."""

    def __init__(self, g, kind, device="cuda", wire=False):
        n = g.numel()
        self.n, self.nb, self.kind = n, norm_blocks(n), kind
        self.g = Win(n, device).put(g)
        self.src = Win(n, device, torch.bfloat16).put(g) if wire else None
        self.dst = Win(n, device) if wire else None
        self.ws_bytes = optim_workspace_for(n)
        self.ws = Win(self.ws_bytes // 4, device)
        self.state = Win(8, device)
        s = NORM_STATE[kind]
        self.start = np.array([NAN, NAN, s["scale"], 0.0, 5.0, NAN, 1.5, 0.0], dtype=f32)
        self.state.put(torch.from_numpy(self.start))

    def guard(self, ws=False, state=False, dst=False):
        g = Guard()
        g.add("grads", self.g)
        if self.src is not None:
            g.add("src", self.src)
            g.add("dst", self.dst, [(0, self.n)] if dst else [])
        g.add("workspace", self.ws, [(0, self.nb)] if ws else [])
        g.add("state", self.state, [(0, 6)] if state else [])
        return g

    def clip(self, L, stream, **over):
        s = NORM_STATE[self.kind]
        a = dict(grads=ptr(self.g.data), n=self.n, maxn=s["maxn"], state=ptr(self.state.data), ws=ptr(self.ws.data),
                 ws_bytes=self.ws_bytes, gi=2000, mode=0, div=s["div"])
        a.update(over)
        return L.sdmi_clip_unscale_ws(*a.values(), stream)

    def sumsq(self, L, stream, lo=0, hi=None, **over):
        hi = self.n if hi is None else hi
        a = dict(grads=ptr(self.g.data[lo:]), n=hi - lo, partial=ptr(self.ws.data[lo // NORM_BLK:]))
        a.update(over)
        return L.sdmi_sumsq_blocks(*a.values(), stream)

    def widen(self, L, stream, partial=True, **over):
        a = dict(src=ptr(self.src.data), dst=ptr(self.dst.data), n=self.n, partial=ptr(self.ws.data) if partial else None)
        a.update(over)
        return L.sdmi_widen_bf16_sumsq(*a.values(), stream)

    def partials(self):
        return self.ws.data[:self.nb].cpu()

    def words(self):
        return self.state.data.cpu().numpy().copy()


class FinalizeProblem:
    """Hand-made partials and a state between NaN pads."""

    def __init__(self, parts, words, device="cuda"):
        parts = torch.as_tensor(np.asarray(parts, dtype=np.float64))
        self.k = parts.numel()
        self.parts = Win(self.k, device).put(parts)
        self.state = Win(8, device).put(torch.from_numpy(np.asarray(words, dtype=f32)))

    def guard(self, writes=True):
        g = Guard()
        g.add("partials", self.parts)
        g.add("state", self.state, [(0, 6)] if writes else [])
        return g

    def run(self, L, stream, maxn, gi, mode, div, **over):
        a = dict(partial=ptr(self.parts.data), n=self.k, maxn=maxn, state=ptr(self.state.data), gi=gi, mode=mode, div=div)
        a.update(over)
        return L.sdmi_clip_finalize(*a.values(), stream)

    def words(self):
        return self.state.data.cpu().numpy().copy()


class AdamProblem:
    """One Adam case on the device with the row's offsets and optional operands."""
    OUT = ("p", "m", "v", "ema", "pb")

    def __init__(self, c, row, device="cuda"):
        n = c["n"]
        self.c, self.n = c, n
        self.with_ema, self.with_pb, self.skip = opt(row, "ema", 1), opt(row, "pb", 1), opt(row, "skip", 0)
        o = byte_offsets(opt(row, "off"))
        mk = lambda name: Win(n, device, off=o[name] // 4)  # noqa: E731
        self.p, self.g, self.m, self.v, self.ema = (mk(k).put(c[x]) for k, x in zip(FP32_OPERANDS, "pgmve"))
        self.pb = Win(n, device, torch.bfloat16, off=o["pb"] // 2)
        self.state = Win(8, device).put(torch.tensor([NAN, c["gs"], NAN, NAN, float(c["step"]), float(self.skip), NAN,
                                                      NAN]))

    def guard(self, writes=True):
        g = Guard()
        w = writes and not self.skip
        for name in self.OUT:
            present = dict(ema=self.with_ema, pb=self.with_pb).get(name, 1)
            g.add(name, getattr(self, name), [(0, self.n)] if w and present else [])
        g.add("g", self.g)
        g.add("state", self.state)
        return g

    def run(self, L, stream, **over):
        c = self.c
        a = dict(p=ptr(self.p.data), g=ptr(self.g.data), m=ptr(self.m.data), v=ptr(self.v.data),
                 ema=ptr(self.ema.data) if self.with_ema else None, n=self.n, state=ptr(self.state.data), lr=c["lr"],
                 b1=c["b1"], b2=c["b2"], eps=c["eps"], decay=c["decay"], alpha=c["alpha"])
        if self.with_pb or "pb" in over:
            a["pb"] = ptr(self.pb.data) if self.with_pb else None
        a.update(over)
        fn = L.sdmi_adam_ema_bf16 if "pb" in a else L.sdmi_adam_ema
        return fn(*a.values(), stream)

    def raw(self):
        return [getattr(self, k).buf.clone() for k in self.OUT]


class CastProblem:
    def __init__(self, x, device="cuda"):
        self.n = x.numel()
        self.src = Win(self.n, device).put(x)
        self.dst = Win(self.n, device, torch.bfloat16)

    def guard(self, writes=True):
        g = Guard()
        g.add("src", self.src)
        g.add("dst", self.dst, [(0, self.n)] if writes else [])
        return g

    def run(self, L, stream, **over):
        a = dict(src=ptr(self.src.data), dst=ptr(self.dst.data), n=self.n)
        a.update(over)
        return L.sdmi_cast_bf16(*a.values(), stream)
