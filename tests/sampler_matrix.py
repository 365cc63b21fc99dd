"""The declared test matrix of the sampling-step and device-noise kernels (csrc/sampler.hip, and sdmi_add_noise of
csrc/misc.hip, the forward half of the same scheduler) and the helpers its exact tests share.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`. The expected launches -- a
fragment of the mangled kernel name and the grid -- are written by hand. The host rules are restated below, also by
hand: NT = 256; the grid is max(1, min(ceil(items / 256), cap)) with cap = 4096 in sampler.hip and 8192 in misc.hip;
items = n for the step kernels, B * per_sample for add_noise, ceil(n / 4) for sdmi_randn and ceil(n / 4) + (txt ? B *
row_elems / 4 : 0) + B for sdmi_step_draw; a second launch <<<1, 64>>> follows iff decrement_t or advance is set
(dec_t_kernel, ddim_advance_kernel, advance_kernel). A `sweep` row issues its launches once per timestep of its table
(DDPM) or once per timestep pair (DDIM) into one guarded [T][n] output, one device timestep / index word per launch,
one synchronise at the end. Error returns, before any launch: -1 for a null required pointer or a non-positive size
(sdmi_ddpm_prev(_dup): xt, eps, t_dev, betas, alphas, abar, s1m, prev, n -- z, prev2, x0 may be null;
sdmi_ddim_prev / sdmi_affine_step: the two inputs, the output, n; sdmi_ddim_prev_dev(_dup): xt, eps, out, ts, tp, idx,
abar, n -- t_dev, noise, out2 may be null; sdmi_randn: out, offset_dev, n; sdmi_step_draw: noise, t, n, B, T;
sdmi_add_noise: every pointer, B, per_sample); sdmi_step_draw with txt set returns -2 for a null text or empty, for
row_elems <= 0 or not a multiple of 4, or for any of the three pointers off a 16-byte boundary.
tests/test_sampler_matrix_cpu.py checks rows against rules and that no row can be removed;
tests/test_sampler_exact_gpu.py that the library launches what the rows say.

Entry points and dims: DDPM sdmi_ddpm_prev (n), sdmi_ddpm_prev_dup where prev2 = 1; options table (cond / uncond: the
golden scheduler tables, T = 1000; syn: T = 64, abar random and strictly decreasing in (0, 1), alphas, betas, s1m derived
in fp32), t, prev2, x0 (0: null), alias (prev == xt), dec (decrement_t), z (0: null). DDIM sdmi_ddim_prev and
sdmi_ddim_prev_dev on the same pair (sdmi_ddim_prev_dev_dup where dup = 1 or out2 = 1), outputs bitwise equal to each
other and to the model; options table (a: the golden abar of beta (0.00085, 0.012); b: cumprod(1 - linspace(0.0001,
0.02, 1000))), eta, noise (0: null), out2, alias (out == xt), adv (advance), idx, tdev (0: null). The sweep rows run
ddim_time_steps(1000, 50, "linear") and "quadratic" complete plus (1, 0) and (999, 998); the others read the pair
through ts = (1, 11, 401, 801), tp = (0, 1, 360, 760) at idx. AFF sdmi_affine_step (n) at t with the golden ddpm_*
coefficients, z (0: null). ADDN sdmi_add_noise (B, per_sample), t distinct per sample with 0 and T - 1 among them.
RANDN sdmi_randn (n) with seed, off, adv. DRAW sdmi_step_draw (n, B, row_elems) with T, txt, keep, pt / pk (p_text /
p_keep; ("own", b): sample b's own uniform as the model computes it, so the strict < keeps that row and the strict >
gives keep = 0).

References.

  steps   a numpy.float32 model, operation by operation in the order of scheduler/linear_noise_scheduler.py (add_noise
          :47-48, sample_prev_timestep :59-78, DDPMSampler :118-134, DDIMSampler :199-206): every + - * / and sqrt on
          float32 in numpy is correctly rounded, which is what div_ieee, sqrt_ieee and contract(off) promise.
          variance ** 0.5 and sigma ** 2 are sqrt and x * x; the clamp is torch.clamp's, which keeps a NaN; null noise
          is an array of +0; eta is 0, 0.5 or 1 (exact in fp32). A NaN matches any NaN; everything else compares by
          bits, -0 included. The CPU test evaluates the same expressions with torch on the CPU on every row's data and
          requires equal bits: the model is the reference's arithmetic, not a restatement of the kernel. One
          substitution: torch's own CPU sqrt and ** 0.5 are not correctly rounded on every host (AVX-512 builds: one
          ulp off for about 0.6 % of arguments), so the torch evaluation takes its square roots -- all of table
          entries, none of data -- through float64 (tsqrt); every + - * / and the clamp are torch's own.
  philox  a pure-integer numpy model (uint64 products masked to 32 bits): per round c = [hi(M1 c2) ^ c1 ^ k0,
          lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], then the key bumps by (0x9E3779B9, 0xBB67AE85); ten rounds;
          pinned to the three published Random123 known answers. Counter (q lo, q hi, off lo, off hi), q the quad
          index for noise and 2^40 + b for sample b's draw; key (seed lo, seed hi).
  draws   exact from the integers: t[b] = (c0 T) >> 32 (the upper word of every t is zero), drop = (c1 >> 8) 2^-24 <
          p_text, keep = (c2 >> 8) 2^-24 > p_keep, txt[b] = empty where dropped else text[b], bitwise.
  noise   float64 on the exact integers: u1 = ((c >> 8) + 1) 2^-24, u2 = (c' >> 8) 2^-24, rad = sqrt(-2 ln u1), theta =
          float64(float32(6.2831853...)) u2 (the kernel's constant is the definition), z = (rad cos theta, rad sin
          theta) for the word pairs (0, 1) and (2, 3). Statement: |z - ref| <= K_Z u rad (1 + theta), u = 2^-24; the
          theta term is the rounding of the fp32 angle.

K_Z is measured, not chosen. tests/test_sampler_matrix_cpu.py runs a float32 emulation of the four lines (logf, sinf
and cosf as the correctly rounded fp32 image of the float64 function, sqrt and the products in numpy.float32) on every
noise row, 2^23 draws and more overall, and measures max |fp32 - float64| / (u rad (1 + theta)) = 2.52. Twice that,
rounded up, is 6. The HIP math documentation is not part of the ROCm install these tests were written on, so the
device library's own error is an allowance, NOT a measurement: 2 ulp each for logf, sinf and cosf. 2 ulp of ln u1 is 4 u
|ln u1|, half of which (the square root) reaches rad: 2 u rad. 2 ulp of a sine or cosine is at most 4 u, times rad: 4 u
rad. LIB_ALLOWANCE = 6 and K_Z = 6 + 6 = 12. The CPU test asserts the emulation stays within 6 / 2, that 2 ratio <= 6
<= 3 ratio, and that each perturbed reference (cos and sin swapped, pairs (0, 2) and (1, 3), u1 without its + 1, >> 9, a
23-bit uniform, nine and eleven rounds, the key bump on the counter, the high word of off dropped, M0 and M1 swapped)
leaves the bound by a factor above 1000 on the same data.

Measured on an MI355X: max(err / bound) of the noise over every RANDN and DRAW row 0.250 (0.247 on the 4194307 draws of
sdmi_randn at (7, 2^32 + 1), 0.250 on those of sdmi_step_draw at (2^63 + 5, 2^62 - 1)). Everything else was bitwise: every DDPM, DDIM, affine and add_noise row against the model (specials, seams, in-place
and second outputs included), sdmi_ddim_prev against sdmi_ddim_prev_dev(_dup), the device words after dec_t /
ddim_advance / advance, t, the text rows and keep of every draw, sdmi_randn against the noise segment of sdmi_step_draw,
sample b's draw for every B, and every bit of a second call. Before the fix of this file's pull request the library
returned x0 = -1 for a NaN prediction (fminf(fmaxf(NaN, -1), 1): v_max / v_min return the other operand); it now
returns the NaN, as torch.clamp does, and every other x0 is bitwise what it was.

Out of scope: quad indices beyond 2^32 (the second counter word) need n > 2^34 floats and are not tested at any sane
size; sdmi_cfg_combine(_nhwc) (tests/test_cfg_sampling_gpu.py); the captured loops themselves.

Guards: every operand and output is a window of a NaN-filled buffer; the device words (t_dev, idx, offset_dev) are
int64 views of NaN-filled fp32 buffers, so they sit between pads too. After a call only the declared outputs may have
changed, bit for bit. No element is excluded from any statement."""
import collections
import functools
import os

import numpy as np
import torch

from tests.optim_matrix import Flat, Guard, Win, bits, cdiv, launches_match, ptr, recorded  # noqa: F401

DDPM, DDIM, AFF, ADDN, RANDN, DRAW = "ddpm", "ddim", "affine", "add_noise", "randn", "draw"
Row = collections.namedtuple("Row", "entry dims launches opt")
f32 = np.float32
U24 = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

EMULATED_RATIO = 2.52     # docstring: K_Z
LIB_ALLOWANCE = 6.0       # 2 ulp each for logf, sinf, cosf: unmeasured
K_Z = 12.0
MEASURED_NOISE = 0.250    # max(err / bound) on an MI355X (docstring)


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/sampler.hip and of sdmi_add_noise, restated
# ----------------------------------------------------------------------------------------------------------------
NT = 256
GRID_CAP = 4096
ADDN_GRID_CAP = 8192
TAIL_THREADS = 64
K_DDPM, K_DEC = "16ddpm_prev_kernel", "12dec_t_kernel"
K_DDIM, K_DDIM_DEV, K_DDIM_ADV = "16ddim_prev_kernel", "20ddim_prev_dev_kernel", "19ddim_advance_kernel"
K_AFF, K_ADDN, K_RANDN, K_DRAW, K_ADV = "13affine_kernel", "16add_noise_kernel", "12randn_kernel", \
    "16step_draw_kernel", "14advance_kernel"


def grid(items, cap=GRID_CAP):
    return max(1, min(cdiv(items, NT), cap))


def draw_items(n, B, row_elems, txt):
    return cdiv(n, 4) + (B * row_elems // 4 if txt else 0) + B


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS). For DDIM: the launch of
    sdmi_ddim_prev, then those of the device form. A sweep row repeats them per timestep / pair."""
    o = dict(options)
    if entry == DDPM:
        return [(K_DDPM, grid(dims[0]))] + ([(K_DEC, 1)] if o.get("dec") else [])
    if entry == DDIM:
        return [(K_DDIM, grid(dims[0])), (K_DDIM_DEV, grid(dims[0]))] + ([(K_DDIM_ADV, 1)] if o.get("adv") else [])
    if entry == AFF:
        return [(K_AFF, grid(dims[0]))]
    if entry == ADDN:
        return [(K_ADDN, grid(dims[0] * dims[1], ADDN_GRID_CAP))]
    if entry == RANDN:
        return [(K_RANDN, grid(cdiv(dims[0], 4)))] + ([(K_ADV, 1)] if o.get("adv") else [])
    assert entry == DRAW
    return [(K_DRAW, grid(draw_items(dims[0], dims[1], dims[2], o.get("txt", 1))))]


def draw_status(n, B, T, txt, text, empty, row_elems, align=(0, 0, 0), noise=1, t=1):
    """The status sdmi_step_draw returns before any launch (0: it launches). txt / text / empty / noise / t: present;
    align: the byte offsets of text, empty and txt from a 16-byte boundary."""
    if not noise or n <= 0 or not t or B <= 0 or T <= 0:
        return -1
    if txt and (not text or not empty or row_elems <= 0 or row_elems % 4 or any(a % 16 for a in align)):
        return -2
    return 0


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
BIG = 4096 * 256 + 77                 # the second turn of the grid-stride loop of a step kernel: 77 elements
BIG4 = 4 * 4096 * 256 + 3             # of the quad loops: one quad, three of its elements
EDGES = ((1, 1), (255, 1), (256, 1), (257, 2), (1027, 5))      # (n, grid)
DDIM_TS, DDIM_TP = (1, 11, 401, 801), (0, 1, 360, 760)
SEED_HI, OFF_HI = 2 ** 63 + 5, 2 ** 62 - 1
SEED_PAIRS = ((0, 0), (7, 1), (2 ** 32 + 7, 1), (7, 2 ** 32 + 1), (SEED_HI, OFF_HI))

ROWS = [
    # every t of each table, n = 67 per t: the seams of the clamp, specials in each operand, abar[t - 1], the last entry
    R(DDPM, (67,), (K_DDPM, 1), table="cond", sweep=1), R(DDPM, (67,), (K_DDPM, 1), table="uncond", sweep=1),
    R(DDPM, (67,), (K_DDPM, 1), table="syn", sweep=1),
    # one element, a block less one, a block, a block and one, five blocks with a ragged last one
    R(DDPM, (1,), (K_DDPM, 1), t=500), R(DDPM, (255,), (K_DDPM, 1), t=500), R(DDPM, (256,), (K_DDPM, 1), t=500),
    R(DDPM, (257,), (K_DDPM, 2), t=500), R(DDPM, (1027,), (K_DDPM, 5), t=500),
    R(DDPM, (BIG,), (K_DDPM, 4096), t=1),
    # the second output, no x0, in place (what the sample loop does), the decrement above and at zero, null noise
    R(DDPM, (257,), (K_DDPM, 2), t=500, prev2=1), R(DDPM, (257,), (K_DDPM, 2), t=999, x0=0),
    R(DDPM, (257,), (K_DDPM, 2), t=1, alias=1),
    R(DDPM, (257,), (K_DDPM, 2), (K_DEC, 1), t=5, dec=1), R(DDPM, (257,), (K_DDPM, 2), (K_DEC, 1), t=0, dec=1),
    R(DDPM, (257,), (K_DDPM, 2), t=0, z=0), R(DDPM, (257,), (K_DDPM, 2), t=300, z=0),
]
ROWS += [R(DDIM, (67,), (K_DDIM, 1), (K_DDIM_DEV, 1), table=tb, eta=eta, sweep=1)
         for tb in ("a", "b") for eta in (0.0, 0.5, 1.0)]
ROWS += [
    R(DDIM, (1,), (K_DDIM, 1), (K_DDIM_DEV, 1)), R(DDIM, (255,), (K_DDIM, 1), (K_DDIM_DEV, 1)),
    R(DDIM, (256,), (K_DDIM, 1), (K_DDIM_DEV, 1)), R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2)),
    R(DDIM, (1027,), (K_DDIM, 5), (K_DDIM_DEV, 5)), R(DDIM, (BIG,), (K_DDIM, 4096), (K_DDIM_DEV, 4096)),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), noise=0),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), out2=1), R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), dup=1),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), alias=1),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), (K_DDIM_ADV, 1), adv=1),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), (K_DDIM_ADV, 1), adv=1, idx=0),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), (K_DDIM_ADV, 1), adv=1, tdev=0),
    R(DDIM, (257,), (K_DDIM, 2), (K_DDIM_DEV, 2), tdev=0),
]
ROWS += [
    R(AFF, (67,), (K_AFF, 1), t=999), R(AFF, (67,), (K_AFF, 1), t=500), R(AFF, (67,), (K_AFF, 1), t=1),
    R(AFF, (67,), (K_AFF, 1), t=0), R(AFF, (67,), (K_AFF, 1), t=0, z=0),
    R(AFF, (1,), (K_AFF, 1), t=500), R(AFF, (255,), (K_AFF, 1), t=500), R(AFF, (256,), (K_AFF, 1), t=500),
    R(AFF, (257,), (K_AFF, 2), t=500), R(AFF, (1027,), (K_AFF, 5), t=500), R(AFF, (BIG,), (K_AFF, 4096), t=500),
]
ROWS += [
    R(ADDN, (1, 1), (K_ADDN, 1)), R(ADDN, (1, 7), (K_ADDN, 1)), R(ADDN, (1, 256), (K_ADDN, 1)),
    R(ADDN, (1, 1000), (K_ADDN, 4)),
    R(ADDN, (3, 1), (K_ADDN, 1)), R(ADDN, (3, 7), (K_ADDN, 1)), R(ADDN, (3, 256), (K_ADDN, 3)),
    R(ADDN, (3, 1000), (K_ADDN, 12)),
    R(ADDN, (5, 1), (K_ADDN, 1)), R(ADDN, (5, 7), (K_ADDN, 1)), R(ADDN, (5, 256), (K_ADDN, 5)),
    R(ADDN, (5, 1000), (K_ADDN, 20)),
    # past one trip of the capped grid of misc.hip (8192 workgroups), samples that straddle the turn
    R(ADDN, (3, 700001), (K_ADDN, 8192)),
]
ROWS += [
    # every tail of the last quad and a block boundary in quads, every word of seed and offset live
    R(RANDN, (1,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI), R(RANDN, (2,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI),
    R(RANDN, (3,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI), R(RANDN, (4,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI),
    R(RANDN, (5,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI), R(RANDN, (1023,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI),
    R(RANDN, (1024,), (K_RANDN, 1), seed=SEED_HI, off=OFF_HI), R(RANDN, (1025,), (K_RANDN, 2), seed=SEED_HI, off=OFF_HI),
    # the low-word twins and the pairs that differ from them in one high word
    R(RANDN, (1025,), (K_RANDN, 2), seed=0, off=0), R(RANDN, (1025,), (K_RANDN, 2), seed=7, off=1),
    R(RANDN, (1025,), (K_RANDN, 2), seed=2 ** 32 + 7, off=1), R(RANDN, (1025,), (K_RANDN, 2), seed=7, off=2 ** 32 + 1),
    R(RANDN, (5,), (K_RANDN, 1), (K_ADV, 1), seed=7, off=2 ** 32 + 1, adv=1),
    R(RANDN, (BIG4,), (K_RANDN, 4096), seed=7, off=2 ** 32 + 1),
]
ROWS += [
    R(DRAW, (1, 1, 0), (K_DRAW, 1), T=1, txt=0, keep=0, pt=0.1, pk=0.1),
    R(DRAW, (5, 3, 4), (K_DRAW, 1), T=1000, txt=1, keep=1, pt=0.1, pk=0.1),
    R(DRAW, (5, 3, 4), (K_DRAW, 1), T=1000, txt=1, keep=1, pt=0.0, pk=1.0),
    R(DRAW, (5, 3, 4), (K_DRAW, 1), T=1000, txt=1, keep=1, pt=1.0, pk=0.0),
    R(DRAW, (5, 3, 4), (K_DRAW, 1), T=2 ** 31 - 1, txt=1, keep=1, pt=("own", 1), pk=("own", 1)),
    R(DRAW, (1024, 1, 4), (K_DRAW, 2), T=2 ** 31 - 1, txt=1, keep=0, pt=0.1, pk=0.1),
    R(DRAW, (1021, 257, 8), (K_DRAW, 5), T=1000, txt=1, keep=1, pt=0.1, pk=0.1),
    R(DRAW, (1021, 257, 8), (K_DRAW, 5), T=1, txt=1, keep=1, pt=("own", 256), pk=("own", 256)),
    # the text and the sample segments fall in the second turn of the capped grid
    R(DRAW, (BIG4, 2, 8), (K_DRAW, 4096), T=1000, txt=1, keep=1, pt=("own", 0), pk=0.1),
]


def row_id(r):
    def s(v):
        return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{s(v)}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------
Table = collections.namedtuple("Table", "betas alphas abar s1m sa T")


def _gen(*key):
    return np.random.default_rng([int(k) % (2 ** 32) for k in key])


def _golden(name):
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, name + ".safetensors"))


@functools.lru_cache(maxsize=None)
def table(name):
    """A DDPM scheduler table as numpy.float32 arrays."""
    if name in ("cond", "uncond"):
        f = _golden(f"scheduler_{name}")
        g = lambda k: f[k].numpy().copy()  # noqa: E731
        return Table(g("betas"), g("alphas"), g("alpha_cum_prod"), g("sqrt_one_minus_alpha_cum_prod"),
                     g("sqrt_alpha_cum_prod"), 1000)
    assert name == "syn"
    T = 64
    abar = np.unique(_gen(11).uniform(0.01, 0.99, 4 * T).astype(f32))[::-1][:2 * T:2].copy()
    assert abar.size == T and bool((np.diff(abar) < 0).all())
    alphas = abar.copy()
    alphas[1:] = abar[1:] / abar[:-1]
    return Table(f32(1) - alphas, alphas, abar, np.sqrt(f32(1) - abar), np.sqrt(abar), T)


@functools.lru_cache(maxsize=None)
def ddim_table(name):
    """abar of a DDIM sampler: a, the golden table of beta (0.00085, 0.012); b, built here from beta (0.0001, 0.02)."""
    if name == "a":
        return _golden("samplers")["ddim_alpha_t_bar"].numpy().copy()
    assert name == "b"
    return torch.cumprod(1.0 - torch.linspace(0.0001, 0.02, 1000, dtype=torch.float32), dim=0).numpy().copy()


@functools.lru_cache(maxsize=None)
def affine_coeffs():
    f = _golden("samplers")
    return tuple(f[f"ddpm_{k}"].numpy().copy() for k in ("coeff_1", "coeff_2", "posterior_variance"))


def ddim_time_steps(T, steps, method):
    """DDIMSampler.forward's pairs (scheduler/linear_noise_scheduler.py:231-242), restated."""
    if method == "linear":
        ts = np.asarray(list(range(0, T, T // steps)))
    else:
        ts = (np.linspace(0, np.sqrt(T * 0.8), steps) ** 2).astype(np.int32)
    ts = ts + 1
    return ts, np.concatenate([[0], ts[:-1]])


@functools.lru_cache(maxsize=None)
def sweep_pairs():
    """(ts, tp) of the DDIM sweep rows: both methods complete, then (1, 0) and (999, 998)."""
    l, q = ddim_time_steps(1000, 50, "linear"), ddim_time_steps(1000, 50, "quadratic")
    ts = np.concatenate([l[0], q[0], [1, 999]]).astype(np.int64)
    tp = np.concatenate([l[1], q[1], [0, 998]]).astype(np.int64)
    return ts, tp


# ----------------------------------------------------------------------------------------------------------------
# the numpy.float32 models of the steps (and the same expressions in torch, for the CPU test)
# ----------------------------------------------------------------------------------------------------------------
def ddpm_model(tab, t, xt, eps, z):
    """sample_prev_timestep (:59-78) for rows of elements: t [R], xt / eps / z [R, n] float32 (z None: +0).
    Returns prev, the clamped x0 and the unclamped x0."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    z = np.zeros_like(xt) if z is None else z
    col = lambda a: a[t][:, None]  # noqa: E731
    with np.errstate(all="ignore"):
        x0u = (xt - col(tab.s1m) * eps) / np.sqrt(col(tab.abar))
        x0 = np.minimum(np.maximum(x0u, f32(-1.0)), f32(1.0))
        mean = xt - (col(tab.betas) * eps) / col(tab.s1m)
        mean = mean / np.sqrt(col(tab.alphas))
        abar_prev = tab.abar[np.maximum(t - 1, 0)][:, None]        # (unused where t == 0)
        variance = (f32(1) - abar_prev) / (f32(1.0) - col(tab.abar))
        variance = variance * col(tab.betas)
        sigma = np.sqrt(variance)
        prev = np.where((t > 0)[:, None], mean + sigma * z, mean)
    assert prev.dtype == f32 and x0.dtype == f32
    return prev, x0, x0u


def tsqrt(x):
    """The correctly rounded float32 square root of a torch tensor (through float64). The sqrt and the ** 0.5 of torch's
    CPU build are not correctly rounded on every host (with AVX-512 about 0.6 % of float32 arguments come out one ulp
    off), and the reference takes them only of table entries, never of data."""
    return torch.from_numpy(np.sqrt(np.atleast_1d(x.double().numpy()))).float().reshape(x.shape)


def ddpm_torch(tab, t, xt, eps, z):
    """The same lines in torch on the CPU for one t (0-dim table entries, as the reference indexes them)."""
    T = {k: torch.from_numpy(getattr(tab, k)) for k in ("betas", "alphas", "abar", "s1m")}
    xt, eps = torch.from_numpy(xt), torch.from_numpy(eps)
    x0 = (xt - (T["s1m"][t] * eps)) / tsqrt(T["abar"][t])
    x0 = torch.clamp(x0, -1., 1.)
    mean = xt - ((T["betas"][t]) * eps) / (T["s1m"][t])
    mean = mean / tsqrt(T["alphas"][t])
    if t == 0:
        return mean.numpy(), x0.numpy()
    variance = (1 - T["abar"][t - 1]) / (1.0 - T["abar"][t])
    variance = variance * T["betas"][t]
    sigma = tsqrt(variance)
    zz = torch.zeros_like(xt) if z is None else torch.from_numpy(z)
    return (mean + sigma * zz).numpy(), x0.numpy()


def ddim_coeffs(at, ap, eta):
    """(sigma, c1, c2, 1 - a_prev - sigma^2) of DDIMSampler.sample_one_step (:199-204) in float32; at, ap arrays."""
    at, ap, eta, one = np.asarray(at, dtype=f32), np.asarray(ap, dtype=f32), f32(eta), f32(1)
    with np.errstate(all="ignore"):
        sigma = eta * np.sqrt((one - ap) / (one - at) * (one - at / ap))
        c1 = np.sqrt(ap / at)
        inner = one - ap - sigma * sigma
        c2 = np.sqrt(inner) - np.sqrt((ap * (one - at)) / at)
    return sigma, c1, c2, inner


def ddim_model(at, ap, eta, x, e, noise):
    """x_{t-1} for rows of elements: at / ap [R], x / e / noise [R, n] float32 (noise None: +0)."""
    sigma, c1, c2, _ = (c.reshape(-1, 1) for c in ddim_coeffs(at, ap, eta))
    noise = np.zeros_like(x) if noise is None else noise
    with np.errstate(all="ignore"):
        out = c1 * x + c2 * e + sigma * noise
    assert out.dtype == f32
    return out


def ddim_torch(at, ap, eta, x, e, noise):
    """:199-206 in torch on the CPU for one pair, the table entries shaped (1, 1) as extract() leaves them."""
    alpha_t, alpha_t_prev = torch.tensor([[float(at)]], dtype=torch.float32), torch.tensor([[float(ap)]], dtype=torch.float32)
    x_t, epsilon_theta_t = torch.from_numpy(x).view(1, -1), torch.from_numpy(e).view(1, -1)
    epsilon_t = torch.zeros_like(x_t) if noise is None else torch.from_numpy(noise).view(1, -1)
    sigma_t = eta * tsqrt((1 - alpha_t_prev) / (1 - alpha_t) * (1 - alpha_t / alpha_t_prev))
    out = (tsqrt(alpha_t_prev / alpha_t) * x_t +
           (tsqrt(1 - alpha_t_prev - sigma_t ** 2) - tsqrt((alpha_t_prev * (1 - alpha_t)) / alpha_t)) *
           epsilon_theta_t + sigma_t * epsilon_t)
    return out.view(-1).numpy()


def affine_model(c1, c2, var, x, e, z):
    """DDPMSampler.sample_one_step (:118-134): (c1 x - c2 eps) + sqrt(var) z; z None: the reference's z = 0."""
    c1, c2, var = f32(c1), f32(c2), f32(var)
    z = np.zeros_like(x) if z is None else z
    with np.errstate(all="ignore"):
        out = (c1 * x - c2 * e) + np.sqrt(var) * z
    assert out.dtype == f32
    return out


def affine_torch(c1, c2, var, x, e, z):
    s = lambda v: torch.tensor([[float(v)]], dtype=torch.float32)  # noqa: E731
    x_t, epsilon_theta = torch.from_numpy(x).view(1, -1), torch.from_numpy(e).view(1, -1)
    mean = s(c1) * x_t - s(c2) * epsilon_theta
    zz = 0 if z is None else torch.from_numpy(z).view(1, -1)
    return (mean + tsqrt(s(var)) * zz).view(-1).numpy()


def add_noise_model(tab, t, x0, eps):
    """add_noise (:47-48): x0 / eps [B, per], t [B]."""
    t = np.asarray(t, dtype=np.int64)
    with np.errstate(all="ignore"):
        out = tab.sa[t][:, None] * x0 + tab.s1m[t][:, None] * eps
    assert out.dtype == f32
    return out


def add_noise_torch(tab, t, x0, eps):
    t = torch.as_tensor(np.asarray(t, dtype=np.int64))
    sa, s1 = torch.from_numpy(tab.sa)[t].reshape(-1, 1), torch.from_numpy(tab.s1m)[t].reshape(-1, 1)
    return (sa * torch.from_numpy(x0) + s1 * torch.from_numpy(eps)).numpy()


def same_bits(a, b):
    """numpy float32 arrays equal bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and bool((a.view(np.int32)[~na] == b.view(np.int32)[~nb]).all())


def differing(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))).sum())


# ----------------------------------------------------------------------------------------------------------------
# data of the step rows
# ----------------------------------------------------------------------------------------------------------------
SPECIALS = (0.0, -0.0, INF, -INF, NAN)
SEAM_OFFSETS = tuple(range(-8, 9))
SEAM_AT = {1.0: 16, -1.0: 16 + len(SEAM_OFFSETS)}        # the first element of each seam group


def _plant_specials(ops):
    """Operand k takes the five specials at elements 5 k .. 5 k + 4 (as far as n reaches); element 15 is x = -0,
    e = +0 (a -0 mean), z = 1."""
    n = ops[0].shape[-1]
    for k, a in enumerate(ops):
        for j, s in enumerate(SPECIALS):
            if 5 * k + j < n:
                a[..., 5 * k + j] = s
    if n > 15:
        ops[0][..., 15], ops[1][..., 15] = -0.0, 0.0
        if len(ops) > 2:
            ops[2][..., 15] = 1.0
    return ops


@functools.lru_cache(maxsize=8)
def step_case(n, key, rows=1, scale=1.0):
    """x, e, z [rows, n] float32: randn (e scaled) with the specials planted."""
    g = _gen(21, n, key, rows)
    x, e, z = (g.standard_normal((rows, n)).astype(f32) for _ in range(3))
    e *= f32(scale)
    return tuple(_plant_specials([x, e, z]))


def _ulp_step(x, k):
    """x moved k units in the last place (by magnitude; the offsets are symmetric)."""
    return (x.view(np.int32) + np.int32(k)).view(f32)


@functools.lru_cache(maxsize=3)
def ddpm_sweep_case(name):
    """t = 0 .. T - 1 and x, e, z [T, 67]: specials at 0 .. 14, then for +1 and for -1 seventeen neighbours of the x
    at which the unclamped x0 crosses the bound (e = sqrt(abar) r, so x stays of the size of sqrt(abar))."""
    tab = table(name)
    T = tab.T
    x, e, z = (a.copy() for a in step_case(67, {"cond": 1, "uncond": 2, "syn": 3}[name], rows=T, scale=0.9))
    g = _gen(22, T)
    sq, s1 = np.sqrt(tab.abar), tab.s1m
    for target, at in SEAM_AT.items():
        ev = (sq * (0.25 * g.standard_normal(T)).astype(f32)).astype(f32)
        xc = (f32(target) * sq + s1 * ev).astype(f32)
        for j, k in enumerate(SEAM_OFFSETS):
            x[:, at + j] = _ulp_step(xc, k)
            e[:, at + j] = ev
    return np.arange(T, dtype=np.int64), x, e, z


def ddpm_row_case(r):
    """(table, t [R], x, e, z [R, n]) of a DDPM row."""
    if opt(r, "sweep"):
        return (table(opt(r, "table")),) + ddpm_sweep_case(opt(r, "table"))
    n, t = r.dims[0], opt(r, "t")
    return (table("cond"), np.array([t], dtype=np.int64)) + step_case(n, 100 + t, scale=0.9)


DDIM_ETA, DDIM_IDX = 0.5, 3


def ddim_row_case(r):
    """(abar, ts [R], tp [R], eta, x, e, noise [R, n]) of a DDIM row: the pairs it steps through."""
    if opt(r, "sweep"):
        ts, tp = sweep_pairs()
        return (ddim_table(opt(r, "table")), ts, tp, opt(r, "eta")) + step_case(67, 40, rows=len(ts))
    i = opt(r, "idx", DDIM_IDX)
    ts, tp = np.array([DDIM_TS[i]], dtype=np.int64), np.array([DDIM_TP[i]], dtype=np.int64)
    return (ddim_table("a"), ts, tp, DDIM_ETA) + step_case(r.dims[0], 41)


def affine_row_case(r):
    c1, c2, var = affine_coeffs()
    t = opt(r, "t")
    return (c1[t], c2[t], var[t]) + step_case(r.dims[0], 42 + t)


ADDN_T = {1: {1: (999,), 7: (0,), 256: (500,), 1000: (999,)}, 3: (0, 999, 500), 5: (999, 0, 1, 500, 998)}


def addn_row_case(r):
    B, per = r.dims
    t = ADDN_T[B][per] if B == 1 else ADDN_T[B]
    g = _gen(23, B, per)
    x0, eps = (g.standard_normal(B * per).astype(f32) for _ in range(2))
    _plant_specials([x0, eps])
    return table("cond"), np.array(t, dtype=np.int64), x0.reshape(B, per), eps.reshape(B, per)


# ----------------------------------------------------------------------------------------------------------------
# Philox4x32-10 and what is drawn from it
# ----------------------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(counter, key, rounds=10, bump="key", swap_m=False):
    """Philox4x32 on four uint64 arrays of 32-bit words. bump = "counter" and swap_m are perturbed references."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1 = (PHILOX_M1, PHILOX_M0) if swap_m else (PHILOX_M0, PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(m0) * c0, np.uint64(m1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & MASK32
        if bump == "key":
            k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
        else:
            c0, c1 = (c0 + np.uint64(PHILOX_W0)) & MASK32, (c1 + np.uint64(PHILOX_W1)) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1)


def _words(q, seed, off, off_hi=True, **pert):
    q = np.asarray(q, dtype=np.uint64)
    lo, hi = off & 0xFFFFFFFF, (off >> 32) if off_hi else 0
    counter = (q & MASK32, q >> np.uint64(32), np.full(q.shape, lo, dtype=np.uint64), np.full(q.shape, hi, dtype=np.uint64))
    return philox(counter, (seed & 0xFFFFFFFF, seed >> 32), **pert)


@functools.lru_cache(maxsize=4)
def noise_words(seed, off, nq):
    """[nq, 4] uint64: the Philox block of every noise quad."""
    return _words(np.arange(nq, dtype=np.uint64), seed, off)


def perturbed_noise_words(seed, off, nq, **pert):
    return _words(np.arange(nq, dtype=np.uint64), seed, off, **pert)


@functools.lru_cache(maxsize=16)
def sample_words(seed, off, B):
    """[B, 4] uint64: sample b's block, quad index 2^40 + b."""
    return _words(np.uint64(2 ** 40) + np.arange(B, dtype=np.uint64), seed, off)


TWO_PI_F32 = float(f32(6.28318530717958647692))


def _uniforms(words, shift=8, plus1=True, scale=U24, pairs=((0, 1), (2, 3))):
    a = np.stack([words[:, p[0]] for p in pairs], axis=1)
    b = np.stack([words[:, p[1]] for p in pairs], axis=1)
    u1 = ((a >> np.uint64(shift)) + np.uint64(1 if plus1 else 0)).astype(np.float64) * scale
    u2 = (b >> np.uint64(shift)).astype(np.float64) * scale
    return u1, u2


def noise_reference(words, swap=False, **pert):
    """(z, rad, theta) [nq, 4] float64. swap and the keywords of _uniforms are perturbed references."""
    u1, u2 = _uniforms(words, **pert)
    with np.errstate(all="ignore"):
        rad = np.sqrt(-2.0 * np.log(u1))
        theta = TWO_PI_F32 * u2
        c, s = rad * np.cos(theta), rad * np.sin(theta)
    if swap:
        c, s = s, c
    il = lambda p, q: np.stack([p[:, 0], q[:, 0], p[:, 1], q[:, 1]], axis=1)  # noqa: E731
    return il(c, s), il(rad, rad), il(theta, theta)


def noise_emulation(words):
    """The four lines in float32: logf, sinf and cosf as the rounded float64 function, the rest in numpy.float32."""
    u1, u2 = _uniforms(words)
    u1, u2 = u1.astype(f32), u2.astype(f32)                     # exact: 24-bit integers times 2^-24
    with np.errstate(all="ignore"):
        rad = np.sqrt(f32(-2.0) * np.log(u1.astype(np.float64)).astype(f32))
        ang = (f32(TWO_PI_F32) * u2).astype(np.float64)
        c, s = rad * np.cos(ang).astype(f32), rad * np.sin(ang).astype(f32)
    assert c.dtype == f32
    return np.stack([c[:, 0], s[:, 0], c[:, 1], s[:, 1]], axis=1).astype(np.float64)


def noise_bound(rad, theta, K=None):
    return (K_Z if K is None else K) * U24 * rad * (1.0 + theta)


def worst_ratio(got, ref, lim):
    """max(err / bound); an error where the bound is zero, a NaN or an inf counts as infinite."""
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err <= lim, np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), 0.0), np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), INF))
        r = np.where(np.isfinite(got) & np.isfinite(err), r, INF)
    return float(r.max()) if r.size else 0.0


def draw_reference(seed, off, B, T, p_text, p_keep):
    """(t [B] int64, drop [B] bool, keep [B] float32, u_text, u_keep [B] float32), exact from the integers."""
    w = sample_words(seed, off, B)
    t = ((w[:, 0] * np.uint64(T)) >> np.uint64(32)).astype(np.int64)
    ut = (w[:, 1] >> np.uint64(8)).astype(f32) * f32(U24)
    uk = (w[:, 2] >> np.uint64(8)).astype(f32) * f32(U24)
    return t, ut < f32(p_text), (uk > f32(p_keep)).astype(f32), ut, uk


DRAW_SEED, DRAW_OFF = SEED_HI, OFF_HI


def draw_probabilities(r, seed=DRAW_SEED, off=DRAW_OFF):
    """(p_text, p_keep) of a DRAW row as the float32 values passed; ("own", b) is sample b's own uniform."""
    B = r.dims[1]
    _, _, _, ut, uk = draw_reference(seed, off, B, 1, 0.0, 0.0)
    pt, pk = opt(r, "pt"), opt(r, "pk")
    pt = float(ut[pt[1]]) if isinstance(pt, tuple) else float(f32(pt))
    pk = float(uk[pk[1]]) if isinstance(pk, tuple) else float(f32(pk))
    return pt, pk


def text_case(B, row_elems):
    """text [B, row_elems] and empty [row_elems] float32, no two rows alike, specials in row 0 and in empty."""
    g = _gen(24, B, row_elems)
    text, empty = g.standard_normal((B, row_elems)).astype(f32), g.standard_normal(row_elems).astype(f32)
    text[0, :3], empty[:2] = (-0.0, INF, NAN), (-0.0, -INF)
    return text, empty


# ----------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ----------------------------------------------------------------------------------------------------------------
class Words:
    """k 64-bit device words as an int64 view of a NaN-filled fp32 buffer (64 floats in front, 256 behind)."""

    def __init__(self, values, device="cuda"):
        values = [int(v) - 2 ** 64 if int(v) >= 2 ** 63 else int(v) for v in values]
        self.k = len(values)
        self.win = Win(2 * self.k, device)
        self.buf, self.front = self.win.buf, self.win.front
        self.data = self.win.data.view(torch.int64)
        self.data.copy_(torch.tensor(values, dtype=torch.int64))

    def get(self):
        return [int(v) % 2 ** 64 for v in self.data.cpu().tolist()]

    def span(self, i, count=1):
        """The writable range of words i .. i + count - 1 in the units of Guard (floats)."""
        return (2 * i, 2 * (i + count))


def dev(a, device="cuda", off=0):
    """A numpy float32 array as a guarded window on the device."""
    a = np.ascontiguousarray(a, dtype=f32)
    return Win(a.size, device, off=off).put(torch.from_numpy(a))


def host(w, *shape):
    """The window's float32 contents as a numpy array."""
    a = w.data.cpu().numpy().copy()
    return a.reshape(*shape) if shape else a
