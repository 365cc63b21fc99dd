"""The declared test matrix of the DiT row and patch-layout kernels (csrc/dit.hip) and the helpers its exact tests
share.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`. The expected launches -- a
fragment of the mangled kernel name with its template argument, and the grid -- are written by hand. The host rules of
dit.hip that decide the grids are restated below, also by hand: the forward runs ceil(rows / 4) workgroups (one wave
per token row); sdmi_ln_chunk_rows is the largest of 8, 4, 2 dividing N, else 1, and the backward runs rows / R
workgroups; grid_for is min(ceil(total / 256), 8192); sdmi_mse_patch launches min(ceil(rows ld / 256), 1024)
workgroups and then one sum_rows_kernel. tests/test_dit_matrix_cpu.py checks rows against rules and that no row can
be removed; tests/test_dit_exact_gpu.py that the library launches what the rows say.

Every tensor of every row has at most 2^21 elements. grid_for caps only beyond that size (8192 * 256 = 2^21 elements):
that branch has no row. The 1024-workgroup cap of sdmi_mse_patch is reached by the row (5, 4, 128, 128, 2), ld = 16:
327680 elements, 1280 > 1024, so the grid-stride loop runs and all 1024 partials are written.

Entry points and dims: LN_FWD sdmi_ln_mod_fwd (B, N, C) with f32 (the stream type, the template argument), res (none /
v / gate: the residual added before the statistics) and mod (shift and scale given); LN_BWD sdmi_ln_mod_bwd (B, N, C)
with f32, mod (none: scale absent, plain LayerNorm as sdmi/leaf.py calls it; both / psh / psc / neither: scale present
and which partial pointers are), dres, gate (with v, dv, pg) and dx16; FINALIZE sdmi_mod_finalize (B, chunks, W);
TO_NCHW sdmi_tokens_to_nchw, TO_TOKENS sdmi_nchw_to_tokens_bf16 and MSE sdmi_mse_patch on (B, C, H, W, p) with pad
(ld = K + pad, K = p p C), f32 (src_f32), gs (val / dev: gscale by value or through gscale_dev) and grad. pred and
grad of sdmi_mse_patch share the one ld. nchw_to_tokens and mse_patch size their grids by ld, so the pad is part of
the row; the row kernels and finalize run every row in a contiguous layout and in a windows layout in which every
stride and column offset differs (multiples of 8 elements, 16-byte aligned pointers, as vec_ok demands; finalize's
scalar accesses get odd ones).

Data, two families. References are float64 on the CPU, computed from the stored inputs; bf16 operands are exact in
bf16; the fp32-stream operands (x, dres) of the soft family are genuine fp32 values.

  exact  x integers in [-8, 8]; v, dy and dres integers in [-4, 4]; gate and scale signed powers of two (2^-2 .. 2^2,
         scale never -1); shift a multiple of 1/8. x + gate v is a multiple of 1/4 below 32: exact in bf16, so both
         streams normalise the same numbers. Every sum of x, dy and of the finalize / MSE terms is an integer or a
         dyadic number below 2^24: one bit pattern in any summation order. With 3 token rows or more the last row is
         constant (x = 2, v = 0: variance exactly 0, rstd = 1 / sqrt(eps), y == shift) and the middle row takes values
         in {1, 1 + 2^-7} (variance <= 1.6e-5: eps = 1e-6 decides its rstd); with 2 rows only the constant one, with
         1 row none. Bitwise: xo, psh, mean where C is a power of two (within 2 ulp otherwise: inv_c = 1.0f / C is
         rounded), finalize, the layouts, the MSE loss fl(S fl(1 / n)) with S the exact sum, and grad where n and
         gscale are powers of two.
  soft   x = 2 randn + 0.5 (rounded to bf16 on the bf16 stream), v, dy = bf16(randn), dres = randn, the modulation
         bf16(0.5 randn). The last row has a large mean (100 + randn), the middle row is quiet (2^-6 randn + 1).

Rounding points of the kernels and the bounds derived from them (u = 2^-24; 2^-8 is the bf16 unit roundoff, the
repository's convention; K = K_SUM):

  xo     x + g v: the product of two bf16 values is exact in fp32, one fp32 rounding follows, then one bf16 rounding
         on the bf16 stream. Bitwise fma32(g, v, x) [RNE to bf16] in both families. Everything downstream is referenced
         on the kernel's own xo.
  mean   per-lane sequential sum of 8, the butterfly wave_sum, times the rounded 1 / C:
         |mean - ref| <= 2^-23 |ref| + K u E|x|.
  rstd   q = sum (x - mu)^2 on the kernel's fp32 mu, times inv_c, plus eps, rsqrtf:
         |rstd - ref| <= rstd (2^-22 + dvar / (2 (var + eps))), dvar = K u (E (x - mean)^2 + eps).
  y      bf16((x - mu) rs (1 + sc) + sh): |y - ref| <= 2^-8 |ref| + 2 K u (|xhat (1 + sc)| + |sh|), ref in float64 on
         the kernel's own mean and rstd.
  dx     xhat and dxh = dy (1 + sc) in fp32, s1 and s2 wave sums times inv_c, dx = dres + rs (dxh - s1 - xhat s2),
         rounded to bf16 on the bf16 stream: |dx - ref| <= [2^-8 |ref|] + K u (|dres| + rstd (|dxh| + E|dxh| +
         |xhat| E|dxh xhat|)). dx16 is bitwise bf16(dx as stored), dv bitwise bf16(fl32(g dx as stored)).
  parts  psh, psc, pg sum dy, dy xhat, dx_stored v over the chunk's rows r = wave, wave + 4, .. and then over waves:
         |p - ref| <= K u sum |term|.
  final  chunk order in fp32, then bf16: 2^-8 |ref| + K u sum |partial|.
  mse    |loss - ref| <= K u ref; grad = bf16(2 d / n gscale): 2^-8 |ref| + 4 u |ref|.

K_SUM is measured, not chosen: tests/test_dit_matrix_cpu.py runs an fp32 emulation of this arithmetic in two orders --
the kernel's (sequential 8, butterfly, waves in order; threads, waves and workgroups in order for the loss) and
pairwise -- on every soft row and measures max |fp32 value - float64 ref| / (u T), T the sum of absolute values of
the bound (for mean the excess over 2^-23 |ref|; for rstd the variance q inv_c + eps against dvar; values before
their bf16 rounding). Accumulating fmas are modelled as a rounded product that is then added, one rounding more per
term than the kernel. The larger of the two orders reached 0.58 (mean), 3.77 (variance), 1.34 (y), 1.76 (dx), 0.46
(psh: sums of bf16 values are nearly exact in fp32), 2.95 (psc), 2.91 (pg), 2.00 (finalize) and 1.94 (loss); the
largest over all rows and quantities is 3.77. The GPU's rsqrtf and its contraction choices are a third variant, so the
constant is twice that, rounded: 8. The CPU test asserts that the emulation stays within K_SUM / 2, that K_SUM is at
most 3 times the largest ratio, and that each perturbed reference leaves its bound.

Measured on an MI355X, max(err / bound) over all rows and layouts, exact family / soft family: mean 0.611 / 0.231, rstd
0.298 / 0.193, y 0.995 / 0.996, dx 0.996 / 0.996, psh 0 / 0.042, psc 0.294 / 0.323, pg 0.187 / 0.319, finalize 0.996 /
0.969, loss 0.138 / 0.242, grad 0.875 / 0.996 (the values near 1 are the bf16 rounding of the output, whose half ulp
reaches 2^-8 |ref| just above a power of two); xo, dx16, dv, the layouts and the zero pad columns bitwise. No row found
a defect in dit.hip.

Guards: every operand and output is a column window of a buffer filled with a NaN bit pattern (front pad, pad
columns, rows past the end); mean, rstd, the partial workspace, loss, gscale_dev, the NCHW images and the mse
workspace sit between NaN pads. A Guard asserts that only the declared windows change, bit for bit: that covers pad
columns, rows past the end, inputs, the columns W .. ws_ld of the partial rows, the partial rows of an absent psh, psc
or pg, and the mse workspace beyond the partials written. The pad columns of nchw_to_tokens and of mse_patch's grad
(K <= col < ld) are written and must be exactly zero."""
import collections
import functools

import numpy as np
import torch

from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401  (shared with the attention tests)
from tests.norm_matrix import (CONTIGUOUS, WINDOWS, Flat, Guard, bf16, bits, cdiv, fma32, is_bf16, ptr,  # noqa: F401
                               sum32, ulp32)

LN_FWD, LN_BWD, FINALIZE, TO_NCHW, TO_TOKENS, MSE = "ln_fwd", "ln_bwd", "finalize", "to_nchw", "to_tokens", "mse"
Row = collections.namedtuple("Row", "entry dims launches opt")
EPS = float(np.float32(1e-6))
U24 = 2.0 ** -24
K_SUM = 8.0
CAP = 2 ** 21


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/dit.hip, restated
# ----------------------------------------------------------------------------------------------------------------
NT = 256
WAVES = 4
MSE_CAP = 1024


def chunk_rows(N):
    """sdmi_ln_chunk_rows: the largest of 8, 4, 2 dividing N, else 1."""
    for r in (8, 4, 2):
        if N % r == 0:
            return r
    return 1


def grid_for(total):
    return min(cdiv(total, 256), 8192)


def fwd_name(f32):
    return f"ln_mod_fwd_kernelILb{int(f32)}EE"


def bwd_name(f32):
    return f"ln_mod_bwd_kernelILb{int(f32)}EE"


def patch_dims(B, C, H, W, p):
    """(token rows, K) of the '(nh nw) (ph pw c)' layout."""
    return B * (H // p) * (W // p), p * p * C


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    o = dict(options)
    if entry == LN_FWD:
        B, N, C = dims
        return [(fwd_name(o["f32"]), cdiv(B * N, WAVES))]
    if entry == LN_BWD:
        B, N, C = dims
        return [(bwd_name(o["f32"]), B * N // chunk_rows(N))]
    if entry == FINALIZE:
        B, chunks, W = dims
        return [("mod_finalize_kernel", grid_for(B * W))]
    rows, K = patch_dims(*dims)
    if entry == TO_NCHW:
        return [("tokens_to_nchw_kernel", grid_for(rows * K))]
    if entry == TO_TOKENS:
        return [("nchw_to_tokens_kernel", grid_for(rows * (K + o["pad"])))]
    assert entry == MSE
    return [("mse_patch_kernel", min(cdiv(rows * (K + o["pad"]), NT), MSE_CAP)), ("sum_rows_kernel", 1)]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
# sdmi_ln_mod_fwd: (B, N, C, res, mod, workgroups) per stream type. (1, 1) leaves three waves of the only workgroup
# without a row; (3, 1), (2, 3) and (2, 5) change the modulation row inside a workgroup and end in a ragged workgroup;
# (2, 64) is 32 full workgroups. C = 8 has one lane on, 504 has 63, 512 all 64; 288 is the bench configuration. All
# 12 combinations of stream, residual and modulation occur, each on a ragged shape.
FWD = {
    0: [(1, 1, 8, "none", 1, 1), (3, 1, 64, "v", 0, 1), (2, 3, 96, "gate", 1, 2), (2, 5, 504, "gate", 0, 3),
        (2, 64, 288, "gate", 1, 32), (2, 5, 512, "none", 0, 3), (2, 3, 288, "v", 1, 2)],
    1: [(1, 1, 8, "v", 1, 1), (3, 1, 64, "gate", 0, 1), (2, 3, 96, "none", 1, 2), (2, 5, 504, "none", 0, 3),
        (2, 64, 288, "v", 0, 32), (2, 5, 512, "gate", 1, 3), (2, 3, 288, "v", 0, 2)],
}
ROWS = [R(LN_FWD, (B, N, C), (fwd_name(f), wg), f32=f, res=res, mod=mod)
        for f in (0, 1) for B, N, C, res, mod, wg in FWD[f]]
# sdmi_ln_mod_bwd: (B, N, C, mod, dres, gate, dx16, workgroups) per stream type. N = 1, 2, 6, 4, 12, 8, 24, 7 is
# R = 1, 2, 2, 4, 4, 8, 8, 1 with 1, 1, 3, 1, 3, 1, 3, 7 chunks per sample; with R < 4 some waves have no row, with
# R = 8 every wave walks two.
BWD = {
    0: [(1, 1, 8, "none", 0, 0, 0, 1), (2, 2, 64, "both", 1, 1, 1, 2), (3, 6, 96, "psh", 1, 0, 0, 9),
        (2, 4, 288, "psc", 0, 1, 0, 2), (1, 12, 504, "neither", 1, 1, 1, 3), (2, 8, 512, "both", 0, 0, 1, 2),
        (3, 24, 288, "both", 1, 1, 0, 9), (2, 7, 96, "both", 1, 1, 0, 14)],
    1: [(1, 1, 8, "both", 1, 1, 1, 1), (2, 2, 64, "none", 1, 0, 1, 2), (3, 6, 96, "neither", 0, 1, 0, 9),
        (2, 4, 288, "psh", 1, 1, 1, 2), (1, 12, 504, "psc", 1, 0, 0, 3), (2, 8, 512, "both", 1, 1, 0, 2),
        (3, 24, 64, "none", 0, 0, 0, 9), (2, 7, 504, "both", 0, 1, 1, 14)],
}
ROWS += [R(LN_BWD, (B, N, C), (bwd_name(f), wg), f32=f, mod=mod, dres=dres, gate=gate, dx16=dx16)
         for f in (0, 1) for B, N, C, mod, dres, gate, dx16, wg in BWD[f]]
# sdmi_mod_finalize: 9 and 7 chunks exercise the remainder of the 8-way unroll; 1, 1, 4 and 7 workgroups
ROWS += [
    R(FINALIZE, (1, 1, 8), ("mod_finalize_kernel", 1)),
    R(FINALIZE, (2, 8, 96), ("mod_finalize_kernel", 1)),
    R(FINALIZE, (3, 9, 288), ("mod_finalize_kernel", 4)),
    R(FINALIZE, (2, 7, 864), ("mod_finalize_kernel", 7)),
]
# the patch layout: ((B, C, H, W, p), workgroups of tokens_to_nchw, of nchw_to_tokens / mse_patch at ld = K, at
# ld = K + 3). One element; the square shape of tests/test_dit_gpu.py; H < W and H > W; p = 1 and p = 4; C = 5.
PATCH = [
    ((1, 1, 1, 1, 1), 1, 1, 1),
    ((2, 4, 8, 8, 2), 2, 2, 3),
    ((2, 3, 4, 6, 2), 1, 1, 1),
    ((3, 4, 6, 4, 1), 2, 2, 2),
    ((1, 2, 8, 12, 4), 1, 1, 1),
    ((2, 5, 6, 10, 2), 3, 3, 3),
]
ROWS += [R(TO_NCHW, d, ("tokens_to_nchw_kernel", g), f32=f, pad=pad) for d, g, _, _ in PATCH for f in (0, 1)
         for pad in (0, 3)]
ROWS += [R(TO_TOKENS, d, ("nchw_to_tokens_kernel", (g0, g3)[pad > 0]), pad=pad) for d, _, g0, g3 in PATCH
         for pad in (0, 3)]
# sdmi_mse_patch: per shape both ld; gscale by value / through gscale_dev and grad present / null in all four pairs
MSE_OPT = {0: ("val", 1), 1: ("dev", 1), 2: ("val", 0), 3: ("dev", 0)}
ROWS += [R(MSE, d, ("mse_patch_kernel", (g0, g3)[pad > 0]), ("sum_rows_kernel", 1), pad=pad,
           gs=MSE_OPT[(i + (pad > 0)) % 4][0], grad=MSE_OPT[(i + (pad > 0)) % 4][1])
         for i, (d, _, g0, g3) in enumerate(PATCH) for pad in (0, 3)]
# the capped grid: 327680 elements on 1024 workgroups, 256 of which run a second grid-stride iteration
ROWS += [R(MSE, (5, 4, 128, 128, 2), ("mse_patch_kernel", 1024), ("sum_rows_kernel", 1), pad=0, gs="val", grad=1)]


def row_id(r):
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{v}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# data (CPU, no library call): float64 tensors holding values exact in the stored type
# ----------------------------------------------------------------------------------------------------------------
def special_rows(rows):
    """(first, second) special token row of a case: the last and the middle one; with two rows only the first kind,
    with one row none, so that an ordinary row always remains."""
    if rows >= 3:
        return rows - 1, rows // 2
    return (1, None) if rows == 2 else (None, None)


def _ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _pow2(gen, *shape):
    """Signed powers of two 2^-2 .. 2^2 without +-1 (1 + scale stays away from 0)."""
    e = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=gen)].double()
    return (_ri(gen, 0, 1, *shape) * 2 - 1) * 2.0 ** e


@functools.lru_cache(maxsize=None)
def ln_case(kind, B, N, C, f32=0):
    """One LayerNorm case: x, v, dy, dres [B * N][C], shift, scale, gate [B][C]. The exact family is the same numbers
    on both streams."""
    rows = B * N
    s1, s2 = special_rows(rows)
    if kind == "exact":
        gen = torch.Generator().manual_seed(3000 + 7 * rows + C)
        x, v = _ri(gen, -8, 8, rows, C), _ri(gen, -4, 4, rows, C)
        dy, dres = _ri(gen, -4, 4, rows, C), _ri(gen, -4, 4, rows, C)
        if s1 is not None:
            x[s1], v[s1] = 2.0, 0.0
        if s2 is not None:
            b = _ri(gen, 0, 1, C)
            b[0], b[-1] = 0.0, 1.0
            x[s2], v[s2] = 1.0 + 2.0 ** -7 * b, 0.0
        shift, scale, gate = _ri(gen, -16, 16, B, C) / 8, _pow2(gen, B, C), _pow2(gen, B, C)
        return dict(kind=kind, B=B, N=N, C=C, f32=0, x=x, v=v, dy=dy, dres=dres, shift=shift, scale=scale, gate=gate,
                    const=s1, near=s2)
    gen = torch.Generator().manual_seed(4000 + 7 * rows + C + 100000 * f32)
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    stream = (lambda t: t.float().double()) if f32 else bf16
    x = rn(rows, C) * 2 + 0.5
    if s1 is not None:
        x[s1] = 100.0 + rn(C)
    if s2 is not None:
        x[s2] = 2.0 ** -6 * rn(C) + 1.0
    return dict(kind=kind, B=B, N=N, C=C, f32=f32, x=stream(x), v=bf16(rn(rows, C)), dy=bf16(rn(rows, C)),
                dres=stream(rn(rows, C)), shift=bf16(0.5 * rn(B, C)), scale=bf16(0.5 * rn(B, C)),
                gate=bf16(0.5 * rn(B, C)), loud=s1, quiet=s2)


@functools.lru_cache(maxsize=None)
def finalize_case(kind, B, chunks, W):
    """Partial rows [B][chunks][W] as fp32 values: integers in [-4096, 4096] (any sum of 9 is exact), or randn."""
    gen = torch.Generator().manual_seed(5000 + B * chunks + W)
    if kind == "exact":
        return _ri(gen, -4096, 4096, B, chunks, W)
    return torch.randn((B, chunks, W), generator=gen, dtype=torch.float64).float().double()


@functools.lru_cache(maxsize=None)
def patch_case(kind, B, C, H, W, p):
    """img, target NCHW fp32 and pred (token layout, fp32): integers in [-3, 3] (d^2 <= 36, 327680 of them below
    2^24), or randn."""
    gen = torch.Generator().manual_seed(6000 + B * C * H * W + p)
    rows, K = patch_dims(B, C, H, W, p)
    if kind == "exact":
        return dict(kind=kind, img=_ri(gen, -8, 8, B, C, H, W), target=_ri(gen, -3, 3, B, C, H, W),
                    pred=_ri(gen, -3, 3, rows, K), gscale=4.0)
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).float().double()  # noqa: E731
    return dict(kind=kind, img=rn(B, C, H, W), target=rn(B, C, H, W), pred=rn(rows, K),
                gscale=float(np.float32(1.7)))


# ----------------------------------------------------------------------------------------------------------------
# references (float64) and bounds
# ----------------------------------------------------------------------------------------------------------------
def per_row(t, N):
    """[B][C] -> [B * N][C]."""
    return t.repeat_interleave(N, 0)


def is_pow2(n):
    return n & (n - 1) == 0


def xo_reference(c, res, f32, ignore_gate=False):
    """The gated residual as the kernel stores it, bitwise: fma32(g, v, x), rounded to bf16 on the bf16 stream."""
    if res == "none":
        return c["x"]
    g = per_row(c["gate"], c["N"]) if (res == "gate" and not ignore_gate) else torch.ones_like(c["x"])
    xo = fma32(g.float(), c["v"].float(), c["x"].float()).double()
    return xo if f32 else bf16(xo)


def xo_unrounded(c, res):
    if res == "none":
        return c["x"]
    g = per_row(c["gate"], c["N"]) if res == "gate" else torch.ones_like(c["x"])
    return c["x"] + g * c["v"]


def row_stats(x, eps=EPS, ddof=0, div=None):
    """mean, var, rstd [rows] in float64 and E|x|; `ddof` = 1 divides the variance by C - 1, `div` replaces C in both
    statistics."""
    C = x.shape[1]
    d = float(div or C)
    mean = x.sum(1) / d
    var = ((x - mean[:, None]) ** 2).sum(1) / (d - ddof)
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), eabs=x.abs().sum(1) / C)


def stats_bounds(kind, C, st, K=None):
    """Allowed |mean - ref| and |rstd - ref| [rows] (docstring: mean, rstd)."""
    K = K_SUM if K is None else K
    if kind == "exact":
        bm = torch.zeros_like(st["mean"]) if is_pow2(C) else 2 * ulp32(st["mean"]) * (st["mean"] != 0)
    else:
        bm = 2.0 ** -23 * st["mean"].abs() + K * U24 * st["eabs"]
    dvar = K * U24 * (st["var"] + EPS)
    return bm, st["rstd"] * (2.0 ** -22 + dvar / (2 * (st["var"] + EPS)))


def mod_rows(c, N=None, neighbour=False):
    """Row index of the modulation table per token row; `neighbour`: the first token of every sample but the first
    reads the previous sample's row."""
    N = N or c["N"]
    b = torch.arange(c["B"] * N) // N
    if neighbour:
        first = (torch.arange(c["B"] * N) % N == 0) & (b > 0)
        b = b - first.long()
    return b


def y_reference(c, xo, mean, rstd, mod, K=None, neighbour=False, scale_only=False):
    """ref = xhat (1 + sc) + sh on the given statistics and the allowed |y - ref| (docstring: y)."""
    K = K_SUM if K is None else K
    xh = (xo - mean[:, None]) * rstd[:, None]
    if mod:
        b = mod_rows(c, neighbour=neighbour)
        sc, sh = c["scale"][b], c["shift"][b]
    else:
        sc = sh = torch.zeros_like(xo)
    a = xh * (sc if scale_only else 1 + sc)
    return a + sh, 2.0 ** -8 * (a + sh).abs() + 2 * K * U24 * (a.abs() + sh.abs()), 2 * (a.abs() + sh.abs())


def host_stats(x):
    """mean and rstd as the backward rows get them: float64 statistics rounded once to fp32."""
    st = row_stats(x)
    return st["mean"].float().double(), st["rstd"].float().double()


def bwd_reference(c, mean, rstd, mod, dres, drop_s1=False, drop_s2=False, s2_ddof=0, drop_dres=False):
    """dx in float64 on the given statistics, the sum of absolute values T that scales its bound, xhat and dxh."""
    x, dy, C = c["x"], c["dy"], c["C"]
    xh = (x - mean[:, None]) * rstd[:, None]
    sc = per_row(c["scale"], c["N"]) if mod != "none" else torch.zeros_like(x)
    dxh = dy * (1 + sc)
    s1 = dxh.sum(1, keepdim=True) / C
    s2 = (dxh * xh).sum(1, keepdim=True) / (C - s2_ddof)
    rr = c["dres"] if (dres and not drop_dres) else torch.zeros_like(x)
    dx = rr + rstd[:, None] * (dxh - (0 if drop_s1 else s1) - (0 if drop_s2 else xh * s2))
    T = rr.abs() + rstd[:, None] * (dxh.abs() + dxh.abs().mean(1, keepdim=True) +
                                    xh.abs() * (dxh * xh).abs().mean(1, keepdim=True))
    return dict(dx=dx, T=T, xh=xh, dxh=dxh)


def dx_bound(ref, T, f32, K=None):
    K = K_SUM if K is None else K
    return K * U24 * T + (0.0 if f32 else 2.0 ** -8 * ref.abs())


def chunk_sums(terms, c, weights=None):
    """[B * chunks][C] sums of `terms` [rows][C] over each chunk of R token rows, and of their absolute values;
    `weights` [rows] counts token rows (2: doubled, 0: omitted)."""
    Rr = chunk_rows(c["N"])
    w = torch.ones(terms.shape[0], dtype=torch.float64) if weights is None else weights.double()
    t = (terms * w[:, None]).view(-1, Rr, terms.shape[1])
    return t.sum(1), terms.abs().view(-1, Rr, terms.shape[1]).sum(1)


def sum_bound(T, K=None, ref=None):
    K = K_SUM if K is None else K
    return K * U24 * T + (2.0 ** -8 * ref.abs() if ref is not None else 0.0)


def dv_reference(c, dx_stored):
    """bf16(fl32(g dx as stored)), bitwise."""
    return bf16((per_row(c["gate"], c["N"]) * dx_stored).float().double())


def finalize_reference(ws, skip=None):
    """[B][W] chunk sums of [B][chunks][W], and of the absolute values; `skip` omits one chunk."""
    keep = [k for k in range(ws.shape[1]) if k != skip]
    return ws[:, keep].sum(1), ws.abs().sum(1)


def tokens_of(img, p, swap_taps=False):
    """NCHW [B][C][H][W] -> '(nh nw) (ph pw c)' tokens [B * N][p p C]; `swap_taps` exchanges ph and pw."""
    B, C, H, W = img.shape
    t = img.view(B, C, H // p, p, W // p, p)
    t = t.permute(0, 2, 4, 5, 3, 1) if swap_taps else t.permute(0, 2, 4, 3, 5, 1)
    return t.reshape(B * (H // p) * (W // p), p * p * C)


def nchw_index(rows, K, C, H, W, p):
    """The index map of dit.hip restated: flat NCHW index of token element (row, col), [rows][K]."""
    row, col = torch.arange(rows)[:, None], torch.arange(K)[None, :]
    nw_cnt = W // p
    N = (H // p) * nw_cnt
    b, n = row // N, row % N
    nh, nw = n // nw_cnt, n % nw_cnt
    tap, ch = col // C, col % C
    ph, pw = tap // p, tap % p
    return ((b * C + ch) * H + nh * p + ph) * W + nw * p + pw


def mse_reference(c, dims, by_tokens=False):
    """loss, the exact sum S of d^2, n, and grad / gscale-free factor 2 d / n [rows][K] in float64."""
    B, C, H, W, p = dims
    d = c["pred"] - tokens_of(c["target"], p)
    S = (d * d).sum()
    n = float(patch_dims(*dims)[0] if by_tokens else B * C * H * W)
    return dict(S=S, n=n, loss=S / n, grad=2 * d / n * c["gscale"], d=d)


def grad_bound(ref):
    return 2.0 ** -8 * ref.abs() + 4 * U24 * ref.abs()


# ----------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' arithmetic in two summation orders (CPU, torch): "kernel" and "pair"
# ----------------------------------------------------------------------------------------------------------------
ORDERS = ("kernel", "pair")


def butterfly32(t):
    """wave_sum over the last dim of 64: lane l adds lane l ^ 32, then ^ 16, .. ^ 1 (every lane ends with the same
    bits, addition being commutative)."""
    assert t.shape[-1] == 64 and t.dtype == torch.float32
    for o in (32, 16, 8, 4, 2, 1):
        t = t[..., :o] + t[..., o:2 * o]
    return t[..., 0]


def seq32(t, dim):
    """fp32 sum along dim, one term after the other from 0."""
    t = t.movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def row_sum32(t, order):
    """Sum over the C channels of [rows][C]: each lane its 8 channels in sequence (lanes past C / 8 hold zeros),
    then the butterfly; or pairwise."""
    assert t.dtype == torch.float32
    if order == "pair":
        return sum32(t, t.dim() - 1, "pair")
    full = torch.zeros(t.shape[:-1] + (512,), dtype=torch.float32)
    full[..., :t.shape[-1]] = t
    return butterfly32(seq32(full.view(t.shape[:-1] + (64, 8)), -1))


def chunk_sum32(t, N, order):
    """[rows][C] -> [B * chunks][C]: each wave its rows r = wave, wave + 4, .. in sequence, then the waves in order;
    or pairwise over the chunk's rows."""
    Rr = chunk_rows(N)
    v = t.view(-1, Rr, t.shape[1])
    if order == "pair":
        return sum32(v, 1, "pair")
    waves = []
    for w in range(WAVES):
        idx = list(range(w, Rr, WAVES))
        waves.append(seq32(v[:, idx], 1) if idx else torch.zeros_like(v[:, 0]))
    return seq32(torch.stack(waves), 0)


def _inv32(n):
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)


def _rsqrt32(t):
    return (1.0 / torch.sqrt(t.double())).float()


def emulate_forward(c, xo, mod, order):
    """mean, var + eps (q inv_c + eps before the rsqrt), rstd and y (before its bf16 rounding) with the kernel's
    rounding points, as float64 copies of the fp32 values."""
    x = xo.float()
    inv_c = _inv32(x.shape[1])
    mu = row_sum32(x, order) * inv_c
    d = x - mu[:, None]
    ve = row_sum32(d * d, order) * inv_c + torch.tensor(EPS, dtype=torch.float32)
    rs = _rsqrt32(ve)
    if mod:
        b = mod_rows(c)
        sc, sh = c["scale"][b].float(), c["shift"][b].float()
    else:
        sc = sh = torch.zeros_like(x)
    y = d * rs[:, None] * (1.0 + sc) + sh
    return dict(mean=mu.double(), ve=ve.double(), rstd=rs.double(), y=y.double())


def emulate_backward(c, mean, rstd, mod, dres, f32, order):
    """dx (before its bf16 rounding on the bf16 stream), dx as stored, psh, psc and pg in fp32."""
    x, dy, N = c["x"].float(), c["dy"].float(), c["N"]
    inv_c = _inv32(x.shape[1])
    mu, rs = mean.float()[:, None], rstd.float()[:, None]
    xh = (x - mu) * rs
    sc = per_row(c["scale"], N).float() if mod != "none" else torch.zeros_like(x)
    dxh = dy * (1.0 + sc)
    s1 = (row_sum32(dxh, order) * inv_c)[:, None]
    s2 = (row_sum32(dxh * xh, order) * inv_c)[:, None]
    rr = c["dres"].float() if dres else torch.zeros_like(x)
    dx = rr + rs * (dxh - s1 - xh * s2)
    stored = dx.double() if f32 else bf16(dx.double())
    return dict(dx=dx.double(), stored=stored, xh=xh.double(), psh=chunk_sum32(dy, N, order).double(),
                psc=chunk_sum32(dy * xh, N, order).double(),
                pg=chunk_sum32(stored.float() * c["v"].float(), N, order).double())


def emulate_finalize(ws, order):
    return sum32(ws.float(), 1, "seq" if order == "kernel" else "pair").double()


def emulate_mse(c, dims, pad, order):
    """The loss in fp32: thread, wave and workgroup order of mse_patch_kernel and sum_rows_kernel, or pairwise."""
    B, C, H, W, p = dims
    rows, K = patch_dims(*dims)
    d = (c["pred"].float() - tokens_of(c["target"], p).float())
    sq = torch.zeros(rows, K + pad, dtype=torch.float32)
    sq[:, :K] = d * d
    sq = sq.view(-1)
    inv_n = _inv32(B * C * H * W)
    if order == "pair":
        return float((sum32(sq, 0, "pair") * inv_n).double())
    blocks = min(cdiv(sq.numel(), NT), MSE_CAP)
    iters = cdiv(sq.numel(), blocks * NT)
    full = torch.zeros(iters * blocks * NT, dtype=torch.float32)
    full[:sq.numel()] = sq
    part = seq32(butterfly32(seq32(full.view(iters, blocks, WAVES, 64), 0)), 1)
    full = torch.zeros(cdiv(blocks, NT) * NT, dtype=torch.float32)
    full[:blocks] = part
    total = seq32(butterfly32(seq32(full.view(-1, WAVES, 64), 0)), 0)
    return float((total * inv_n).double())


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
LAYOUTS = (CONTIGUOUS, WINDOWS)
# (extra row stride, first column) of the row kernels' operands as windows of wider buffers: all differ
_WINDOW = dict(x=(8, 0), v=(16, 8), xo=(24, 16), y=(32, 8), dy=(40, 24), dres=(48, 16), dx=(56, 32), dx16=(64, 40),
               dv=(72, 48))
_STREAM = ("x", "xo", "dres", "dx")    # operands of the residual stream's type
MOD_PAD, MOD_COL = 32, (8, 16, 24)     # shift | scale | gate at columns 8, C + 16, 2 C + 24 of [B][3 C + 32]
WS_PAD = 5                             # psh | psc | pg at columns 0, C, 2 C of partial rows of 3 C (+ 5) floats


class LnProblem:
    """One LayerNorm case on the device in one layout and stream type."""

    def __init__(self, c, layout, f32, device="cuda"):
        B, N, C = c["B"], c["N"], c["C"]
        rows = B * N
        wide = layout == WINDOWS
        self.c, self.dims, self.f32, self.rows = c, (B, N, C), int(f32), rows
        self.bufs, self.win = {}, {}
        for name, (pad, col0) in _WINDOW.items():
            dt = torch.float32 if (f32 and name in _STREAM) else torch.bfloat16
            b = Buf(rows, C + (pad if wide else 0), dt, device)
            b.col0 = col0 if wide else 0
            self.bufs[name], self.win[name] = b, b.window(b.col0, C)
            if name in c:
                self.win[name].copy_(c[name].to(dt))
        self.mod = Buf(B, 3 * C + (MOD_PAD if wide else 0), torch.bfloat16, device)
        cols = [j * C + (MOD_COL[j] if wide else 0) for j in range(3)]
        self.shift, self.scale, self.gate = (self.mod.window(k, C) for k in cols)
        for w, name in ((self.shift, "shift"), (self.scale, "scale"), (self.gate, "gate")):
            w.copy_(c[name].to(torch.bfloat16))
        self.mean, self.rstd = Flat(rows, device), Flat(rows, device)
        self.chunks = N // chunk_rows(N)
        self.ws_ld = 3 * C + (WS_PAD if wide else 0)
        self.ws = Flat(B * self.chunks * self.ws_ld, device)

    def ld(self, name):
        return self.win[name].stride(0)

    def part(self, j):
        """Pointer of partial j (0 psh, 1 psc, 2 pg): column j C of the workspace rows."""
        return ptr(self.ws.data[j * self.dims[2]:])

    def guard(self, outputs, parts=()):
        """A Guard over every buffer; `outputs` names those a call may write (their logical windows only), `parts`
        the partials (0, 1, 2) it may write (their C columns of every workspace row)."""
        g = Guard()
        C = self.dims[2]
        for name, b in self.bufs.items():
            g.add(name, b, [("w", b.col0, C)] if name in outputs else [])
        g.add("modulation", self.mod)
        for name in ("mean", "rstd"):
            f = getattr(self, name)
            g.add(name, f, [(0, f.n)] if name in outputs else [])
        g.add("workspace", self.ws, [(k * self.ws_ld + j * C, k * self.ws_ld + (j + 1) * C)
                                     for k in range(self.dims[0] * self.chunks) for j in parts])
        return g

    def out(self, name):
        return self.win[name].cpu().double()

    def partial(self, j):
        C = self.dims[2]
        return self.ws.get(self.dims[0] * self.chunks, self.ws_ld)[:, j * C:(j + 1) * C]

    def fwd_args(self, res, mod, **over):
        B, N, C = self.dims
        a = dict(x=ptr(self.win["x"]), ldx=self.ld("x"), v=ptr(self.win["v"]) if res != "none" else None,
                 ldv=self.ld("v"), gate=ptr(self.gate) if res == "gate" else None,
                 xo=ptr(self.win["xo"]) if res != "none" else None, ldxo=self.ld("xo"),
                 shift=ptr(self.shift) if mod else None, scale=ptr(self.scale) if mod else None,
                 ld_mod=self.mod.ld, y=ptr(self.win["y"]), ldy=self.ld("y"), mean=ptr(self.mean.data),
                 rstd=ptr(self.rstd.data), rows=self.rows, C=C, N=N, eps=EPS, f32=self.f32)
        a.update(over)
        return tuple(a.values())

    def fwd(self, L, res, mod, stream, **over):
        return L.sdmi_ln_mod_fwd(*self.fwd_args(res, mod, **over), stream)

    def bwd_args(self, mod, dres, gate, dx16, **over):
        B, N, C = self.dims
        a = dict(x=ptr(self.win["x"]), ldx=self.ld("x"), mean=ptr(self.mean.data), rstd=ptr(self.rstd.data),
                 dy=ptr(self.win["dy"]), lddy=self.ld("dy"), scale=ptr(self.scale) if mod != "none" else None,
                 ld_mod=self.mod.ld, dres=ptr(self.win["dres"]) if dres else None, lddres=self.ld("dres"),
                 dx=ptr(self.win["dx"]), lddx=self.ld("dx"), psh=self.part(0) if mod in ("both", "psh") else None,
                 psc=self.part(1) if mod in ("both", "psc") else None, ws_ld=self.ws_ld,
                 gate=ptr(self.gate) if gate else None, v=ptr(self.win["v"]) if gate else None, ldv=self.ld("v"),
                 dv=ptr(self.win["dv"]) if gate else None, lddv=self.ld("dv"), pg=self.part(2) if gate else None,
                 rows=self.rows, C=C, N=N, f32=self.f32, dx16=ptr(self.win["dx16"]) if dx16 else None,
                 ld16=self.ld("dx16"))
        a.update(over)
        return tuple(a.values())

    def bwd(self, L, mod, dres, gate, dx16, stream, **over):
        return L.sdmi_ln_mod_bwd(*self.bwd_args(mod, dres, gate, dx16, **over), stream)


class FinalizeProblem:
    """Partial rows [B * chunks][ws_ld] fp32 and the bf16 table [B][ldo]; windows: ws_ld = W + 5, the table at column
    3 of rows of W + 7 (scalar accesses: odd strides and offsets are legal)."""

    def __init__(self, ws, layout, device="cuda"):
        B, chunks, W = ws.shape
        wide = layout == WINDOWS
        self.dims = (B, chunks, W)
        self.ws_ld = W + (5 if wide else 0)
        self.ws = Flat(B * chunks * self.ws_ld, device)
        self.ws.data.view(B * chunks, self.ws_ld)[:, :W].copy_(ws.reshape(B * chunks, W).float())
        self.outb = Buf(B, W + (7 if wide else 0), torch.bfloat16, device)
        self.outb.col0 = 3 if wide else 0
        self.out = self.outb.window(self.outb.col0, W)

    def guard(self, writes=True):
        g = Guard()
        g.add("workspace", self.ws)
        g.add("out", self.outb, [("w", self.outb.col0, self.dims[2])] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, chunks, W = self.dims
        a = dict(ws=ptr(self.ws.data), B=B, chunks=chunks, ws_ld=self.ws_ld, W=W, out=ptr(self.out), ldo=self.outb.ld)
        a.update(over)
        return L.sdmi_mod_finalize(*a.values(), stream)


class PatchProblem:
    """One patch-layout case on the device: tokens [rows][K + pad] (bf16 or fp32) and NCHW fp32 images between NaN
    pads. An input token tensor of a padded row starts at column 1 (its pad columns stay NaN); the outputs of
    nchw_to_tokens and mse_patch (grad) are written across the whole ld."""

    def __init__(self, dims, pad, device="cuda"):
        self.dims, self.pad = dims, pad
        self.rows, self.K = patch_dims(*dims)
        self.ld = self.K + pad
        B, C, H, W, p = dims
        self.n = B * C * H * W
        self.device = device

    def tokens(self, dtype, values=None):
        """A token buffer: with `values` an input window [rows][K], without an output written whole."""
        b = Buf(self.rows, self.ld, dtype, self.device)
        b.col0 = (1 if self.pad else 0) if values is not None else 0
        w = b.window(b.col0, self.K if values is not None else self.ld)
        if values is not None:
            w.copy_(values.to(dtype))
        return b, w

    def image(self, values=None):
        f = Flat(self.n, self.device)
        return f.put(values) if values is not None else f
