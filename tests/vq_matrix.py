"""The declared test matrix of the VQ latent-interface kernels (csrc/vqvae.hip) and the helpers its exact tests share.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`. The expected launches -- a
fragment of the mangled kernel name with its template argument, and the grid -- are written by hand. The host rules of
vqvae.hip are restated below, also by hand: sdmi_vq_quantize launches ceil(P / 32) workgroups of
vq_quantize_kernel<EN>, EN iff K <= 16384, then one vq_loss_kernel; sdmi_vq_bwd launches min(512, ceil(P / 256))
workgroups of vq_bwd_kernel, one vq_bwd_finish_kernel and ceil(K / 64) workgroups of vq_codebook_grad_kernel;
sdmi_pointwise_in launches min(ceil(P ld / 256), 8192); sdmi_vq_workspace is 4 ceil(P / 32) bytes and
sdmi_vq_bwd_workspace 512 (2 * 64 + 16) 4 bytes. The search splits the codebook by per = ceil(K / 16): wave w owns
[w per, min(K, (w + 1) per)) and its halves meet at w0 + ceil(per / 2). tests/test_vq_matrix_cpu.py checks rows
against rules and that no row can be removed; tests/test_vq_exact_gpu.py that the library launches what the rows say.

Entry points and dims: QUANT sdmi_vq_quantize (B, HW, C, K) with ldz, conv (none / w / wb: the kernel's own 1x1
convolution absent, without and with bias) and xq (the optional output); BWD sdmi_vq_bwd (B, HW, C, K) with ld (the
strides of dzin / z_enc / dz_enc), add (dzq_add), lw (loss_w) and null (none / post / pre: which of the dw / db pairs
is absent), each run with three index distributions (uniform; collapsed: every pixel one code; sparse: three codes
used, the rows of all others must become exact zeros over the NaN fill); POINT sdmi_pointwise_in (B, C, HW, cout, ld)
with bias. QUANT and BWD run in a contiguous layout (the row's strides, the channels at column 0) and in a windows
layout (z, z_enc at column 1 of rows 3 floats wider, dzin at column 2 of rows 6 elements wider); dz_enc and the
pointwise output are written across their whole row stride, so their stride is the row's in both.

Data, two families. References are float64 on the CPU, computed from the stored inputs.

  exact  Small integers. The codebook is 2 r + parity (|value| <= 4, one parity per channel), so the midpoint of any
         two codes is an integer vector; x is integer with |x| <= 4: every d^2 is an integer below 2^10, exact in any
         order and under any contraction, and distinct d^2 stay distinct after sqrtf. With a convolution the stored z
         is W^-1 (x - b) for a unimodular W with entries in {-1, 0, 1, 2} (2 x 2 blocks of determinant 1, rows and
         columns permuted), b integer: the kernel's fma chain returns the planted x exactly. The codebook carries
         duplicates planted on the seams of the row's slice rule in the first, the middle and the last (ragged) live
         wave: rows s - 1 and s equal for s = wm (across halves), s = w1 (across waves), s = w0 + 1 and wm + 1 (inside
         a half). One third of the pixels are copies of a duplicated code (distance 0: the clamp), one third sit at the
         midpoint of two different codes, the rest are random. The index is the first minimum of the integer d^2 on
         every pixel, zq == q and xq == x bitwise, the loss is fl(S fl(1 / n)) bitwise. Backward: dzin, zq, xq, z_enc,
         dzq_add integers in [-4, 4], weights in {-1, 0, 1, 2}, beta = n / 2^k and codebook_weight = n / 2^j (n = P C
         exact in fp32), loss_w signed powers of two, so both gradient scales are powers of two; k is the largest of
         4 .. 0 at which every sum of absolute terms stays below 2^24 units. Every backward sum and demb is bitwise.
  soft   z, x, the codebook, the weights and biases randn in fp32, dzin = bf16(1e-3 randn), beta = 0.25,
         codebook_weight = 1, loss_w = (1.3, 0.7).

Statements and bounds (u = 2^-24):

  xq     bitwise the fma32 chain from the bias, ci ascending (explicit fmaf in the source), both families.
  zq     bitwise fl(x + fl(q - x)) on that x and the kernel's own index.
  index  T = |x|^2 + |e|^2 + 2 sum |x_c e_c|, tol = K_D u T + 2^-22 d^2; a code is admissible iff d^2 - tol <=
         min_k (d^2 + tol) in float64. The kernel's index is admissible on every pixel and equals argmin on every
         pixel with one admissible code; at most 1 % of a row's pixels may have more (a guard against a vacuous test).
  loss   |loss - ref| <= K_S u ref, ref in float64 on the kernel's own index.
  point  bitwise the fma32 chain then RNE to bf16; pad columns written and exactly zero.
  dz_enc bitwise: dzq the fma32 chain (co ascending) plus one fp32 add of dzq_add; dx = fma32(g, fl(x - q), dzq),
         g = fl(fl(fl(2 beta) / fl(n)) loss_w[1]); the fma32 chain (co ascending); RNE to bf16; pad columns zero.
  sums   dw_post, db_post, dw_pre, db_pre: |sum - ref| <= K_S u sum |term|, ref in float64 on the bitwise dx.
  demb   <= K_S u |g| (count |e| + sum |x_p|) + 2 u |ref|; rows of unused codes exactly 0.

K_D and K_S are measured, not chosen: tests/test_vq_matrix_cpu.py runs an fp32 emulation of each sum in the kernel's
order (c ascending and (dot + |x|^2) + |e|^2; per pixel, the 32-pixel butterfly, vq_loss_kernel's strided threads and
four waves; per thread its grid-stride pixels, the butterfly, the waves and the workgroups in order; per code the 8
waves' matches in pixel order, then the waves in order) and pairwise, every product rounded separately, on every soft
row and measures max |fp32 - float64| / (u T) (for demb the excess over 2 u |ref|). The larger of the two orders
reached: d^2 3.16 (0.73 .. 3.16 over the rows); loss 2.03 (on the 5-pixel and the C = 1 rows: fl(q - x) alone puts
2 u on a term), dw_post 1.79, db_post 0.07 (sums of bf16 values are nearly exact), dw_pre 1.72, db_pre 1.22, demb 0.87.
The GPU's contraction choices are a third variant, so a constant is twice the largest ratio of its kind, rounded up:
K_D = 8. For the sums twice the largest ratio is 4.06 and the next power of two, 8, is more than 3 times the ratio, so
K_S = 6: the CPU test asserts that the emulations stay within K / 2 and that 2 ratio <= K <= 3 ratio for both, and
that each perturbed reference (the lowest tied index replaced by the next tied one, a pixel dropped from a sum, a
round's pixels counted twice in demb, 1 ulp in dz_enc) leaves its statement.

Measured on an MI355X, max(err / bound) over all rows, layouts and index distributions, exact family / soft family:
loss 0.239 / 0.338 (the exact family's loss is also bitwise fl(S fl(1 / n)); 0.239 is that value against S / n),
dw_post 0 / 0.221, db_post 0 / 0.012, dw_pre 0 / 0.286, db_pre 0 / 0.203, demb 0 / 0.231; the index was the float64
argmin on every soft pixel (no pixel of any row has a second admissible code) and the first minimum on every exact
pixel; xq, zq, dz_enc, the pointwise output and all zero pads bitwise; every backward sum and demb of the exact family
bitwise; a second call repeats every bit. The K = 16384 row launched: 65536 bytes of dynamic LDS on top of 4096 static.
No row found a defect in the kernels of vqvae.hip. Reading the host code found one: sdmi_pointwise_in did not check w,
which its kernel dereferences unconditionally; it now returns -1, and the error-return test covers it.

Guards: every operand and output is a window of a NaN-filled buffer (front pad, pad columns, rows past the end); idx,
loss and both workspaces sit between NaN pads. After a call only the declared outputs may have changed, bit for bit:
that covers the inputs, the quantize workspace beyond ceil(P / 32) floats, the backward workspace beyond blocks * 144
floats, an absent xq and absent dw / db."""
import collections
import functools

import numpy as np
import torch

from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401  (shared with the attention tests)
from tests.dit_matrix import butterfly32, seq32
from tests.norm_matrix import (CONTIGUOUS, WINDOWS, Flat, Guard, bf16, bits, cdiv, fma32, is_bf16, ptr,  # noqa: F401
                               sum32, ulp32)

QUANT, BWD, POINT = "quant", "bwd", "pointwise"
Row = collections.namedtuple("Row", "entry dims launches opt")
U24 = 2.0 ** -24
K_D = 8.0
K_S = 6.0
DISTS = ("uniform", "collapsed", "sparse")
LAYOUTS = (CONTIGUOUS, WINDOWS)
ORDERS = ("kernel", "pair")


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/vqvae.hip, restated
# ----------------------------------------------------------------------------------------------------------------
VQ_WAVES = 16
MAXC = 8
EN_MAX = 16384
QUANT_PIX = 32
BWD_NT, BWD_CAP, BWD_PART = 256, 512, 2 * 64 + 16
CB_CODES, CB_ROUND, CB_WAVES = 64, 1024, 8
POINT_CAP = 8192


def quant_name(en):
    return f"vq_quantize_kernelILb{int(en)}EE"


def quant_workspace(P):
    return 4 * cdiv(P, QUANT_PIX)


def bwd_workspace():
    return BWD_CAP * BWD_PART * 4


def bwd_blocks(P):
    return min(BWD_CAP, cdiv(P, BWD_NT))


def slices(K):
    """(w0, wm, w1) of the 16 waves: wave w scans [w0, wm) on lanes 0-31 and [wm, w1) on lanes 32-63. A wave past
    the codebook has w1 = wm = K <= w0 and scans nothing."""
    per = cdiv(K, VQ_WAVES)
    out = []
    for w in range(VQ_WAVES):
        w0 = w * per
        w1 = min(K, w0 + per)
        out.append((w0, min(w1, w0 + (per + 1) // 2), w1))
    return out


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    if entry == QUANT:
        B, HW, C, K = dims
        return [(quant_name(K <= EN_MAX), cdiv(B * HW, QUANT_PIX)), ("vq_loss_kernel", 1)]
    if entry == BWD:
        B, HW, C, K = dims
        return [("vq_bwd_kernel", bwd_blocks(B * HW)), ("vq_bwd_finish_kernel", 1),
                ("vq_codebook_grad_kernel", cdiv(K, CB_CODES))]
    assert entry == POINT
    B, C, HW, cout, ld = dims
    return [("pointwise_in_kernel", min(cdiv(B * HW * ld, 256), POINT_CAP))]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
_QT, _QF, _LOSS = "vq_quantize_kernelILb1EE", "vq_quantize_kernelILb0EE", ("vq_loss_kernel", 1)
ROWS = [
    # K = 1 and fewer pixels than one workgroup
    R(QUANT, (1, 5, 4, 1), (_QT, 1), _LOSS, ldz=4, conv="none", xq=0),
    # the MNIST shape: the second workgroup has 10 live pixels and straddles the two images; waves 10-15 are empty
    R(QUANT, (2, 21, 3, 20), (_QT, 2), _LOSS, ldz=8, conv="wb", xq=1),
    # per = 1: every second half is empty; exactly one full workgroup
    R(QUANT, (1, 32, 4, 16), (_QT, 1), _LOSS, ldz=4, conv="w", xq=0),
    # C = 1; wave 8 has one code, waves 9+ have w0 > K
    R(QUANT, (1, 33, 1, 17), (_QT, 2), _LOSS, ldz=8, conv="none", xq=1),
    # C = 8; per = 3: halves of 2 + 1; the last slice is ragged
    R(QUANT, (3, 35, 8, 37), (_QT, 4), _LOSS, ldz=8, conv="wb", xq=1),
    R(QUANT, (2, 63, 5, 512), (_QT, 4), _LOSS, ldz=8, conv="wb", xq=1),
    # the bench codebook; the largest LDS table; <false> with the odd per = 1025
    R(QUANT, (1, 40, 4, 8192), (_QT, 2), _LOSS, ldz=8, conv="wb", xq=0),
    R(QUANT, (1, 40, 4, 16384), (_QT, 2), _LOSS, ldz=4, conv="none", xq=1),
    R(QUANT, (1, 40, 4, 16385), (_QF, 2), _LOSS, ldz=8, conv="none", xq=1),
    # 258 partials: vq_loss_kernel loops
    R(QUANT, (1, 8225, 2, 5), (_QT, 258), _LOSS, ldz=2, conv="none", xq=0),
]
_FIN = ("vq_bwd_finish_kernel", 1)
ROWS += [
    R(BWD, (1, 3, 4, 5), ("vq_bwd_kernel", 1), _FIN, ("vq_codebook_grad_kernel", 1), ld=(4, 4, 4), add=0, lw=0,
      null="none"),
    R(BWD, (2, 63, 4, 37), ("vq_bwd_kernel", 1), _FIN, ("vq_codebook_grad_kernel", 1), ld=(8, 8, 8), add=0, lw=0,
      null="none"),
    # two workgroups, the second with one pixel; the wide pad
    R(BWD, (1, 257, 3, 20), ("vq_bwd_kernel", 2), _FIN, ("vq_codebook_grad_kernel", 1), ld=(8, 8, 16), add=0, lw=0,
      null="none"),
    # P = 1029: the sxb branch, five pixels into a second round with -1 padding inside an int4, three codebook
    # workgroups of which the last has two live lanes
    R(BWD, (3, 343, 8, 130), ("vq_bwd_kernel", 5), _FIN, ("vq_codebook_grad_kernel", 3), ld=(8, 8, 8), add=1, lw=1,
      null="none"),
    # three rounds; each pair of weight / bias gradients absent in turn
    R(BWD, (2, 1100, 5, 64), ("vq_bwd_kernel", 9), _FIN, ("vq_codebook_grad_kernel", 1), ld=(8, 8, 8), add=0, lw=0,
      null="post"),
    R(BWD, (2, 1100, 5, 64), ("vq_bwd_kernel", 9), _FIN, ("vq_codebook_grad_kernel", 1), ld=(8, 8, 8), add=0, lw=0,
      null="pre"),
    # the 512-workgroup cap: all of block 0 takes a second trip, plus one thread of block 1
    R(BWD, (1, 131329, 4, 70), ("vq_bwd_kernel", 512), _FIN, ("vq_codebook_grad_kernel", 2), ld=(8, 8, 8), add=0,
      lw=1, null="none"),
]
ROWS += [
    R(POINT, (1, 4, 5, 4, 8), ("pointwise_in_kernel", 1), bias=1),
    R(POINT, (2, 3, 21, 3, 8), ("pointwise_in_kernel", 2), bias=0),
    R(POINT, (1, 8, 33, 8, 8), ("pointwise_in_kernel", 2), bias=1),
    R(POINT, (2, 4, 63, 4, 16), ("pointwise_in_kernel", 8), bias=1),
    R(POINT, (1, 4, 40, 6, 8), ("pointwise_in_kernel", 2), bias=1),
    # 2 101 264 elements > 2^21: the capped grid and the grid-stride loop
    R(POINT, (1, 4, 131329, 4, 16), ("pointwise_in_kernel", 8192), bias=1),
]


def row_id(r):
    def s(v):
        return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{s(v)}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# data (CPU, no library call): float64 tensors holding values exact in the stored type; pixel-major [P][C]
# ----------------------------------------------------------------------------------------------------------------
def _ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _rn(gen, *shape):
    return torch.randn(shape, generator=gen, dtype=torch.float64).float().double()


def nchw(t, B, HW):
    """[P][C] -> flat NCHW."""
    return t.view(B, HW, -1).permute(0, 2, 1).reshape(-1)


def from_nchw(flat, B, HW, C):
    return flat.view(B, C, HW).permute(0, 2, 1).reshape(B * HW, C)


_BLOCKS = (((1, 2), (0, 1)), ((2, 1), (1, 1)), ((1, -1), (0, 1)), ((2, -1), (1, 0)))


def unimodular(gen, C):
    """An integer matrix with entries in {-1, 0, 1, 2} whose inverse is integer: 2 x 2 blocks of determinant 1 (and
    a -1 for an odd C) on the diagonal, rows and columns permuted. Returns (W, W^-1)."""
    W = torch.zeros(C, C, dtype=torch.float64)
    i = 0
    while i + 1 < C:
        W[i:i + 2, i:i + 2] = torch.tensor(_BLOCKS[int(torch.randint(0, 4, (1,), generator=gen))], dtype=torch.float64)
        i += 2
    if i < C:
        W[i, i] = -1.0
    W = W[torch.randperm(C, generator=gen)][:, torch.randperm(C, generator=gen)]
    Wi = torch.linalg.inv(W).round()
    assert torch.equal(W @ Wi, torch.eye(C, dtype=torch.float64))
    return W, Wi


def planted_seams(K):
    """The rows s whose code is made a copy of row s - 1, by kind, in the first, the middle and the last live wave."""
    sl = [s for s in slices(K) if s[0] < K]
    out = dict(within=[], halves=[], waves=[])
    for w0, wm, w1 in {sl[0], sl[len(sl) // 2], sl[-1], sl[max(len(sl) - 2, 0)]}:
        if wm - w0 >= 2:
            out["within"].append(w0 + 1)
        if w1 - wm >= 2:
            out["within"].append(wm + 1)
        if w0 < wm < w1:
            out["halves"].append(wm)
        if w1 < K:
            out["waves"].append(w1)
    return {k: sorted(set(v)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def quant_case(kind, B, HW, C, K, conv):
    """z [P][C], w (C, C) and b (C) or None, the codebook (K, C); the exact family also its planted x and seams."""
    P = B * HW
    gen = torch.Generator().manual_seed((11000 if kind == "exact" else 12000) + 7 * P + 3 * K + C)
    if kind == "soft":
        w = _rn(gen, C, C) if conv != "none" else None
        b = _rn(gen, C) if conv == "wb" else None
        return dict(kind=kind, B=B, HW=HW, C=C, K=K, z=_rn(gen, P, C), w=w, b=b, codebook=_rn(gen, K, C))
    parity = _ri(gen, 0, 1, C)
    code = 2 * _ri(gen, -2, 1, K, C) + parity
    seams = planted_seams(K)
    for s in sorted(set(sum(seams.values(), []))):
        code[s] = code[s - 1]
    bases = sorted({s - 1 for v in seams.values() for s in v})
    x = _ri(gen, -4, 4, P, C)
    for p in range(P):
        j = p // 3
        if p % 3 == 0:
            x[p] = code[bases[j % len(bases)] if bases else j % K]
        elif p % 3 == 1 and K >= 2:
            i = bases[j % len(bases)] if (bases and j % 2) else int(torch.randint(0, K, (1,), generator=gen))
            other = [k for k in torch.randperm(K, generator=gen)[:8].tolist() if not torch.equal(code[k], code[i])]
            if other:
                x[p] = (code[i] + code[other[0]]) / 2
    w = b = None
    z = x
    if conv != "none":
        w, wi = unimodular(gen, C)
        b = _ri(gen, -4, 4, C) if conv == "wb" else None
        z = (x - (b if b is not None else 0.0)) @ wi.T
    return dict(kind=kind, B=B, HW=HW, C=C, K=K, z=z, w=w, b=b, codebook=code, x=x, seams=seams)


def _codes(dist, K, P, gen):
    if dist == "uniform":
        return torch.randint(0, K, (P,), generator=gen)
    if dist == "collapsed":
        return torch.full((P,), (2 * K) // 3, dtype=torch.int64)
    used = torch.tensor(sorted({0, K // 2, K - 1}))
    return used[torch.randint(0, len(used), (P,), generator=gen)]


def scale32(weight, n, lw=None):
    """fl(fl(fl(2 weight) / fl(n)) lw) as the host and the kernels form it."""
    g = np.float32(weight) * np.float32(2.0) / np.float32(n)
    return float(g * np.float32(lw) if lw is not None else g)


@functools.lru_cache(maxsize=None)
def bwd_case(kind, B, HW, C, K, dist, add, lw):
    P = B * HW
    n = P * C
    gen = torch.Generator().manual_seed((13000 if kind == "exact" else 14000) + 7 * P + 3 * K + C + DISTS.index(dist))
    idx = _codes(dist, K, P, gen)
    if kind == "soft":
        c = dict(dzin=bf16(1e-3 * _rn(gen, P, C)), zq=_rn(gen, P, C), xq=_rn(gen, P, C), z_enc=_rn(gen, P, C),
                 w_post=_rn(gen, C, C), w_pre=_rn(gen, C, C), codebook=_rn(gen, K, C),
                 add=_rn(gen, P, C) if add else None, beta=0.25, cbw=1.0,
                 loss_w=(float(np.float32(1.3)), float(np.float32(0.7))) if lw else None)
    else:
        c = dict(dzin=_ri(gen, -4, 4, P, C), zq=_ri(gen, -4, 4, P, C), xq=_ri(gen, -4, 4, P, C),
                 z_enc=_ri(gen, -4, 4, P, C), w_post=_ri(gen, -1, 2, C, C), w_pre=_ri(gen, -1, 2, C, C),
                 codebook=_ri(gen, -4, 4, K, C), add=_ri(gen, -4, 4, P, C) if add else None, cbw=n / 8.0,
                 loss_w=(-0.5, 2.0) if lw else None)
    c.update(kind=kind, B=B, HW=HW, C=C, K=K, idx=idx, dist=dist)
    if kind == "exact":
        for k in (4, 3, 2, 1, 0):
            c["beta"] = n / 2.0 ** k
            if exact_margin(c) < 2.0 ** 24:
                break
        else:
            raise AssertionError("no exact commitment scale")
    return c


def exact_margin(c):
    """The largest sum of absolute terms of any backward sum of an exact case, in units of its last bit."""
    r = bwd_reference(c)
    unit = min(1.0, abs(r["g"]))
    return max(float(r["T_dw_pre"].max()), float(r["T_db_pre"].max()), float(r["T_dw_post"].max())) / unit


@functools.lru_cache(maxsize=None)
def point_case(kind, B, C, HW, cout, bias):
    P = B * HW
    gen = torch.Generator().manual_seed((15000 if kind == "exact" else 16000) + 7 * P + 3 * cout + C)
    if kind == "exact":
        return dict(z=_ri(gen, -4, 4, P, C), w=_ri(gen, -1, 2, cout, C), b=_ri(gen, -4, 4, cout) if bias else None)
    return dict(z=_rn(gen, P, C), w=_rn(gen, cout, C), b=_rn(gen, cout) if bias else None)


# ----------------------------------------------------------------------------------------------------------------
# references (float64) and bounds
# ----------------------------------------------------------------------------------------------------------------
def conv_chain(z, w, b):
    """out[p][co] = the fma32 chain from the bias (or 0) over ci ascending, as float64 copies of the fp32 values;
    w None: the identity."""
    if w is None:
        return z
    s = (b if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)).float().expand(z.shape[0], -1)
    for ci in range(w.shape[1]):
        s = fma32(w[:, ci].float()[None, :], z[:, ci].float()[:, None], s)
    return s.double()


def dist2(x, e):
    """d^2 [P][K] in float64, directly."""
    return ((x[:, None, :] - e[None, :, :]) ** 2).sum(-1)


def dist_scale(x, e):
    """T = |x|^2 + |e|^2 + 2 sum |x_c e_c| [P][K]."""
    return (x * x).sum(1)[:, None] + (e * e).sum(1)[None, :] + 2 * x.abs() @ e.abs().T


def admissible(x, e, K=None):
    """[P][K] bool: the codes a correct fp32 search may return (docstring: index), and argmin64."""
    K = K_D if K is None else K
    d = dist2(x, e)
    tol = K * U24 * dist_scale(x, e) + 2.0 ** -22 * d
    return (d - tol) <= (d + tol).min(1, keepdim=True)[0], d.argmin(1)


def zq_reference(x, e, idx):
    """fl(x + fl(q - x)), float64 copies."""
    q = e[idx].float()
    return (x.float() + (q - x.float())).double()


def loss_reference(x, e, idx, weights=None):
    """(loss, S): S the float64 sum of (q - x)^2 on the given index, loss = S / n; `weights` [P] counts pixels."""
    sq = ((e[idx] - x) ** 2).sum(1)
    S = (sq * weights).sum() if weights is not None else sq.sum()
    return S / x.numel(), S


def exact_loss(S, n):
    return float(np.float32(float(S)) * (np.float32(1.0) / np.float32(n)))


def tie_kinds(d2, K):
    """Per kind the number of pixels whose first minimum is tied with a code inside the same half of its wave's slice,
    in the other half of that slice, and in a later wave."""
    sl = slices(K)
    per = cdiv(K, VQ_WAVES)
    wm = torch.tensor([s[1] for s in sl])
    first = d2.argmin(1)
    wave = first // per
    tied = d2 == d2.min(1, keepdim=True)[0]
    k = torch.arange(K)[None, :]
    later = tied & (k > first[:, None])
    kw = (k // per) == wave[:, None]
    khalf = k >= wm[wave][:, None]
    fhalf = (first >= wm[wave])[:, None]
    return dict(within=int((later & kw & (khalf == fhalf)).any(1).sum()),
                halves=int((later & kw & khalf & ~fhalf).any(1).sum()),
                waves=int((later & ~kw).any(1).sum()))


def next_tied(d2):
    """The perturbed index: on pixels with a tied minimum the second tied code instead of the first."""
    first = d2.argmin(1)
    tied = d2 == d2.min(1, keepdim=True)[0]
    tied[torch.arange(d2.shape[0]), first] = False
    second = tied.float().argmax(1)
    return torch.where(tied.any(1), second, first)


def search(d, K, half_le=False, wave_le=False):
    """The slice / half / wave merge of vq_quantize_kernel on distances d [P][K] (fp32 values): every half keeps its
    first minimum, the second half wins only when strictly nearer, the waves likewise in ascending order."""
    P = d.shape[0]
    inf = torch.full((P,), float("inf"), dtype=d.dtype)
    bd, bk = inf.clone(), torch.zeros(P, dtype=torch.int64)
    for w, (w0, wm, w1) in enumerate(slices(K)):
        hd, hk = [], []
        for lo, hi in ((w0, wm), (wm, w1)):
            if hi > lo:
                i = d[:, lo:hi].argmin(1)       # (the first of equal values, as one ascending scan keeps it)
                hd.append(d[:, lo:hi].gather(1, i[:, None])[:, 0])
                hk.append(i + lo)
            else:
                hd.append(inf)
                hk.append(torch.full((P,), lo, dtype=torch.int64))
        take = (hd[1] <= hd[0]) if half_le else (hd[1] < hd[0])
        wd, wk = torch.where(take, hd[1], hd[0]), torch.where(take, hk[1], hk[0])
        if w == 0:
            bd, bk = wd, wk
        else:
            take = (wd <= bd) if wave_le else (wd < bd)
            bd, bk = torch.where(take, wd, bd), torch.where(take, wk, bk)
    return bk


def point_reference(c, drop_bias=False):
    return bf16(conv_chain(c["z"], c["w"], None if drop_bias else c["b"]))


def bwd_reference(c, weights=None, demb_weights=None):
    """Everything sdmi_vq_bwd returns: dz (bitwise, [P][C]), the bitwise dx it is built on, the four sums with the
    sums of absolute terms that scale their bounds, demb with its bound scale. `weights` [P] counts pixels in the four
    sums, `demb_weights` in the codebook gradient (0: dropped, 2: twice)."""
    P, C, K = c["B"] * c["HW"], c["C"], c["K"]
    n = P * C
    lw = c["loss_w"]
    g = scale32(c["beta"], n, lw[1] if lw else None)
    gcb = scale32(c["cbw"], n, lw[0] if lw else None)
    dzin, idx = c["dzin"], c["idx"]
    s = torch.zeros(P, C, dtype=torch.float32)
    for co in range(C):
        s = fma32(c["w_post"][co].float()[None, :], dzin[:, co].float()[:, None], s)
    if c["add"] is not None:
        s = s + c["add"].float()
    q = c["codebook"][idx]
    dx = fma32(torch.tensor(g, dtype=torch.float32), c["xq"].float() - q.float(), s)
    t = torch.zeros(P, C, dtype=torch.float32)
    for co in range(C):
        t = fma32(c["w_pre"][co].float()[None, :], dx[:, co][:, None], t)
    dx = dx.double()
    w = torch.ones(P, dtype=torch.float64) if weights is None else weights.double()
    dzw, dxw = dzin * w[:, None], dx * w[:, None]
    out = dict(g=g, gcb=gcb, dx=dx, dz=bf16(t.double()),
               dw_post=dzw.T @ c["zq"], T_dw_post=dzin.abs().T @ c["zq"].abs(),
               db_post=dzw.sum(0), T_db_post=dzin.abs().sum(0),
               dw_pre=dxw.T @ c["z_enc"], T_dw_pre=dx.abs().T @ c["z_enc"].abs(),
               db_pre=dxw.sum(0), T_db_pre=dx.abs().sum(0))
    wd = torch.ones(P, dtype=torch.float64) if demb_weights is None else demb_weights.double()
    count = torch.zeros(K, dtype=torch.float64).index_add_(0, idx, wd)
    sx = torch.zeros(K, C, dtype=torch.float64).index_add_(0, idx, c["xq"] * wd[:, None])
    sax = torch.zeros(K, C, dtype=torch.float64).index_add_(0, idx, c["xq"].abs())
    true_count = torch.zeros(K, dtype=torch.float64).index_add_(0, idx, torch.ones(P, dtype=torch.float64))
    out.update(demb=gcb * (count[:, None] * c["codebook"] - sx),
               T_demb=abs(gcb) * (true_count[:, None] * c["codebook"].abs() + sax), count=true_count)
    return out


def sum_bound(T, K=None):
    return (K_S if K is None else K) * U24 * T


def demb_bound(ref, T, K=None):
    return (K_S if K is None else K) * U24 * T + 2 * U24 * ref.abs()


# ----------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' sums in two orders (CPU, torch), every product rounded separately
# ----------------------------------------------------------------------------------------------------------------
def emulate_d2(x, e, order):
    """|x|^2 + |e|^2 - 2 x.e in fp32: c ascending and (dot + xn) + en, or pairwise."""
    x, e = x.float(), e.float()
    m2 = -2.0 * x
    prod = m2[:, None, :] * e[None, :, :]
    if order == "kernel":
        return ((seq32(prod, 2) + seq32(x * x, 1)[:, None]) + seq32(e * e, 1)[None, :]).double()
    return (sum32(prod, 2, "pair") + (sum32(x * x, 1, "pair")[:, None] + sum32(e * e, 1, "pair")[None, :])).double()


def _inv32(n):
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)


def _pad(t, n):
    out = torch.zeros((n,) + t.shape[1:], dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def emulate_loss(x, e, idx, order):
    """The loss in fp32: c ascending per pixel, the butterfly of each 32-pixel workgroup, then vq_loss_kernel's
    strided threads, butterflies and four waves; or pairwise over all terms."""
    diff = e.float()[idx] - x.float()
    sq = diff * diff
    inv_n = _inv32(sq.numel())
    if order == "pair":
        return float((sum32(sq.reshape(-1), 0, "pair") * inv_n).double())
    P = sq.shape[0]
    blocks = cdiv(P, QUANT_PIX)
    lanes = torch.zeros(blocks, 64, dtype=torch.float32)
    lanes[:, :32] = _pad(seq32(sq, 1), blocks * 32).view(blocks, 32)
    part = butterfly32(lanes)
    trips = cdiv(blocks, 256)
    t = seq32(_pad(part, trips * 256).view(trips, 4, 64), 0)
    return float((seq32(butterfly32(t), 0) * inv_n).double())


def emulate_bwd_sum(terms, order):
    """Sum over pixels of terms [P][Q] (fp32, already rounded products) as vq_bwd_kernel and vq_bwd_finish_kernel
    add them: each thread its grid-stride pixels in sequence, the butterfly, the four waves, the workgroups in order."""
    terms = terms.float()
    if order == "pair":
        return sum32(terms, 0, "pair").double()
    P, Q = terms.shape
    grid = bwd_blocks(P)
    trips = cdiv(P, grid * BWD_NT)
    t = seq32(_pad(terms, trips * grid * BWD_NT).view(trips, grid, 4, 64, Q), 0)
    t = seq32(butterfly32(t.movedim(2, -1)), 1)       # [grid][4][Q][64] -> [grid][4][Q] -> [grid][Q]
    return seq32(t, 0).double()


def emulate_demb(c, gcb, order):
    """demb of the used codes in fp32: per code each of the 8 waves subtracts its matches in pixel order (wave w owns
    pixels [128 w, 128 w + 128) of every 1024-pixel round), the waves are added in order, then g fma(count, e, acc);
    or the matches summed pairwise. Returns (codes, [codes][C])."""
    x, idx = c["xq"].float(), c["idx"]
    used = torch.unique(idx)
    wave = (torch.arange(idx.numel()) % CB_ROUND) // (CB_ROUND // CB_WAVES)
    out = []
    for k in used.tolist():
        m = idx == k
        if order == "pair":
            acc = -sum32(x[m], 0, "pair")
        else:
            parts = [x[m & (wave == w)] for w in range(CB_WAVES)]
            L = max(p.shape[0] for p in parts)
            acc = -seq32(seq32(torch.stack([_pad(p, L) for p in parts]), 1), 0)
        tc = torch.tensor(float(m.sum()), dtype=torch.float32)
        out.append(torch.tensor(gcb, dtype=torch.float32) * fma32(tc, c["codebook"][k].float(), acc))
    return used, torch.stack(out).double()


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
_WIDE32, _WIDE16 = (3, 1), (6, 2)     # (extra row stride, first column) of fp32 and bf16 operands in windows


class Idx(Flat):
    """n int64 indices between NaN pads (two fp32 words each): `ids` is the int64 view of the logical window."""

    def __init__(self, n, device):
        super().__init__(2 * n, device)
        self.ids = self.data.view(torch.int64)


def _window(rows, ld, cols, dtype, layout, device, values=None):
    extra, col0 = (0, 0) if layout == CONTIGUOUS else (_WIDE32 if dtype == torch.float32 else _WIDE16)
    b = Buf(rows, ld + extra, dtype, device)
    b.col0 = col0
    w = b.window(col0, cols)
    if values is not None:
        w.copy_(values.to(dtype))
    return b, w


def _flat(n, device, values=None):
    f = Flat(max(n, 1), device)
    return f.put(values) if values is not None else f


class QuantProblem:
    """One quantize case on the device in one layout."""

    def __init__(self, c, row, layout, device="cuda"):
        B, HW, C, K = row.dims
        P = B * HW
        self.c, self.dims, self.P = c, row.dims, P
        self.conv, self.with_xq = opt(row, "conv"), opt(row, "xq")
        self.zb, self.z = _window(P, opt(row, "ldz"), C, torch.float32, layout, device, c["z"])
        self.w = _flat(C * C, device, c["w"])
        self.b = _flat(C, device, c["b"])
        self.codebook = _flat(K * C, device, c["codebook"])
        self.zq, self.xq = _flat(P * C, device), _flat(P * C, device)
        self.idx = Idx(P, device)
        self.blocks = cdiv(P, QUANT_PIX)
        self.ws, self.loss = _flat(self.blocks, device), _flat(1, device)

    def guard(self, writes=True):
        g = Guard()
        g.add("z", self.zb)
        for name in ("w", "b", "codebook"):
            g.add(name, getattr(self, name))
        P, C = self.P, self.dims[2]
        g.add("zq", self.zq, [(0, P * C)] if writes else [])
        g.add("xq", self.xq, [(0, P * C)] if writes and self.with_xq else [])
        g.add("idx", self.idx, [(0, 2 * P)] if writes else [])
        g.add("workspace", self.ws, [(0, self.blocks)] if writes else [])
        g.add("loss", self.loss, [(0, 1)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, HW, C, K = self.dims
        a = dict(z=ptr(self.z), ldz=self.z.stride(0), w=ptr(self.w.data) if self.conv != "none" else None,
                 b=ptr(self.b.data) if self.conv == "wb" else None, codebook=ptr(self.codebook.data), K=K, B=B, HW=HW,
                 C=C, zq=ptr(self.zq.data), idx=ptr(self.idx.data), xq=ptr(self.xq.data) if self.with_xq else None,
                 ws=ptr(self.ws.data), loss=ptr(self.loss.data))
        a.update(over)
        return L.sdmi_vq_quantize(*a.values(), stream)

    def outputs(self):
        """idx, zq, xq [P][C], loss, the partials: CPU copies (float64; idx int64)."""
        B, HW, C, K = self.dims
        return dict(idx=self.idx.ids.cpu(), zq=from_nchw(self.zq.get(self.P * C), B, HW, C),
                    xq=from_nchw(self.xq.get(self.P * C), B, HW, C), loss=float(self.loss.get(1)),
                    partial=self.ws.get(self.blocks))

    def raw(self):
        return [t.buf.clone() for t in (self.zq, self.xq, self.idx, self.ws, self.loss)]


class BwdProblem:
    """One backward case on the device in one layout."""
    OUT = ("dw_post", "db_post", "dw_pre", "db_pre")

    def __init__(self, c, row, layout, device="cuda"):
        B, HW, C, K = row.dims
        P = B * HW
        ld_dzin, ldz, ld_out = opt(row, "ld")
        self.c, self.dims, self.P, self.null = c, row.dims, P, opt(row, "null")
        self.dzinb, self.dzin = _window(P, ld_dzin, C, torch.bfloat16, layout, device, c["dzin"])
        self.zeb, self.z_enc = _window(P, ldz, C, torch.float32, layout, device, c["z_enc"])
        self.dzb = Buf(P, ld_out, torch.bfloat16, device)
        self.dz = self.dzb.window(0, ld_out)
        self.zq, self.xq = _flat(P * C, device, nchw(c["zq"], B, HW)), _flat(P * C, device, nchw(c["xq"], B, HW))
        self.add = _flat(P * C, device, nchw(c["add"], B, HW) if c["add"] is not None else None)
        self.w_post, self.w_pre = _flat(C * C, device, c["w_post"]), _flat(C * C, device, c["w_pre"])
        self.codebook = _flat(K * C, device, c["codebook"])
        self.idx = Idx(P, device)
        self.idx.ids.copy_(c["idx"])
        self.loss_w = _flat(2, device, torch.tensor(c["loss_w"]) if c["loss_w"] else None)
        self.blocks = bwd_blocks(P)
        self.ws = _flat(BWD_CAP * BWD_PART, device)
        self.dw_post, self.dw_pre = _flat(C * C, device), _flat(C * C, device)
        self.db_post, self.db_pre = _flat(C, device), _flat(C, device)
        self.demb = _flat(K * C, device)

    def given(self, name):
        return not ((self.null == "post" and name.endswith("post")) or (self.null == "pre" and name.endswith("pre")))

    def guard(self, writes=True):
        g = Guard()
        g.add("dzin", self.dzinb)
        g.add("z_enc", self.zeb)
        for name in ("zq", "xq", "add", "w_post", "w_pre", "codebook", "idx", "loss_w"):
            g.add(name, getattr(self, name))
        g.add("dz_enc", self.dzb, [("w", 0, self.dzb.ld)] if writes else [])
        g.add("workspace", self.ws, [(0, self.blocks * BWD_PART)] if writes else [])
        for name in self.OUT:
            f = getattr(self, name)
            g.add(name, f, [(0, f.n)] if writes and self.given(name) else [])
        g.add("demb", self.demb, [(0, self.demb.n)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, HW, C, K = self.dims
        c = self.c
        a = dict(dzin=ptr(self.dzin), ld_dzin=self.dzin.stride(0), zq=ptr(self.zq.data), w_post=ptr(self.w_post.data),
                 xq=ptr(self.xq.data), idx=ptr(self.idx.data), codebook=ptr(self.codebook.data), K=K,
                 z_enc=ptr(self.z_enc), ldz=self.z_enc.stride(0), w_pre=ptr(self.w_pre.data), B=B, HW=HW, C=C,
                 beta=c["beta"], cbw=c["cbw"], dz_enc=ptr(self.dz), ld_out=self.dzb.ld, ws=ptr(self.ws.data))
        for name in self.OUT:
            a[name] = ptr(getattr(self, name).data) if self.given(name) else None
        a.update(demb=ptr(self.demb.data), dzq_add=ptr(self.add.data) if c["add"] is not None else None,
                 loss_w=ptr(self.loss_w.data) if c["loss_w"] else None)
        a.update(over)
        return L.sdmi_vq_bwd(*a.values(), stream)

    def outputs(self):
        C, K = self.dims[2], self.dims[3]
        out = dict(dz=self.dz.cpu().double(), demb=self.demb.get(K, C))
        for name in self.OUT:
            if self.given(name):
                out[name] = getattr(self, name).get(*((C, C) if name.startswith("dw") else (C,)))
        return out

    def raw(self):
        return [t.buf.clone() for t in (self.dzb, self.ws, self.dw_post, self.db_post, self.dw_pre, self.db_pre,
                                        self.demb)]


class PointProblem:
    """One pointwise case on the device: z NCHW fp32 between NaN pads, the output [P][ld] bf16 written whole."""

    def __init__(self, c, row, device="cuda"):
        B, C, HW, cout, ld = row.dims
        self.c, self.dims, self.P, self.bias = c, row.dims, B * HW, opt(row, "bias")
        self.z = _flat(self.P * C, device, nchw(c["z"], B, HW))
        self.w, self.b = _flat(cout * C, device, c["w"]), _flat(cout, device, c["b"])
        self.outb = Buf(self.P, ld, torch.bfloat16, device)
        self.out = self.outb.window(0, ld)

    def guard(self, writes=True):
        g = Guard()
        for name in ("z", "w", "b"):
            g.add(name, getattr(self, name))
        g.add("out", self.outb, [("w", 0, self.outb.ld)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, C, HW, cout, ld = self.dims
        a = dict(z=ptr(self.z.data), B=B, C=C, HW=HW, w=ptr(self.w.data), b=ptr(self.b.data) if self.bias else None,
                 cout=cout, out=ptr(self.out), ld=ld)
        a.update(over)
        return L.sdmi_pointwise_in(*a.values(), stream)
