"""The declared test matrix of the LPIPS kernels (csrc/lpips.hip: eight entry points, seven kernels) and the helpers its
exact tests share. The pattern is tests/kl_matrix.py's.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`, the launches -- a fragment of
the kernel name and the grid -- written by hand (the distance rows through the hand-written tables _DIST and _LONG of
(P, workgroups per sample)). The host rules of lpips.hip are restated below, also by hand: the element-wise kernels
(prep, image_grad, maxpool2_fwd, maxpool2_bwd) launch min(65536, max(1, ceil(work / 256))) workgroups of 256 threads
with work = 2 B HW, B HW, N (H/2)(W/2)(C/8) and N ceil(H/2) ceil(W/2) (C/8); the distance kernels cover
ppb(C) = 8 * 4 * (512 / C) pixels per workgroup (256, 128, 64, 32 for C = 64, 128, 256, 512) on a grid
(ceil(P / ppb), B); sdmi_lpips_dist_fwd is two launches, the forward and lpips_dist_sum_kernel with B workgroups of 64
threads; sdmi_lpips_dist_workspace is 4 B ceil(P / ppb) bytes; sdmi_lpips_mean is one workgroup.
tests/test_lpips_matrix_cpu.py checks rows against rules; tests/test_lpips_exact_gpu.py that the library launches what
the rows say. The 65536-workgroup cap of the element-wise kernels needs more than 16.7 million work items: the second
grid-stride trip is NOT reached at test size and no row claims to cover it.

Shapes (ppw = 512 / C pixels per wave):
  distance   each C in {64, 128, 256, 512} at P in {1, ppw + 1, ppb - 1, ppb, ppb + 1, 3 ppb + 5} with B in {1, 3}, and at
             P = 64 ppb + 1 with B = 2 (65 partials: the second trip of the sum kernel's loop). Every shape is a full row
             (rn, g, gscale != 1, addend, accumulate onto a prior value) and a bare row (none of them, accumulate 0);
             the backward rows run both sides; every row runs contiguous and as column windows of wider NaN-filled
             buffers in which ld, ld_add and ld_dy all differ. ws is a guarded buffer of exactly the workspace size.
  max-pool   (N, H, W, C) = (1, 2, 2, 8), (1, 3, 3, 8), (1, 2, 9, 16), (1, 9, 2, 16), (2, 5, 7, 128), (3, 6, 10, 64),
             (2, 4, 4, 512).
  prep, image_grad  (B, H, W) = (1, 1, 1), (2, 5, 7), (1, 16, 16), (3, 33, 40); prep in all four source layouts and both
             normalize values; image_grad in five operand modes (out_nchw; acc add; both; acc whole with mse; that with
             out_nchw), each with both normalize values.
  mean       B in {1, 3, 65}.

Data families:
  exact    (distance) every feature row holds n in {0, 1, 4, 16, 64} equal entries 2^k, k in [-1, 1] per row, spread over
           the row with a random rotation (so over different lanes' 8-channel groups and both halves of every shuffle),
           the rest zero: sum a^2 = n 4^k, its root a power of two, the unit vector 1 / sqrt(n). The rows of the two
           images are drawn independently (sharing some channels or none), or identical, or all zero on one side or
           on both. w in {1, 2, 3, 4} / 4, g in {1, 2, 3, 4} / 2, addend multiples of 1 / 8 in [-1/2, 1/2]. P a power
           of two: gscale = 2 and a prior val of quarter units; otherwise gscale = 2 P (so coef = 2 g exactly whatever
           the rounding of 1 / P) and a prior val of 0 (so the last fma is fl(S fl(1 / P))). Every operation is exact,
           so every output is bitwise, the lane shuffles included; the CPU test checks for every row that each partial
           sum stays below 2^24 units of its last bit and that every gradient is an fp32 value.
  soft     (distance) bf16(relu(randn)): half the entries zero; planted all-zero rows in image 0 only, image 1 only and
           both; one row whose entries are all tiny but non-zero (around 2^-30). Domain: a row's norm is 0 or at least
           2^-28, far above the 1e-12 clamp and the fp32 underflow of the squares, so the float64 reference is also the
           answer of an fp32 reference. w = |randn| / C, g in [0.5, 1.5], gscale 0.75, addend bf16(1e-3 randn), a
           randn prior val.
  ties / special  (pool pair) small integers (ties in almost every window); and draws from {+-0, +-inf, NaN, bf16
           subnormals, +-1, +-2} with planted windows: NaN at each of the four window positions and at two at once,
           windows mixing -0 and +0, all-equal windows. Odd H and W are in the shapes.
  soft / special  (prep, image_grad, mean) uniform / randn data; and +-0, +-inf, NaN, fp32 and bf16 subnormals among
           ordinary values. Pad channels of NHWC sources hold NaN and 7.

Statements (u = 2^-24):
  prep        bitwise fl(fl(fl(2x) - 1) - shift) / scale correctly rounded (without normalize fl(x - shift) / scale), then
              RNE to bf16; channels 3..7 are +0; junk in the pad channels of an NHWC source never reaches the output.
  image_grad  bitwise in every mode: g = fl(d / scale) (x 2); out_nchw = g; acc add: bf16(fl(acc + g)) in channels 0..2,
              channels 3..7 (the one the kernel rewrites and the four it does not touch) bit for bit unchanged; whole:
              bf16(fl(fl(fl(2 fl(pred - target)) / fl32(3 B HW)) + g)), channels 3..7 +0.
  pool fwd    bitwise the first maximum in scan order (0,0), (0,1), (1,0), (1,1); any NaN in the window gives NaN; a
              window mixing -0 and +0 returns the first of them.
  pool bwd    bitwise: dy goes to the first maximum, or to the last NaN; every other element of dx -- the dropped odd
              row and column included -- is +0.
  rn          |rn - rn64| <= K_RN u rn64, rn64 = 1 / max(sqrt(sum a^2), 1e-12) in float64; exactly fl32(1e12) for an
              all-zero row; exact family: bitwise.
  partials    what the kernel leaves in ws: |partial - S64| <= K_D u M with S64 the float64 sum over the workgroup's
              pixels and M = sum_pixels sum_c w_c (|u0_c| + |u1_c|)^2 (not |val|, which cancels); exact family: equal.
  val         bitwise given the partials: per lane of the sum kernel its strided trips in sequence, the butterfly, then
              fma(S, fl(1 / P), prior) rounded once (prior 0 without accumulate: fl(S fl(1 / P))). The kernel states the
              fma; the compiler had contracted the plain expression to the same instruction.
  mean        bitwise the ordered sum times scale.
  dy          bf16(x) with |x - ref64| <= K_G u T_c, T_c = |coef| rn (|t_c| + |u_c| sum_k |t_k u_k|) + |addend_c|, ref64
              the float64 gradient through the tap's ReLU on the same bf16 inputs (checked against autograd through
              F.normalize on the CPU); the assertion allows half a bf16 ulp of ref64 on top. Elements with a <= 0 are
              exact zeros. The kernel is given rn = fl32(rn64). Exact family: bitwise (ref64 is an fp32 value; in a bare
              row off a power of two coef = fl(1 / P) and the one inexact product is rounded to fp32 first).
  A second call repeats every bit. After a call only the declared outputs differ from the NaN fill: ws, rn and the
  windows of wider buffers included.

K_RN, K_D and K_G are measured, not chosen: tests/test_lpips_matrix_cpu.py emulates every sum in fp32 in the kernel's
order (8 channels per lane in sequence, the xor butterfly below C / 8 lanes, the 8 passes, the wave butterfly, the four
waves in order, then the sum kernel), every product rounded on its own (the coarser model: the kernel contracts some
into fmas), on every soft row and takes the largest ratio to u rn64, u M and u T_c. The largest ratios were 2.432 (rn, the
(2, 8193, 128) row), 3.382 (partials, the one-pixel row (3, 1, 256): the roundings of u0 and u1 enter t squared) and
12.581 (dy, the bare (2, 16385, 64) row, side 0: T_c carries |t_c| = 2 w |u_a - u_o|, and where u_a and u_o nearly
cancel the roundings of the two products are large against it; over a million elements one such channel is met); each
constant lies between twice and three times its ratio: K_RN = 6, K_D = 8, K_G = 32. The CPU test asserts those
relations and that each perturbed reference (the pair's
shuffle width halved, rn of the other image used for the own rows, 1 / P dropped, the ReLU select dropped, addend
ignored, the projection term dropped, the two sides swapped, the pool's last maximum in place of the first, the pool's
NaN rule removed) leaves its statement.

Measured on an MI355X over all rows, families and layouts: max |rn - rn64| / (K_RN u rn64) 0.405 (the (2, 8193, 128)
row; 2.43 u rn64, as the emulation says); max |partial - S64| / (K_D u M) 0.423 (the one-pixel rows (3, 1, 256), 0.407 on
(3, 1, 64); at most 0.20 on every row of more than one pixel); dy: the part of |dy - ref64| beyond half a bf16 ulp is at
most 0.152 of K_G u T_c ((2, 8193, 128) bare), so the bound is held by the bf16 rounding almost alone (max |dy - ref64| /
bound 0.999); the exact family, val given the partials, mean, prep, image_grad and the pool pair bitwise in every row; a
second call repeats every bit.

Guards: every operand and output sits between NaN pads; after a call only the declared outputs may have changed, bit for
bit."""
import collections
import functools

import numpy as np
import torch

from sdmi import _lib
from tests import vq_matrix as VM
from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401
from tests.dit_matrix import butterfly32, seq32
from tests.norm_matrix import CONTIGUOUS, WINDOWS, Flat, Guard, bf16, bits, cdiv, fma32, ptr, ulp32  # noqa: F401

PREP, IGRAD, POOLF, POOLB, DFWD, DBWD, MEAN = "prep", "image_grad", "pool_fwd", "pool_bwd", "dist_fwd", "dist_bwd", "mean"
ENTRY = {PREP: "sdmi_lpips_prep", IGRAD: "sdmi_lpips_image_grad", POOLF: "sdmi_maxpool2_fwd", POOLB: "sdmi_maxpool2_bwd",
         DFWD: "sdmi_lpips_dist_fwd", DBWD: "sdmi_lpips_dist_bwd", MEAN: "sdmi_lpips_mean", "ws": "sdmi_lpips_dist_workspace"}
ARITY = {name: len(_lib.SIGNATURES[name][0]) for name in ENTRY.values()}
Row = collections.namedtuple("Row", "entry dims launches opt")
U24 = 2.0 ** -24
K_RN, K_D, K_G = 6.0, 8.0, 32.0
# largest emulated ratios over the soft rows (the CPU test checks them)
MEASURED = dict(rn=2.432, partial=3.382, dy=12.581)
LAYOUTS = (CONTIGUOUS, WINDOWS)
KINDS = ("exact", "soft")
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
RN_ZERO = float(np.float32(1e12))
SOFT_GSCALE = 0.75
MODES = ("nchw", "acc", "nchw_acc", "mse", "mse_nchw")

NT, GRID_CAP, PASSES = 256, 65536, 8
TAP_CHANNELS = (64, 128, 256, 512)


def grid_for(work):
    return min(GRID_CAP, max(1, cdiv(work, NT)))


def ppw(C):
    return 512 // C


def ppb(C):
    return PASSES * (NT // 64) * ppw(C)


def blocks(P, C):
    return cdiv(P, ppb(C))


def workspace(B, P, C):
    return 4 * B * blocks(P, C)


def work_of(entry, dims):
    if entry == PREP:
        return 2 * dims[0] * dims[1] * dims[2]
    if entry == IGRAD:
        return dims[0] * dims[1] * dims[2]
    N, H, W, C = dims
    return N * (H // 2) * (W // 2) * (C // 8) if entry == POOLF else N * cdiv(H, 2) * cdiv(W, 2) * (C // 8)


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=0):
    return dict(r.opt).get(key, default)


_KP, _KI, _KF, _KB = "lpips_prep_kernel", "lpips_image_grad_kernel", "maxpool2_fwd_kernel", "maxpool2_bwd_kernel"
_KD, _KS, _KG, _KM = "lpips_dist_fwd_kernel", "lpips_dist_sum_kernel", "lpips_dist_bwd_kernel", "lpips_mean_kernel"
KERNEL = {PREP: _KP, IGRAD: _KI, POOLF: _KF, POOLB: _KB, MEAN: _KM}


def expected_launches(entry, dims):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    if entry in (DFWD, DBWD):
        B, P, C = dims
        g = blocks(P, C) * B
        return [(_KD, g), (_KS, B)] if entry == DFWD else [(_KG, g)]
    if entry == MEAN:
        return [(_KM, 1)]
    return [(KERNEL[entry], grid_for(work_of(entry, dims)))]


# (P, workgroups per sample) of the distance rows, by hand: 1, ppw + 1, ppb - 1, ppb, ppb + 1, 3 ppb + 5
_DIST = {64: ((1, 1), (9, 1), (255, 1), (256, 1), (257, 2), (773, 4)),
         128: ((1, 1), (5, 1), (127, 1), (128, 1), (129, 2), (389, 4)),
         256: ((1, 1), (3, 1), (63, 1), (64, 1), (65, 2), (197, 4)),
         512: ((1, 1), (2, 1), (31, 1), (32, 1), (33, 2), (101, 4))}
_LONG = {64: 16385, 128: 8193, 256: 4097, 512: 2049}     # 64 ppb + 1: 65 workgroups per sample, B = 2
# (N, H, W, C), forward workgroups, backward workgroups
_POOL = (((1, 2, 2, 8), 1, 1), ((1, 3, 3, 8), 1, 1), ((1, 2, 9, 16), 1, 1), ((1, 9, 2, 16), 1, 1), ((2, 5, 7, 128), 1, 2),
         ((3, 6, 10, 64), 2, 2), ((2, 4, 4, 512), 2, 2))
# (B, H, W), prep workgroups, image_grad workgroups
_IMG = (((1, 1, 1), 1, 1), ((2, 5, 7), 1, 1), ((1, 16, 16), 2, 1), ((3, 33, 40), 31, 16))

ROWS = [R(PREP, d, (_KP, gp), nhwc0=a, nhwc1=b, normalize=n) for d, gp, _ in _IMG for a in (0, 1) for b in (0, 1) for n in (0, 1)]
ROWS += [R(IGRAD, d, (_KI, gi), mode=m) for d, _, gi in _IMG for m in MODES]
ROWS += [R(POOLF, d, (_KF, gf)) for d, gf, _ in _POOL] + [R(POOLB, d, (_KB, gb)) for d, _, gb in _POOL]
for _C, _tab in _DIST.items():
    for _P, _nb in _tab:
        for _B in (1, 3):
            for _full in (1, 0):
                ROWS += [R(DFWD, (_B, _P, _C), (_KD, _nb * _B), (_KS, _B), full=_full),
                         R(DBWD, (_B, _P, _C), (_KG, _nb * _B), full=_full)]
    for _full in (1, 0):
        ROWS += [R(DFWD, (2, _LONG[_C], _C), (_KD, 130), (_KS, 2), full=_full), R(DBWD, (2, _LONG[_C], _C), (_KG, 130), full=_full)]
ROWS += [R(MEAN, (B,), (_KM, 1)) for B in (1, 3, 65)]


def row_id(r):
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{v}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


def status(entry, a):
    """What the entry point returns for the arguments a (pointers as truth values), restated by hand."""
    pos = lambda *ks: all(a[k] >= 1 for k in ks)  # noqa: E731
    ld_ok = lambda k: a[k] >= a["C"] and a[k] % 8 == 0  # noqa: E731
    if entry == PREP:
        ok = all(a[k] for k in ("in0", "in1", "shift", "scale", "out")) and pos("B", "H", "W")
    elif entry == IGRAD:
        ok = a["d"] and a["scale"] and (a["nchw"] or a["acc"]) and pos("B", "H", "W") and \
            bool(a["pred"]) == bool(a["target"]) and not (a["pred"] and not a["acc"])
    elif entry in (POOLF, POOLB):
        ok = a["x"] and a["y"] and (entry == POOLF or a["dy"]) and a["N"] >= 1 and a["H"] >= 2 and a["W"] >= 2 and \
            a["C"] >= 8 and a["C"] % 8 == 0
    elif entry == DFWD:
        ok = all(a[k] for k in ("f", "w", "ws", "val")) and a["C"] in TAP_CHANNELS and ld_ok("ld") and 1 <= a["B"] <= 65535 and pos("P")
    elif entry == DBWD:
        ok = all(a[k] for k in ("f", "w", "rn", "dy")) and a["C"] in TAP_CHANNELS and ld_ok("ld") and ld_ok("ld_dy") and \
            1 <= a["B"] <= 65535 and pos("P") and a["side"] in (0, 1) and (not a["addend"] or ld_ok("ld_add"))
    elif entry == MEAN:
        ok = a["val"] and a["out"] and pos("B")
    else:
        raise KeyError(entry)
    return 0 if ok else -1


# ----------------------------------------------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------------------------------------------
def same_bits(got, ref):
    """Bit for bit, any NaN standing for any NaN (a conversion may quieten a payload)."""
    got, ref = got.contiguous().cpu(), ref.contiguous().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    n = torch.isnan(ref)
    return bool(torch.equal(torch.isnan(got), n)) and bool(torch.equal(bits(got)[~n], bits(ref)[~n]))


def is_f32(x):
    return bool(torch.equal(x.float().double(), x))


def ulp_bf16(x):
    """The bf16 unit in the last place at |x| (float64 tensor)."""
    return ulp32(x) * 2.0 ** 16


# ----------------------------------------------------------------------------------------------------------------
# distance: data (CPU, float64 tensors holding values exact in the stored type)
# ----------------------------------------------------------------------------------------------------------------
def _exact_rows(gen, T, C):
    f = torch.zeros(T, C, dtype=torch.float64)
    n = torch.tensor([0, 1, 4, 16, 64])[torch.randint(0, 5, (T,), generator=gen)]
    k = torch.randint(-1, 2, (T,), generator=gen)
    rot = torch.randint(0, C, (T,), generator=gen)
    j = torch.arange(64)[None, :]
    cols = (rot[:, None] + j * (C // n.clamp_min(1))[:, None]) % C          # entry j of a row: n of them, C / n apart
    on = j < n[:, None]
    rows = torch.arange(T)[:, None].expand(T, 64)
    f[rows[on], cols[on]] = (2.0 ** k.double())[:, None].expand(T, 64)[on]
    return f


@functools.lru_cache(maxsize=None)
def dist_case(kind, B, P, C):
    T = B * P
    gen = torch.Generator().manual_seed((41000 if kind == "exact" else 42000) + 7 * P + 3 * C + B)
    c = dict(kind=kind, B=B, P=P, C=C)
    if kind == "exact":
        f = torch.stack([_exact_rows(gen, T, C), _exact_rows(gen, T, C)])
        mode = torch.randint(0, 6, (T,), generator=gen)        # 0, 1: as drawn; 2: identical; 3, 4: one side zero; 5: both
        if T >= 6:
            mode[torch.randperm(T, generator=gen)[:6]] = torch.arange(6)
        f[1, mode == 2] = f[0, mode == 2]
        f[0, (mode == 3) | (mode == 5)] = 0
        f[1, (mode == 4) | (mode == 5)] = 0
        pow2 = P & (P - 1) == 0
        c.update(f=f, w=VM._ri(gen, 1, 4, C) / 4.0, g=VM._ri(gen, 1, 4, B) / 2.0, gscale=2.0 if pow2 else 2.0 * P,
                 addend=VM._ri(gen, -4, 4, T, C) / 8.0, prev=VM._ri(gen, -8, 8, B) / 4.0 if pow2 else torch.zeros(B, dtype=torch.float64))
    else:
        f = bf16(torch.relu(torch.randn(2, T, C, generator=gen, dtype=torch.float64)))
        spots = [] if T == 1 else [(T // 3, (0,)), ((2 * T) // 3, (1,)), (T - 1, (0, 1))]
        if T == 3:
            spots = [(0, (0,)), (1, (1,)), (2, (0, 1))]
        for r, sides in spots:
            for s in sides:
                f[s, r] = 0
        if T > 4:   # all tiny, none zero
            f[1, 0] = bf16(2.0 ** -30 * (1.0 + torch.rand(C, generator=gen, dtype=torch.float64)))
        c.update(f=f, w=(torch.randn(C, generator=gen).abs() / C).double(), g=(torch.rand(B, generator=gen) + 0.5).double(),
                 gscale=SOFT_GSCALE, addend=bf16(1e-3 * VM._rn(gen, T, C)), prev=VM._rn(gen, B), spots=spots)
    return c


# ----------------------------------------------------------------------------------------------------------------
# distance: float64 references. The keyword arguments are the perturbations of the CPU test.
# ----------------------------------------------------------------------------------------------------------------
def _halves(x, half):
    """Sum over the channels; half: what each lane holds after a butterfly that starts at a quarter of the pair's lanes
    -- the sum of its own half of the channels ([..., 2])."""
    if not half:
        return x.sum(-1, keepdim=True)
    C = x.shape[-1]
    return x.view(x.shape[:-1] + (2, C // 2)).sum(-1)


def inv_norm64(f, half=False):
    """[..., 1] (or [..., 2] halves): 1 / max(|f|, 1e-12)."""
    return 1.0 / torch.sqrt(_halves(f * f, half)).clamp_min(1e-12)


def rn_reference(c, half=False):
    """[2][B P] float64: what lane 0 of each pixel stores."""
    return inv_norm64(c["f"], half)[..., 0]


def rn_input(c):
    """[2][B P] fp32 values (as float64): fl32(rn64), fl32(1e12) for an all-zero row."""
    rn = rn_reference(c).float().double()
    rn[(c["f"] == 0).all(-1)] = RN_ZERO
    return rn


def pixel_terms(c, half=False):
    """(d, M) [B][P] float64: sum_c w_c (u0 - u1)^2 and sum_c w_c (|u0| + |u1|)^2 of every pixel."""
    f, w = c["f"], c["w"]
    if half:
        C = c["C"]
        f, w = f[..., :C // 2], w[:C // 2]
    rn = inv_norm64(f)
    u0, u1 = f[0] * rn[0], f[1] * rn[1]
    d = (w * (u0 - u1) ** 2).sum(-1)
    M = (w * (u0.abs() + u1.abs()) ** 2).sum(-1)
    return d.view(c["B"], c["P"]), M.view(c["B"], c["P"])


def block_sums(x, C):
    """[B][P] float64 -> [B][blocks]: the sum over each workgroup's pixels."""
    B, P = x.shape
    nb = blocks(P, C)
    pad = torch.zeros(B, nb * ppb(C), dtype=x.dtype)
    pad[:, :P] = x
    return pad.view(B, nb, ppb(C)).sum(-1)


def inv_p32(P, drop=False):
    return torch.tensor(1.0, dtype=torch.float32) if drop else torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(P), dtype=torch.float32)


def val_from_partials(part, P, prev=None, drop_inv_p=False):
    """[B] fp32 from the fp32 partials [B][blocks]: lane l of the sum kernel adds partials l, l + 64, .. in sequence,
    the butterfly, then fma(S, fl(1 / P), prev)."""
    B, nb = part.shape
    trips = cdiv(nb, 64)
    t = torch.zeros(B, trips * 64, dtype=torch.float32)
    t[:, :nb] = part.float()
    S = butterfly32(seq32(t.view(B, trips, 64), 1))
    z = torch.zeros(B, dtype=torch.float32) if prev is None else prev.float()
    return fma32(S, inv_p32(P, drop_inv_p), z)


def coef64(c, full, drop_inv_p=False):
    """[B P][1] float64 copies of the kernel's fp32 coef = fl(fl(g gscale) / P)."""
    B, P = c["B"], c["P"]
    g = c["g"].float() if full else torch.ones(B, dtype=torch.float32)
    gs = torch.tensor(c["gscale"] if full else 1.0, dtype=torch.float32)
    co = g * gs if drop_inv_p else (g * gs) / torch.tensor(float(P), dtype=torch.float32)
    return co.double().repeat_interleave(P)[:, None]


def dy_reference(c, side, full, other_rn=False, drop_inv_p=False, drop_relu=False, drop_addend=False, drop_proj=False,
                 swap=False, half=False):
    """(ref64, T) [B P][C] float64: the gradient through the tap's ReLU and its uncertainty scale T_c."""
    f, w = c["f"], c["w"]
    side = 1 - side if swap else side
    a, o = f[side], f[1 - side]
    rn_a, rn_o = inv_norm64(a), inv_norm64(o)
    ua, uo = a * (rn_o if other_rn else rn_a), o * rn_o
    t = 2.0 * w * (ua - uo)
    if half:
        C = c["C"]
        s = _halves(t * ua, True).repeat_interleave(C // 2, -1)
        sa = _halves((t * ua).abs(), True).repeat_interleave(C // 2, -1)
    else:
        s, sa = _halves(t * ua, False), _halves((t * ua).abs(), False)
    co = coef64(c, full, drop_inv_p)
    x = co * rn_a * (t if drop_proj else t - ua * s)
    T = co.abs() * rn_a * (t.abs() + ua.abs() * sa)
    if full and not drop_addend:
        x = x + c["addend"]
    if full:
        T = T + c["addend"].abs()
    if not drop_relu:
        x = torch.where(a <= 0, torch.zeros_like(x), x)
    return x, T


def dy_within(dy, ref, T, K=None):
    """Largest |dy - ref64| / (K u T_c + half a bf16 ulp of ref64); an element whose bound is 0 must be equal."""
    bound = (K_G if K is None else K) * U24 * T + 0.5 * ulp_bf16(ref) * (ref != 0)
    err = (dy - ref).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def dy_beyond_rounding(dy, ref, T, K=None):
    """Largest (|dy - ref64| - half a bf16 ulp of ref64) / (K u T_c): the share of K_G that the fp32 value used."""
    over = ((dy - ref).abs() - 0.5 * ulp_bf16(ref) * (ref != 0)).clamp_min(0.0)
    on = T > 0
    return float((over[on] / ((K_G if K is None else K) * U24 * T[on])).max()) if bool(on.any()) else 0.0


# ----------------------------------------------------------------------------------------------------------------
# distance: fp32 emulation in the kernels' order, every product rounded on its own
# ----------------------------------------------------------------------------------------------------------------
def lane_sum32(x, half=False):
    """[..., C] fp32 -> [...]: each of the C / 8 lanes its 8 channels in sequence, then the xor butterfly below C / 8
    lanes (offsets C / 16 .. 1; lanes past the pixel's hold zeros here, and x + 0 is x). half: the butterfly starts one
    offset lower, and lane 0 ends with its half of the lanes only."""
    C = x.shape[-1]
    lpp = C // 8
    v = seq32(x.float().view(x.shape[:-1] + (lpp, 8)), -1)
    if half:
        v = v[..., :lpp // 2]
    full = torch.zeros(v.shape[:-1] + (64,), dtype=torch.float32)
    full[..., :v.shape[-1]] = v
    return butterfly32(full)


def emulate_rn(f, half=False):
    """fp32 1 / max(sqrt(s), 1e-12f), both correctly rounded: formed in float64 and rounded to fp32, which for a root
    and a quotient of fp32 values is the correctly rounded fp32 result (53 >= 2 * 24 + 2), whatever the host's vector
    code does."""
    s = lane_sum32(f.float() * f.float(), half)
    root = torch.sqrt(s.double()).float().clamp_min(np.float32(1e-12))
    return (1.0 / root.double()).float()


def emulate_forward(c, half=False):
    """(rn32 [2][B P], partials [B][blocks]) fp32."""
    B, P, C = c["B"], c["P"], c["C"]
    f, w = c["f"].float(), c["w"].float()
    rn = emulate_rn(f, half)
    t = f[0] * rn[0][:, None] - f[1] * rn[1][:, None]
    d = lane_sum32((w * t) * t, half).view(B, P)
    nb, pw, lpp = blocks(P, C), ppw(C), C // 8
    pad = torch.zeros(B, nb * ppb(C), dtype=torch.float32)
    pad[:, :P] = d
    acc = seq32(pad.view(B, nb, PASSES, NT // 64, pw), 2)           # each lane's 8 passes in sequence
    lanes = torch.zeros(B, nb, NT // 64, 64, dtype=torch.float32)
    lanes[..., ::lpp] = acc
    return rn, seq32(butterfly32(lanes), -1)


def emulate_dy(c, side, full):
    """[B P][C] fp32: the kernel's value before its bf16 rounding, on rn = rn_input(c)."""
    f, w = c["f"].float(), c["w"].float()
    rn = rn_input(c).float()
    a, o, ia, io = f[side], f[1 - side], rn[side][:, None], rn[1 - side][:, None]
    ua = a * ia
    t = (2.0 * w) * (ua - o * io)
    s = lane_sum32(t * ua)[:, None]
    co = coef64(c, full).float()
    out = (co * ia) * (t - (a * ia) * s)
    if full:
        out = out + c["addend"].float()
    return torch.where(a <= 0, torch.zeros_like(out), out)


# ----------------------------------------------------------------------------------------------------------------
# pool pair: data, index models (bf16 tensors [N][H][W][C])
# ----------------------------------------------------------------------------------------------------------------
_NAN, _INF = float("nan"), float("inf")
_SUB16 = 2.0 ** -130          # a bf16 subnormal
_SUB32 = 2.0 ** -140          # an fp32 subnormal
_SPECIAL16 = (0.0, -0.0, _INF, -_INF, _NAN, _SUB16, -_SUB16, 1.0, -1.0, 2.0, -2.0, 0.5)
# window patterns (0,0), (0,1), (1,0), (1,1), planted into window 0 of sample 0, channel by channel
_WINDOWS = ((_NAN, 1, 2, 3), (3, _NAN, 2, 1), (3, 1, _NAN, 2), (1, 2, 3, _NAN), (1, _NAN, _NAN, 5), (-0.0, 0.0, 0.0, -0.0),
            (0.0, -0.0, -0.0, 0.0), (1, 1, 1, 1), (_NAN, 5, 1, _NAN), (_NAN, _NAN, _NAN, _NAN), (-_INF, -_INF, -_INF, -_INF),
            (_INF, _NAN, _INF, 1), (-0.0, -0.0, -0.0, 0.0), (_SUB16, -_SUB16, 0.0, _SUB16), (2, _INF, _INF, 2), (-1, -2, -1, -2))


def _draw(gen, values, *shape):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


@functools.lru_cache(maxsize=None)
def pool_case(kind, N, H, W, C):
    gen = torch.Generator().manual_seed((43000 if kind == "ties" else 44000) + 7 * H + 3 * W + C + N)
    OH, OW = H // 2, W // 2
    if kind == "ties":
        x = torch.randint(0, 3, (N, H, W, C), generator=gen).double()
        dy = VM._rn(gen, N, OH, OW, C)
    else:
        x = _draw(gen, _SPECIAL16, N, H, W, C)
        for ch, pat in enumerate(_WINDOWS[:C]):
            for k, v in enumerate(pat):
                x[0, k >> 1, k & 1, ch] = v
        dy = torch.where(torch.rand(N, OH, OW, C, generator=gen) < 0.25, _draw(gen, (0.0, -0.0, _INF, -_INF, _SUB16), N, OH, OW, C),
                         VM._rn(gen, N, OH, OW, C))
    return dict(x=x.to(torch.bfloat16), dy=dy.to(torch.bfloat16))


def pool_model(x, last_max=False, nan_rule=True):
    """(y, arg) of [N][H][W][C]: scan (0,0), (0,1), (1,0), (1,1); a later element replaces the running maximum when it
    is greater (last_max: or equal) or (nan_rule) a NaN."""
    N, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    win = [x[:, (k >> 1):2 * OH:2, (k & 1):2 * OW:2].float() for k in range(4)]
    m, arg = win[0].clone(), torch.zeros(N, OH, OW, C, dtype=torch.int64)
    for k in range(1, 4):
        v = win[k]
        take = (v >= m) if last_max else (v > m)
        if nan_rule:
            take = take | torch.isnan(v)
        m = torch.where(take, v, m)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return m.to(torch.bfloat16), arg


def pool_bwd_model(x, dy, **kw):
    N, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    _, arg = pool_model(x, **kw)
    dx = torch.zeros(N, H, W, C, dtype=torch.bfloat16)
    for k in range(4):
        dx[:, (k >> 1):2 * OH:2, (k & 1):2 * OW:2] = torch.where(arg == k, dy, torch.zeros_like(dy))
    return dx


# ----------------------------------------------------------------------------------------------------------------
# prep, image_grad, mean: data and references (fp32 / bf16 tensors; torch's CPU fp32 operators round each operation)
# ----------------------------------------------------------------------------------------------------------------
_SPECIAL32 = (0.0, -0.0, _INF, -_INF, _NAN, _SUB32, -_SUB32, _SUB16, 2.0 ** -126, 0.5, 1.0, -1.0)


def _mix(gen, soft, special, kind, frac=0.3):
    if kind != "special":
        return soft
    pick = torch.rand(soft.shape, generator=gen) < frac
    return torch.where(pick, _draw(gen, special, *soft.shape).to(soft.dtype), soft)


@functools.lru_cache(maxsize=None)
def image_case(kind, B, H, W):
    """Two images (B, 3, H, W) fp32; d and the prior acc [B HW][8] bf16 (pads: junk); pred rows / target for mse."""
    gen = torch.Generator().manual_seed((45000 if kind == "soft" else 46000) + 7 * H + 3 * W + B)
    HW = H * W
    ims = [_mix(gen, torch.rand(B, 3, H, W, generator=gen) * 2 - 1, _SPECIAL32, kind) for _ in range(2)]
    d = _mix(gen, torch.randn(B * HW, 8, generator=gen), _SPECIAL16, kind).to(torch.bfloat16)
    acc = _mix(gen, torch.randn(B * HW, 8, generator=gen), _SPECIAL16, kind).to(torch.bfloat16)
    acc[:, 3:] = _draw(gen, _SPECIAL16, B * HW, 5).to(torch.bfloat16)         # the pads: anything, NaN included
    target = _mix(gen, torch.rand(B, 3, H, W, generator=gen) * 2 - 1, _SPECIAL32, kind)
    pred = target + 0.1 * torch.randn(B, 3, H, W, generator=gen)
    return dict(ims=ims, d=d, acc=acc, target=target, pred=_mix(gen, pred, _SPECIAL32, kind, 0.1))


def nhwc8(x, junk=True):
    """(B, 3, H, W) fp32 -> [B HW][8] fp32 with junk (NaN, 7) in the pad channels."""
    B = x.shape[0]
    t = torch.full((x.shape[0] * x.shape[2] * x.shape[3], 8), 7.0 if junk else 0.0)
    if junk:
        t[:, 3::2] = _NAN
    t[:, :3] = x.permute(0, 2, 3, 1).reshape(-1, 3)
    return t


def prep_reference(ims, normalize):
    """[2 B HW][8] bf16."""
    shift, scale = torch.tensor(SHIFT).view(1, 3, 1, 1), torch.tensor(SCALE).view(1, 3, 1, 1)
    out = []
    for x in ims:
        v = 2.0 * x - 1.0 if normalize else x
        v = (v - shift) / scale
        out.append(torch.nn.functional.pad(v.permute(0, 2, 3, 1).reshape(-1, 3), (0, 5)))
    return torch.cat(out).to(torch.bfloat16)


def image_grad_reference(c, B, H, W, normalize, mode):
    """dict(nchw=fp32 (B, 3, H, W) or None, acc=bf16 [B HW][8] or None)."""
    HW = H * W
    g = c["d"][:, :3].float() / torch.tensor(SCALE)
    if normalize:
        g = g * 2.0
    out = dict(nchw=None, acc=None)
    if "nchw" in mode:
        out["nchw"] = g.view(B, HW, 3).permute(0, 2, 1).reshape(B, 3, H, W).contiguous()
    if mode.startswith("mse"):
        n = torch.tensor(float(3 * B * HW), dtype=torch.float32)
        m = (2.0 * (nhwc8(c["pred"], False)[:, :3] - nhwc8(c["target"], False)[:, :3])) / n
        out["acc"] = torch.nn.functional.pad(m + g, (0, 5)).to(torch.bfloat16)
    elif "acc" in mode:
        out["acc"] = torch.cat([(c["acc"][:, :3].float() + g).to(torch.bfloat16), c["acc"][:, 3:]], 1)
    return out


@functools.lru_cache(maxsize=None)
def mean_case(kind, B):
    gen = torch.Generator().manual_seed(47000 + B)
    v = _mix(gen, torch.randn(B, generator=gen), _SPECIAL32, kind)
    return dict(val=v, scale=0.37)


def mean_reference(c):
    return (seq32(c["val"], 0) * torch.tensor(c["scale"], dtype=torch.float32)).reshape(1)


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
# (extra row stride, first column) of the bf16 operands as windows of wider buffers: every stride differs
_WIN = dict(f=(16, 8), addend=(24, 16), dy=(32, 24))


def _window(name, rows, C, layout, device, values=None):
    extra, col0 = (0, 0) if layout == CONTIGUOUS else _WIN[name]
    b = Buf(rows, C + extra, torch.bfloat16, device)
    b.col0 = col0
    w = b.window(col0, C)
    if values is not None:
        w.copy_(values.to(torch.bfloat16))
    return b, w


def _flat(n, device, values=None):
    return VM._flat(n, device, values)


class DistProblem:
    """One distance row on the device in one layout; side matters to the backward only."""

    def __init__(self, c, row, layout, side=0, device="cuda"):
        B, P, C = row.dims
        self.c, self.row, self.dims, self.side, self.full = c, row, row.dims, side, bool(opt(row, "full"))
        self.nb = blocks(P, C)
        self.fb, self.f = _window("f", 2 * B * P, C, layout, device, c["f"].reshape(2 * B * P, C))
        self.w = _flat(C, device, c["w"])
        if row.entry == DFWD:
            self.rn, self.ws = _flat(2 * B * P, device), Flat(B * self.nb, device)
            self.val = _flat(B, device, c["prev"] if self.full else None)
        else:
            self.rn, self.g = _flat(2 * B * P, device, rn_input(c).reshape(-1)), _flat(B, device, c["g"])
            self.addb, self.addend = _window("addend", B * P, C, layout, device, c["addend"])
            self.dyb, self.dy = _window("dy", B * P, C, layout, device)

    def guard(self, writes=True):
        B, P, C = self.dims
        g = Guard()
        g.add("f", self.fb)
        g.add("w", self.w)
        if self.row.entry == DFWD:
            g.add("rn", self.rn, [(0, 2 * B * P)] if writes and self.full else [])
            g.add("ws", self.ws, [(0, B * self.nb)] if writes else [])
            g.add("val", self.val, [(0, B)] if writes else [])
        else:
            g.add("rn", self.rn)
            g.add("g", self.g)
            g.add("addend", self.addb)
            g.add("dy", self.dyb, [("w", self.dyb.col0, C)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, P, C = self.dims
        if self.row.entry == DFWD:
            a = dict(f=ptr(self.f), ld=self.f.stride(0), w=ptr(self.w.data), B=B, P=P, C=C,
                     rn=ptr(self.rn.data) if self.full else None, ws=ptr(self.ws.data), accumulate=int(self.full),
                     val=ptr(self.val.data))
            a.update(over)
            return L.sdmi_lpips_dist_fwd(*a.values(), stream)
        full = self.full
        a = dict(f=ptr(self.f), ld=self.f.stride(0), w=ptr(self.w.data), rn=ptr(self.rn.data),
                 g=ptr(self.g.data) if full else None, gscale=float(self.c["gscale"]) if full else 1.0, B=B, P=P, C=C,
                 side=self.side, addend=ptr(self.addend) if full else None, ld_add=self.addend.stride(0) if full else 0,
                 dy=ptr(self.dy), ld_dy=self.dy.stride(0))
        a.update(over)
        return L.sdmi_lpips_dist_bwd(*a.values(), stream)

    def raw(self):
        if self.row.entry == DFWD:
            return [self.rn.buf.clone(), self.ws.buf.clone(), self.val.buf.clone()]
        return [self.dyb.buf.clone()]
