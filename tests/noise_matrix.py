"""The declared test matrix of the latent-range noise kernels (csrc/latent_noise.hip) and the helpers its exact tests
share. The pattern is tests/vq_matrix.py's.

ROWS is data: one row per launch shape, `(entry point, dims, expected launches, options)`, the launches -- a fragment
of the mangled kernel name with its template argument, and the grid -- written by hand. The host rules of
latent_noise.hip are restated below, also by hand: the flat kernels (latent_range_kernel, latent_noise_bwd_kernel) run
min(256, ceil(n / 1024)) workgroups of 256 threads, a workgroup taking 1024 consecutive elements per grid-stride trip;
the pixel kernels (latent_noise_fwd_kernel<ZIN>, latent_noise_dot_kernel) run min(256, ceil(P / 256)) workgroups, one
thread per pixel and trip; sdmi_latent_noise_workspace(n) is 16 bytes per range workgroup. sdmi_latent_range is one
launch, sdmi_latent_noise_fwd one (with or without the fused post_quant_conv), sdmi_latent_noise_bwd two: the forward
at n_scale != 0 is the randn launch plus 2, the backward 2, and n_scale == 0 launches nothing.
tests/test_noise_matrix_cpu.py checks rows against rules and that no row can be removed;
tests/test_noise_exact_gpu.py that the library launches what the rows say.

Entry points and dims: RANGE sdmi_latent_range (n); FWD sdmi_latent_noise_fwd (B, C, HW) with zin (the fused
pointwise output), ld, cout and bias; BWD sdmi_latent_noise_bwd (B, C, HW) with dzin, add (dz_add) and ld. FWD and BWD
read range partials written by the host (partials(), the layout the RANGE rows pin down), so each entry point is tested
on its own. dzin is also run as a column window of a wider NaN-filled buffer (the windows layout of vq_matrix.py).

Every row runs every plant of PLANTS on its z:

  first   the maximum in the first element, the minimum in the last (ragged) element;
  seam    two maxima on a workgroup seam (elements 1023 | 1024, or the middle of a shorter tensor), one minimum;
  spread  2^k maxima and 2^(k-1) minima evenly spread over the whole tensor (over all workgroups);
  equal   every element the same: range 0, both counts n, out == z bitwise, corr == 0 (every element doubly extremal);
  zeros   only +0.0 and -0.0: max == min although the bits differ, counts n;
  nan     `first` with one NaN: both extremes NaN, every element of out (and of zin) NaN, r == dz_add;
  ties    (soft family only) 3 copies of the maximum and 5 of the minimum: counts that are no powers of two.

Data, two families. References are computed on the CPU from the stored inputs.

  exact  z integers in [-3, 3] with the plants at +-4; eps multiples of 1 / 4 in [-4, 4]; dz_add and dzin integers
         (|value| <= m, m the largest of 4, 2, 1 at which the sum of |g eps| stays below 2^24 quarter units), W_post in
         {-1, 0, 1, 2}, the bias integer, n_scale = 2^-3, tie counts powers of two. Everything is bitwise, S included.
  soft   z, eps, dz_add, the weights randn in fp32, dzin = bf16(1e-3 randn); n_scale 0.2 and 0.074.

Statements (u = 2^-24):

  range  each partial {min, max, cnt_min, cnt_max} equals the host's over the workgroup's elements (by value: which
         of two equal zeros a partial keeps is not stated); a NaN gives {NaN, NaN, 0, 0}.
  out    bitwise fl(z + fl(fl(fl(max - min) n_scale) eps)) in fp32, every operation rounded on its own.
  zin    bitwise the fma32 chain from the bias over ci ascending on that out, RNE to bf16; pad columns zero.
  S      the kernel's own S is the last stage (one butterfly over the partials, four waves in order) of the partials
         it leaves in ws. |S - S64| <= K_S u sum |g eps|, S64 the float64 sum over the fp32 g (the fma32 chain over co
         ascending plus one fp32 add of dz_add); exact family: S == S64.
  r      bitwise fl(dz_add + corr) given that S: t = fl(n_scale S), c_max = fl(t / cnt_max), c_min = fl(t / cnt_min),
         corr = c_max at the maximum, -c_min at the minimum, fl(c_max - c_min) where both, 0 elsewhere.

K_S is measured, not chosen: tests/test_noise_matrix_cpu.py emulates S in fp32 in the kernel's order (per thread its
trips and channels in sequence, the butterfly, the four waves, then the last stage) and pairwise, every product
rounded on its own, on every soft row, and measures |S32 - S64| / (u sum |g eps|). Both orders reached 0.535, on the
one-element row (a single product's rounding, which no order can avoid; the kernel order reached 0.212 and the
pairwise 0.176 on the rows with more than one term). K_S is between twice and three times that ratio: 1.5. The CPU
test asserts 2 ratio <= K_S <= 3 ratio, that the emulations stay within K_S / 2 and that each perturbed reference
(a tie count off by one, the sign of the minimum's share flipped, c_max instead of fl(c_max - c_min) on a doubly
extremal element, 1 ulp in out) leaves its bitwise statement.

Measured on an MI355X, max(|S - S64| / bound) over all rows, plants, layouts and both n_scale: 0.356 on the one-element
row, 0.141 on the others (the products and sums are not contracted: every row's figure is the kernel-order emulation's
ratio over K_S); the exact family's S was S64 on every row; every partial, out, zin with its zero pads and r
bitwise; a second call repeats every bit.

Guards: every operand and output sits between NaN pads (dzin and zin with pad columns and rows past the end); after a
call only the declared outputs may have changed, bit for bit: the inputs, the range workspace a consumer reads, the
workspaces beyond what the launches write."""
import collections
import functools

import numpy as np
import torch

from sdmi import _lib
from tests import vq_matrix as VM
from tests.attn_matrix import Buf, launches_match, recorded  # noqa: F401
from tests.dit_matrix import butterfly32, seq32
from tests.norm_matrix import CONTIGUOUS, WINDOWS, Flat, Guard, bf16, bits, cdiv, fma32, ptr, sum32  # noqa: F401

RANGE, FWD, BWD = "range", "fwd", "bwd"
# the entry points under test and the number of arguments their bindings take, the stream included (a KeyError here:
# the library has no such entry point and nothing below can run)
ARITY = {name: len(_lib.SIGNATURES[name][0]) for name in
         ("sdmi_latent_noise_workspace", "sdmi_latent_range", "sdmi_latent_noise_fwd", "sdmi_latent_noise_bwd")}
Row = collections.namedtuple("Row", "entry dims launches opt")
U24 = 2.0 ** -24
K_S = 1.5
# largest emulated |S32 - S64| / (u sum |g eps|) over the soft rows, kernel order / pairwise (the CPU test checks them)
MEASURED = dict(kernel=0.535, pair=0.535)
PLANTS = ("first", "seam", "spread", "equal", "zeros", "nan")
SOFT_PLANTS = ("none", "ties")
SOFT_SCALES = (0.2, 0.074)
EXACT_SCALE = 0.125
LAYOUTS = (CONTIGUOUS, WINDOWS)
ORDERS = ("kernel", "pair")


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=None):
    return dict(r.opt).get(key, default)


# ----------------------------------------------------------------------------------------------------------------
# the host rules of csrc/latent_noise.hip, restated
# ----------------------------------------------------------------------------------------------------------------
NT, SPAN, CAP, MAXC = 256, 1024, 256, 8


def flat_blocks(n):
    return min(CAP, cdiv(n, SPAN))


def pixel_blocks(P):
    return min(CAP, cdiv(P, NT))


def workspace(n):
    return 16 * flat_blocks(n)


def fwd_name(zin):
    return f"latent_noise_fwd_kernelILb{int(bool(zin))}EE"


def numel(r):
    n = 1
    for d in r.dims:
        n *= d
    return n


def pixels(r):
    return r.dims[0] * r.dims[2]


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    if entry == RANGE:
        return [("latent_range_kernel", flat_blocks(dims[0]))]
    B, C, HW = dims
    if entry == FWD:
        return [(fwd_name(dict(options).get("zin")), pixel_blocks(B * HW))]
    assert entry == BWD
    return [("latent_noise_dot_kernel", pixel_blocks(B * HW)), ("latent_noise_bwd_kernel", flat_blocks(B * C * HW))]


# ----------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------
_RG, _F0, _F1 = "latent_range_kernel", "latent_noise_fwd_kernelILb0EE", "latent_noise_fwd_kernelILb1EE"
_DOT, _APP = "latent_noise_dot_kernel", "latent_noise_bwd_kernel"
ROWS = [
    R(RANGE, (1,), (_RG, 1)),
    R(RANGE, (5,), (_RG, 1)),
    # one short of a workgroup's span and one past it
    R(RANGE, (1023,), (_RG, 1)),
    R(RANGE, (1025,), (_RG, 2)),
    # three workgroups, the last ragged
    R(RANGE, (3000,), (_RG, 3)),
    # the cap: every workgroup's first trip is full, workgroup 0 takes five elements of a second one
    R(RANGE, (262149,), (_RG, 256)),
]
ROWS += [
    R(FWD, (1, 1, 1), (_F0, 1), zin=0),
    R(FWD, (1, 1, 5), (_F0, 1), zin=0),
    # one pixel short of a workgroup; C = 4, the trainer's call
    R(FWD, (1, 4, 255), (_F1, 1), zin=1, ld=8, cout=4, bias=1),
    # one pixel past it; C = 8; three range partials
    R(FWD, (1, 8, 257), (_F1, 2), zin=1, ld=8, cout=8, bias=1),
    # C = 1, no bias, a workgroup that straddles the two images, a ragged last workgroup
    R(FWD, (2, 1, 300), (_F1, 3), zin=1, ld=8, cout=1, bias=0),
    # cout != C and pad columns past the eighth
    R(FWD, (1, 4, 40), (_F1, 1), zin=1, ld=16, cout=3, bias=1),
    # a flat tensor one element past the range span: two partials to merge (add_noise's call)
    R(FWD, (1, 1, 1025), (_F0, 5), zin=0),
    # three images without the pointwise (the inference engine's call)
    R(FWD, (3, 4, 343), (_F0, 5), zin=0),
    # both caps: 256 range partials, 256 pixel workgroups of which workgroup 0 takes one pixel of a second trip
    R(FWD, (1, 4, 65537), (_F1, 256), zin=1, ld=8, cout=4, bias=1),
]
ROWS += [
    R(BWD, (1, 1, 1), (_DOT, 1), (_APP, 1), dzin=0, add=1),
    R(BWD, (1, 1, 5), (_DOT, 1), (_APP, 1), dzin=0, add=1),
    R(BWD, (1, 4, 255), (_DOT, 1), (_APP, 1), dzin=1, add=1, ld=8),
    # dz_add absent; C = 8
    R(BWD, (1, 8, 257), (_DOT, 2), (_APP, 3), dzin=1, add=0, ld=8),
    R(BWD, (2, 1, 300), (_DOT, 3), (_APP, 1), dzin=1, add=1, ld=16),
    R(BWD, (1, 1, 1025), (_DOT, 5), (_APP, 2), dzin=0, add=1),
    R(BWD, (3, 4, 343), (_DOT, 5), (_APP, 5), dzin=1, add=1, ld=8),
    R(BWD, (1, 4, 65537), (_DOT, 256), (_APP, 256), dzin=1, add=1, ld=8),
]


def row_id(r):
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{v}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# data (CPU, no library call): float64 tensors holding values exact in the stored type; flat NCHW unless said
# ----------------------------------------------------------------------------------------------------------------
def _pow2_below(v):
    k = 1
    while 2 * k <= v:
        k *= 2
    return k


def plant_positions(n, plant):
    """(positions of the maximum, positions of the minimum) the plant puts into a tensor of n elements."""
    if plant in ("first", "nan"):
        return [0], [n - 1]
    if plant == "seam":
        if n < 3:
            return [0], [n - 1]
        s = SPAN if n > SPAN + 1 else n // 2
        return [s - 1, s], [n - 1]
    if plant == "spread":
        if n < 4:
            return [0], [n - 1]
        cnt = _pow2_below(min(n // 2, 64))
        top = [(k * n) // cnt for k in range(cnt)]
        low = [p + max(1, n // (2 * cnt)) for p in top][::2]
        return top, low
    raise AssertionError(plant)


@functools.lru_cache(maxsize=None)
def z_case(kind, n, plant):
    """The clean latent, flat, float64 copies of fp32 values."""
    gen = torch.Generator().manual_seed((21000 if kind == "exact" else 22000) + 13 * n + len(plant))
    if kind == "soft":
        z = VM._rn(gen, n)
        if plant == "ties" and n >= 16:
            hi, lo = int(z.argmax()), int(z.argmin())
            free = [i for i in torch.randperm(n, generator=gen).tolist() if i not in (hi, lo)]
            z[free[:2]] = float(z[hi])
            z[free[2:6]] = float(z[lo])
        return z
    if plant == "equal":
        return torch.full((n,), 3.0, dtype=torch.float64)
    if plant == "zeros":
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        sign[0], sign[-1] = -1.0, (1.0 if n > 1 else -1.0)
        return torch.zeros(n, dtype=torch.float64) * sign
    z = VM._ri(gen, -3, 3, n)
    top, low = plant_positions(n, plant)
    z[low] = -4.0
    z[top] = 4.0                  # (n = 1: the one element is both)
    if plant == "nan":
        z[n // 2] = float("nan")
    return z


def eps_case(kind, n, gen):
    return VM._ri(gen, -16, 16, n) / 4.0 if kind == "exact" else VM._rn(gen, n)


@functools.lru_cache(maxsize=None)
def fwd_case(kind, B, C, HW, cout, bias):
    n = B * C * HW
    gen = torch.Generator().manual_seed((23000 if kind == "exact" else 24000) + 7 * n + 3 * C + (cout or 0))
    c = dict(kind=kind, B=B, C=C, HW=HW, eps=eps_case(kind, n, gen), w=None, b=None, cout=cout)
    if cout:
        c["w"] = VM._ri(gen, -1, 2, cout, C) if kind == "exact" else VM._rn(gen, cout, C)
        if bias:
            c["b"] = VM._ri(gen, -4, 4, cout) if kind == "exact" else VM._rn(gen, cout)
    return c


@functools.lru_cache(maxsize=None)
def bwd_case(kind, B, C, HW, dzin, add):
    P, n = B * HW, B * C * HW
    gen = torch.Generator().manual_seed((25000 if kind == "exact" else 26000) + 7 * n + 3 * C + 2 * dzin + add)
    c = dict(kind=kind, B=B, C=C, HW=HW, eps=eps_case(kind, n, gen), dzin=None, add=None, w_post=None)
    if kind == "soft":
        if dzin:
            c.update(dzin=bf16(1e-3 * VM._rn(gen, P, C)), w_post=VM._rn(gen, C, C))
        if add:
            c["add"] = 1e-3 * VM._rn(gen, n) if dzin else VM._rn(gen, n)
            c["add"] = c["add"].float().double()
        return c
    if dzin:
        c["w_post"] = VM._ri(gen, -1, 2, C, C)
    unit_dz, unit_add = VM._ri(gen, -4, 4, P, C), VM._ri(gen, -4, 4, n)
    for m in (1, 2, 4):          # the largest magnitude whose sum of |g eps| stays exact in any order
        trial = dict(c, dzin=(unit_dz / m).trunc() if dzin else None, add=(unit_add / m).trunc() if add else None)
        if exact_margin(trial) < 2.0 ** 24:
            return trial
    raise AssertionError("no exact magnitude")


def exact_margin(c):
    """sum |g eps| of an exact case in units of its last possible bit (eps is a multiple of 1 / 4)."""
    g = g_reference(c)
    return float((g * VM.from_nchw(c["eps"], c["B"], c["HW"], c["C"])).abs().sum()) * 4.0


# ----------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------
def range_reference(z):
    """(min, max, cnt_min, cnt_max) as torch does: a NaN anywhere makes both extremes NaN (counts 0)."""
    if bool(torch.isnan(z).any()):
        return float("nan"), float("nan"), 0, 0
    mn, mx = float(z.min()), float(z.max())
    return mn, mx, int((z == mn).sum()), int((z == mx).sum())


def block_of(n):
    """The range workgroup of every element."""
    return (torch.arange(n) // SPAN) % flat_blocks(n)


def partials(z):
    """What latent_range_kernel leaves in ws: per workgroup (min, max, cnt_min, cnt_max), as ([grid][2] float64,
    [grid][2] int64)."""
    n, grid = z.numel(), flat_blocks(z.numel())
    blk = block_of(n)
    val, cnt = torch.zeros(grid, 2, dtype=torch.float64), torch.zeros(grid, 2, dtype=torch.int64)
    for b in range(grid):
        mn, mx, cmn, cmx = range_reference(z[blk == b])
        val[b, 0], val[b, 1], cnt[b, 0], cnt[b, 1] = mn, mx, cmn, cmx
    return val, cnt


def partial_words(z):
    """The partials as the fp32 words of the workspace (counts as int bits)."""
    val, cnt = partials(z)
    w = torch.empty(val.shape[0], 4, dtype=torch.float32)
    w[:, :2] = val.float()
    w[:, 2:] = cnt.to(torch.int32).view(torch.float32)
    return w.reshape(-1)


def scale32(z, n_scale):
    """fl(fl(max - min) n_scale) in fp32."""
    mn, mx, _, _ = range_reference(z)
    return np.float32(np.float32(mx) - np.float32(mn)) * np.float32(n_scale)


def out_reference(z, eps, n_scale):
    """fl(z + fl(s eps)), float64 copies; torch's CPU fp32 operators round every operation on its own."""
    s = torch.tensor(float(scale32(z, n_scale)), dtype=torch.float32)
    return (z.float() + s * eps.float()).double()


def zin_reference(c, out):
    """[P][cout]: the fma32 chain from the bias over ci ascending on out, RNE to bf16 (NaN stays NaN)."""
    o = VM.from_nchw(out, c["B"], c["HW"], c["C"])
    return bf16(VM.conv_chain(o, c["w"], c["b"]))


def g_reference(c):
    """g [P][C]: the fma32 chain over co ascending of W_post^T dzin plus one fp32 add of dz_add; float64 copies."""
    B, C, HW = c["B"], c["C"], c["HW"]
    add = VM.from_nchw(c["add"], B, HW, C) if c["add"] is not None else None
    if c["dzin"] is None:
        return add
    s = torch.zeros(B * HW, C, dtype=torch.float32)
    for co in range(C):
        s = fma32(c["w_post"][co].float()[None, :], c["dzin"][:, co].float()[:, None], s)
    if add is not None:
        s = s + add.float()
    return s.double()


def s_reference(c):
    """(terms [P][C] fp32 rounded products, S64, T = sum |g eps|)."""
    g = g_reference(c)
    e = VM.from_nchw(c["eps"], c["B"], c["HW"], c["C"])
    return g.float() * e.float(), float((g * e).sum()), float((g * e).abs().sum())


def r_reference(c, z, S, n_scale, count_off=0, flip_min=False, both_is_max=False):
    """fl(dz_add + corr) given the fp32 S; flat float64. The keyword arguments are the perturbations of the CPU test."""
    mn, mx, cmn, cmx = range_reference(z)
    add = c["add"].float() if c["add"] is not None else torch.zeros(z.numel(), dtype=torch.float32)
    if mn != mn:
        return add.double()
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.float32(n_scale) * np.float32(S)
        c_max, c_min = t / np.float32(cmx + count_off), t / np.float32(cmn)
        both = c_max if both_is_max else c_max - c_min
    at_max, at_min = z == mx, z == mn
    corr = torch.zeros(z.numel(), dtype=torch.float32)
    corr[at_min] = float(c_min if flip_min else -c_min)
    corr[at_max] = float(c_max)
    corr[at_max & at_min] = float(both)
    return (add + corr).double()


def sum_bound(T, K=None):
    return (K_S if K is None else K) * U24 * T


# ----------------------------------------------------------------------------------------------------------------
# fp32 emulation of S in two orders (CPU, torch), every product rounded on its own
# ----------------------------------------------------------------------------------------------------------------
def last_stage(part):
    """latent_noise_bwd_kernel's S from the partials: thread t holds partial t (or 0), one butterfly per wave, the
    four waves in order."""
    return seq32(butterfly32(VM._pad(part.float(), NT).view(NT // 64, 64)), 0)


def emulate_partials(terms):
    """latent_noise_dot_kernel: each thread adds its trips' pixels, channels ascending, in sequence; the butterfly; the
    four waves in order. [grid] fp32."""
    P, C = terms.shape
    grid = pixel_blocks(P)
    trips = cdiv(P, grid * NT)
    t = VM._pad(terms.float(), trips * grid * NT).view(trips, grid, NT // 64, 64, C)
    t = seq32(t.permute(0, 4, 1, 2, 3).reshape(trips * C, grid, NT // 64, 64), 0)
    return seq32(butterfly32(t), 1)


def emulate_S(terms, order):
    if order == "pair":
        return float(sum32(terms.float().reshape(-1), 0, "pair"))
    return float(last_stage(emulate_partials(terms)))


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
def _flat(n, device, values=None):
    return VM._flat(n, device, values)


class RangeProblem:
    def __init__(self, z, device="cuda"):
        self.n = z.numel()
        self.blocks = flat_blocks(self.n)
        self.z = _flat(self.n, device, z)
        self.ws = _flat(workspace(self.n) // 4, device)

    def guard(self, writes=True):
        g = Guard()
        g.add("z", self.z)
        g.add("workspace", self.ws, [(0, 4 * self.blocks)] if writes else [])
        return g

    def run(self, L, stream, **over):
        a = dict(z=ptr(self.z.data), n=self.n, ws=ptr(self.ws.data))
        a.update(over)
        return L.sdmi_latent_range(*a.values(), stream)

    def outputs(self):
        """([grid][2] float64 extremes, [grid][2] int64 counts)."""
        w = self.ws.data.cpu().view(self.blocks, 4)
        return w[:, :2].double(), w[:, 2:].contiguous().view(torch.int32).long()

    def raw(self):
        return [self.ws.buf.clone()]


class FwdProblem:
    def __init__(self, c, z, row, n_scale, device="cuda"):
        B, C, HW = row.dims
        self.c, self.dims, self.P, self.n, self.n_scale = c, row.dims, B * HW, B * C * HW, n_scale
        self.with_zin, self.ld, self.cout = bool(opt(row, "zin")), opt(row, "ld", 0), opt(row, "cout", 0)
        self.z, self.eps = _flat(self.n, device, z), _flat(self.n, device, c["eps"])
        self.ws = _flat(workspace(self.n) // 4, device, partial_words(z))
        self.out = _flat(self.n, device)
        self.w = _flat(max(self.cout, 1) * C, device, c["w"])
        self.b = _flat(max(self.cout, 1), device, c["b"])
        self.zinb = Buf(self.P, max(self.ld, 1), torch.bfloat16, device)
        self.zin = self.zinb.window(0, max(self.ld, 1))

    def guard(self, writes=True):
        g = Guard()
        for name in ("z", "eps", "ws", "w", "b"):
            g.add(name, getattr(self, name))
        g.add("out", self.out, [(0, self.n)] if writes else [])
        g.add("zin", self.zinb, [("w", 0, self.zinb.ld)] if writes and self.with_zin else [])
        return g

    def run(self, L, stream, **over):
        B, C, HW = self.dims
        on = self.with_zin
        a = dict(z=ptr(self.z.data), eps=ptr(self.eps.data), B=B, C=C, HW=HW, n_scale=self.n_scale,
                 ws=ptr(self.ws.data), out=ptr(self.out.data), w_post=ptr(self.w.data) if on else None,
                 b_post=ptr(self.b.data) if on and self.c["b"] is not None else None, cout=self.cout,
                 zin=ptr(self.zin) if on else None, ld=self.ld)
        a.update(over)
        return L.sdmi_latent_noise_fwd(*a.values(), stream)

    def raw(self):
        return [self.out.buf.clone(), self.zinb.buf.clone()]


class BwdProblem:
    def __init__(self, c, z, row, n_scale, layout, device="cuda"):
        B, C, HW = row.dims
        self.c, self.dims, self.P, self.n, self.n_scale = c, row.dims, B * HW, B * C * HW, n_scale
        self.blocks = pixel_blocks(self.P)
        self.z, self.eps = _flat(self.n, device, z), _flat(self.n, device, c["eps"])
        self.add = _flat(self.n, device, c["add"])
        self.w_post = _flat(C * C, device, c["w_post"])
        self.dzinb, self.dzin = VM._window(self.P, opt(row, "ld", C), C, torch.bfloat16, layout, device, c["dzin"])
        self.ws_range = _flat(workspace(self.n) // 4, device, partial_words(z))
        self.ws = _flat(workspace(self.n) // 4, device)
        self.r = _flat(self.n, device)

    def guard(self, writes=True):
        g = Guard()
        g.add("dzin", self.dzinb)
        for name in ("z", "eps", "add", "w_post", "ws_range"):
            g.add(name, getattr(self, name))
        g.add("workspace", self.ws, [(0, self.blocks)] if writes else [])
        g.add("r", self.r, [(0, self.n)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, C, HW = self.dims
        c = self.c
        on = c["dzin"] is not None
        a = dict(dzin=ptr(self.dzin) if on else None, ld_dzin=self.dzin.stride(0) if on else 0,
                 w_post=ptr(self.w_post.data) if on else None, dz_add=ptr(self.add.data) if c["add"] is not None else None,
                 eps=ptr(self.eps.data), z=ptr(self.z.data), B=B, C=C, HW=HW, n_scale=self.n_scale,
                 ws_range=ptr(self.ws_range.data), ws=ptr(self.ws.data), r=ptr(self.r.data))
        a.update(over)
        return L.sdmi_latent_noise_bwd(*a.values(), stream)

    def raw(self):
        return [self.ws.buf.clone(), self.r.buf.clone()]
