"""The declared test matrix of the KL autoencoder's latent kernels (csrc/kl_latent.hip) and the helpers its exact tests
share. The pattern is tests/noise_matrix.py's.

ROWS is data: one row per launch shape, `(entry point, (B, z, HW), expected launches, options)`, the launches -- a
fragment of the kernel name and the grid -- written by hand. The host rules of kl_latent.hip are restated below, also by
hand: both pixel kernels run min(256, ceil(P / 256)) workgroups of 256 threads, one thread per pixel and grid-stride trip
(P = B HW); the two finishers are one workgroup. sdmi_kl_sample is one launch, two with kl; sdmi_kl_bwd two.
sdmi_kl_workspace(P) is 4 bytes per pixel workgroup, sdmi_kl_bwd_workspace() 256 rows of PART = 92 floats.
tests/test_kl_matrix_cpu.py checks rows against rules; tests/test_kl_exact_gpu.py that the library launches what the rows
say.

Shapes: (1, 1, 1) the smallest; (1, 3, 255) and (2, 4, 257) ragged tails on either side of one workgroup; (2, 4, 1025)
several workgroups; (2, 4, 33000) 66 000 pixels, more than the 65 536 a capped grid covers in one trip. Every shape
runs a full row (eps, zin, both biases, kl; dzin, eps, dsample_add, dmom_add, kl_weight) and a bare row (none of the
optional operands), a few shapes mixed rows; every row runs with the leading dimensions equal to the widths and as
column windows of wider NaN-filled buffers, in two data families. M = 2z.

  exact  h integers in [-2, 2]; w_pre's mean rows one +-1 each and an integer bias, its log-variance rows and their
         bias zero, so that logvar = 0, std = 1 and exp(logvar) - 1 = 0 exactly: no exp rounding enters anywhere. eps
         multiples of 1 / 4 in [-2, 2]; w_post in {-1, 0, 1}, dzin in {-1, 0, 1}, dsample_add integer, dmom_add quarter
         units, kl_weight = B / 8 (so c = 1 / 8). Everything is bitwise, the sums included (every partial sum stays
         below 2^24 units of its last bit; the CPU test checks that margin for every row).
  soft   h, eps, the weights and biases randn in fp32 (w_pre scaled by 1 / 2); dzin = bf16(1e-3 randn), dsample_add
         and dmom_add 1e-3 randn, kl_weight 1e-4.

Statements (u = 2^-24):

  moments  bitwise the fma32 chain from the bias (0 without) over ci ascending.
  exp      the kernel's expf is observed through the kernel itself: with mean 0 and eps 1 the sample IS std, so a probe
           call (device_exp in the GPU test) returns expf(x) for any fp32 x. std32 = expf(fl(0.5 logvar)) and E32 =
           expf(logvar) each lie within E_ULPS = 2 ulps of the float64 exp (ROCm documents its device expf at 1 ulp; 2
           lets any conforming expf pass and a missing 0.5 misses by orders of magnitude).
  sample   bitwise fl(mean + fl(std32 eps)); without eps the mean. zin bitwise the fma32 chain from the bias over ci
           ascending on that sample, RNE to bf16, pad columns zero.
  KL       terms fl(fl(fl(E32 + fl(mean mean)) - 1) - logvar); the kernel's kl is bitwise fl(fl(0.5 S) / B) of the last
           stage over the partials it leaves in ws; |S - S64| <= K_KL u sum |terms|, S64 the float64 sum of the fp32
           terms; exact family: S == S64.
  dmom     bitwise given std32 and t32 = fl(E32 - 1): g the fma32 chain over co ascending then one add of dsample_add;
           dmean = g, + dmom_add, + fl(c mean); dlogvar = fl(fl(fl(g eps) 0.5) std32), + dmom_add, + fl(fl(c 0.5) t32);
           c = fl(kl_weight / B). dh bitwise the fma32 chain over co ascending on that dmom, RNE to bf16, pads zero.
  sums     dW_post, db_post, dW_pre, db_pre within K_KL u sum |terms| of the float64 sum of the exact products of the fp32
           factors; exact family: equal.

K_KL is measured, not chosen: tests/test_kl_matrix_cpu.py emulates every sum in fp32 in the kernel's order (per thread
its trips in sequence, channels ascending for KL; the butterfly; the four waves in order; then the workgroups in order,
or for KL the last stage's butterfly), every product rounded on its own (one rounding more per term than the kernel's
fma: the coarser model), on every soft row and measures |S32 - S64| / (u sum |terms|). The largest ratio was 0.904 (the KL
sum of the 765 terms of the (1, 3, 255) row; 0.725 on the one-pixel row's dW_pre, a single product's rounding; at most
0.34 on every other row and sum). K_KL is between twice and three times that: 2.25. The CPU test asserts
2 ratio <= K_KL <= 3 ratio and that each perturbed reference (the 0.5 in std dropped, the -1 in dlogvar dropped, 1 / B
replaced by 1 / (B P), the mean and log-variance halves swapped, dmom_add ignored) leaves its statement.

Measured on an MI355X over all rows, families and layouts: the kernel's expf at most 0.83 ulps from the float64 exp;
max(|S - S64| / bound) 0.334 (the KL sum of the (1, 3, 255) row; 0.32 on the one-pixel rows, at most 0.15 elsewhere); the
exact family's sums equal; everything else bitwise; a second call repeats every bit.

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
from tests.noise_matrix import emulate_partials, last_stage
from tests.norm_matrix import CONTIGUOUS, WINDOWS, Flat, Guard, bf16, bits, cdiv, fma32, ptr, ulp32  # noqa: F401

SAMPLE, BWD = "sample", "bwd"
ARITY = {name: len(_lib.SIGNATURES[name][0]) for name in
         ("sdmi_kl_workspace", "sdmi_kl_bwd_workspace", "sdmi_kl_sample", "sdmi_kl_bwd")}
Row = collections.namedtuple("Row", "entry dims launches opt")
U24 = 2.0 ** -24
E_ULPS = 2.0
K_KL = 2.25
MEASURED = 0.904  # largest emulated |S32 - S64| / (u sum |terms|) over the soft rows (the CPU test checks it)
LAYOUTS = (CONTIGUOUS, WINDOWS)
KINDS = ("exact", "soft")
SOFT_KW = 1e-4

NT, CAP, MAXC, MAXZ = 256, 256, 8, 4
PART = MAXZ * MAXZ + MAXZ + MAXC * MAXC + MAXC


def pixel_blocks(P):
    return min(CAP, cdiv(P, NT))


def workspace(P):
    return 4 * pixel_blocks(P)


def bwd_workspace():
    return 4 * CAP * PART


def R(entry, dims, *launches, **opt):
    return Row(entry, tuple(dims), launches, tuple(sorted(opt.items())))


def opt(r, key, default=0):
    return dict(r.opt).get(key, default)


def expected_launches(entry, dims, options=()):
    """The launches of one row by the restated rules (used by the CPU test, never by ROWS)."""
    B, z, HW = dims
    g = pixel_blocks(B * HW)
    if entry == SAMPLE:
        return [("kl_sample_kernel", g)] + ([("kl_loss_kernel", 1)] if dict(options).get("kl") else [])
    return [("kl_bwd_kernel", g), ("kl_bwd_finish_kernel", 1)]


_S, _KL, _B, _BF = "kl_sample_kernel", "kl_loss_kernel", "kl_bwd_kernel", "kl_bwd_finish_kernel"
_FULL_S = dict(eps=1, zin=1, ld=8, bias=1, kl=1)
_FULL_B = dict(dzin=1, ld=8, eps=1, dsample=1, dmom=1, kw=1, dh=1, ld_out=8)
_BARE_B = dict(dzin=1, ld=8, dh=1, ld_out=8)
ROWS = [
    R(SAMPLE, (1, 1, 1), (_S, 1), (_KL, 1), **_FULL_S),
    R(SAMPLE, (1, 1, 1), (_S, 1)),
    R(SAMPLE, (1, 3, 255), (_S, 1), (_KL, 1), **_FULL_S),
    R(SAMPLE, (1, 3, 255), (_S, 1)),
    # pad columns past the eighth, no bias, no kl
    R(SAMPLE, (1, 3, 255), (_S, 1), eps=1, zin=1, ld=16),
    R(SAMPLE, (2, 4, 257), (_S, 3), (_KL, 1), **_FULL_S),
    R(SAMPLE, (2, 4, 257), (_S, 3)),
    # zin = post_quant_conv(mean): nothing random
    R(SAMPLE, (2, 4, 257), (_S, 3), (_KL, 1), zin=1, ld=8, bias=1, kl=1),
    R(SAMPLE, (2, 4, 1025), (_S, 9), (_KL, 1), **_FULL_S),
    R(SAMPLE, (2, 4, 1025), (_S, 9)),
    # the cap: 464 pixels go to a second grid-stride trip
    R(SAMPLE, (2, 4, 33000), (_S, 256), (_KL, 1), **_FULL_S),
    R(SAMPLE, (2, 4, 33000), (_S, 256)),
]
ROWS += [
    R(BWD, (1, 1, 1), (_B, 1), (_BF, 1), **_FULL_B),
    R(BWD, (1, 1, 1), (_B, 1), (_BF, 1), **_BARE_B),
    R(BWD, (1, 3, 255), (_B, 1), (_BF, 1), **_FULL_B),
    R(BWD, (1, 3, 255), (_B, 1), (_BF, 1), **_BARE_B),
    # the leaf path's call: no decoder gradient, no dh, the fp32 gradient of the moments alone
    R(BWD, (1, 3, 255), (_B, 1), (_BF, 1), eps=1, dsample=1, dmom=1),
    R(BWD, (2, 4, 257), (_B, 3), (_BF, 1), **_FULL_B),
    R(BWD, (2, 4, 257), (_B, 3), (_BF, 1), **_BARE_B),
    # the module's call: the user's KL gradient through dmom_add, kl_weight 0, wide dzin and dh
    R(BWD, (2, 4, 257), (_B, 3), (_BF, 1), dzin=1, ld=16, eps=1, dmom=1, dh=1, ld_out=16),
    R(BWD, (2, 4, 1025), (_B, 9), (_BF, 1), **_FULL_B),
    R(BWD, (2, 4, 1025), (_B, 9), (_BF, 1), **_BARE_B),
    R(BWD, (2, 4, 33000), (_B, 256), (_BF, 1), **_FULL_B),
    R(BWD, (2, 4, 33000), (_B, 256), (_BF, 1), **_BARE_B),
]


def row_id(r):
    return f"{r.entry}-" + "x".join(str(d) for d in r.dims) + "".join(f"-{k}{v}" for k, v in r.opt)


def rows_of(*entries):
    return [r for r in ROWS if r.entry in entries]


# ----------------------------------------------------------------------------------------------------------------
# data (CPU): float64 tensors holding values exact in the stored type; rows are [P][channels], flat ones NCHW
# ----------------------------------------------------------------------------------------------------------------
def _mean_rows(gen, z):
    """w_pre of the exact family: mean row co has one +-1, the log-variance rows are zero."""
    M = 2 * z
    w = torch.zeros(M, M, dtype=torch.float64)
    for co in range(z):
        w[co, int(torch.randint(0, M, (1,), generator=gen))] = 1.0 if int(torch.randint(0, 2, (1,), generator=gen)) else -1.0
    return w


@functools.lru_cache(maxsize=None)
def sample_case(kind, B, z, HW, bias):
    P, M = B * HW, 2 * z
    gen = torch.Generator().manual_seed((31000 if kind == "exact" else 32000) + 7 * P + 3 * z + bias)
    c = dict(kind=kind, B=B, z=z, HW=HW, b_pre=None, b_post=None)
    if kind == "exact":
        c.update(h=VM._ri(gen, -2, 2, P, M), w_pre=_mean_rows(gen, z), eps=VM._ri(gen, -8, 8, B * z * HW) / 4.0,
                 w_post=VM._ri(gen, -1, 1, z, z))
        if bias:
            c["b_pre"] = torch.cat([VM._ri(gen, -1, 1, z), torch.zeros(z, dtype=torch.float64)])
            c["b_post"] = VM._ri(gen, -4, 4, z)
    else:
        c.update(h=VM._rn(gen, P, M), w_pre=(0.5 * VM._rn(gen, M, M)).float().double(), eps=VM._rn(gen, B * z * HW),
                 w_post=VM._rn(gen, z, z))
        if bias:
            c["b_pre"], c["b_post"] = VM._rn(gen, M), VM._rn(gen, z)
    return c


@functools.lru_cache(maxsize=None)
def bwd_case(kind, B, z, HW):
    P, M = B * HW, 2 * z
    gen = torch.Generator().manual_seed((33000 if kind == "exact" else 34000) + 7 * P + 3 * z)
    c = dict(kind=kind, B=B, z=z, HW=HW)
    if kind == "exact":
        mom = torch.cat([VM._ri(gen, -3, 3, P, z), torch.zeros(P, z, dtype=torch.float64)], 1)
        c.update(dzin=VM._ri(gen, -1, 1, P, z), w_post=VM._ri(gen, -1, 1, z, z), sample=VM._ri(gen, -16, 16, P, z) / 4.0,
                 moments=mom, eps=VM._ri(gen, -8, 8, P, z) / 4.0, h=VM._ri(gen, -2, 2, P, M),
                 w_pre=VM._ri(gen, -1, 2, M, M), dsample=VM._ri(gen, -2, 2, P, z), dmom=VM._ri(gen, -8, 8, P, M) / 4.0,
                 kw=B / 8.0)
    else:
        f = lambda t: t.float().double()  # noqa: E731
        c.update(dzin=bf16(1e-3 * VM._rn(gen, P, z)), w_post=VM._rn(gen, z, z), sample=VM._rn(gen, P, z),
                 moments=VM._rn(gen, P, M), eps=VM._rn(gen, P, z), h=VM._rn(gen, P, M), w_pre=VM._rn(gen, M, M),
                 dsample=f(1e-3 * VM._rn(gen, P, z)), dmom=f(1e-3 * VM._rn(gen, P, M)), kw=SOFT_KW)
    return c


def nchw(rows, B, HW):
    return VM.nchw(rows, B, HW)


def rows_of_nchw(flat, B, HW, C):
    return VM.from_nchw(flat, B, HW, C)


# ----------------------------------------------------------------------------------------------------------------
# references. exp32: a callable fp32 tensor -> fp32 tensor, the expf in use (torch's on the CPU, the kernel's own --
# observed through the probe -- on the GPU)
# ----------------------------------------------------------------------------------------------------------------
def cpu_exp32(x):
    return torch.exp(x.float())


def exp_within(got32, x32, ulps=E_ULPS):
    """Largest |got - exp64(x)| / (ulps ulp(exp64(x))) over the elements."""
    ref = torch.exp(x32.double())
    return float(((got32.double() - ref).abs() / (ulps * ulp32(ref))).max()) if got32.numel() else 0.0


def moments_reference(c, with_bias=True):
    """[P][M] float64 copies of the fp32 fma chain."""
    return VM.conv_chain(c["h"], c["w_pre"], c["b_pre"] if with_bias else None)


def halves(mom, z, swap=False):
    mean, lv = mom[:, :z].float(), mom[:, z:].float()
    return (lv, mean) if swap else (mean, lv)


def std_of(lv, exp32=cpu_exp32, half=0.5):
    return exp32(np.float32(half) * lv)


def sample_reference(mom, z, eps_rows, std32, swap=False):
    """[P][z]: fl(mean + fl(std32 eps)) (torch's CPU fp32 operators round each operation on its own)."""
    mean, _ = halves(mom, z, swap)
    if eps_rows is None:
        return mean.double()
    return (mean + std32.float() * eps_rows.float()).double()


def zin_reference(sample_rows, w_post, b_post):
    return bf16(VM.conv_chain(sample_rows, w_post, b_post))


def kl_terms(mom, z, E32):
    mean, lv = halves(mom, z)
    return ((E32.float() + mean * mean) - 1.0) - lv


def kl_value(S32, B):
    return float((np.float32(0.5) * np.float32(S32)) / np.float32(B))


def g_reference(c, row):
    """[P][z] fp32: the fma32 chain from 0 over co ascending of W_post^T dzin, then one fp32 add of dsample_add."""
    z = c["z"]
    s = torch.zeros(c["B"] * c["HW"], z, dtype=torch.float32)
    if opt(row, "dzin"):
        for co in range(z):
            s = fma32(c["w_post"][co].float()[None, :], c["dzin"][:, co].float()[:, None], s)
    if opt(row, "dsample"):
        s = s + c["dsample"].float()
    return s


def kw_of(c, row):
    return float(c["kw"]) if opt(row, "kw") else 0.0


def dmom_reference(c, row, std32, t32, minus_one=True, per_pixel=False, use_add=True, E32=None):
    """[P][M] float64 copies of the fp32 gradient of the moments. t32 = fl(E32 - 1); the keyword arguments are the
    perturbations of the CPU test (minus_one False: E32 in place of t32)."""
    z, B = c["z"], c["B"]
    g = g_reference(c, row)
    mean = c["moments"][:, :z].float()
    dm = g.clone()
    dl = ((g * c["eps"].float()) * 0.5) * std32.float() if opt(row, "eps") else torch.zeros_like(g)
    if opt(row, "dmom") and use_add:
        dm = dm + c["dmom"][:, :z].float()
        dl = dl + c["dmom"][:, z:].float()
    kw = kw_of(c, row)
    cc = np.float32(kw) / np.float32(B * (c["B"] * c["HW"]) if per_pixel else B)
    if cc != 0:
        dm = dm + float(cc) * mean
        dl = dl + float(np.float32(cc) * np.float32(0.5)) * (t32.float() if minus_one else E32.float())
    return torch.cat([dm, dl], 1).double()


def dh_reference(dmom, w_pre):
    """[P][M]: the fma32 chain from 0 over co ascending of w_pre[co][ci] dmom[co], RNE to bf16."""
    M = w_pre.shape[0]
    s = torch.zeros(dmom.shape[0], M, dtype=torch.float32)
    for co in range(M):
        s = fma32(w_pre[co].float()[None, :], dmom[:, co].float()[:, None], s)
    return bf16(s)


def grad_terms(c, row, dmom):
    """{name: (exact products [P][n] float64, shape)} of the four parameter-gradient sums."""
    z, M = c["z"], 2 * c["z"]
    out = {}
    if opt(row, "dzin"):
        out["dw_post"] = ((c["dzin"][:, :, None] * c["sample"][:, None, :]).reshape(-1, z * z), (z, z))
        out["db_post"] = (c["dzin"].clone(), (z,))
    out["dw_pre"] = ((dmom[:, :, None] * c["h"][:, None, :]).reshape(-1, M * M), (M, M))
    out["db_pre"] = (dmom.clone(), (M,))
    return out


def sum_bound(T, K=None):
    return (K_KL if K is None else K) * U24 * T


# ----------------------------------------------------------------------------------------------------------------
# fp32 emulation of the sums in the kernels' order (CPU, torch), every product rounded on its own
# ----------------------------------------------------------------------------------------------------------------
def emulate_kl_S(terms):
    """kl_sample_kernel's partials and kl_loss_kernel's last stage."""
    return float(last_stage(emulate_partials(terms)))


def emulate_grad(terms):
    """kl_bwd_kernel + kl_bwd_finish_kernel over [P][n] fp32 terms: per thread its trips in sequence, the butterfly, the
    four waves in order, then the workgroups in order. [n] fp32."""
    P, n = terms.shape
    grid = pixel_blocks(P)
    trips = cdiv(P, grid * NT)
    t = VM._pad(terms.float(), trips * grid * NT).view(trips, grid, NT // 64, 64, n)
    t = seq32(t, 0).permute(0, 1, 3, 2).contiguous()             # [grid][4][n][64]
    return seq32(seq32(butterfly32(t), 1), 0)


# ----------------------------------------------------------------------------------------------------------------
# guarded device problems
# ----------------------------------------------------------------------------------------------------------------
def _flat(n, device, values=None):
    return VM._flat(n, device, values)


class SampleProblem:
    def __init__(self, c, row, layout, device="cuda", w_pre=None, b_pre="case", h=None, eps="case"):
        B, z, HW = row.dims
        P, M = B * HW, 2 * z
        self.c, self.dims, self.P, self.M = c, row.dims, P, M
        self.with_eps, self.with_zin, self.with_kl = bool(opt(row, "eps")), bool(opt(row, "zin")), bool(opt(row, "kl"))
        self.ld = opt(row, "ld", 0)
        self.blocks = pixel_blocks(P)
        self.hb, self.h = VM._window(P, M, M, torch.float32, layout, device, c["h"] if h is None else h)
        self.w_pre = _flat(M * M, device, c["w_pre"] if w_pre is None else w_pre)
        bp = c["b_pre"] if isinstance(b_pre, str) else b_pre
        self.has_b_pre = bp is not None
        self.b_pre = _flat(M, device, bp)
        e = c["eps"] if isinstance(eps, str) else eps
        self.eps = _flat(B * z * HW, device, e)
        self.moments, self.sample = _flat(B * M * HW, device), _flat(B * z * HW, device)
        self.w_post, self.b_post = _flat(z * z, device, c["w_post"]), _flat(z, device, c["b_post"])
        # (an output's row stride is the width the kernel writes, pad columns included: windows are for operands)
        self.zinb = Buf(P, max(self.ld, 1), torch.bfloat16, device)
        self.zin = self.zinb.window(0, max(self.ld, 1))
        self.ws, self.kl = _flat(self.blocks, device), _flat(1, device)

    def guard(self, writes=True):
        B, z, HW = self.dims
        g = Guard()
        g.add("h", self.hb)
        for name in ("w_pre", "b_pre", "eps", "w_post", "b_post"):
            g.add(name, getattr(self, name))
        g.add("moments", self.moments, [(0, B * self.M * HW)] if writes else [])
        g.add("sample", self.sample, [(0, B * z * HW)] if writes else [])
        g.add("zin", self.zinb, [("w", 0, max(self.ld, 1))] if writes and self.with_zin else [])
        g.add("workspace", self.ws, [(0, self.blocks)] if writes and self.with_kl else [])
        g.add("kl", self.kl, [(0, 1)] if writes and self.with_kl else [])
        return g

    def run(self, L, stream, **over):
        B, z, HW = self.dims
        on = self.with_zin
        a = dict(h=ptr(self.h), ldh=self.h.stride(0), w_pre=ptr(self.w_pre.data),
                 b_pre=ptr(self.b_pre.data) if self.has_b_pre else None,
                 eps=ptr(self.eps.data) if self.with_eps else None, B=B, z=z, HW=HW, moments=ptr(self.moments.data),
                 sample=ptr(self.sample.data), w_post=ptr(self.w_post.data) if on else None,
                 b_post=ptr(self.b_post.data) if on and self.c["b_post"] is not None else None,
                 zin=ptr(self.zin) if on else None, ld=self.zin.stride(0) if on else 0,
                 ws=ptr(self.ws.data) if self.with_kl else None, kl=ptr(self.kl.data) if self.with_kl else None)
        a.update(over)
        return L.sdmi_kl_sample(*a.values(), stream)

    def rows(self, flat, C):
        B, z, HW = self.dims
        return rows_of_nchw(flat.get(B * C * HW), B, HW, C)

    def raw(self):
        return [self.moments.buf.clone(), self.sample.buf.clone(), self.zinb.buf.clone(), self.ws.buf.clone(),
                self.kl.buf.clone()]


class BwdProblem:
    def __init__(self, c, row, layout, device="cuda", kw=None):
        B, z, HW = row.dims
        P, M = B * HW, 2 * z
        self.c, self.row, self.dims, self.P, self.M = c, row, row.dims, P, M
        self.blocks = pixel_blocks(P)
        self.kw = kw_of(c, row) if kw is None else kw
        self.dzinb, self.dzin = VM._window(P, max(opt(row, "ld", z), z), z, torch.bfloat16, layout, device, c["dzin"])
        self.hb, self.h = VM._window(P, M, M, torch.float32, layout, device, c["h"])
        ldo = max(opt(row, "ld_out", M), M)
        self.dhb = Buf(P, ldo, torch.bfloat16, device)
        self.dh = self.dhb.window(0, ldo)
        self.w_post, self.w_pre = _flat(z * z, device, c["w_post"]), _flat(M * M, device, c["w_pre"])
        self.sample = _flat(P * z, device, nchw(c["sample"], B, HW))
        self.moments = _flat(P * M, device, nchw(c["moments"], B, HW))
        self.eps = _flat(P * z, device, nchw(c["eps"], B, HW))
        self.dsample = _flat(P * z, device, nchw(c["dsample"], B, HW))
        self.dmom_add = _flat(P * M, device, nchw(c["dmom"], B, HW))
        self.dmom = _flat(P * M, device)
        self.ws = _flat(CAP * PART, device)
        self.dw_post, self.db_post = _flat(z * z, device), _flat(z, device)
        self.dw_pre, self.db_pre = _flat(M * M, device), _flat(M, device)

    def guard(self, writes=True):
        row, z, M = self.row, self.dims[1], self.M
        on = bool(opt(row, "dzin"))
        g = Guard()
        g.add("dzin", self.dzinb)
        g.add("h", self.hb)
        for name in ("w_post", "w_pre", "sample", "moments", "eps", "dsample", "dmom_add"):
            g.add(name, getattr(self, name))
        g.add("dh", self.dhb, [("w", 0, self.dh.shape[1])] if writes and opt(row, "dh") else [])
        g.add("dmom", self.dmom, [(0, self.P * M)] if writes else [])
        g.add("workspace", self.ws, [(0, self.blocks * PART)] if writes else [])
        g.add("dw_post", self.dw_post, [(0, z * z)] if writes and on else [])
        g.add("db_post", self.db_post, [(0, z)] if writes and on else [])
        g.add("dw_pre", self.dw_pre, [(0, M * M)] if writes else [])
        g.add("db_pre", self.db_pre, [(0, M)] if writes else [])
        return g

    def run(self, L, stream, **over):
        B, z, HW = self.dims
        row = self.row
        on, dh = bool(opt(row, "dzin")), bool(opt(row, "dh"))
        a = dict(dzin=ptr(self.dzin) if on else None, ld_dzin=self.dzin.stride(0) if on else 0,
                 w_post=ptr(self.w_post.data) if on else None, sample=ptr(self.sample.data) if on else None,
                 moments=ptr(self.moments.data), eps=ptr(self.eps.data) if opt(row, "eps") else None,
                 h=ptr(self.h), ldh=self.h.stride(0), w_pre=ptr(self.w_pre.data), B=B, z=z, HW=HW, kl_weight=self.kw,
                 loss_w=None, dsample_add=ptr(self.dsample.data) if opt(row, "dsample") else None,
                 dmom_add=ptr(self.dmom_add.data) if opt(row, "dmom") else None, dh=ptr(self.dh) if dh else None,
                 ld_out=self.dh.stride(0) if dh else 0, dmom=ptr(self.dmom.data), ws=ptr(self.ws.data),
                 dw_post=ptr(self.dw_post.data) if on else None, db_post=ptr(self.db_post.data) if on else None,
                 dw_pre=ptr(self.dw_pre.data), db_pre=ptr(self.db_pre.data))
        a.update(over)
        return L.sdmi_kl_bwd(*a.values(), stream)

    def raw(self):
        return [t.buf.clone() for t in (self.dhb, self.dmom, self.ws, self.dw_post, self.db_post, self.dw_pre,
                                        self.db_pre)]
