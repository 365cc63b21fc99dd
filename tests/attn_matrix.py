"""The declared test matrix of the attention kernels (csrc/attention.hip) and the helpers its exact tests share.

ROWS is data: one row per kernel instantiation, `(entry point, d, B, H, N, S, group size, expected launches)`. The
expected launches -- a fragment of the mangled kernel name with its template arguments, and the 1-D grid -- are written
by hand from the rules in the comments of sdmi_attn_fwd, sdmi_attn_bwd and sdmi_attn_bwd_fused; they are the
independent statement of what should run, never computed by calling the library. tests/test_attn_exact_gpu.py records
every call as a launch plan and asserts that the recorded kernels and grids agree; tests/test_attn_matrix_cpu.py
asserts that the rows cover every instantiation the three entry points can launch and checks the exactness argument
below on the CPU.

Exact data, three families (all values exact in bf16; B >= 2 batches share key codes and selections but differ in V and
dO, so a read past S lands in the next batch's real rows and ties with a real key; H >= 3 heads with independent data):

  uniform   Q = 0 (or K = 0): every score is 0 and P = 1 on exactly the S valid keys -- zero-filled padding keys differ
            from real ones only by the mask. V has column sums S * m, so O == m; lse == log2 S. The backward is exact
            for S a power of two.
  selector  the first nb columns of a head are code columns: K carries a +-1 code shared by the g keys of a group, Q
            carries M = 512 times the code of the group it selects; the other columns of Q are 0, of K arbitrary. Then
            P is 1 / g on the selected group and 0 elsewhere up to a relative fuzz far below half a bf16 ulp (the
            nearest other key is >= 160 binary orders of magnitude down), every accumulated product is a small dyadic
            number, exact in fp32 in any order, and the kernel's outputs equal float64 maths with the kernel's rounding
            points, bitwise. Groups span 64-key tiles and 128-key blocks; rows meet their maximum in the first, a middle
            and the last key tile, so the running-maximum rescale is exactly 0 or exactly 1.
  soft      randn data (Q scaled by 4) against componentwise bounds derived from the rounding points.

A group that is left with a size that is no power of two, or for which the 2^nb codes have run out, gets the all-zero
code and no query selects it (its score 0 is M * nb below the selected one).

Guards: every operand and output is a column window of a larger buffer filled with a NaN bit pattern (front pad, pad
columns, rows past the end). An unmasked read poisons the output; a store outside the logical windows changes guard
bits. Everything stays inside the allocations."""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

FWD, BWD, FUSED = "fwd", "bwd", "fused"
Row = collections.namedtuple("Row", "entry d B H N S g launches")
M_CODE = 512
LOG2E = float(np.float32(1.4426950408889634))


def R(entry, d, B, H, N, S, g, *launches):
    return Row(entry, d, B, H, N, S, g, launches)


# forward: attn_fwd_kernel<DT, ONES>, DT = ceil(d / 16), ONES where d % 16 == 8; grid = ceil(N / 128) * B * H.
# N = S = 130 rows are self-attention (packed q | k | v operands), the others cross-attention (5 key tiles, the last
# with one key)
ROWS = [
    R(FWD, 8, 2, 3, 130, 257, 4, ("attn_fwd_kernelILi1ELb1EE", 12)),
    R(FWD, 16, 2, 3, 130, 130, 2, ("attn_fwd_kernelILi1ELb0EE", 12)),
    R(FWD, 24, 2, 3, 130, 257, 2, ("attn_fwd_kernelILi2ELb1EE", 12)),
    R(FWD, 32, 2, 3, 130, 130, 4, ("attn_fwd_kernelILi2ELb0EE", 12)),
    R(FWD, 40, 2, 3, 130, 257, 4, ("attn_fwd_kernelILi3ELb1EE", 12)),
    R(FWD, 48, 2, 3, 130, 130, 2, ("attn_fwd_kernelILi3ELb0EE", 12)),
    R(FWD, 56, 2, 3, 130, 257, 2, ("attn_fwd_kernelILi4ELb1EE", 12)),
    R(FWD, 64, 2, 3, 130, 130, 4, ("attn_fwd_kernelILi4ELb0EE", 12)),
]
# two-pass backward: attn_bwd_dq_kernel<DT, G> then attn_bwd_dkv_kernel<DT, G>; G = 4 (256 rows per workgroup) where
# d <= 32, N <= 256, S <= 256 and B * H * ceil(min(N, S) / 256) >= 512, else G = 2 (128 rows); grids
# ceil(N / rows) * B * H and ceil(S / rows) * B * H
ROWS += [
    R(BWD, 16, 2, 3, 130, 130, 2, ("attn_bwd_dq_kernelILi1ELi2EE", 12), ("attn_bwd_dkv_kernelILi1ELi2EE", 12)),
    R(BWD, 24, 2, 3, 130, 257, 4, ("attn_bwd_dq_kernelILi2ELi2EE", 12), ("attn_bwd_dkv_kernelILi2ELi2EE", 18)),
    R(BWD, 48, 2, 3, 130, 130, 4, ("attn_bwd_dq_kernelILi3ELi2EE", 12), ("attn_bwd_dkv_kernelILi3ELi2EE", 12)),
    R(BWD, 64, 2, 3, 130, 257, 2, ("attn_bwd_dq_kernelILi4ELi2EE", 12), ("attn_bwd_dkv_kernelILi4ELi2EE", 18)),
    R(BWD, 8, 8, 64, 40, 77, 2, ("attn_bwd_dq_kernelILi1ELi4EE", 512), ("attn_bwd_dkv_kernelILi1ELi4EE", 512)),
    R(BWD, 16, 8, 64, 40, 77, 4, ("attn_bwd_dq_kernelILi1ELi4EE", 512), ("attn_bwd_dkv_kernelILi1ELi4EE", 512)),
    R(BWD, 24, 8, 64, 40, 77, 2, ("attn_bwd_dq_kernelILi2ELi4EE", 512), ("attn_bwd_dkv_kernelILi2ELi4EE", 512)),
    R(BWD, 32, 8, 64, 40, 77, 4, ("attn_bwd_dq_kernelILi2ELi4EE", 512), ("attn_bwd_dkv_kernelILi2ELi4EE", 512)),
    # the second 128 rows of a 256-row block hold real data and the block is ragged (200 queries, 130 keys)
    R(BWD, 16, 8, 64, 200, 130, 2, ("attn_bwd_dq_kernelILi1ELi4EE", 512), ("attn_bwd_dkv_kernelILi1ELi4EE", 512)),
    # just below the threshold: 511 workgroups run G = 2
    R(BWD, 16, 7, 73, 40, 77, 2, ("attn_bwd_dq_kernelILi1ELi2EE", 511), ("attn_bwd_dkv_kernelILi1ELi2EE", 511)),
]
# fused backward: attn_delta_kernel (one thread per (b, q, h): ceil(B * N * H / 256) workgroups) then
# attn_bwd_fused_kernel<DT> on ceil(S / 128) * B * H workgroups; one key block with 4 query tiles (the cross-attention
# form, dQ stored directly) and 3 key blocks with 3 query tiles (fp32 dQ partials and arrival counters)
ROWS += [
    R(FUSED, 8, 2, 3, 200, 77, 2, ("attn_delta_kernel", 5), ("attn_bwd_fused_kernelILi1EE", 6)),
    R(FUSED, 8, 2, 3, 130, 257, 4, ("attn_delta_kernel", 4), ("attn_bwd_fused_kernelILi1EE", 18)),
    R(FUSED, 32, 2, 3, 200, 77, 4, ("attn_delta_kernel", 5), ("attn_bwd_fused_kernelILi2EE", 6)),
    R(FUSED, 32, 2, 3, 130, 257, 2, ("attn_delta_kernel", 4), ("attn_bwd_fused_kernelILi2EE", 18)),
    R(FUSED, 40, 2, 3, 200, 77, 2, ("attn_delta_kernel", 5), ("attn_bwd_fused_kernelILi3EE", 6)),
    R(FUSED, 40, 2, 3, 130, 257, 4, ("attn_delta_kernel", 4), ("attn_bwd_fused_kernelILi3EE", 18)),
    R(FUSED, 64, 2, 3, 200, 77, 4, ("attn_delta_kernel", 5), ("attn_bwd_fused_kernelILi4EE", 6)),
    R(FUSED, 64, 2, 3, 130, 257, 2, ("attn_delta_kernel", 4), ("attn_bwd_fused_kernelILi4EE", 18)),
]

# further exact shapes: the counter test alternates the 3 x 3 fused row with this one (3 key blocks, 4 query tiles)
EXTRA = [
    R(FUSED, 32, 2, 3, 200, 257, 2, ("attn_delta_kernel", 5), ("attn_bwd_fused_kernelILi2EE", 18)),
]

# the ragged sweep of the uniform family
SWEEP_LENS = (1, 17, 64, 65, 128, 129, 257)
SWEEP_D = (8, 48)   # DP 32 with the ones column; DP 64 without
# soft family: (B, H, N, S, d), every row with 3 key tiles or more; the last runs the G = 4 two-pass kernels (4 key
# tiles, the second 128 keys of the 256-key dkv block filled and ragged)
SOFT = ((2, 3, 130, 257, 24), (2, 3, 130, 257, 64), (8, 64, 40, 200, 16))


def row_id(r):
    return f"{r.entry}-d{r.d}-B{r.B}H{r.H}-N{r.N}-S{r.S}-g{r.g}"


def instantiations():
    """Every (kernel, template arguments) the rows launch, as the mangled fragments."""
    return {name for r in ROWS for name, _ in r.launches}


# ----------------------------------------------------------------------------------------------------------------
# exact data (CPU, no library call). Tensors are float64 [B][H][L][d] holding bf16-representable values.
# ----------------------------------------------------------------------------------------------------------------
def _sparse_signs(shape, rng):
    """At most 4 nonzeros per row (last dim), each +-1."""
    out = np.zeros(shape)
    flat = out.reshape(-1, shape[-1])
    for _ in range(4):
        col = rng.integers(0, shape[-1], flat.shape[0])
        flat[np.arange(flat.shape[0]), col] = rng.choice([-1.0, 1.0], flat.shape[0])
    return out


def nb_of(d):
    return min(d - 2, 8)


def key_groups(S, g, rng):
    """Key groups of one head: the first lies wholly in the last 64-key tile, the second (three tiles or more) has its
    first member in tile 1 and the others in later tiles, the rest are a random partition (members mostly in
    different tiles and 128-key blocks)."""
    T = -(-S // 64)
    free = set(range(S))
    groups = []
    if T >= 2:
        last = np.arange(64 * (T - 1), S)
        n = 1 << (min(g, len(last)).bit_length() - 1)
        if n == len(last) > 1:
            n //= 2   # leave a key of the last tile (and key block) for a group that spans tiles
        groups.append(sorted(int(k) for k in rng.permutation(last)[:n]))
        free -= set(groups[-1])
    if T >= 3:
        mid = []
        for i in range(g):
            t = min(1 + i, T - 1)
            cand = [k for k in range(64 * t, min(64 * t + 64, S)) if k in free and k not in mid]
            if not cand:
                cand = [k for k in range(128, S) if k in free and k not in mid] or \
                       [k for k in range(64, S) if k in free and k not in mid]
            mid.append(int(rng.choice(cand)))
        groups.append(sorted(mid))
        free -= set(mid)
    rest = rng.permutation(sorted(free))
    groups += [sorted(int(k) for k in rest[i:i + g]) for i in range(0, len(rest), g)]
    return groups


@functools.lru_cache(maxsize=None)
def selector_case(B, H, N, S, d, g, seed=0):
    nb = nb_of(d)
    assert g in (2, 4) and nb >= 1 and d - nb >= 2
    Q = np.zeros((B, H, N, d))
    K = np.zeros((B, H, S, d))
    sel_keys = np.zeros((H, N, S), dtype=bool)   # the keys query i of head h selects
    heads = []
    for h in range(H):
        rng = np.random.default_rng([seed, h, N, S, d, g])
        groups = key_groups(S, g, rng)
        ok = [j for j, m in enumerate(groups) if len(m) & (len(m) - 1) == 0][:2 ** nb]
        codes = rng.permutation(2 ** nb)[:len(ok)]
        code = np.zeros((len(groups), nb))
        for j, cnum in zip(ok, codes):
            code[j] = [1.0 if (cnum >> b) & 1 else -1.0 for b in range(nb)]
        for j, m in enumerate(groups):
            K[:, h, m, :nb] = code[j]
        sel = rng.choice(ok, N)
        # the special groups (last tile only; first met in tile 1) at the first rows, and the last tile once more at
        # the last row of the query range
        for i, j in ((0, 0), (1, 1), (N - 1, 0)):
            if 0 <= i < N and j in ok and (j == 0 or S > 128):
                sel[i] = j
        for i in range(N):
            Q[:, h, i, :nb] = M_CODE * code[sel[i]]
            sel_keys[h, i, groups[sel[i]]] = True
        heads.append(dict(groups=groups, selectable=ok, sel=sel))
    rng = np.random.default_rng([seed, 99, N, S, d, g])
    K[..., nb:] = rng.integers(-2, 3, (B, H, S, d - nb))
    V = rng.integers(-2, 3, (B, H, S, d)).astype(np.float64)
    dO = _sparse_signs((B, H, N, d), rng)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()  # noqa: E731
    return dict(kind="selector", B=B, H=H, N=N, S=S, d=d, g=g, nb=nb, Q=t(Q), K=t(K), V=t(V), dO=t(dO), heads=heads,
                sel_keys=torch.from_numpy(sel_keys))


@functools.lru_cache(maxsize=None)
def uniform_case(B, H, N, S, d, zero, seed=0):
    """zero = 'q': Q = 0, K integers in [-2, 2]; zero = 'k': K = 0, Q integers. V integers with column sums S * m,
    integer |m| <= 8 per (batch, head, column)."""
    rng = np.random.default_rng([seed, 7, N, S, d, zero == "q"])
    Q = np.zeros((B, H, N, d)) if zero == "q" else rng.integers(-2, 3, (B, H, N, d)).astype(np.float64)
    K = np.zeros((B, H, S, d)) if zero == "k" else rng.integers(-2, 3, (B, H, S, d)).astype(np.float64)
    m = rng.integers(-8, 9, (B, H, 1, d)).astype(np.float64)
    w = rng.integers(-2, 3, (B, H, S, d)).astype(np.float64)
    r = w.sum(2)   # take the column sums out again, one unit per key from the first key on
    while np.any(r != 0):
        take = np.sign(r)[:, :, None, :] * (np.arange(S)[None, None, :, None] < np.abs(r)[:, :, None, :])
        w -= take
        r = w.sum(2)
    V = m + w
    dO = _sparse_signs((B, H, N, d), rng)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()  # noqa: E731
    return dict(kind="uniform", B=B, H=H, N=N, S=S, d=d, g=S, zero=zero, Q=t(Q), K=t(K), V=t(V), dO=t(dO),
                m=t(np.array(np.broadcast_to(m, (B, H, N, d)))))


@functools.lru_cache(maxsize=None)
def soft_case(B, H, N, S, d, seed=5):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda L, s: (s * torch.randn(B, H, L, d, generator=gen)).to(torch.bfloat16).double()  # noqa: E731
    return dict(kind="soft", B=B, H=H, N=N, S=S, d=d, Q=mk(N, 4.0), K=mk(S, 1.0), V=mk(S, 1.0), dO=mk(N, 1.0))


# ----------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------
def scale32(d):
    """1 / sqrt(d) formed in fp32 as the host entry points do."""
    return np.float32(1.0) / np.sqrt(np.float32(d))


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).double()


def is_bf16(x):
    return bool(torch.equal(bf16(x), x))


def ulp32(x):
    """The fp32 unit in the last place at |x| (float)."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x else 2.0 ** -149


def scaled_bf16(x, d):
    """bf16(fp32(x) * s): the kernels' dQ / dK store of an exactly accumulated fp32 value."""
    x32 = x.to(torch.float32)
    assert torch.equal(x32.double(), x), "the accumulated value is not exact in fp32"
    return (x32 * float(scale32(d))).to(torch.bfloat16).double()


def exact_p(c):
    """P of the exact families: 1 / (number of maximal scores) on the maximal scores, 0 elsewhere."""
    s = c["Q"] @ c["K"].transpose(-1, -2)
    top = s == s.amax(-1, keepdim=True)
    return s, top.double() / top.sum(-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _exact_reference(kind, args):
    c = {"selector": selector_case, "uniform": uniform_case}[kind](*args)
    d = c["d"]
    s, P = exact_p(c)
    cc = float(scale32(d)) * LOG2E
    O = bf16(P @ c["V"])
    dV = bf16(P.transpose(-1, -2) @ c["dO"])
    delta = (c["dO"] * O).sum(-1, keepdim=True)
    dS = bf16(P * (c["dO"] @ c["V"].transpose(-1, -2) - delta))
    accQ, accK = dS @ c["K"], dS.transpose(-1, -2) @ c["Q"]
    lse = s.amax(-1) * cc + torch.log2((s == s.amax(-1, keepdim=True)).sum(-1).double())
    return dict(P=P, s=s, O=O, dV=dV, delta=delta.squeeze(-1), dS=dS, accQ=accQ, accK=accK,
                dQ=scaled_bf16(accQ, d), dK=scaled_bf16(accK, d), lse=lse, lse_scale=float((s.abs() * cc).max()))


def exact_reference(c):
    """float64 maths with the kernels' rounding points: O = bf16(P V); dV = bf16(P^T dO); delta from the bf16 O;
    dS = bf16(P (dP - delta)); dQ = bf16(fp32(dS K) * s), dK = bf16(fp32(dS^T Q) * s). Computed once per case and shared by the tests."""
    if c["kind"] == "selector":
        return _exact_reference("selector", (c["B"], c["H"], c["N"], c["S"], c["d"], c["g"]))
    return _exact_reference("uniform", (c["B"], c["H"], c["N"], c["S"], c["d"], c["zero"]))


def soft_forward_reference(c):
    s = float(scale32(c["d"]))
    sc = c["Q"] @ c["K"].transpose(-1, -2) * s
    P = torch.softmax(sc, -1)
    lse = torch.logsumexp(sc, -1) * math.log2(math.e)
    return dict(P=P, O=P @ c["V"], O_bound=2.0 ** -7 * (P @ c["V"].abs()), lse=lse,
                lse_scale=float((sc.abs() * math.log2(math.e)).max()))


# The forward's lse where d % 16 == 8 (the ones column): the row sum is accumulated by the PV MFMA, i.e. of the bf16
# P, one more rounding point than the fp32 row sum of the other head dims. The bound of 8 fp32 ulps of
# max |score * c| that holds for the fp32 row sum does not admit it: emulate_lse_ones (the rounding points in torch, no
# library call) is off by about 119.5 times that bound at SOFT[0] (1.82e-3 absolute), so the constant was too tight
# for these rows; twice the emulation's worst ratio would allow 3.7e-3. The bound in use is the analytic one, which
# is tighter and holds at any shape: round-to-nearest moves every positive term of the row sum by at most 2^-9
# relative, hence the sum by at most 2^-9 relative and its log2 by at most -log2(1 - 2^-9) = 2.82e-3; the 8 ulps of
# the fp32 arithmetic come on top. tests/test_attn_matrix_cpu.py checks that the emulation exceeds the 8 ulps and
# stays inside this bound.
LSE_ULPS = 8
LSE_ONES_ROUNDING = -math.log2(1.0 - 2.0 ** -9)


def lse_bound(d, lse_scale):
    """The allowed |lse - ref|: 8 fp32 ulps of max |score * c|, plus the bf16 rounding of P where d % 16 == 8."""
    return LSE_ULPS * ulp32(lse_scale) + (LSE_ONES_ROUNDING if d % 16 == 8 else 0.0)


def emulate_lse_ones(c):
    """lse of the ones-column forward with its rounding points: per 64-key tile the running maximum m, e = bf16(2^(s c -
    m)), l = l * 2^(m_old - m) + sum e; lse = m + log2 l. float64 but for the bf16 conversion of e."""
    cc = float(scale32(c["d"])) * LOG2E
    s = c["Q"] @ c["K"].transpose(-1, -2) * cc
    m = torch.full(s.shape[:-1], -math.inf, dtype=torch.float64)
    l = torch.zeros_like(m)
    for k0 in range(0, s.shape[-1], 64):
        t = s[..., k0:k0 + 64]
        mn = torch.maximum(m, t.amax(-1))
        l = l * torch.exp2(m - mn) + bf16(torch.exp2(t - mn[..., None])).sum(-1)
        m = mn
    return m + torch.log2(l)


def soft_backward_reference(c, fw, o_kernel):
    """delta from the kernel's own bf16 O ([B][H][N][d] float64); componentwise bounds from the rounding points: P,
    dS and the outputs are each rounded to bf16 once (2^-9 relative), with margin."""
    s = float(scale32(c["d"]))
    P, dO, V, Q, K = fw["P"], c["dO"], c["V"], c["Q"], c["K"]
    delta = (dO * o_kernel).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2)
    dS = P * (dP - delta)
    E = P * (2.0 ** -7 * (dP.abs() + delta.abs()) + 2.0 ** -8 * (dO.abs() * o_kernel.abs()).sum(-1, keepdim=True))
    out = dict(dV=P.transpose(-1, -2) @ dO, dQ=dS @ K * s, dK=dS.transpose(-1, -2) @ Q * s)
    # delta is an fp32 sum of d exact products: (d + 1) * 2^-24 of sum |dO| |O| in any order
    out["delta"] = delta.squeeze(-1)
    out["delta_bound"] = (c["d"] + 1) * 2.0 ** -24 * (dO.abs() * o_kernel.abs()).sum(-1)
    out["dV_bound"] = 2.0 ** -7 * (P.transpose(-1, -2) @ dO.abs()) + 2.0 ** -8 * out["dV"].abs()
    out["dQ_bound"] = s * (E @ K.abs()) + 2.0 ** -8 * out["dQ"].abs()
    out["dK_bound"] = s * (E.transpose(-1, -2) @ Q.abs()) + 2.0 ** -8 * out["dK"].abs()
    return out


def emulate_with_fuzz(c, fuzz=5e-4, seed=1):
    """The kernels' arithmetic with every P perturbed by up to +-fuzz relative before its bf16 conversion (what the
    rounding of mx * c and the hardware exp2 / log2 may do): unnormalised e in the forward with its row sum, the
    normalised P in the backward. Returns O, dV, dQ, dK as float64 holding bf16 values."""
    gen = torch.Generator().manual_seed(seed)
    wob = lambda x: x * (1.0 + fuzz * (2.0 * torch.rand(x.shape, generator=gen, dtype=torch.float64) - 1.0))  # noqa
    d = c["d"]
    s, P = exact_p(c)
    e = wob((P > 0).double())
    lsum = e.sum(-1, keepdim=True)   # the fp32 row sum of the unrounded e (without the ones column)
    inv = (1.0 / lsum.to(torch.float32)).double()
    O = bf16(((bf16(e) @ c["V"]).to(torch.float32) * inv.to(torch.float32)).double())
    Pn = wob(P)
    dV = bf16(bf16(Pn).transpose(-1, -2) @ c["dO"])
    delta = (c["dO"] * O).sum(-1, keepdim=True)
    dS = bf16((Pn * (c["dO"] @ c["V"].transpose(-1, -2) - delta)).to(torch.float32).double())
    return dict(O=O, dV=dV, dQ=scaled_bf16(dS @ c["K"], d), dK=scaled_bf16(dS.transpose(-1, -2) @ c["Q"], d))


def rows_of(x):
    """[B][H][L][d] -> the kernels' [B * L][H * d] layout."""
    B, H, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * d)


def heads_of(x, B, H):
    """[B * L][H * d] -> [B][H][L][d]."""
    L, d = x.shape[0] // B, x.shape[1] // H
    return x.reshape(B, L, H, d).permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------------------------------------------
# guarded device buffers and launches
# ----------------------------------------------------------------------------------------------------------------
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
CONTIGUOUS, PACKED = "contiguous", "packed"


class Buf:
    """[rows][ld] elements after a 64-element front pad, `tail` whole rows after the end, all filled with a NaN bit
    pattern; operands and outputs are column windows of it."""

    def __init__(self, rows, ld, dtype, device, tail=8, front=64):
        self.buf = torch.full((front + (rows + tail) * ld,), float("nan"), dtype=dtype, device=device)
        self.rows, self.ld, self.front = rows, ld, front

    def window(self, col0, cols):
        assert col0 + cols <= self.ld
        return self.buf[self.front + col0:].as_strided((self.rows, cols), (self.ld, 1))

    def outside_untouched(self, windows):
        """Everything but the listed (col0, cols) windows still holds the fill pattern, bit for bit."""
        z = self.buf.clone()
        for col0, cols in windows:
            z[self.front + col0:].as_strided((self.rows, cols), (self.ld, 1)).fill_(float("nan"))
        return torch.equal(z.view(_BITS[z.dtype]), torch.full_like(z, float("nan")).view(_BITS[z.dtype]))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class Problem:
    """One case on the device in one layout. contiguous: every operand its own [rows][H * d] buffer. packed: q | k | v
    (self-attention, N == S) are column windows of one [rows][3 H d + 8] buffer and dq | dk | dv of another; with
    N != S, k | v are windows of a [B * S][2 H d + 8] buffer (dk | dv likewise) and q / dq sit in [B * N][H d + 8]
    buffers; o and dout are windows at column 8 of [B * N][H d + 16] buffers."""

    def __init__(self, c, layout, device="cuda"):
        B, H, N, S, d = (c[k] for k in "BHNSd")
        C = H * d
        self.c, self.dims, self.C = c, (B, H, N, S, d), C
        bf = torch.bfloat16
        mk = lambda rows, ld: Buf(rows, ld, bf, device)  # noqa: E731
        if layout == CONTIGUOUS:
            bq, bk, bv, gq, gk, gv = mk(B * N, C), mk(B * S, C), mk(B * S, C), mk(B * N, C), mk(B * S, C), mk(B * S, C)
            bo, bdo = mk(B * N, C), mk(B * N, C)
            self.q, self.k, self.v = bq.window(0, C), bk.window(0, C), bv.window(0, C)
            self.dq, self.dk, self.dv = gq.window(0, C), gk.window(0, C), gv.window(0, C)
            self.o, self.do = bo.window(0, C), bdo.window(0, C)
            self.inputs = [bq, bk, bv, bdo]
            self.grads = [(gq, [(0, C)]), (gk, [(0, C)]), (gv, [(0, C)])]
            self.obuf = (bo, [(0, C)])
        else:
            if N == S:
                inp, g = mk(B * N, 3 * C + 8), mk(B * N, 3 * C + 8)
                self.q, self.k, self.v = inp.window(0, C), inp.window(C, C), inp.window(2 * C, C)
                self.dq, self.dk, self.dv = g.window(0, C), g.window(C, C), g.window(2 * C, C)
                self.inputs = [inp]
                self.grads = [(g, [(0, 3 * C)])]
            else:
                bq, kv, gq, gkv = mk(B * N, C + 8), mk(B * S, 2 * C + 8), mk(B * N, C + 8), mk(B * S, 2 * C + 8)
                self.q, self.k, self.v = bq.window(0, C), kv.window(0, C), kv.window(C, C)
                self.dq, self.dk, self.dv = gq.window(0, C), gkv.window(0, C), gkv.window(C, C)
                self.inputs = [bq, kv]
                self.grads = [(gq, [(0, C)]), (gkv, [(0, 2 * C)])]
            bo, bdo = mk(B * N, C + 16), mk(B * N, C + 16)
            self.o, self.do = bo.window(8, C), bdo.window(8, C)
            self.inputs.append(bdo)
            self.obuf = (bo, [(8, C)])
        for dst, name in ((self.q, "Q"), (self.k, "K"), (self.v, "V"), (self.do, "dO")):
            dst.copy_(rows_of(c[name]).to(bf))
        n = B * H * N
        self.lse_buf = Buf(1, n, torch.float32, device, tail=64)
        self.delta_buf = Buf(1, n, torch.float32, device, tail=64)
        self.lse, self.delta = self.lse_buf.window(0, n)[0], self.delta_buf.window(0, n)[0]
        self.ws_buf = None
        self.snapshot = [b.buf.clone() for b in self.inputs]
        self.fwd_snapshot = None

    def keep_forward(self):
        """Copy the forward's o and lse buffers (stream-ordered, after the forward): the backward reads them and must
        leave them bitwise as they are."""
        self.fwd_snapshot = (self.obuf[0].buf.clone(), self.lse_buf.buf.clone())

    def args_fwd(self):
        B, H, N, S, d = self.dims
        ld = lambda t: t.stride(0)  # noqa: E731
        return (_ptr(self.q), ld(self.q), _ptr(self.k), ld(self.k), _ptr(self.v), ld(self.v), _ptr(self.o), ld(self.o),
                _ptr(self.lse), B, H, N, S, d)

    def fwd(self, L, stream):
        return L.sdmi_attn_fwd(*self.args_fwd(), stream)

    def args_bwd(self, ws=None):
        B, H, N, S, d = self.dims
        ld = lambda t: t.stride(0)  # noqa: E731
        head = (_ptr(self.q), ld(self.q), _ptr(self.k), ld(self.k), _ptr(self.v), ld(self.v), _ptr(self.o), ld(self.o),
                _ptr(self.do), ld(self.do), _ptr(self.lse), _ptr(self.delta))
        tail = (_ptr(self.dq), ld(self.dq), _ptr(self.dk), ld(self.dk), _ptr(self.dv), ld(self.dv), B, H, N, S, d)
        return head + (ws if ws is not None else ()) + tail

    def bwd(self, L, stream, fused):
        self.keep_forward()
        if not fused:
            return L.sdmi_attn_bwd(*self.args_bwd(), stream)
        need = L.sdmi_attn_bwd_workspace(*self.dims)
        assert need % 4 == 0
        self.ws_need = need
        self.ws_buf = Buf(1, max(need // 4, 1), torch.float32, self.q.device, tail=64)
        return L.sdmi_attn_bwd_fused(*self.args_bwd((_ptr(self.ws_buf.window(0, 1)), need)), stream)

    def guards_ok(self, backward):
        """None, or what changed outside the logical windows (inputs included: they must be bitwise as placed; after
        the backward also its operands out and lse, as the forward left them)."""
        n = self.dims[0] * self.dims[1] * self.dims[2]
        bad = [f"input buffer {i}" for i, (b, s) in enumerate(zip(self.inputs, self.snapshot)) if
               not torch.equal(b.buf.view(torch.int16), s.view(torch.int16))]
        if not self.obuf[0].outside_untouched(self.obuf[1]):
            bad.append("outside out")
        if not self.lse_buf.outside_untouched([(0, n)]):
            bad.append("outside lse")
        if backward:
            assert self.fwd_snapshot is not None, "keep_forward() was not called before the backward"
            for what, b, s in zip(("out", "lse"), (self.obuf[0], self.lse_buf), self.fwd_snapshot):
                if not torch.equal(b.buf.view(_BITS[b.buf.dtype]), s.view(_BITS[s.dtype])):
                    bad.append(f"the backward's operand {what}")
            bad += [f"outside gradient buffer {i}" for i, (b, w) in enumerate(self.grads) if not b.outside_untouched(w)]
            if not self.delta_buf.outside_untouched([(0, n)]):
                bad.append("outside delta")
            ws_window = [(0, self.ws_need // 4)] if self.ws_buf is not None and self.ws_need else []
            if self.ws_buf is not None and not self.ws_buf.outside_untouched(ws_window):
                bad.append("outside the fused workspace")
        else:
            bad += [f"gradient buffer {i} written by the forward" for i, (b, _) in enumerate(self.grads) if
                    not b.outside_untouched([])]
        return ", ".join(bad) or None

    def out(self, name):
        """An output as float64 [B][H][L][d] on the CPU."""
        B, H = self.dims[:2]
        return heads_of(getattr(self, name).cpu().double(), B, H)

    def stat(self, name):
        B, H, N = self.dims[:3]
        return getattr(self, name).cpu().double().view(B, H, N)


def recorded(L, call):
    """Run `call` between sdmi_plan_begin and sdmi_plan_end (recording still issues the launches) and return its
    status and the recorded launches as (kernel name, grid[0] * grid[1] * grid[2])."""
    assert L.sdmi_plan_begin() == 0
    plan = ctypes.c_void_p()
    try:
        rc = call()
    finally:
        assert L.sdmi_plan_end(ctypes.byref(plan)) == 0
    try:
        n = ctypes.c_int()
        assert L.sdmi_plan_info(plan, ctypes.byref(n), None) == 0
        kind, name, grid = ctypes.c_int(), ctypes.c_char_p(), (ctypes.c_int * 3)()
        ops = []
        for i in range(n.value):
            assert L.sdmi_plan_op_info(plan, i, ctypes.byref(kind), ctypes.byref(name), grid, None, None) == 0
            if kind.value == 0:
                ops.append((name.value.decode(errors="replace") if name.value else "?", grid[0] * grid[1] * grid[2]))
    finally:
        L.sdmi_plan_destroy(plan)
    return rc, ops


def launches_match(ops, want):
    """The recorded launches are exactly the row's, in order: the name holds the mangled fragment, the grid is equal."""
    return len(ops) == len(want) and all(w[0] in o[0] and o[1] == w[1] for o, w in zip(ops, want))
