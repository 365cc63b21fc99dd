"""Every kernel of csrc/adda.hip, exact and guarded (statements: tests/adda_ref.py; launches: DESIGN.md section 18).

Operands and outputs sit between NaN pads; after a call only the declared outputs may have changed; a second identical
call gives identical bits; the recorded launches are the kernels and grids DESIGN.md declares. The slices, the packed
weight, pre, the mask words, T, the masked operands U / V, dx and the unpacked weight gradient are bitwise the CPU
emulation (integer weight codes: every partial sum is exact); the reductions (the ADC scale's gradient, ds of the input
quantiser) lie within K_LSQ u of the float64 sum of their fp32 terms' absolute values."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adda_ref as A
from tests import lsq_ref as LR
from tests.attn_matrix import launches_match, recorded
from tests.norm_matrix import bits, ptr
from tests.test_lsq_kernels_gpu import Box, _check, _guard, _same

pytestmark = pytest.mark.gpu
MS = {1: (1, 1), 63: (7, 9), 130: (2, 65)}  # M = B P
NS = (1, 24, 136)
# (K, row block): one block; ragged blocks of 40; the reference's 576; blocks of 8 (13 blocks: with 7 slices 91 mask
# bits, three words)
KS = ((8, 8), (100, 40), (616, 576), (100, 8))
BITS = ((8, 5), (8, 2), (5, 5))  # (input, DAC)


def _L():
    from sdmi import _lib
    return _lib.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag):
    rc, ops = recorded(L, call)
    assert rc == 0, f"{tag}: returned {rc}"
    assert launches_match(ops, want), f"{tag}: launched {ops}, DESIGN.md section 18 says {want}"
    torch.cuda.synchronize()


def _case(M, N, K, ib, wb, seed):
    gen = torch.Generator().manual_seed(seed)
    B, P = MS[M]
    s_in, s_w = torch.tensor(0.0371), torch.tensor(0.0173)
    x = torch.randn(B, K, P, generator=gen) * (0.6 * LR.qp_of(ib)) * s_in
    qw = LR.qp_of(wb)
    w = torch.randint(-qw, qw + 1, (N, K), generator=gen).float()
    return dict(x=x, w=w, s_in=s_in, s_w=s_w, bias=torch.randn(N, generator=gen), gen=gen, B=B, P=P)


@pytest.mark.parametrize("ib,db", BITS)
@pytest.mark.parametrize("K,rb", KS)
def test_forward_kernels(K, rb, ib, db):
    L, st = _L(), _st()
    worst = 0
    for vi, (M, N) in enumerate((m, n) for m in MS for n in NS):
        adc, wb = ((8, 4), (4, 8), (8, 8), (4, 4))[vi % 4]
        adc_noise, want_bwd, lo, null = vi % 2 == 1, vi % 3 != 2, vi % 4 < 2, vi % 5 == 4
        tag = f"M={M} N={N} K={K}/{rb} bits=({ib},{db}) adc={adc} w={wb} noise={adc_noise} bwd={want_bwd} lo={lo} null={null}"
        c = _case(M, N, K, ib, wb, 1000 * M + 10 * N + K + ib + db)
        cfg = dict(input_bit=ib, dac_bit=db, adc_bit=adc)
        B, P = c["B"], c["P"]
        g_in = LR.g_of(ib, c["x"].numel())
        # ---- the slices ----
        ref_s, g = A.emulate_in_fwd(c["x"], c["s_in"], ib, db, rb)
        nL, Mp, Np, Kp, nb = g["L"], g["Mp"], -(-N // 64) * 64, g["Kp"], g["nb"]
        ins = dict(x=Box(c["x"].numel(), values=c["x"]), s_in=Box(1, values=c["s_in"]), s_w=Box(1, values=c["s_w"]),
                   bias=Box(N, values=c["bias"]))
        xs = Box(nL * Mp * Kp, torch.bfloat16)
        gd = _guard(ins, dict(xs=xs))

        def in_fwd():
            return L.sdmi_adda_in_fwd(ptr(ins["x"].data), B, K, P, ptr(ins["s_in"].data), g_in, ib, db, rb, ptr(xs.data), st)
        _run(L, in_fwd, [("adda_in_fwd_kernel", LR.item_blocks(Mp * (Kp // 8)))], tag)
        _check(gd, dict(xs=xs), in_fwd, tag)
        _same(xs.cpu(nL, Mp, Kp), ref_s, "slices", tag)
        # ---- the packed weight ----
        hi_ref, lo_ref, _ = A.emulate_pack_w(c["w"], rb)
        ins["w"] = Box(N * K, values=c["w"])
        hi, lob = Box(Np * Kp, torch.bfloat16), Box(Np * Kp, torch.bfloat16)
        outs = dict(hi=hi, lo=lob) if lo else dict(hi=hi)
        gd = _guard(ins, outs)

        def pack():
            return L.sdmi_adda_pack_w(ptr(ins["w"].data), N, K, rb, ptr(hi.data), ptr(lob.data) if lo else None, st)
        _run(L, pack, [("adda_pack_w_kernel", LR.item_blocks(Np * (Kp // 8)))], tag)
        _check(gd, outs, pack, tag)
        _same(hi.cpu(Np, Kp), hi_ref, "hi", tag)
        if lo:
            _same(lob.cpu(Np, Kp), lo_ref, "lo", tag)
        # ---- the product: a scale that saturates part of the ADC inputs ----
        X = A.slices32(A.xq32(c["x"], c["s_in"], ib).permute(0, 2, 1).reshape(M, K), ib, db)
        R = 2 ** (adc - 1) - 1
        probe = A.emulate_gemm(X, c["w"], rb, cfg, torch.tensor(1.0), None, None, None)
        top = max(float(p.abs().max()) for p in probe["P"].values())
        a_s = torch.tensor(R / (0.55 * top) if top else 0.5, dtype=torch.float32)
        gn = torch.randn(1000, generator=c["gen"]) * 0.05 if adc_noise else None
        on = torch.randn(1000, generator=c["gen"]) * 0.05 if adc_noise else None
        s_w, s_in, bias = (None, None, None) if null else (c["s_w"], c["s_in"], c["bias"])
        ref = A.emulate_gemm(X, c["w"], rb, cfg, a_s, s_w, s_in, bias, gn, on)
        ld = (N + 7) // 8 * 8
        nw = -(-nb * nL // 32)
        ins.update(xs=xs, hi=hi, a_s=Box(1, values=a_s))
        if lo:
            ins["lo"] = lob
        if adc_noise:
            ins.update(gn=Box(1000, values=gn), on=Box(1000, values=on))
        pre, mask, T = Box(M * ld), Box(nw * M * ld), Box(M * ld)
        outs = dict(pre=pre, mask=mask, T=T) if want_bwd else dict(pre=pre)
        gd = _guard(ins, outs)

        def gemm():
            return L.sdmi_adda_gemm(ptr(xs.data), ptr(hi.data), ptr(lob.data) if lo else None, M, N, K, rb, ib, db, adc,
                                    ptr(ins["a_s"].data), ptr(ins["gn"].data) if adc_noise else None,
                                    ptr(ins["on"].data) if adc_noise else None, None if null else ptr(ins["s_w"].data),
                                    None if null else ptr(ins["s_in"].data), None if null else ptr(ins["bias"].data),
                                    ptr(pre.data), ld, ptr(mask.data) if want_bwd else None,
                                    ptr(T.data) if want_bwd else None, st)
        _run(L, gemm, [("adda_gemm_kernel", (Np // 64) * (Mp // 64))], tag)
        _check(gd, outs, gemm, tag)
        got = pre.cpu(M, ld)
        _same(got[:, :N], ref["pre"], "pre", tag)
        assert bool(torch.isnan(got[:, N:]).all()), f"{tag}: pre written beyond column N"
        if want_bwd:
            gm = mask.cpu().view(torch.int32).view(nw, M, ld)[:, :, :N].to(torch.int64) & 0xFFFFFFFF
            assert torch.equal(gm, ref["words"]), f"{tag}: mask words differ in {int((gm != ref['words']).sum())} elements"
            _same(T.cpu(M, ld)[:, :N], ref["T"], "T", tag)
            ones = sum(int(((ref["words"][b // 32] >> (b % 32)) & 1).sum()) for b in range(nb * nL))
            worst = max(worst, nb * nL * M * N - ones)
    assert worst > 0 or K == 8, "no ADC input saturated in any variant: the masks were not exercised"


@pytest.mark.parametrize("ib,db", BITS)
@pytest.mark.parametrize("K,rb", KS)
def test_backward_kernels(K, rb, ib, db):
    L, st = _L(), _st()
    for vi, (M, N) in enumerate((m, n) for m in MS for n in NS):
        adc, wb = ((8, 4), (4, 8))[vi % 2]
        null = vi % 4 == 3
        tag = f"M={M} N={N} K={K}/{rb} bits=({ib},{db}) adc={adc} null={null}"
        c = _case(M, N, K, ib, wb, 77 + 1000 * M + 10 * N + K + ib + db)
        gen, B, P = c["gen"], c["B"], c["P"]
        cfg = dict(input_bit=ib, dac_bit=db, adc_bit=adc)
        sb = db - 1
        g = A.geometry(M, N, K, rb, ib, db)
        nL, Mp, Kp, nb, rbp = g["L"], g["Mp"], g["Kp"], g["nb"], g["rbp"]
        X = A.slices32(A.xq32(c["x"], c["s_in"], ib).permute(0, 2, 1).reshape(M, K), ib, db)
        R = 2 ** (adc - 1) - 1
        probe = A.emulate_gemm(X, c["w"], rb, cfg, torch.tensor(1.0), None, None, None)
        top = max(float(p.abs().max()) for p in probe["P"].values())
        a_s = torch.tensor(R / (0.55 * top) if top else 0.5, dtype=torch.float32)
        s_w, s_in, bias = (None, None, None) if null else (c["s_w"], c["s_in"], c["bias"])
        fw = A.emulate_gemm(X, c["w"], rb, cfg, a_s, s_w, s_in, bias)
        ld = (N + 7) // 8 * 8
        nw = fw["words"].shape[0]
        # ---- the masked operands and the ADC scale's gradient ----
        dpre = torch.zeros(M, ld)
        dpre[:, :N] = torch.randn(M, N, generator=gen)
        dpre = dpre.to(torch.bfloat16)
        nanpad = lambda t: torch.cat([t, torch.full((*t.shape[:-1], ld - N), float("nan"))], -1)  # noqa: E731
        words = torch.zeros(nw, M, ld, dtype=torch.int64)
        words[:, :, :N] = fw["words"]
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        ins = dict(dpre=Box(M * ld, torch.bfloat16, values=dpre), pre=Box(M * ld, values=nanpad(fw["pre"])),
                   T=Box(M * ld, values=nanpad(fw["T"])), mask=Box(nw * M * ld), a_s=Box(1, values=a_s),
                   s_w=Box(1, values=c["s_w"]), s_in=Box(1, values=c["s_in"]), bias=Box(N, values=c["bias"]))
        ins["mask"].data.view(torch.int32).copy_(words.reshape(-1))
        U, V = Box(nb * M * ld, torch.bfloat16), Box(nb * nL * Mp * ld, torch.bfloat16)
        ws, ds = Box(512), Box(3)
        nblk = LR.item_blocks(Mp * (ld // 8))
        gd = _guard(ins, dict(U=U, V=V, ds=ds))
        gd.add("workspace", ws, [(0, nblk), (256, 256 + nblk)])

        def ops():
            return L.sdmi_adda_bwd_ops(ptr(ins["dpre"].data), ld, ptr(ins["pre"].data), ld,
                                       None if null else ptr(ins["bias"].data), ptr(ins["T"].data), ptr(ins["mask"].data),
                                       M, N, nb, nL, sb, ptr(ins["a_s"].data), None if null else ptr(ins["s_w"].data),
                                       None if null else ptr(ins["s_in"].data), ptr(U.data), ptr(V.data), ptr(ws.data),
                                       ptr(ds.data), st)
        _run(L, ops, [("adda_bwd_ops_kernel", nblk), ("adda_scale_finish_kernel", 1)], tag)
        _check(gd, dict(U=U, V=V, ds=ds, ws=ws), ops, tag)
        ref = A.emulate_bwd_ops(dpre[:, :N], fw["pre"], bias, fw["T"], fw["words"], nb, nL, sb, a_s, s_w, s_in)
        _same(U.cpu(nb, M, ld)[:, :, :N], ref["U"], "U", tag)
        gv = V.cpu(nb, nL, Mp, ld)
        _same(gv[:, :, :M, :N], ref["V"], "V", tag)
        assert bool((gv[:, :, M:].float() == 0).all()) and bool((gv[:, :, :, N:].float() == 0).all()), f"{tag}: V pads"
        assert bool((U.cpu(nb, M, ld)[:, :, N:].float() == 0).all()), f"{tag}: U pads"
        s1, s2 = float(ref["t1"].double().sum()), float(ref["t2"].double().sum())
        a1, a2 = float(ref["t1"].double().abs().sum()), float(ref["t2"].double().abs().sum())
        want = s1 - s2 / float(a_s)
        bound = LR.K_LSQ * LR.U24 * (a1 + a2 / float(a_s)) + 4 * LR.U24 * (abs(s1) + abs(s2) / float(a_s))
        got = float(ds.cpu()[0])
        assert abs(got - want) <= bound, f"{tag}: d adc_scale {got!r} is {abs(got - want) / bound:.3f} bounds from {want!r}"
        # ---- the input quantiser's backward on the block-padded data gradient ----
        G = torch.randn(M, K, generator=gen)
        Gp = torch.full((M, Kp), float("nan"))
        for j in range(nb):
            n = min(g["rb"], K - j * g["rb"])
            Gp[:, j * rbp:j * rbp + n] = G[:, j * g["rb"]:j * g["rb"] + n]
        n_el = c["x"].numel()
        g_in = LR.g_of(ib, n_el)
        ins2 = dict(x=Box(n_el, values=c["x"]), G=Box(M * Kp, values=Gp), s_in=ins["s_in"], a_s=ins["a_s"])
        dx, ws2, ds2 = Box(n_el), Box(256), Box(1)
        fb = LR.flat_blocks(n_el)
        gd = _guard(ins2, dict(dx=dx, ds=ds2))
        gd.add("workspace", ws2, [(0, fb)])

        def in_bwd():
            return L.sdmi_adda_in_bwd(ptr(ins2["x"].data), ptr(ins2["G"].data), B, K, P, rb, ptr(ins2["s_in"].data), g_in, ib,
                                      db, ptr(ins2["a_s"].data), ptr(dx.data), ptr(ws2.data), ptr(ds2.data), st)
        _run(L, in_bwd, [("adda_in_bwd_kernel", fb), ("lsq_finish_kernel", 1)], tag)
        _check(gd, dict(dx=dx, ds=ds2, ws=ws2), in_bwd, tag)
        se = LR.effective_step(c["s_in"], ib, n_el)
        up = ((G * (a_s / float(nL))) / se).reshape(B, P, K).permute(0, 2, 1).contiguous()
        xr, sr = c["x"].clone().requires_grad_(True), c["s_in"].clone().requires_grad_(True)
        LR.quant_lsq(xr, ib, sr).backward(up)
        _same(dx.cpu(B, K, P), xr.grad, "dx", tag)
        t = LR.terms(c["x"], up, c["s_in"], ib)["t"]
        gg = LR.g32(ib, n_el)
        assert abs(float(ds2.cpu()) - LR.ds64(t, gg)) <= LR.sum_bound(t, gg), f"{tag}: ds_in"
        # ---- the weight gradient out of its padded layout ----
        N8 = ld
        G2 = torch.randn(N8, K, generator=gen)
        G2p = torch.full((N8, Kp), float("nan"))
        for j in range(nb):
            n = min(g["rb"], K - j * g["rb"])
            G2p[:, j * rbp:j * rbp + n] = G2[:, j * g["rb"]:j * g["rb"] + n]
        ins3 = dict(G2=Box(N8 * Kp, values=G2p), a_s=ins["a_s"])
        out = Box(N * K)
        gd = _guard(ins3, dict(out=out))

        def unpack():
            return L.sdmi_adda_unpack_wgrad(ptr(ins3["G2"].data), N, K, rb, ptr(ins3["a_s"].data), ptr(out.data), st)
        _run(L, unpack, [("adda_unpack_wgrad_kernel", LR.flat_blocks(N * K))], tag)
        _check(gd, dict(out=out), unpack, tag)
        _same(out.cpu(N, K), a_s * G2[:N], "unpacked weight gradient", tag)


@pytest.mark.parametrize("n", (1, 63, 1025, 300000))
def test_absmax(n):
    L, st = _L(), _st()
    gen = torch.Generator().manual_seed(n)
    for kind in ("randn", "zero", "nan"):
        x = torch.randn(n, generator=gen) * 3.7
        if kind == "zero":
            x = torch.zeros(n)
        if kind == "nan":
            x[n // 3] = float("nan")
        xb, ws, out = Box(n, values=x), Box(256), Box(1)
        fb = LR.flat_blocks(n)
        gd = _guard(dict(x=xb), dict(out=out))
        gd.add("workspace", ws, [(0, fb)])

        def call():
            return L.sdmi_adda_absmax(ptr(xb.data), n, ptr(ws.data), ptr(out.data), st)
        _run(L, call, [("lsq_absmax_kernel", fb), ("adda_absmax_finish_kernel", 1)], f"n={n} {kind}")
        _check(gd, dict(out=out, ws=ws), call, f"n={n} {kind}")
        got = float(out.cpu()[0])
        assert np.isnan(got) if kind == "nan" else got == float(x.abs().max()), (n, kind, got)


def test_non_integer_weight_packs_into_high_and_low_parts():
    L, st = _L(), _st()
    N, K, rb = 24, 100, 40
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(3)) * 5
    hi_ref, lo_ref, g = A.emulate_pack_w(w, rb)
    wb, hi, lo = Box(N * K, values=w), Box(g["Np"] * g["Kp"], torch.bfloat16), Box(g["Np"] * g["Kp"], torch.bfloat16)
    assert L.sdmi_adda_pack_w(ptr(wb.data), N, K, rb, ptr(hi.data), ptr(lo.data), st) == 0
    torch.cuda.synchronize()
    _same(hi.cpu(g["Np"], g["Kp"]), hi_ref, "hi", "pack")
    _same(lo.cpu(g["Np"], g["Kp"]), lo_ref, "lo", "pack")
    assert float(lo_ref.float().abs().max()) > 0
    full = A.pad_cols(w, g, K)
    assert float((full - hi_ref[:N].float() - lo_ref[:N].float()).abs().max()) <= 2.0 ** -16 * float(w.abs().max())


def test_error_returns_launch_nothing():
    L, st = _L(), _st()
    x, s, out = Box(64), Box(1, values=torch.tensor(0.1)), Box(4096, torch.bfloat16)
    f32 = Box(4096)
    snap = [b.buf.clone() for b in (out, f32)]
    calls = (
        lambda: L.sdmi_adda_in_fwd(ptr(x.data), 2, 8, 4, ptr(s.data), 0.01, 10, 5, 8, ptr(out.data), st),  # 10 bits
        lambda: L.sdmi_adda_in_fwd(ptr(x.data), 2, 8, 4, ptr(s.data), 0.01, 8, 1, 8, ptr(out.data), st),  # dac 1
        lambda: L.sdmi_adda_in_fwd(ptr(x.data), 2, 8, 4, ptr(s.data), 0.01, 8, 5, 0, ptr(out.data), st),  # no rows
        lambda: L.sdmi_adda_in_fwd(ptr(x.data), 2, 8, 4, None, 0.01, 8, 5, 8, ptr(out.data), st),
        lambda: L.sdmi_adda_in_fwd(ptr(x.data), 2, 8, 4, ptr(s.data), 0.01, 8, 5, 8, ptr(out.data[1:]), st),  # align
        lambda: L.sdmi_adda_pack_w(ptr(x.data), 8, 8, 8, None, None, st),
        lambda: L.sdmi_adda_gemm(ptr(out.data), ptr(out.data), None, 8, 8, 8, 8, 8, 5, 8, ptr(s.data), None, None, None,
                                 None, None, ptr(f32.data), 4, None, None, st),  # ld < N
        lambda: L.sdmi_adda_gemm(ptr(out.data), ptr(out.data), None, 8, 8, 8, 8, 8, 5, 8, ptr(s.data), ptr(x.data), None,
                                 None, None, None, ptr(f32.data), 8, None, None, st),  # one noise vector only
        lambda: L.sdmi_adda_gemm(ptr(out.data), ptr(out.data), None, 8, 8, 8, 8, 8, 5, 8, ptr(s.data), None, None, None,
                                 None, None, ptr(f32.data), 8, ptr(f32.data), None, st),  # mask without T
        lambda: L.sdmi_adda_absmax(ptr(x.data), 0, ptr(f32.data), ptr(f32.data), st),
    )
    for i, call in enumerate(calls):
        rc, ops = recorded(L, call)
        assert rc == -1 and ops == [], f"call {i}: returned {rc}, launched {ops}"
    torch.cuda.synchronize()
    for a, b in zip(snap, (out, f32)):
        assert torch.equal(bits(a), bits(b.buf))
