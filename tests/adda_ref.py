"""The reference's ADC/DAC-aware CIM layers restated by hand in torch (cim_layers/layers_qn_lsq_adda_cim.py,
layers_utils_adda.py, layers_utils_lsq.py, quant_noise_utils.py), for fp32 and fp64, and what the ADC tests share: the
fixture's cases, the fp32 emulation of the kernels of csrc/adda.hip, and the derived bounds.

Statements (u = 2^-24, sb = dac_bit - 1, L = ceil((input_bit - 1) / sb), R = 2^(adc_bit-1) - 1, W2 = weight.reshape(N, -1).T):

  forward  Without weight noise every partial sum P is an integer below 2^24 (576 rows x 15 x 127 = 1 097 280), exact in
           fp32 in any order, and every later operation is one fp32 operation on its own: y, pre, the slices, the mask
           bits and T are bitwise the restatement's. No ADC input needs to stay away from a rounding tie for that: the
           reference, the restatement and the kernel all form fl(as P) from the same two numbers. The three LSQ
           quantisers' inputs are kept TIE_DISTANCE away from ties as in tests/lsq_ref.py.
  backward The one rounding the HIP path adds is bf16 (8 significant bits: a relative error of at most 2^-8) on the masked
           operands, which are products of d_pre (already bf16 from the output quantiser's backward) with a count 0 .. L
           or a power of two: U = bf16(dZ cnt) rounds a second time (cnt is not a power of two), V = bf16(dZ 2^(i sb)) of
           dZ = fl(fl(fl(d_pre / as) / is) / ws) rounds the three divisions' result. Each operand element is therefore
           within BWD_REL = 2^-8 + 2^-8 + 2^-16 of its float64 value, the fp32 roundings (a few u) included. Pushed through absolute values of the same chain
           (grad_bounds):
             e_x  = BWD_REL (as / L) (|dZ| M_j) |W2|^T                    per row block, into d x_q
             e_w  = BWD_REL as sum_i 2^(i sb) |X_i|^T (|dZ| mask_ij)      into d w_qn
             dx, dw: the quantiser's dx is the incoming gradient or 0: |dx - dx64| <= e_x / se_x (e_w / se_w)
             ds_in, ds_w: g sum e m / se + the summation term of tests/lsq_ref.py, m = |q - v| inside and Qp outside
             d adc_scale = S1 - S2 / as, S1 = sum dZ T, S2 = sum d_pre (pre - bias): |.| <= BWD_REL (sum |dZ T| +
               sum |d_pre (pre - bias)| / as) + K_LSQ u (the same sums); adc_gain.grad is that times |d as / d gain|
             ds_out, db: as in section 17 (ds_out is formed before the rounding; db sums bf16 d_pre: at most BWD_REL sum |d_pre|)
  noise    With weight noise w_qn is not an integer. The kernel multiplies the slices (exact in bf16) by hi = bf16(w) and
           lo = bf16(w - hi): |w - hi - lo| <= 2^-18 |w|, and the fp32 accumulation of the block's 2 rbp products (high and
           low part, rbp the block's padded length) adds at most 2 rbp u sum |x w|. So the kernel's A = as P is within
             tau = as (2^-18 + 2 rbp u) (|X_i| |W2|)     (per block and slice)
           of the float64 value, and an ADC code may differ from the float64 restatement's only where the float64 A lies
           within tau of a rounding tie or of a clamp edge (near_tie).
"""
import math

import torch

from tests import lsq_ref as LR

U24 = LR.U24
BWD_REL = 2.0 ** -8 + 2.0 ** -8 + 2.0 ** -16
GRID = 2.0 ** -10  # the fixture's weights are int8 multiples of this
TIE_DISTANCE = LR.TIE_DISTANCE

# name -> (kind, (in, out[, H, W]), input shape, blocks, config). Config keys as the reference's constructor.
_BASE = dict(weight_bit=4, input_bit=8, output_bit=8, noise_scale=0, dac_bit=5, adc_bit=8, adc_gain_1_scale=9.071428571,
             adc_gain_range=[1 / 64, 1 / 64], adc_adjust_mode="current", gain_noise_scale=0, offset_noise_scale=0, seed=0)
_SMALL = dict(_BASE, adc_gain_range=[1 / 64, 1 / 4])


def _case(kind, geo, shape, blocks, cfg, **extra):
    return dict(dict(kind=kind, geo=geo, shape=shape, blocks=blocks, cfg=cfg, fresh=False, gain=None, data=None), **extra)


CASES = {
    "c1_ref": _case("linear", (1300, 96), (2, 1300), (576, 2048), _BASE),
    "c2_small": _case("linear", (200, 40), (2, 3, 200), (64, 16), _SMALL, gain=1 / 24),
    "c3_conv": _case("conv", (72, 24), (1, 72, 5, 5), (32, 2048), _SMALL, gain=1 / 16),
    "c4_7slices": _case("linear", (200, 40), (2, 3, 200), (64, 16), dict(_SMALL, dac_bit=2, adc_bit=4), gain=1 / 40,
                        data="c2_small"),
    "c5_gain": _case("linear", (200, 40), (2, 3, 200), (64, 16),
                     dict(_SMALL, adc_adjust_mode="gain", adc_gain_range=[1, 16], adc_gain_1_scale=0.0125), gain=3.3,
                     data="c2_small"),
    "c6_adcnoise": _case("linear", (200, 40), (2, 3, 200), (64, 16),
                         dict(_SMALL, gain_noise_scale=0.05, offset_noise_scale=0.05, seed=5), gain=1 / 24,
                         data="c2_small"),
    "c7_fresh": dict(_case("linear", (1300, 96), (2, 1300), (576, 2048), _BASE, data="c1_ref"), fresh=True),
    "c8_wnoise": _case("linear", (200, 40), (2, 3, 200), (64, 16), dict(_SMALL, noise_scale=0.08), gain=1 / 24,
                       data="c2_small"),
}
# the weight sits on a grid: a factor of 0.8 puts k 7 / (0.8 k_max) on exact ties (k_max = 28: k = 8 -> 2.5)
STEP_FACTORS = dict(input=0.75, output=0.7)
WEIGHT_FACTORS = tuple(round(0.7 + 0.005 * i, 3) for i in range(60))  # candidates (make_golden_adda.py weight_plan)
DW_ROWS = {"c1_ref": 32, "c7_fresh": 32, "c3_conv": 1}  # every n-th row of dw is recorded (default 8)


def dw_rows(name, N):
    return list(range(0, N, DW_ROWS.get(name, 8)))


def split_dict(rows, cols, blocks):
    out = {}
    for rb in range(-(-rows // blocks[0])):
        for cb in range(-(-cols // blocks[1])):
            out[f"{rb}_{cb}"] = dict(start_row=rb * blocks[0], start_col=cb * blocks[1],
                                     row_num=min(blocks[0], rows - rb * blocks[0]),
                                     col_num=min(blocks[1], cols - cb * blocks[1]))
    return out


def n_slices(input_bit, dac_bit):
    return int(math.ceil((input_bit - 1) / (dac_bit - 1)))


# ---- the reference's functions -------------------------------------------------------------------------------------------
round_pass, clamp_pass, grad_scale = LR.round_pass, LR.clamp_pass, LR.grad_scale


def adc_scale_of(gain, cfg):
    lo, hi = float(cfg["adc_gain_range"][0]), float(cfg["adc_gain_range"][1])
    g = clamp_pass(gain, lo, hi)
    g = round_pass(g) if cfg["adc_adjust_mode"] == "gain" else 1 / round_pass(1 / g)
    return g * cfg["adc_gain_1_scale"]


def quant_int(x, bit, step):
    """data_quant_lsq(isint=True): the code with the gradient of q se / se.detach()."""
    qp = LR.qp_of(bit)
    se = grad_scale(step, LR.g_of(bit, x.numel()))
    q = round_pass(torch.clamp(x / se, -qp, qp))
    return q * se / se.detach()


def floor_pass(x):
    y = torch.floor(x.abs().detach()) * x.sign().detach()
    return (y - x).detach() + x


def split(xq, input_bit, sb, twos=False):
    """bit_split_tensor: the L slices of xq, each with gradient 1 / (L 2^(i sb)) to xq. twos: two's-complement slices
    (floor towards minus infinity), a perturbation."""
    nL = int(math.ceil((input_bit - 1) / sb))
    out = []
    for i in range(nL):
        lsb, msb = i * sb, min((i + 1) * sb, input_bit - 1)
        if twos:
            shift = (torch.floor(xq / 2 ** lsb) - xq / 2 ** lsb).detach() + xq / 2 ** lsb
            resid = torch.floor(xq / 2 ** msb).detach() * 2 ** sb
        else:
            shift = floor_pass(xq / 2 ** lsb)
            t = xq / 2 ** msb
            resid = torch.where(t >= 0, t.floor(), t.ceil()).detach() * 2 ** sb
        bit = shift - resid
        out.append((bit - shift / nL).detach() + shift / nL)
    return out


def rows_of(kind, x):
    """The layer's input as [rows..., K]."""
    if kind == "conv":
        B, C, H, W = x.shape
        return x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    return x


def unrows(kind, z, x):
    if kind == "conv":
        B, _, H, W = x.shape
        return z.permute(0, 2, 1).reshape(B, z.shape[-1], H, W)
    return z


def _sub(t, value):
    """t with its value replaced (the gradient still flows through t)."""
    return (value.to(t.dtype) - t).detach() + t


def layer_forward(kind, x, w, b, steps, gain, cfg, mapping, *, eps=None, gain_noise=None, offset_noise=None, perturb=None,
                  keep=None, decide=None, pre_hook=None):
    """The reference layer's forward (use_FP=False) in the precision of its arguments. steps: (input, weight, output).
    perturb: 'clamp_R' (lower clamp at -R), 'adc_recombined' (one ADC on the recombined sum of a block), 'merged' (the
    row blocks merged into one), 'no_mask' (the clamp passes every gradient), 'twos' (two's-complement slices).
    keep: a dict that receives the ADC inputs A [(block key, slice)], the partial sums P, w_qn and the values of x_q and
    of the weight codes. decide: the `keep` of an fp32 run whose x_q, weight codes and ADC inputs replace this run's
    values: a float64 run then takes every discrete decision (the floor of the slices, the ADC's clamp and rounding)
    as fp32 took it -- q se / se is not q in either precision, and not at the same codes. Returns (y, pre)."""
    ib, sb = cfg["input_bit"], cfg["dac_bit"] - 1
    R = 2 ** (cfg["adc_bit"] - 1) - 1
    a_s = adc_scale_of(gain, cfg)
    xq = quant_int(x, ib, steps[0])
    wq = quant_int(w, cfg["weight_bit"], steps[1])
    if decide is not None:
        xq, wq = _sub(xq, decide["xq_v"]), _sub(wq, decide["wq_v"])
    if keep is not None:
        keep.update(xq_v=xq.detach(), wq_v=wq.detach())
    if keep is not None and xq.requires_grad:
        xq.retain_grad()
        wq.retain_grad()
        keep.update(xq_t=xq, wq_t=wq)
    X = [rows_of(kind, s) for s in split(xq, ib, sb, twos=perturb == "twos")]
    if cfg["noise_scale"] != 0:
        wq = wq + (wq.max() - wq.min()) * cfg["noise_scale"] * eps
    W2 = wq.reshape(w.shape[0], -1).t()
    Z = torch.zeros(*X[0].shape[:-1], w.shape[0], dtype=x.dtype, device=x.device)
    if perturb == "merged":
        mapping = {"0_0": dict(start_row=0, start_col=0, row_num=W2.shape[0], col_num=W2.shape[1])}
    noisy = cfg["gain_noise_scale"] != 0 or cfg["offset_noise_scale"] != 0
    lo_edge = -R if perturb == "clamp_R" else -R - 1
    for key, m in mapping.items():
        r0, rn, c0, cn = m["start_row"], m["row_num"], m["start_col"], m["col_num"]
        Ps = [Xi[..., r0:r0 + rn] @ W2[r0:r0 + rn, c0:c0 + cn] for Xi in X]
        if perturb == "adc_recombined":
            Ps = [sum(P * 2 ** (i * sb) for i, P in enumerate(Ps))]
        acc = 0
        for i, P in enumerate(Ps):
            A = a_s * P
            if noisy:
                n = A * (1 + gain_noise[c0:c0 + cn].to(x.dtype)) + R * offset_noise[c0:c0 + cn].to(x.dtype)
                A = (n - A).detach() + A
            if decide is not None and "A" in decide and perturb is None:
                A = _sub(A, decide["A"][(key, i)])
            if keep is not None:
                keep.setdefault("A", {})[(key, i)] = A.detach()
                keep.setdefault("P", {})[(key, i)] = P.detach()
            C = clamp_pass(A, lo_edge, R) if perturb == "no_mask" else torch.clamp(A, lo_edge, R)
            acc = acc + round_pass(C) * 2 ** (i * sb)
        Z = Z + torch.nn.functional.pad(acc, (c0, Z.shape[-1] - c0 - cn))
    ws, is_ = (1 / steps[1]).detach(), (1 / steps[0]).detach()
    pre = unrows(kind, Z / ws / is_ / a_s, x)
    if b is not None:
        pre = pre + (b.view(1, -1, 1, 1) if kind == "conv" else b)
    if keep is not None:
        keep.update(wq=wq.detach(), a_s=a_s.detach(), X=[s.detach() for s in X])
    if pre_hook is not None:
        pre = pre_hook(pre)
    return LR.quant_lsq(pre, cfg["output_bit"], steps[2]), pre


def layer_grads(case, f, dtype, **kw):
    """Forward and backward of the restatement on fixture tensors f in dtype: y, pre, d_pre and every gradient. In
    float64 the discrete decisions are those of an fp32 run (layer_forward `decide`); with weight noise, whose fp32
    partial sums depend on the order of the additions, only those of x_q and the weight codes."""
    decide = None
    if dtype == torch.float64 and "decide" not in kw:
        decide = {}
        with torch.no_grad():
            layer_forward(case["kind"], f["x"], f["w"], f["b"], (f["s_in"], f["s_w"], f["s_out"]), f["gain"], case["cfg"],
                          split_dict(case["geo"][0], case["geo"][1], case["blocks"]), eps=f.get("eps"),
                          gain_noise=f.get("gain_noise"), offset_noise=f.get("offset_noise"), keep=decide)
        if case["cfg"]["noise_scale"] != 0:
            del decide["A"]
        kw["decide"] = decide
    leaf = {k: f[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b", "s_in", "s_w", "s_out", "gain")}
    keep = {}
    y, pre = layer_forward(case["kind"], leaf["x"], leaf["w"], leaf["b"], (leaf["s_in"], leaf["s_w"], leaf["s_out"]),
                           leaf["gain"], case["cfg"], split_dict(case["geo"][0], case["geo"][1], case["blocks"]),
                           eps=f["eps"].to(dtype) if "eps" in f else None, gain_noise=f.get("gain_noise"),
                           offset_noise=f.get("offset_noise"), keep=keep, **kw)
    pre.retain_grad()
    y.backward(f["dy"].to(dtype))
    out = dict(y=y.detach(), pre=pre.detach(), d_pre=pre.grad, dx=leaf["x"].grad, dw=leaf["w"].grad, db=leaf["b"].grad,
               ds_in=leaf["s_in"].grad, ds_w=leaf["s_w"].grad, ds_out=leaf["s_out"].grad, dgain=leaf["gain"].grad)
    out["keep"] = keep
    return out


def saturation(keep, cfg):
    """Fraction of the (block, slice, element) ADC inputs outside [-R-1, R]."""
    R = 2 ** (cfg["adc_bit"] - 1) - 1
    tot = sum(A.numel() for A in keep["A"].values())
    return sum(int(((A < -R - 1) | (A > R)).sum()) for A in keep["A"].values()) / tot


def near_tie(keep, cfg, mapping):
    """Per (block, slice): where the float64 ADC input lies within tau of a rounding tie or of a clamp edge."""
    R = 2 ** (cfg["adc_bit"] - 1) - 1
    W2 = keep["wq"].double().reshape(keep["wq"].shape[0], -1).t().abs()
    out = {}
    for (key, i), A in keep["A"].items():
        m = mapping[key]
        r0, rn, c0, cn = m["start_row"], m["row_num"], m["start_col"], m["col_num"]
        tau = float(keep["a_s"]) * (2.0 ** -18 + 2 * (-(-rn // 32) * 32) * U24) * (keep["X"][i][..., r0:r0 + rn].double().abs() @ W2[r0:r0 + rn, c0:c0 + cn])
        A = A.double()
        frac = (A - torch.floor(A) - 0.5).abs()
        out[(key, i)] = (frac <= tau) | ((A + R + 1).abs() <= tau) | ((A - R).abs() <= tau)
    return out


def grad_bounds(case, f, rel=BWD_REL, sum_rel=LR.K_LSQ * U24, w_rel=0.0):
    """(float64 reference, bound) of dx, dw (element-wise tensors) and of ds_in, ds_w, ds_out, dgain, db (module
    docstring), from the float64 restatement. rel: the relative error of an operand element of the two gradient
    products; sum_rel: that of a scalar sum against the sum of its terms' absolute values. The defaults are the HIP
    path's; for the reference's own fp32 autograd on the CPU (the fixture) they are cpu_rels(). w_rel: the relative
    error of the weight operand of the data-gradient product: 2^-8 on the HIP path with weight noise, where the
    non-integer w_qn enters that product as its bf16 high part alone (the forward adds the low part)."""
    d = torch.float64
    cfg = case["cfg"]
    ib, wb, sb = cfg["input_bit"], cfg["weight_bit"], cfg["dac_bit"] - 1
    R = 2 ** (cfg["adc_bit"] - 1) - 1
    r = layer_grads(case, f, d)
    k = r["keep"]
    mapping = split_dict(case["geo"][0], case["geo"][1], case["blocks"])
    nL = n_slices(ib, cfg["dac_bit"])
    a_s = float(k["a_s"])
    ws, is_ = 1 / float(f["s_w"]), 1 / float(f["s_in"])
    dpre = rows_of(case["kind"], r["d_pre"]) if case["kind"] == "conv" else r["d_pre"]
    dZ = (dpre / a_s / is_ / ws).abs()
    W2 = k["wq"].reshape(k["wq"].shape[0], -1).t().abs()
    e_x = torch.zeros_like(k["X"][0])
    e_w = torch.zeros_like(W2)
    T = torch.zeros_like(dZ)
    for (key, i), A in k["A"].items():
        m = mapping[key]
        r0, rn, c0, cn = m["start_row"], m["row_num"], m["start_col"], m["col_num"]
        mask = ((A >= -R - 1) & (A <= R)).to(d)
        g = dZ[..., c0:c0 + cn] * mask
        e_x[..., r0:r0 + rn] += (a_s / nL) * (g @ W2[r0:r0 + rn, c0:c0 + cn].t())
        Xi = k["X"][i][..., r0:r0 + rn].abs().reshape(-1, rn)
        e_w[r0:r0 + rn, c0:c0 + cn] += a_s * 2 ** (i * sb) * (Xi.t() @ g.reshape(-1, cn))
        T[..., c0:c0 + cn] += 2 ** (i * sb) * mask * k["P"][(key, i)]
    x, w = f["x"].to(d), f["w"].to(d)
    se_x = LR.effective_step(f["s_in"].to(d), ib, x.numel())
    se_w = LR.effective_step(f["s_w"].to(d), wb, w.numel())
    e_x = (rel + w_rel + rel * w_rel) * (unrows(case["kind"], e_x, x) if case["kind"] == "conv" else e_x) / se_x
    e_w = rel * e_w.t().reshape(w.shape) / se_w
    out = dict(dx=(r["dx"], e_x + 4 * U24 * r["dx"].abs()), dw=(r["dw"], e_w + 4 * U24 * r["dw"].abs()))
    if cfg["noise_scale"] != 0:
        # the range's gradient lands on the extreme codes: at most the whole error sum times noise_scale |eps|
        e_w = e_w + cfg["noise_scale"] * float((e_w * f["eps"].to(d).abs()).sum())
        out["dw"] = (r["dw"], e_w + 4 * U24 * r["dw"].abs())
    # the gradients entering the two quantisers (x_q = q se / se.detach(): divided by the step), in float64
    for name, xx, ss, bit, e, up in (("ds_in", x, f["s_in"].to(d), ib, e_x, k["xq_t"].grad / se_x),
                                     ("ds_w", w, f["s_w"].to(d), wb, e_w, k["wq_t"].grad / se_w)):
        m = LR.terms(xx, torch.ones_like(xx), ss, bit)["t"].abs()  # |q - v| inside, Qp outside
        g = LR.g_of(bit, xx.numel())
        out[name] = (float(r[name]), g * float((e * m).sum()) + sum_rel * g * float(LR.terms(xx, up, ss, bit)["t"].abs().sum())
                     + 4 * U24 * abs(float(r[name])))
    pre_nb = r["pre"] - (f["b"].to(d).view(1, -1, 1, 1) if case["kind"] == "conv" else f["b"].to(d))
    s1 = float(((dpre / a_s / is_ / ws) * T).abs().sum())
    s2 = float((r["d_pre"] * pre_nb).abs().sum()) / a_s
    leaf = f["gain"].to(d).clone().requires_grad_(True)
    adc_scale_of(leaf, cfg).backward()
    out["dgain"] = (float(r["dgain"]), (rel + sum_rel) * (s1 + s2) * abs(float(leaf.grad)))
    # ds_out is formed before any bf16 rounding, from fp32 pre (the reference's bitwise): the summation term, and v in
    # fp32 against float64 (4 u (Qp + 1) per element)
    qo = LR.qp_of(cfg["output_bit"])
    to = LR.terms(r["pre"], f["dy"].to(d), f["s_out"].to(d), cfg["output_bit"])
    g = LR.g_of(cfg["output_bit"], r["pre"].numel())
    out["ds_out"] = (float(r["ds_out"]), sum_rel * g * float(to["t"].abs().sum()) + g * 4 * U24 * (qo + 1) * float(f["dy"].abs().sum()))
    red = [i for i in range(r["d_pre"].dim()) if i != (1 if case["kind"] == "conv" else r["d_pre"].dim() - 1)]
    out["db"] = (r["db"], rel * r["d_pre"].abs().sum(red) + 4 * U24 * r["db"].abs())
    return out, r


# ---- the kernels of csrc/adda.hip in fp32 on the CPU -------------------------------------------------------------------
def geometry(M, N, K, rb, input_bit, dac_bit):
    rb = min(rb, K)
    rbp = -(-rb // 32) * 32
    nb = -(-K // rb)
    return dict(nb=nb, rbp=rbp, L=n_slices(input_bit, dac_bit), Mp=-(-M // 64) * 64, Np=-(-N // 64) * 64, Kp=nb * rbp,
                rb=rb)


def pad_cols(t, g, K):
    """[..., K] -> [..., Kp]: row blocks padded with zeros to rbp columns."""
    out = torch.zeros(*t.shape[:-1], g["Kp"], dtype=t.dtype)
    for j in range(g["nb"]):
        n = min(g["rb"], K - j * g["rb"])
        out[..., j * g["rbp"]:j * g["rbp"] + n] = t[..., j * g["rb"]:j * g["rb"] + n]
    return out


def codes32(x, step, bit):
    return LR.codes_of(x.float(), step.float(), bit)[0]


def xq32(x, step, bit):
    """x_q = fl(fl(q se) / se) in fp32."""
    q, se = LR.codes_of(x.float(), step.float(), bit)
    return q * se / se


def slices32(xq, input_bit, dac_bit):
    """The L sign-magnitude slices of x_q (fp32), the kernel's expression."""
    sb = dac_bit - 1
    a = xq.abs()
    out = []
    for i in range(n_slices(input_bit, dac_bit)):
        hi = min((i + 1) * sb, input_bit - 1)
        v = torch.floor(a / 2 ** (i * sb)) - torch.floor(a / 2 ** hi) * 2 ** sb
        out.append(torch.where(xq < 0, -v, v))
    return out


def emulate_in_fwd(x, step, input_bit, dac_bit, rb):
    """sdmi_adda_in_fwd: x (B, C, P) -> bf16 [L][Mp][Kp]."""
    B, C, P = x.shape
    g = geometry(B * P, 1, C, rb, input_bit, dac_bit)
    q = xq32(x, step, input_bit).permute(0, 2, 1).reshape(B * P, C)
    out = torch.zeros(g["L"], g["Mp"], g["Kp"])
    for i, s in enumerate(slices32(q, input_bit, dac_bit)):
        out[i, :B * P] = pad_cols(s, g, C)
    return out.to(torch.bfloat16), g


def emulate_pack_w(w, rb):
    """sdmi_adda_pack_w: w [N][K] fp32 -> hi, lo bf16 [Np][Kp]."""
    N, K = w.shape
    g = geometry(1, N, K, rb, 2, 2)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    out = []
    for t in (hi, lo):
        full = torch.zeros(g["Np"], g["Kp"], dtype=torch.bfloat16)
        full[:N] = pad_cols(t, g, K)
        out.append(full)
    return out[0], out[1], g


def emulate_gemm(X, w, rb, cfg, a_s, s_w, s_in, bias, gain_noise=None, offset_noise=None):
    """sdmi_adda_gemm on slices X (list of [M][K] fp32 integer tensors) and weight codes w [N][K] (fp32): pre, the mask
    words (int64 holding 32 bits each) [nwords][M][N], T, and the float64 partial sums; every operation in fp32 in the
    kernel's order. The partial sums are formed in float64 (exact for integer operands)."""
    M, K = X[0].shape
    N = w.shape[0]
    sb = cfg["dac_bit"] - 1
    R = float(2 ** (cfg["adc_bit"] - 1) - 1)
    g = geometry(M, N, K, rb, cfg["input_bit"], cfg["dac_bit"])
    f32 = torch.float32
    a_s = a_s.to(f32)
    Z, T = torch.zeros(M, N), torch.zeros(M, N)
    words = torch.zeros(-(-g["nb"] * g["L"] // 32), M, N, dtype=torch.int64)
    Ps = {}
    if gain_noise is not None:
        gf, go = 1 + gain_noise[:N].to(f32), R * offset_noise[:N].to(f32)
    for j in range(g["nb"]):
        r0, rn = j * g["rb"], min(g["rb"], K - j * g["rb"])
        for i, Xi in enumerate(X):
            P64 = Xi[:, r0:r0 + rn].double() @ w[:, r0:r0 + rn].double().t()
            Ps[(j, i)] = P64
            P = P64.to(f32)
            A = a_s * P
            if gain_noise is not None:
                n = A * gf + go
                A = (n - A) + A
            inside = (A >= -R - 1) & (A <= R)
            C = torch.clamp(A, -R - 1, R)
            Q = (torch.round(C) - C) + C
            pw = float(2 ** (i * sb))
            Z = Z + pw * Q
            T = T + torch.where(inside, pw * P, torch.zeros_like(P))
            bit = j * g["L"] + i
            words[bit // 32] |= inside.to(torch.int64) << (bit % 32)
    pre = Z
    if s_w is not None:
        pre = pre / (1 / s_w.to(f32))
    if s_in is not None:
        pre = pre / (1 / s_in.to(f32))
    pre = pre / a_s
    if bias is not None:
        pre = pre + bias.to(f32)
    return dict(pre=pre, words=words, T=T, P=Ps, geo=g)


def emulate_bwd_ops(dpre, pre, bias, T, words, nb, nL, sb, a_s, s_w, s_in):
    """sdmi_adda_bwd_ops on d_pre (bf16 [M][N]): U [nb][M][N], V [nb][L][M][N] (bf16), the fp32 terms of the two sums."""
    f32 = torch.float32
    d = dpre.float()
    dz = d / a_s.to(f32)
    if s_in is not None:
        dz = dz / (1 / s_in.to(f32))
    if s_w is not None:
        dz = dz / (1 / s_w.to(f32))
    U, V = [], []
    for j in range(nb):
        cnt = torch.zeros_like(dz)
        row = []
        for i in range(nL):
            bit = j * nL + i
            b = ((words[bit // 32] >> (bit % 32)) & 1).to(f32)
            cnt = cnt + b
            row.append(torch.where(b > 0, dz * float(2 ** (i * sb)), torch.zeros_like(dz)).to(torch.bfloat16))
        V.append(torch.stack(row))
        U.append((dz * cnt).to(torch.bfloat16))
    t1 = dz * T
    t2 = d * ((pre - bias.to(f32)) if bias is not None else pre)
    return dict(U=torch.stack(U), V=torch.stack(V), t1=t1, t2=t2, dz=dz)


def cpu_rels(case):
    """(rel, sum_rel) of grad_bounds for fp32 autograd on the CPU: a dot product of n terms is within n u of its
    absolute-value sum whatever the order, n at most the longest of the layer's sums (a row block, the output columns,
    the rows times the slices) plus the handful of elementwise roundings around it; a scalar sum over a whole tensor
    likewise with n its element count."""
    K, N = case["geo"]
    rows = 1
    for s in case["shape"]:
        rows *= s
    rows //= K
    nL = n_slices(case["cfg"]["input_bit"], case["cfg"]["dac_bit"])
    return (max(min(K, case["blocks"][0]), N, rows * nL) + 32) * U24, max(K * N, rows * K, rows * N) * U24


# ---- the fixture ----------------------------------------------------------------------------------------------------------
SCALARS = ("s_in", "s_w", "s_out", "gain", "ds_in", "ds_w", "ds_out", "dgain", "s_in0", "gain0")


def load_fixture():
    """tests/golden/adda_layers.safetensors: ({case: tensors, shared data resolved, w rebuilt from w_k}, metadata)."""
    import os
    from safetensors import safe_open
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adda_layers.safetensors")
    with safe_open(path, "pt") as fh:
        t = {k: fh.get_tensor(k) for k in fh.keys()}
        meta = fh.metadata()
    out = {}
    for name, c in CASES.items():
        own = c["data"] or name
        f = {k.split(".", 1)[1]: v for k, v in t.items() if k.startswith(name + ".")}
        for k in ("x", "b", "dy"):
            f.setdefault(k, t[f"{own}.{k}"])
        f["w"] = t[f"{own}.w_k"].float() * GRID
        for k in SCALARS:
            if k in f:
                f[k] = f[k].reshape(())
        if "eps" in f:
            f["eps"] = f["eps"].float()
        f["map"] = {key: dict(zip(("start_row", "start_col", "row_num", "col_num"), (int(v) for v in row)))
                    for key, row in zip(meta[f"{name}.map_keys"].split(","), f["mapping"])}
        out[name] = f
    return out, meta


# ---- the reference layers as modules (for whole-model comparisons) -------------------------------------------------------
class _RefMixin:
    def _setup(self, cfg, blocks):
        self.cfg, self.round_dpre = dict(cfg), False
        for k in ("input", "output", "weight"):
            setattr(self, f"step_size_{k}", torch.nn.Parameter(torch.tensor(1.0)))
        self.adc_gain = torch.nn.Parameter(torch.tensor(float(cfg["adc_gain_range"][0])))
        self.map = split_dict(self.weight[0].numel(), self.weight.shape[0], blocks)

    def _fwd(self, x, **kw):
        kind = "conv" if isinstance(self, torch.nn.Conv2d) else "linear"
        if self.cfg["noise_scale"] != 0:
            kw["eps"] = torch.randn_like(self.weight)
        return layer_forward(kind, x, self.weight, self.bias, (self.step_size_input, self.step_size_weight,
                                                               self.step_size_output), self.adc_gain, self.cfg, self.map, **kw)

    def forward(self, x):
        cfg = self.cfg
        with torch.no_grad():  # first use, in the reference's order: input step, weight step, gain, output step
            for which, t in (("input", x), ("weight", self.weight)):
                s = getattr(self, f"step_size_{which}")
                if s == 1:
                    s.data = LR.init_step(t.detach(), cfg[f"{which}_bit"]).to(s.device)
            if self.adc_gain == float(cfg["adc_gain_range"][0]):
                keep = {}
                self._fwd(x, keep=keep)
                first = next(iter(self.map))
                top = max(float(keep["P"][(first, i)].abs().max()) for i in range(n_slices(cfg["input_bit"], cfg["dac_bit"])))
                if top != 0:
                    R = 2 ** (cfg["adc_bit"] - 1) - 1
                    gain = torch.clamp(R / torch.tensor(top) / cfg["adc_gain_1_scale"], min=0.8 * cfg["adc_gain_range"][0],
                                       max=1.2 * cfg["adc_gain_range"][1])
                    self.adc_gain.data.copy_(gain)
            if self.step_size_output == 1:
                self.step_size_output.data = LR.init_step(self._fwd(x)[1], cfg["output_bit"]).to(x.device)
        return self._fwd(x, pre_hook=LR._RoundGrad.apply if self.round_dpre else None)[0]


class RefConv2d(_RefMixin, torch.nn.Conv2d):
    pass


class RefLinear(_RefMixin, torch.nn.Linear):
    pass


def convert_ref(model, cfg, blocks):
    """Every exact nn.Conv2d / nn.Linear of model -> the restatement layer on the same Parameters."""
    nn = torch.nn
    todo = []
    for name, m in model.named_modules():
        if type(m) is nn.Conv2d:
            new = RefConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=m.bias is not None)
        elif type(m) is nn.Linear:
            new = RefLinear(m.in_features, m.out_features, bias=m.bias is not None)
        else:
            continue
        new.weight = m.weight
        if m.bias is not None:
            new.bias = m.bias
        new._setup(cfg, blocks)
        new.to(m.weight.device)
        todo.append((name, new))
    for name, new in todo:
        parent = model.get_submodule(name.rsplit(".", 1)[0]) if "." in name else model
        setattr(parent, name.rsplit(".", 1)[-1], new)
    return [n for n, _ in todo]
