"""The reference's LSQ quantiser and quantise-and-noise layers restated by hand in torch (cim_layers/quant_noise_utils.py:
51-69, 101-120; layers_utils_lsq.py:31-83; layers_qn_lsq.py:100-121, 195-216), for fp32 and fp64, and what the LSQ tests
share: the per-element step-gradient terms, the fp32 emulation of the kernels' summation order and the derived bounds.

Statements (u = 2^-24, Qp = 2^(bit-1) - 1, g = fp32(1 / sqrt(Qp numel)), se the step's forward value):

  y, dx    bitwise the restatement's value / autograd gradient in fp32.
  ds       the kernels form t_i = dy_i (q_i - v_i) inside the clamp range and dy_i q_i outside, per element, and add them
           in a fixed order; |ds - ds64| <= K_LSQ u g sum |t_i| with ds64 the float64 sum of the fp32 terms times g
           (sum_bound). K_LSQ is measured, not chosen: tests/test_lsq_cpu.py emulates the kernels' order in fp32
           (emulate_flat: a thread's elements 4t .. 4t+3 of each of its 1024-element spans in sequence, the butterfly,
           the four waves in order, then the finisher's butterfly and waves and its one multiplication by g;
           emulate_items: lsq_out_bwd's items) on every case of the GPU kernel test (quant_case) and on the output
           quantiser of every fixture case, and K_LSQ lies between twice and three times the largest |ds32 - ds64| /
           (u g sum |t|) seen: MEASURED = 1.645 (the output quantiser of the 6x24 linear case at 8 bit, 240 terms that
           hardly cancel, so that the last multiplication's rounding alone is close to 1; 1.138 on the kernel cases, at
           most 0.77 on the fixture's input and weight sums), K_LSQ = 4.
  layer    y of a layer equals the reference's bitwise when every quantiser input is 1e-3 code units from a rounding
           tie and from +-Qp (equal codes times the same se). The one approximation in the backward is d_pre rounded to
           bf16, a relative error of at most 2^-9 per element. Pushed through the absolute values of the same chain it
           bounds the step gradients (step_grad_bounds):
             e_w = 2^-9 se_x (|d_pre|^T |codes_x|),   |d ds_w| <= g_w sum e_w m_w + the summation term of ds_w
             e_x = 2^-9 se_w (|d_pre| |codes_w|),     |d ds_x| <= g_x sum e_x m_x + the summation term of ds_x
           with m = |q - v| inside and Qp outside; the output quantiser sits before the rounding, so ds_out gets the
           summation term alone, against the float64 sum of the terms decided in fp32 from pre = fl(fl(acc fl(se_x
           se_w)) + bias), acc the exact integer dot product.
"""
import contextlib
import io

import numpy as np
import torch
import torch.nn.functional as F

from tests.dit_matrix import butterfly32, seq32
from tests.vq_matrix import _pad

NT, SPAN, CAP = 256, 1024, 256
U24 = 2.0 ** -24
BF16_REL = 2.0 ** -9
K_LSQ = 4.0
MEASURED = 1.645  # largest emulated |ds32 - ds64| / (u g sum |t|) (tests/test_lsq_cpu.py checks 2 x <= K_LSQ <= 3 x)
TIE_DISTANCE = 1e-3

# (name, kind, (cin, cout, k, stride, pad) or (fin, fout, bias), input shape) of the fixture tests/golden/lsq_layers.safetensors
CASES = (("conv3", "conv", (5, 12, 3, 1, 1), (2, 5, 12, 10)),
         ("conv4s2", "conv", (16, 16, 4, 2, 1), (2, 16, 12, 10)),
         ("conv1", "conv", (18, 32, 1, 1, 0), (2, 18, 6, 5)),
         ("lin_b", "linear", (24, 40, True), (2, 7, 24)),
         ("lin", "linear", (24, 40, False), (6, 24)))
WEIGHT_BITS = (8, 4)
FEATURE_BIT = 8
STEP_FACTORS = dict(input=0.75, weight=0.8, output=0.7)


def qp_of(bit):
    return 2 ** (bit - 1) - 1


def g_of(bit, numel):
    """grad_scale_factor in double, as the reference computes it."""
    return 1.0 / ((qp_of(bit) * numel) ** 0.5)


def g32(bit, numel):
    return float(np.float32(g_of(bit, numel)))


def grad_scale(x, scale):
    y_grad = x * scale
    return (x - y_grad).detach() + y_grad


def round_pass(x):
    return (torch.round(x) - x).detach() + x


def clamp_pass(x, lo, hi):
    return (torch.clamp(x, lo, hi) - x).detach() + x


def quant_lsq(x, bit, step, *, perturb=None):
    """data_quant_lsq / weight_quant_lsq with isint=False. perturb: 'no_g' (the gradient scale dropped), 'no_mask' (the
    clamp passes every gradient), 'q_only' (the step gradient misses the -v part)."""
    qp = qp_of(bit)
    se = step if perturb == "no_g" else grad_scale(step, g_of(bit, x.numel()))
    v = x / (se.detach() if perturb == "q_only" else se)
    c = clamp_pass(v, -qp, qp) if perturb == "no_mask" else torch.clamp(v, -qp, qp)
    return round_pass(c) * se


def init_step(x, bit):
    """init_step_size: 1 / (1 / range * Qp), the reference's rounding order; 1.0 at range 0."""
    r = x.abs().max()
    if r == 0:
        return torch.ones((), dtype=x.dtype)
    return 1 / (1 / r * qp_of(bit))


def effective_step(step, bit, numel):
    """The forward value of grad_scale(step, g) in the step's own precision."""
    with torch.no_grad():
        return grad_scale(step, g_of(bit, numel))


def terms(x, dy, step, bit):
    """v, q, inside and the step-gradient terms t_i of one quantiser in the precision of its arguments, every operation
    rounded on its own."""
    qp = qp_of(bit)
    se = effective_step(step, bit, x.numel())
    v = x / se
    c = torch.clamp(v, -qp, qp)
    q = (torch.round(c) - c) + c  # round_pass's value: round(c) with a zero result always +0
    inside = (v >= -qp) & (v <= qp)
    t = dy * torch.where(inside, q - v, q)
    return dict(v=v, q=q, inside=inside, t=t, se=se)


def sum_bound(t, g, K=None):
    return (K_LSQ if K is None else K) * U24 * g * float(t.double().abs().sum())


def flat_blocks(n):
    return min(CAP, -(-n // SPAN))


def item_blocks(n):
    return min(CAP, -(-n // NT))


def emulate_flat(t):
    """S of the flat kernels (lsq_quant_bwd / lsq_in_bwd) in fp32 in their order; t flat fp32."""
    n = t.numel()
    grid = flat_blocks(n)
    trips = -(-n // (grid * SPAN))
    a = _pad(t.float().reshape(-1), trips * grid * SPAN).view(trips, grid, NT // 64, 64, 4)
    a = seq32(a.permute(0, 4, 1, 2, 3).reshape(trips * 4, grid, NT // 64, 64), 0)
    part = seq32(butterfly32(a), 1)
    return float(seq32(butterfly32(_pad(part, NT).view(NT // 64, 64)), 0))


def emulate_items(t):
    """S of lsq_out_bwd: t is [groups][B P][8] (item = group * BP + pixel, channels ascending within an item)."""
    G, BP, _ = t.shape
    items = G * BP
    grid = item_blocks(items)
    trips = -(-items // (grid * NT))
    a = _pad(t.float().reshape(items, 8), trips * grid * NT).view(trips, grid, NT // 64, 64, 8)
    a = seq32(a.permute(0, 4, 1, 2, 3).reshape(trips * 8, grid, NT // 64, 64), 0)
    part = seq32(butterfly32(a), 1)
    return float(seq32(butterfly32(_pad(part, NT).view(NT // 64, 64)), 0))


# ---- one layer ---------------------------------------------------------------------------------------------------------
def matmul_of(kind, geo):
    if kind == "conv":
        _, _, _, s, p = geo
        return lambda x, w, b: F.conv2d(x, w, b, stride=s, padding=p)
    return lambda x, w, b: F.linear(x, w, b)


def bf16r(t):
    """Round to bf16 and back (RNE), keeping the dtype; the gradient passes."""
    return (t.detach().to(torch.float32).to(torch.bfloat16).to(t.dtype) - t).detach() + t


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float32).to(torch.bfloat16).to(g.dtype)


def layer_forward(kind, geo, x, w, b, steps, bits, *, quant=(True, True, True), perturb=None, noise=None,
                  bf16_ops=False):
    """The reference layer's forward (use_FP=False). steps / bits / quant: (input, weight, output). noise: (n_scale,
    eps) or None. perturb: a quant_lsq perturbation applied to all three quantisers, or 'no_factor' (the GEMM runs on
    the codes and the se_x se_w factor is forgotten). bf16_ops: operands of the GEMM and d_pre rounded to bf16 (the HIP
    path's plain-leaf approximation, for measuring the whole-model tolerance). Returns (y, pre, GEMM operands x, w)."""
    mm = matmul_of(kind, geo)
    qp = perturb if perturb != "no_factor" else None
    xq = quant_lsq(x, bits[0], steps[0], perturb=qp) if quant[0] else x
    wq = quant_lsq(w, bits[1], steps[1], perturb=qp) if quant[1] else w
    if noise is not None and noise[0] != 0:
        wq = wq + (wq.max() - wq.min()) * noise[0] * noise[1]
    if perturb == "no_factor":
        xq = xq / effective_step(steps[0], bits[0], x.numel()) if quant[0] else xq
        wq = wq / effective_step(steps[1], bits[1], w.numel()) if quant[1] else wq
    if bf16_ops:
        xq, wq = bf16r(xq), bf16r(wq)
    pre = mm(xq, wq, b)
    if bf16_ops:
        pre = _RoundGrad.apply(pre)
    y = quant_lsq(pre, bits[2], steps[2], perturb=qp) if quant[2] else pre
    return y, pre, xq, wq


def layer_grads(kind, geo, f, wbit, dtype, **kw):
    """Forward and backward of the restatement on fixture tensors `f` (x, w, b or None, s_in, s_w, s_out, dy) in dtype:
    dict of y, pre, dx, dw, db, ds_in, ds_w, ds_out."""
    leaf = {k: f[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "s_in", "s_w", "s_out")}
    b = f["b"].to(dtype).clone().requires_grad_(True) if f.get("b") is not None else None
    y, pre, xq, wq = layer_forward(kind, geo, leaf["x"], leaf["w"], b, (leaf["s_in"], leaf["s_w"], leaf["s_out"]),
                                   (FEATURE_BIT, wbit, FEATURE_BIT), **kw)
    for t in (pre, xq, wq):
        t.retain_grad()
    y.backward(f["dy"].to(dtype))
    out = dict(y=y.detach(), pre=pre.detach(), xq=xq.detach(), wq=wq.detach(), d_pre=pre.grad, d_xq=xq.grad,
               d_wq=wq.grad, dx=leaf["x"].grad,
               dw=leaf["w"].grad,
               ds_in=leaf["s_in"].grad, ds_w=leaf["s_w"].grad, ds_out=leaf["s_out"].grad)
    if b is not None:
        out["db"] = b.grad
    return out


def codes_of(x, step, bit):
    se = effective_step(step, bit, x.numel())
    qp = qp_of(bit)
    c = torch.clamp(x / se, -qp, qp)
    return (torch.round(c) - c) + c, se


def pre32(kind, geo, f, wbit):
    """The HIP path's pre-activation bit for bit: the exact integer dot product of the fp32-decided codes (formed in
    float64, where it is exact), then fl(fl(acc fl(se_x se_w)) + bias) in fp32."""
    x, w = f["x"].float(), f["w"].float()
    cx, sex = codes_of(x, f["s_in"].float(), FEATURE_BIT)
    cw, sew = codes_of(w, f["s_w"].float(), wbit)
    acc = matmul_of(kind, geo)(cx.double(), cw.double(), None)
    assert float(acc.abs().max()) < 2 ** 24
    pre = acc.float() * (sex * sew)
    if f.get("b") is not None:
        b = f["b"].float()
        pre = pre + (b.view(1, -1, 1, 1) if kind == "conv" else b)
    return pre


def quantiser_inputs64(kind, geo, f, wbit):
    """The three quantisers' inputs in code units, evaluated in float64: v_x, v_w, v_pre."""
    d = torch.float64
    x, w = f["x"].to(d), f["w"].to(d)
    s = [f[k].to(d) for k in ("s_in", "s_w", "s_out")]
    b = f["b"].to(d) if f.get("b") is not None else None
    with torch.no_grad():
        _, pre, _, _ = layer_forward(kind, geo, x, w, b, s, (FEATURE_BIT, wbit, FEATURE_BIT))
    return (x / effective_step(s[0], FEATURE_BIT, x.numel()), w / effective_step(s[1], wbit, w.numel()),
            pre / effective_step(s[2], FEATURE_BIT, pre.numel()))


def tie_distance(v, bit):
    """Smallest distance (code units) of v from a rounding tie (k + 0.5, inside the range) and from +-Qp."""
    qp = qp_of(bit)
    frac = (v - torch.floor(v) - 0.5).abs()
    frac = torch.where(v.abs() < qp, frac, torch.full_like(frac, float("inf")))
    return float(torch.minimum(frac, (v.abs() - qp).abs()).min())


def step_grad_bounds(kind, geo, f, wbit, K=None):
    """The derived bounds of the module docstring for (ds_in, ds_w, ds_out), and their float64 references:
    dict name -> (reference, bound)."""
    d = torch.float64
    r = layer_grads(kind, geo, f, wbit, d)
    mm = matmul_of(kind, geo)
    x, w = f["x"].to(d), f["w"].to(d)
    s_in, s_w = f["s_in"].to(d), f["s_w"].to(d)
    cx, sex = codes_of(x, s_in, FEATURE_BIT)
    cw, sew = codes_of(w, s_w, wbit)
    # |d_pre| against |codes| through the same conv / linear: gradients of sum(mm(|cx|, |cw|) * |d_pre|)
    ax, aw = cx.abs().requires_grad_(True), cw.abs().requires_grad_(True)
    (mm(ax, aw, None) * r["d_pre"].abs()).sum().backward()
    e_x, e_w = BF16_REL * sew * ax.grad, BF16_REL * sex * aw.grad
    out = {}
    for name, xx, ss, bit, e, up in (("ds_in", x, s_in, FEATURE_BIT, e_x, r["d_xq"]),
                                     ("ds_w", w, s_w, wbit, e_w, r["d_wq"])):
        m = terms(xx, torch.ones_like(xx), ss, bit)["t"].abs()  # |q - v| inside, Qp outside
        t = terms(xx, up, ss, bit)["t"]  # the float64 terms of the reference itself
        g = g_of(bit, xx.numel())
        out[name] = (float(r[name]), g * float((e * m).sum()) + sum_bound(t, g, K))
    p32 = pre32(kind, geo, f, wbit)
    to = terms(p32, f["dy"].float(), f["s_out"].float(), FEATURE_BIT)
    g = g32(FEATURE_BIT, p32.numel())
    out["ds_out"] = (float(to["t"].double().sum()) * g, sum_bound(to["t"], g, K))
    return out


def quiet(fn, *a, **kw):
    """Call fn with stdout swallowed (the reference prints on every step initialisation)."""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


# ---- the kernel tests' cases (shared by the CPU emulation that measures K_LSQ and the GPU test) --------------------------
KERNEL_SIZES = (1, 63, 257, 1025, 300000)  # the last: more than the 262 144 elements a capped grid covers in one trip
KERNEL_BITS = (2, 4, 8, 9)
STEP_FAMILIES = ("dyadic", "soft")


def planted(bit):
    """Code-unit values planted at the front of a case: ties (0.5, 1.5, 2.5 -> 0, 2, 2 and their negatives), exactly
    +-Qp (inside), one ulp beyond (outside), -0.0 (whose code and y are +0: round_pass adds c back)."""
    qp = float(qp_of(bit))
    up = float(np.nextafter(np.float32(qp), np.float32(np.inf)))
    return [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, qp, -qp, up, -up, -0.0]


def quant_case(n, bit, family, nan=False):
    """x, dy, step (fp32, CPU) of one flat quantiser problem. dyadic: step 2^-4, whose effective step is itself, so the
    planted code-unit values are exact; soft: step 0.0371. x spreads over +-1.5 Qp code units."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * bit + STEP_FAMILIES.index(family))
    step = torch.tensor(0.0625 if family == "dyadic" else 0.0371, dtype=torch.float32)
    se = effective_step(step, bit, n)
    x = torch.randn(n, generator=gen) * (0.6 * qp_of(bit)) * se
    dy = torch.randn(n, generator=gen)
    p = torch.tensor(planted(bit), dtype=torch.float32)[:n]
    x[:p.numel()] = p * se
    if nan:
        x[n // 2] = float("nan")
    return dict(x=x, dy=dy, step=step)


def emulate_ds(t, g, order="flat"):
    """The kernels' ds in fp32: S in their order, then one multiplication by g."""
    S = emulate_flat(t) if order == "flat" else emulate_items(t)
    return float(np.float32(S) * np.float32(g))


def ds64(t, g):
    return float(t.double().sum()) * float(np.float32(g))


# ---- the reference layers as modules (for whole-model comparisons) -------------------------------------------------------
class _RefMixin:
    def _setup(self, weight_bit, input_bit, output_bit, noise_scale, input_quant=True, output_quant=True,
               weight_quant=True):
        self.weight_bit, self.input_bit, self.output_bit, self.noise_scale = weight_bit, input_bit, output_bit, noise_scale
        self.input_quant, self.output_quant, self.weight_quant = input_quant, output_quant, weight_quant
        self.bf16_ops = False
        for k in ("input", "output", "weight"):
            setattr(self, f"step_size_{k}", torch.nn.Parameter(torch.tensor(1.0)))

    def _step(self, which, x):
        s = getattr(self, f"step_size_{which}")
        if s == 1:
            s.data = init_step(x.detach(), getattr(self, f"{which}_bit")).to(s.device)
        return s

    def forward(self, x):
        conv = isinstance(self, torch.nn.Conv2d)
        kind = "conv" if conv else "linear"
        geo = (0, 0, 0, self.stride[0], self.padding[0]) if conv else None
        xq = quant_lsq(x, self.input_bit, self._step("input", x)) if self.input_quant else x
        wq = quant_lsq(self.weight, self.weight_bit, self._step("weight", self.weight)) if self.weight_quant else self.weight
        if self.noise_scale != 0:
            wq = wq + (wq.max() - wq.min()) * self.noise_scale * torch.randn_like(wq)
        if self.bf16_ops:
            xq, wq = bf16r(xq), bf16r(wq)
        pre = matmul_of(kind, geo)(xq, wq, self.bias)
        if self.bf16_ops:
            pre = _RoundGrad.apply(pre)
        return quant_lsq(pre, self.output_bit, self._step("output", pre)) if self.output_quant else pre


class RefConv2d(_RefMixin, torch.nn.Conv2d):
    pass


class RefLinear(_RefMixin, torch.nn.Linear):
    pass


def convert_ref(model, **kw):
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
        new._setup(**kw)
        new.to(m.weight.device)
        new.weight = m.weight
        if m.bias is not None:
            new.bias = m.bias
        todo.append((name, new))
    for name, new in todo:
        parent = model.get_submodule(name.rsplit(".", 1)[0]) if "." in name else model
        setattr(parent, name.rsplit(".", 1)[-1], new)
    return [n for n, _ in todo]


def ds_out_operand_bound(pre, dy, s_out, e_pre, bit):
    """How far ds_out may move when every pre-activation moves by at most e_pre (same units as pre; e.g. a GEMM operand
    rounded to bf16: 2^-9 |x| |w| through the same conv / linear). m = q - v moves by at most the shift of v, by one
    more where v lies within the shift of a rounding tie (the code may flip), and by Qp more where |v| lies within the
    shift of Qp (the element may change sides of the clamp); an element that stays outside keeps m = +-Qp."""
    qp = qp_of(bit)
    se = effective_step(s_out.double(), bit, pre.numel())
    v, e = pre.double() / se, e_pre.double() / se
    tie = (v - torch.floor(v) - 0.5).abs() < e
    edge = (v.abs() - qp).abs() < e
    stays_out = v.abs() > qp + e
    dm = torch.where(stays_out, torch.zeros_like(e), e + tie.double() + qp * edge.double())
    return g_of(bit, pre.numel()) * float((dy.double().abs() * dm).sum())


def noise_step_grad_bounds(kind, geo, f, wbit, ns, eps, K=None):
    """(reference, bound) of ds_in and ds_w for a layer with input and weight quantisers, range noise (ns, eps) and NO
    output quantiser, against the float64 restatement on the same draw. What the HIP path rounds: d_pre = dy to bf16
    (2^-9 each) and the noisy weight operand fl(w_qn / se_w) to bf16 (2^-9 each; the input codes are exact). Pushed
    through absolute values:
      d w_qn   off by e_w = 2^-9 se_x (|dy|^T |codes_x|)
      noise    r = d w_qn + n S [max] / cnt_max - n S [min] / cnt_min, S = sum d w_qn eps: r off by e_w + n E ([max] /
               cnt_max + [min] / cnt_min), E = sum e_w |eps|
      ds_w     off by g_w sum (that) m_w, plus its summation term
      d x_q    = se_w (d_pre codes_w), both operands rounded: off by e_x = (2 2^-9 + 2^-18) (|dy| |w_qn|); ds_in off by
               g_x sum e_x m_x, plus its summation term
    with m = |q - v| inside and Qp outside."""
    d = torch.float64
    eps = eps.to(d)
    r = layer_grads(kind, geo, f, wbit, d, quant=(True, True, False), noise=(ns, eps))
    mm = matmul_of(kind, geo)
    x, w, s_in, s_w = f["x"].to(d), f["w"].to(d), f["s_in"].to(d), f["s_w"].to(d)
    cx, sex = codes_of(x, s_in, FEATURE_BIT)
    cw, sew = codes_of(w, s_w, wbit)
    ax, aw = cx.abs().requires_grad_(True), r["wq"].abs().requires_grad_(True)
    (mm(ax, aw, None) * f["dy"].to(d).abs()).sum().backward()
    e_w = BF16_REL * sex * aw.grad
    e_x = (2 * BF16_REL + BF16_REL ** 2) * ax.grad
    wq = (cw * sew).requires_grad_(True)
    ((wq + (wq.max() - wq.min()) * ns * eps) * r["d_wq"]).sum().backward()  # wq.grad: the gradient entering the quantiser
    at_max, at_min = (wq == wq.max()).to(d), (wq == wq.min()).to(d)
    dr = e_w + ns * float((e_w * eps.abs()).sum()) * (at_max / at_max.sum() + at_min / at_min.sum())
    out = {}
    for name, xx, ss, bit, e, up in (("ds_in", x, s_in, FEATURE_BIT, e_x, r["d_xq"]), ("ds_w", w, s_w, wbit, dr, wq.grad)):
        m = terms(xx, torch.ones_like(xx), ss, bit)["t"].abs()
        g = g_of(bit, xx.numel())
        out[name] = (float(r[name]), g * float((e * m).sum()) + sum_bound(terms(xx, up, ss, bit)["t"], g, K))
    return out, r
