"""The reference's LSQ quantise-and-noise layers (cim_layers/layers_qn_lsq.py, layers_utils_lsq.py) on the HIP leaf path.

`Conv2d_qn_lsq` / `Linear_qn_lsq` carry learned-step-size quantisers on input, weight and output and range noise on the
quantised weight. ProgressiveTrain.convert_to_layers('layers_qn_lsq') (cim_qn_train/progressive_qn_train.py:576-651)
swaps them in for every nn.Conv2d / nn.Linear; `convert` below does the same without the reference's trainer and
`register` makes the reference's own call pick these classes. sdmi.leaf.call runs a swapped layer through its own
forward, so a converted model runs on the leaf path as it stands.

Forward of one layer on cuda fp32 tensors (kernels: csrc/lsq.hip, arithmetic: DESIGN.md section 17):

    input   sdmi_lsq_in_fwd: x -> integer codes q_x, NHWC bf16 (exact for bit widths <= 9)
    weight  sdmi_lsq_quant_fwd: w -> codes q_w (fp32, a per-module buffer) [+ range noise on w_q = q_w se_w through
            sdmi_latent_range / sdmi_latent_noise_fwd, then codes = w_qn / se_w], packed to bf16 by the leaf PackPlan
    GEMM    the implicit-GEMM conv / linear over the codes, fp32 accumulator: without noise an exact integer dot product
    output  sdmi_lsq_out_fwd: pre = acc (se_x se_w) + bias, the output quantiser, NCHW fp32

and the backward runs the same GEMMs' data / weight gradients on d_pre (bf16, the one approximation left) with the
quantisers' backward kernels around them. No torch elementwise op sits on the quantised path.

Difference from the reference. It reads each step on the host in every forward (`if module.step_size_input == 1`,
layers_utils_lsq.py:40, 57, 74) to initialise it on first use. Here a quantiser's step is read until it has been seen
!= 1 and then never again; `update_para`, `load_state_dict` and `reset_step_cache()` forget that. A step that is set back
to exactly 1.0 by other means is therefore not re-initialised until one of those is called. `step_reads` counts the reads.

One more limit: the packed weight codes live in one buffer per module. A backward whose forward was followed by another
forward of the same module with other codes (noise_scale != 0, or the weight written in between) raises a RuntimeError
rather than run its data gradient on the later codes. The reference's models call each layer once per forward.
"""
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from . import leaf as LF

_CPU_MSG = "layers_qn_lsq runs on the MI355X HIP path only (move the module and its input to cuda)"


def _qp(bit):
    if not isinstance(bit, int) or not 2 <= bit <= 9:
        raise ValueError(f"layers_qn_lsq: bit width {bit!r} outside 2 .. 9")
    return 2 ** (bit - 1) - 1


def _g(qp, numel):
    """grad_scale_factor (quant_noise_utils.py:57-58) in double; the kernels take it rounded to fp32."""
    return 1.0 / ((qp * numel) ** 0.5)


def _ws(device):
    return torch.empty(_lib.lib().sdmi_lsq_workspace() // 4, dtype=torch.float32, device=device)


def _cuda_f32(t, what):
    if not t.is_cuda:
        raise RuntimeError(_CPU_MSG)
    if t.dtype != torch.float32:
        raise TypeError(f"layers_qn_lsq: {what} must be fp32, got {t.dtype}")
    return t.detach().contiguous()


def _step_ptr(step):
    s = step.detach()
    if not s.is_cuda:
        raise RuntimeError(_CPU_MSG)
    if s.numel() != 1 or s.dtype != torch.float32:
        raise TypeError("layers_qn_lsq: a step size is one fp32 element")
    return s


# ---- thin wrappers over the C ABI -----------------------------------------------------------------------------------
def quant_fwd(x, step, qp, g, y=None, codes=None):
    _lib.check(_lib.lib().sdmi_lsq_quant_fwd(x.data_ptr(), x.numel(), step.data_ptr(), g, qp, K._p(y), K._p(codes),
                                             K._stream()), "sdmi_lsq_quant_fwd")


def quant_bwd(x, dy, step, qp, g, dx, ds, scale=None, scale_g=0.0):
    _lib.check(_lib.lib().sdmi_lsq_quant_bwd(x.data_ptr(), dy.data_ptr(), x.numel(), step.data_ptr(), g, qp,
                                             K._p(scale), scale_g, dx.data_ptr(), _ws(x.device).data_ptr(),
                                             ds.data_ptr(), K._stream()), "sdmi_lsq_quant_bwd")


def scale(x, step, g, divide, out):
    _lib.check(_lib.lib().sdmi_lsq_scale(x.data_ptr(), x.numel(), step.data_ptr(), g, 1 if divide else 0,
                                         out.data_ptr(), K._stream()), "sdmi_lsq_scale")
    return out


def init_step(x, qp, step):
    """step[0] = 1 / ((1 / max|x|) * Qp) on the device; untouched when max|x| == 0."""
    _lib.check(_lib.lib().sdmi_lsq_init_step(x.data_ptr(), x.numel(), qp, _ws(x.device).data_ptr(), step.data_ptr(),
                                             K._stream()), "sdmi_lsq_init_step")


# ---- the exported functions of quant_noise_utils.py / layers_utils_lsq.py --------------------------------------------
class _Quant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, step, bit):
        qp = _qp(bit)
        xf = _cuda_f32(x, "the quantised tensor")
        s = _step_ptr(step)
        g = _g(qp, xf.numel())
        y = torch.empty_like(xf)
        if xf.numel():
            quant_fwd(xf, s, qp, g, y=y)
        ctx.saved = (xf, s, qp, g, step.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        xf, s, qp, g, sshape = ctx.saved
        dx = torch.empty_like(xf)
        ds = torch.zeros((), dtype=torch.float32, device=xf.device)
        if xf.numel():
            quant_bwd(xf, dy.float().contiguous(), s, qp, g, dx, ds)
        return dx, ds.reshape(sshape), None


def data_quant_lsq(data_float, data_bit, step_size, isint=False):
    """quant_noise_utils.py:101-120 for cuda fp32 tensors: (quantised tensor, 1.0), differentiable in the data and
    the step."""
    if isint:
        raise NotImplementedError("layers_qn_lsq: isint=True is not on the HIP path")
    _qp(data_bit)
    if not data_float.is_cuda:
        raise RuntimeError(_CPU_MSG)
    _lib.lib()
    return _Quant.apply(data_float, step_size, data_bit), 1.0


weight_quant_lsq = data_quant_lsq  # the reference's two functions are the same expression (quant_noise_utils.py:160)


def init_step_size(x, data_bit):
    """layers_utils_lsq.py:31-34: the 0-dim step 1 / ((1 / max|x|) * Qp), 1.0 for an all-zero x. No host read."""
    qp = _qp(data_bit)
    xf = _cuda_f32(x, "the tensor")
    step = torch.ones((), dtype=torch.float32, device=xf.device)
    if xf.numel():
        init_step(xf, qp, step)
    return step


from models.vqvae_noise import add_noise  # noqa: E402  (re-exported: quant_noise_utils.add_noise on the HIP path)


def weight_quant_noise(module, isint=False):
    """layers_utils_lsq.py:53-68: (w_qn, 1.0) of a layer, differentiable in its weight and step_size_weight; one
    randn_like(weight) draw from the device generator when noise_scale != 0, none otherwise."""
    if isint:
        raise NotImplementedError("layers_qn_lsq: isint=True is not on the HIP path")
    w_q = module.weight
    if not w_q.is_cuda:
        raise RuntimeError(_CPU_MSG)
    if module.weight_quant:
        module._ensure_step("weight", w_q.detach())
        w_q, _ = weight_quant_lsq(module.weight, module.weight_bit, module.step_size_weight)
    return add_noise(w_q, n_scale=module.noise_scale), 1.0


# ---- one layer: autograd Function over the kernels and the leaf path's GEMMs -----------------------------------------
class _PackSrc:
    """What leaf._pack_conv / _pack_linear read of a module, with the code buffer as the weight."""
    weight = stride = None


def _pack(mod, src, conv):
    ps = mod.__dict__.get("_pack_src")
    if ps is None:
        ps = _PackSrc()
        ps.stride = mod.stride if conv else None
        mod.__dict__["_pack_src"] = ps
    ps.weight = src
    LF.invalidate_pack(ps)  # the kernels rewrite the buffer in place: always repack
    return LF._pack_conv(ps) if conv else LF._pack_linear(ps)


class _QNLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, weight, bias, s_in, s_w, s_out):
        conv = isinstance(mod, nn.Conv2d)
        dev = x.device
        xf = _cuda_f32(x, "the input")
        w = _cuda_f32(weight, "the weight")
        if conv:
            B, I, H, W = xf.shape
            O, _, KH, KW = w.shape
            s, p = mod.stride[0], mod.padding[0]
            OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
            Bn, Pin, Pout = B, H * W, OH * OW
            oshape = (B, O, OH, OW)
        else:
            O, I = w.shape
            Bn, Pin, Pout = xf.numel() // I, 1, 1
            oshape = (*xf.shape[:-1], O)
        Ip, Op = LF._r8(I), LF._r8(O)
        L = _lib.lib()
        st = K._stream()
        # input: integer codes, NHWC bf16
        q_in = None
        if mod.input_quant:
            mod._ensure_step("input", xf)
            q_in = (_step_ptr(s_in), _g(_qp(mod.input_bit), xf.numel()), _qp(mod.input_bit))
            xin = torch.empty(Bn * Pin, Ip, dtype=torch.bfloat16, device=dev)
            _lib.check(L.sdmi_lsq_in_fwd(xf.data_ptr(), Bn, I, Pin, q_in[0].data_ptr(), q_in[1], q_in[2],
                                         xin.data_ptr(), Ip, st), "sdmi_lsq_in_fwd")
        else:
            xin = LF._nhwc(xf.reshape(Bn, I, Pin), Ip)
        # weight: codes (+ noise) into the module's buffer, packed like a plain leaf weight
        q_w, noise = None, None
        ns = float(mod.noise_scale)
        n = w.numel()
        src = w
        if mod.weight_quant:
            mod._ensure_step("weight", w)
            q_w = (_step_ptr(s_w), _g(_qp(mod.weight_bit), n), _qp(mod.weight_bit))
            src = mod._code_buffer(w)
            if ns == 0:
                quant_fwd(w, q_w[0], q_w[2], q_w[1], codes=src)
            else:
                w_q = torch.empty_like(w)
                quant_fwd(w, q_w[0], q_w[2], q_w[1], y=w_q)
        else:
            w_q = w
        if ns != 0:
            eps = torch.randn_like(w)
            rws = K.latent_range(w_q, K.latent_noise_ws(n, dev))
            if mod.weight_quant:
                w_qn = K.latent_noise_fwd(w_q, eps, 1, 1, n, ns, rws, torch.empty_like(w))
                scale(w_qn, q_w[0], q_w[1], True, src)
            else:
                src = K.latent_noise_fwd(w_q, eps, 1, 1, n, ns, rws, mod._code_buffer(w))
            noise = (w_q, eps, rws, ns)
        pk = _pack(mod, src, conv)
        # the packed codes live once per module: a backward whose forward was not the module's last is only right
        # when the later forwards packed the same codes (no noise, the weight not written in between)
        serial = mod.__dict__.get("_fwd_serial", 0) + 1
        mod.__dict__["_fwd_serial"] = serial
        wver = (weight._version, s_w._version, mod.weight_bit, mod.weight_quant)
        if ns != 0 or wver != mod.__dict__.get("_fwd_wver"):
            mod.__dict__["_codes_serial"] = serial
        mod.__dict__["_fwd_wver"] = wver
        ctx.codes_serial = mod.__dict__["_codes_serial"]
        # GEMM over the codes, fp32 accumulator, no bias
        acc = torch.empty(Bn * Pout, Op, dtype=torch.float32, device=dev)
        if conv:
            K.conv_fwd(xin, B, H, W, Ip, Ip, pk.view("f"), Op, KH, KW, s, p, acc, Op, n_store=O)
        else:
            K.linear(xin, pk.view("f"), acc, n_store=O)
        # output stage: pre in place of acc, y in the caller's layout
        y = torch.empty(oshape, dtype=torch.float32, device=dev)
        q_out = None

        def out_stage(qp, have_pre):
            _lib.check(L.sdmi_lsq_out_fwd(acc.data_ptr(), Op, Bn, O, Pout, q_in[0].data_ptr() if q_in else None,
                                          q_in[1] if q_in else 0.0, q_w[0].data_ptr() if q_w else None,
                                          q_w[1] if q_w else 0.0, K._p(bias), q_out[0].data_ptr() if qp else None,
                                          q_out[1] if qp else 0.0, qp, have_pre, y.data_ptr(), st), "sdmi_lsq_out_fwd")
        if mod.output_quant:
            q_out = (_step_ptr(s_out), _g(_qp(mod.output_bit), y.numel()), _qp(mod.output_bit))
            have_pre = 0
            if mod._step_unseen("output"):  # first use: the step is initialised on the pre-activation
                out_stage(0, 0)
                mod._ensure_step("output", y)
                have_pre = 1
            out_stage(q_out[2], have_pre)
        else:
            out_stage(0, 0)
        ctx.saved = (mod, conv, xf if mod.input_quant else None, w, xin, acc, pk, noise, q_in, q_w, q_out,
                     (Bn, I, O, Pin, Pout), (B, H, W, KH, KW, s, p, OH, OW) if conv else None, x.shape, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mod, conv, xf, w, xin, pre, pk, noise, q_in, q_w, q_out, (Bn, I, O, Pin, Pout), geo, xshape,
         has_bias) = ctx.saved
        ctx.saved = None
        if ctx.codes_serial != mod.__dict__.get("_codes_serial"):
            raise RuntimeError("layers_qn_lsq: the layer ran forward again with other weight codes (noise, or a written "
                               "weight) before this backward; its packed codes are gone")
        dev = dy.device
        L = _lib.lib()
        st = K._stream()
        Ip, Op = LF._r8(I), LF._r8(O)
        dyf = dy.float().contiguous()
        ds_in = ds_w = ds_out = None
        # output quantiser: d_pre as the GEMMs' NHWC bf16 operand
        if q_out:
            dpre = torch.empty(Bn * Pout, Op, dtype=torch.bfloat16, device=dev)
            ds_out = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(L.sdmi_lsq_out_bwd(pre.data_ptr(), Op, dyf.data_ptr(), Bn, O, Pout, q_out[0].data_ptr(), q_out[1],
                                          q_out[2], dpre.data_ptr(), Op, _ws(dev).data_ptr(), ds_out.data_ptr(), st),
                       "sdmi_lsq_out_bwd")
        else:
            dpre = LF._nhwc(dyf.reshape(Bn, O, Pout), Op)
        # weight gradient in code space (and the bias gradient in the same launch)
        db = torch.empty(O, dtype=torch.float32, device=dev) if has_bias else None
        if conv:
            B, H, W, KH, KW, s, p, OH, OW = geo
            G2 = torch.empty_like(w)
            K.conv_wgrad(dpre, Op, xin, B, H, W, Ip, Ip, Op, KH, KW, s, p, G2, OH, OW, cvalid=I, m_store=O,
                         bias_grad=db)
        elif I == Ip:
            G2 = torch.empty_like(w)
            K.linear_wgrad(dpre, xin, G2, bias_grad=db, m_store=O)
        else:
            G2p = torch.empty(O, Ip, dtype=torch.float32, device=dev)
            K.linear_wgrad(dpre, xin, G2p, bias_grad=db, m_store=O)
            G2 = LF._unrows(G2p, Ip, O, I)
        sc_in = (q_in[0], q_in[1]) if q_in else (None, 0.0)
        if noise is not None:  # d w_qn = se_x G2, through the noise (the range is differentiable), then the quantiser
            w_q, eps, rws, ns = noise
            gw = scale(G2, q_in[0], q_in[1], False, torch.empty_like(G2)) if q_in else G2
            n = w.numel()
            gw = K.latent_noise_bwd(None, 0, None, gw, eps, w_q, 1, 1, n, ns, rws, K.latent_noise_ws(n, dev),
                                    torch.empty_like(G2))
            sc_in = (None, 0.0)
        else:
            gw = G2
        if q_w:
            dw = torch.empty_like(w)
            ds_w = torch.empty((), dtype=torch.float32, device=dev)
            quant_bwd(w, gw, q_w[0], q_w[2], q_w[1], dw, ds_w, scale=sc_in[0], scale_g=sc_in[1])
        elif sc_in[0] is not None:
            dw = scale(gw, sc_in[0], sc_in[1], False, torch.empty_like(gw))
        else:
            dw = gw
        # data gradient in code space, then the input quantiser
        dx = None
        if ctx.needs_input_grad[1] or (q_in and ctx.needs_input_grad[4]):
            G1 = torch.empty(Bn * Pin, Ip, dtype=torch.float32, device=dev)
            if not conv:
                K.linear_dgrad(dpre, pk.view("f"), G1)
            elif s == 1:
                K.conv_fwd(dpre, B, OH, OW, Op, Op, pk.view("d"), Ip, KH, KW, 1, KH - 1 - p, G1, Ip)
            else:
                K.conv_dgrad_phases(dpre, B, H, W, Op, Op, [pk.view(f"d{a}{b}") for a in range(2) for b in range(2)],
                                    Ip, G1, Ip)
            if q_in:
                dx = torch.empty(xshape, dtype=torch.float32, device=dev)
                ds_in = torch.empty((), dtype=torch.float32, device=dev)
                _lib.check(L.sdmi_lsq_in_bwd(xf.data_ptr(), G1.data_ptr(), Ip, Bn, I, Pin, q_in[0].data_ptr(), q_in[1],
                                             q_in[2], q_w[0].data_ptr() if q_w else None, q_w[1] if q_w else 0.0,
                                             dx.data_ptr(), _ws(dev).data_ptr(), ds_in.data_ptr(), st),
                           "sdmi_lsq_in_bwd")
            else:
                dx = LF._nchw(G1, Ip, (Bn, I, Pin)).reshape(xshape)
                if q_w:
                    scale(dx, q_w[0], q_w[1], False, dx)
        return None, dx, dw, db, ds_in, ds_w, ds_out


_STEPS = ("input", "weight", "output")


class _QNMixin:
    """State and methods shared by the two layers (the reference repeats them in each class)."""

    def _init_qn(self, weight_bit, input_bit, output_bit, noise_scale, input_quant, output_quant, weight_quant,
                 gain_noise_scale, offset_noise_scale):
        self.use_FP = False
        self.weight_bit = weight_bit
        self.input_bit = input_bit
        self.output_bit = output_bit
        self.noise_scale = noise_scale
        self.gain_noise_scale = gain_noise_scale  # stored and unused, as in the reference's forward
        self.offset_noise_scale = offset_noise_scale
        self.input_quant = input_quant
        self.output_quant = output_quant
        self.weight_quant = weight_quant
        self.step_size_input = nn.Parameter(torch.tensor(1.0))
        self.step_size_output = nn.Parameter(torch.tensor(1.0))
        self.step_size_weight = nn.Parameter(torch.tensor(1.0))
        self.step_reads = 0
        self.reset_step_cache()

    def reset_step_cache(self):
        """Forget which steps were seen != 1: the next forward reads them on the host again."""
        self.__dict__["_step_seen"] = {k: False for k in _STEPS}

    def _step_unseen(self, which):
        return not self.__dict__["_step_seen"][which]

    def _ensure_step(self, which, x):
        """The reference's `if step == 1: step.data = init_step_size(x, bit)` until the step was seen != 1."""
        seen = self.__dict__["_step_seen"]
        if seen[which]:
            return
        step = getattr(self, f"step_size_{which}")
        self.step_reads += 1
        if float(step.detach()) == 1:
            if x.numel():
                init_step(x, _qp(getattr(self, f"{which}_bit")), step.detach())
            self.step_reads += 1
            seen[which] = float(step.detach()) != 1
        else:
            seen[which] = True

    def _code_buffer(self, w):
        buf = self.__dict__.get("_codes")
        if buf is None or buf.shape != w.shape or buf.device != w.device:
            buf = torch.empty_like(w)
            self.__dict__["_codes"] = buf
        return buf

    def update_para(self, use_FP=False, weight_bit=None, input_bit=None, output_bit=None, noise_scale=None,
                    gain_noise_scale=0, offset_noise_scale=0):
        old = {k: getattr(self, f"{k}_bit") for k in _STEPS}
        self.use_FP = use_FP
        if weight_bit is not None:
            self.weight_bit = weight_bit
        if input_bit is not None:
            self.input_bit = input_bit
        if output_bit is not None:
            self.output_bit = output_bit
        if noise_scale is not None:
            self.noise_scale = noise_scale
        if gain_noise_scale is not None:
            self.gain_noise_scale = gain_noise_scale
        if offset_noise_scale is not None:
            self.offset_noise_scale = offset_noise_scale
        for k in ("weight", "input", "output"):  # update_step_size (layers_utils_lsq.py:11-28)
            new = getattr(self, f"{k}_bit")
            if new != old[k]:
                getattr(self, f"step_size_{k}").data /= 2 ** (new - old[k])
        self.reset_step_cache()

    def _load_from_state_dict(self, *args, **kwargs):
        self.reset_step_cache()
        return super()._load_from_state_dict(*args, **kwargs)

    def _qn_forward(self, x):
        if not x.is_cuda or not self.weight.is_cuda:
            raise RuntimeError(_CPU_MSG)
        if self.use_FP:
            return LF.conv2d(self, x) if isinstance(self, nn.Conv2d) else LF.linear(self, x)
        for k in _STEPS:
            if getattr(self, f"{k}_quant"):
                _qp(getattr(self, f"{k}_bit"))
        if isinstance(self, nn.Conv2d):
            LF.check_conv_geometry(self, x)
        _lib.lib()
        return _QNLayer.apply(self, x, self.weight, self.bias, self.step_size_input, self.step_size_weight,
                              self.step_size_output)


class Conv2d_qn_lsq(_QNMixin, nn.Conv2d):
    """cim_layers/layers_qn_lsq.py:17-121 on the HIP leaf path (module docstring); geometries of sdmi.leaf.conv2d."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, groups, weight_bit, input_bit,
                 output_bit, noise_scale, input_quant=True, output_quant=True, weight_quant=True, gain_noise_scale=0,
                 offset_noise_scale=0, bias=True):
        nn.Conv2d.__init__(self, in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                           stride=stride, padding=padding, groups=groups, bias=bias)
        self._init_qn(weight_bit, input_bit, output_bit, noise_scale, input_quant, output_quant, weight_quant,
                      gain_noise_scale, offset_noise_scale)

    def forward(self, x):
        return self._qn_forward(x)


class Linear_qn_lsq(_QNMixin, nn.Linear):
    """cim_layers/layers_qn_lsq.py:126-216 on the HIP leaf path (module docstring)."""

    def __init__(self, in_features, out_features, weight_bit, input_bit, output_bit, noise_scale, input_quant=True,
                 output_quant=True, weight_quant=True, gain_noise_scale=0, offset_noise_scale=0, bias=False):
        nn.Linear.__init__(self, in_features, out_features, bias)
        self._init_qn(weight_bit, input_bit, output_bit, noise_scale, input_quant, output_quant, weight_quant,
                      gain_noise_scale, offset_noise_scale)

    def forward(self, x):
        return self._qn_forward(x)


# ---- conversion ------------------------------------------------------------------------------------------------------
def convert(model, *, weight_bit, input_bit, output_bit, noise_scale, exclude=None, assign=None, **flags):
    """ProgressiveTrain.convert_to_layers(tar_layer_type='layers_qn_lsq') (progressive_qn_train.py:608-650): every
    exact nn.Conv2d / nn.Linear of `model` (not in `exclude`; only those in `assign` when given) becomes a
    Conv2d_qn_lsq / Linear_qn_lsq holding the same weight / bias Parameter objects; step sizes are copied from a layer
    that has them. Returns the names of the replaced layers."""
    if exclude is not None and assign is not None:
        raise ValueError("Either 'exclude' or 'assign' should be provided, but not both.")
    kw = dict(weight_bit=weight_bit, input_bit=input_bit, output_bit=output_bit, noise_scale=noise_scale, **flags)
    todo = []
    for name, m in model.named_modules():
        if (exclude and name in exclude) or (assign and name not in assign):
            continue
        if type(m) is nn.Conv2d:
            new = Conv2d_qn_lsq(in_channels=m.in_channels, out_channels=m.out_channels, kernel_size=m.kernel_size,
                                stride=m.stride, padding=m.padding, groups=m.groups, bias=m.bias is not None, **kw)
        elif type(m) is nn.Linear:
            new = Linear_qn_lsq(in_features=m.in_features, out_features=m.out_features, bias=m.bias is not None, **kw)
        else:
            continue
        new.weight = m.weight
        if m.bias is not None:
            new.bias = m.bias
        for attr in ("name", "layer_flag"):
            if hasattr(m, attr):
                setattr(new, attr, getattr(m, attr))
        for k in _STEPS:
            if hasattr(m, f"step_size_{k}"):
                getattr(new, f"step_size_{k}").data = getattr(m, f"step_size_{k}").data
            else:
                p = getattr(new, f"step_size_{k}")
                p.data = p.data.to(m.weight.device)
        new.train(m.training)
        todo.append((name, new))
    for name, new in todo:
        parent = model
        *path, leaf_name = name.split(".")
        for part in path:
            parent = getattr(parent, part)
        setattr(parent, leaf_name, new)
    return [name for name, _ in todo]


def register(reg_dict):
    """Prepend the two classes to the reference's cim_layers.register_dict tuples, so that its own
    convert_to_layers(tar_layer_type='layers_qn_lsq') picks them (it takes the first class whose module path holds
    the name) and its type checks (qn_layers, custom_layers, op_layers) know them."""
    conv, lin = (Conv2d_qn_lsq,), (Linear_qn_lsq,)
    for name, add in (("conv_layers", conv), ("qn_conv_layers", conv), ("custom_conv_layers", conv),
                      ("linear_layers", lin), ("qn_linear_layers", lin), ("custom_linear_layers", lin),
                      ("qn_layers", lin + conv), ("custom_layers", lin + conv), ("op_layers", lin + conv)):
        cur = getattr(reg_dict, name, None)
        if cur is not None:
            setattr(reg_dict, name, add + tuple(c for c in cur if c not in add))
    return reg_dict
