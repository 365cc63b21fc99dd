"""The reference's ADC/DAC-aware compute-in-memory layers (cim_layers/layers_qn_lsq_adda_cim.py, layers_utils_adda.py)
on the HIP leaf path: the last stage (`LSQ_ADDA`) of its DiT training (Model_DiT_9L_train.py:576-623).

`Linear_lsq_adda_cim` / `Conv2d_lsq_adda_cim` (1x1) are the LSQ layers of sdmi.layers_qn_lsq with the product taken the
way the arrays take it: the input's integer codes are cut into L = ceil((input_bit - 1) / (dac_bit - 1)) sign-magnitude
slices, the weight's codes are mapped onto row blocks (`weight_mapping_info`, written by `map_weight`), and every
(row block, slice) partial sum passes an ADC -- scaled by `adc_scale`, noised, clamped to [-R-1, R] and rounded -- before
the sums are added. Kernels: csrc/adda.hip; arithmetic, launches and what is saved: DESIGN.md section 18.

Forward of one layer on cuda fp32 tensors:

    input   sdmi_adda_in_fwd: x -> the L slices of its codes, bf16, row blocks padded to the k tile
    weight  sdmi_lsq_quant_fwd: codes (fp32) [+ range noise in code space through sdmi_latent_range /
            sdmi_latent_noise_fwd], sdmi_adda_pack_w: bf16 [columns][padded rows]; with noise a bf16 high and low part
    gain    first use only: per mapping block, in the reference's order, while adc_gain still equals adc_gain_min: the
            block's plain products (the leaf GEMM, one per slice, two with noise), sdmi_adda_absmax, host reads
    scale   adc_gain -> adc_scale: 0-dim torch operations (clamp_pass, round_pass, a reciprocal in 'current' mode, one
            multiplication), 4 to 9 tiny launches; autograd carries the scale's gradient to adc_gain
    product sdmi_adda_gemm: pre, and the mask words and T when a backward will follow
    output  sdmi_lsq_out_fwd(have_pre=1): the output quantiser of pre

Backward: sdmi_lsq_out_bwd (d_pre, bf16), sdmi_adda_bwd_ops (the masked operands and the scale's gradient), per row block
one data-gradient and one weight-gradient GEMM of the leaf path (the slices are stacked along the GEMM's sum), then
sdmi_adda_in_bwd and sdmi_adda_unpack_wgrad / sdmi_latent_noise_bwd / sdmi_lsq_scale / sdmi_lsq_quant_bwd. No torch
matmul, linear, conv or unfold runs on the quantised path.

Differences from the reference. (1) Host reads: the steps as in sdmi.layers_qn_lsq; adc_gain is compared with
adc_gain_min on the host until it has been seen to differ (`gain_reads` counts the reads); `update_para`,
`load_state_dict` and `reset_step_cache()` forget that. (2) When the first-use gain is found at a later block than the
first (the earlier blocks' products were all zero), the reference has already pushed those blocks through the ADC at the
old scale; their partial sums are zero at any scale, so the result is the same. Should the first block's ideal gain
come out exactly equal to adc_gain_min, the reference initialises again at the next block and mixes two scales in one
forward; here the forward runs at the last scale. (3) Only the layer kinds the stage trains: input and weight quantisers
on (the output quantiser may be off), a convolution of kernel 1, stride 1, padding 0, groups 1, and a mapping whose row
blocks have one length (the last may be shorter) -- what `map_weight` writes. Anything else raises.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from . import leaf as LF
from . import layers_qn_lsq as LQ

_CPU_MSG = "layers_qn_lsq_adda_cim runs on the MI355X HIP path only (move the module and its input to cuda)"
NOISE_ENTRIES = 1000  # gen_adc_noise draws 1000 gain and 1000 offset values per layer


def clamp_pass(x, lo, hi):
    return (torch.clamp(x, lo, hi) - x).detach() + x


def round_pass(x):
    return (torch.round(x) - x).detach() + x


def get_adc_scale(module, adc_gain, mode="gain"):
    """layers_utils_adda.py:40-49."""
    g = clamp_pass(adc_gain, module.adc_gain_min, module.adc_gain_max)
    g = round_pass(g) if mode == "gain" else 1 / round_pass(1 / g)
    return g * module.adc_gain_1_scale


def gen_adc_noise(module):
    """layers_utils_adda.py:100-105, the global generator seeded as there (the reference's random sequence depends on it)."""
    torch.manual_seed(module.seed)
    dev = module.weight.device
    module.gain_noise = torch.randn(NOISE_ENTRIES, device=dev) * module.gain_noise_scale
    module.offset_noise = torch.randn(NOISE_ENTRIES, device=dev) * module.offset_noise_scale


def geometry(M, N, Kd, rb, input_bit, dac_bit):
    """sdmi_adda_geometry: dict of nb, rbp, L, Mp, Np, Kp."""
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.lib().sdmi_adda_geometry(M, N, Kd, rb, input_bit, dac_bit, out), "sdmi_adda_geometry")
    return dict(zip(("nb", "rbp", "L", "Mp", "Np", "Kp"), out))


def row_blocks(mapping, Kd, N):
    """The row-block length of a weight_mapping_info over a [Kd][N] weight, after checking that its blocks tile the
    weight: rows in blocks of one length (the last may be shorter), each row block's columns covered once."""
    rows = {}
    for info in mapping.values():
        rows.setdefault((info["start_row"], info["row_num"]), []).append((info["start_col"], info["col_num"]))
    starts = sorted(rows)
    rb = starts[0][1]
    for j, (r0, rn) in enumerate(starts):
        if r0 != j * rb or rn != min(rb, Kd - r0) or rn <= 0:
            raise NotImplementedError(f"layers_qn_lsq_adda_cim: row blocks {starts} of a {Kd}-row weight are not blocks "
                                      "of one length")
        c = 0
        for c0, cn in sorted(rows[(r0, rn)]):
            if c0 != c or cn <= 0:
                raise ValueError(f"layers_qn_lsq_adda_cim: the columns of row block {r0} do not tile 0 .. {N}")
            c += cn
        if c != N:
            raise ValueError(f"layers_qn_lsq_adda_cim: the columns of row block {r0} do not tile 0 .. {N}")
    if starts[-1][0] + starts[-1][1] != Kd:
        raise ValueError(f"layers_qn_lsq_adda_cim: the mapping covers {starts[-1][0] + starts[-1][1]} of {Kd} rows")
    return rb


class _Operands:
    """What the forward prepares before the ADC scale is final: the slices, the packed weight, the noise state."""
    __slots__ = ("xf", "w", "xs", "hi", "lo", "codes", "noise", "geo", "rb", "dims", "q_in", "q_w")


class _ADDALayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, weight, bias, s_in, s_w, s_out, adc_scale, ops):
        dev = x.device
        L = _lib.lib()
        st = K._stream()
        Bn, I, O, P, oshape = ops.dims
        g = ops.geo
        M, Op = Bn * P, LF._r8(O)
        need_bwd = any(ctx.needs_input_grad)
        a_s = adc_scale.detach().float().contiguous()
        adc_noise = mod.gain_noise_scale != 0 or mod.offset_noise_scale != 0
        pre = torch.empty(M, Op, dtype=torch.float32, device=dev)
        nwords = -(-g["nb"] * g["L"] // 32)
        mask = torch.empty(nwords, M, Op, dtype=torch.int32, device=dev) if need_bwd else None
        T = torch.empty(M, Op, dtype=torch.float32, device=dev) if need_bwd else None
        _lib.check(L.sdmi_adda_gemm(ops.xs.data_ptr(), ops.hi.data_ptr(), K._p(ops.lo), M, O, I, ops.rb, mod.input_bit,
                                    mod.dac_bit, mod.adc_bit, a_s.data_ptr(),
                                    mod.gain_noise.data_ptr() if adc_noise else None,
                                    mod.offset_noise.data_ptr() if adc_noise else None, ops.q_w[0].data_ptr(),
                                    ops.q_in[0].data_ptr(), K._p(bias), pre.data_ptr(), Op, K._p(mask), K._p(T), st),
                   "sdmi_adda_gemm")
        y = torch.empty(oshape, dtype=torch.float32, device=dev)
        q_out = None

        def out_stage(qp):
            _lib.check(L.sdmi_lsq_out_fwd(pre.data_ptr(), Op, Bn, O, P, None, 0.0, None, 0.0, None,
                                          q_out[0].data_ptr() if qp else None, q_out[1] if qp else 0.0, qp, 1,
                                          y.data_ptr(), st), "sdmi_lsq_out_fwd")
        if mod.output_quant:
            q_out = (LQ._step_ptr(s_out), LQ._g(LQ._qp(mod.output_bit), y.numel()), LQ._qp(mod.output_bit))
            if mod._step_unseen("output"):  # first use: the step is initialised on the pre-activation
                out_stage(0)
                mod._ensure_step("output", y)
            out_stage(q_out[2])
        else:
            out_stage(0)
        ctx.saved = (mod.input_bit, mod.dac_bit, ops, pre, mask, T, a_s, q_out, x.shape, bias, adc_scale.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        input_bit, dac_bit, ops, pre, mask, T, a_s, q_out, xshape, bias, as_shape = ctx.saved
        ctx.saved = None
        dev = dy.device
        L = _lib.lib()
        st = K._stream()
        Bn, I, O, P, _ = ops.dims
        g = ops.geo
        M, Op, nb, nL, Mp, Kp, rbp = Bn * P, LF._r8(O), g["nb"], g["L"], g["Mp"], g["Kp"], g["rbp"]
        q_in, q_w = ops.q_in, ops.q_w
        dyf = dy.float().contiguous()
        ds_out = None
        if q_out:
            dpre = torch.empty(M, Op, dtype=torch.bfloat16, device=dev)
            ds_out = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(L.sdmi_lsq_out_bwd(pre.data_ptr(), Op, dyf.data_ptr(), Bn, O, P, q_out[0].data_ptr(), q_out[1],
                                          q_out[2], dpre.data_ptr(), Op, LQ._ws(dev).data_ptr(), ds_out.data_ptr(), st),
                       "sdmi_lsq_out_bwd")
        else:
            dpre = LF._nhwc(dyf.reshape(Bn, O, P), Op)
        db = None
        if bias is not None:
            dbp = torch.empty(Op, dtype=torch.float32, device=dev)
            K.chan_sum(dpre, Bn, P, Op, per_c=dbp, c_store=O)
            db = dbp[:O]
        # the masked operands of the two products and the gradient of the ADC scale
        U = torch.empty(nb, M, Op, dtype=torch.bfloat16, device=dev)
        V = torch.empty(nb, nL * Mp, Op, dtype=torch.bfloat16, device=dev)
        dscale = torch.empty(3, dtype=torch.float32, device=dev)
        ws = torch.empty(L.sdmi_adda_workspace() // 4, dtype=torch.float32, device=dev)
        _lib.check(L.sdmi_adda_bwd_ops(dpre.data_ptr(), Op, pre.data_ptr(), Op, K._p(bias), T.data_ptr(), mask.data_ptr(),
                                       M, O, nb, nL, dac_bit - 1, a_s.data_ptr(), q_w[0].data_ptr(), q_in[0].data_ptr(),
                                       U.data_ptr(), V.data_ptr(), ws.data_ptr(), dscale.data_ptr(), st),
                   "sdmi_adda_bwd_ops")
        hi = ops.hi.view(g["Np"], Kp)
        xs = ops.xs.view(nL * Mp, Kp)
        # weight gradient in code space, one GEMM per row block over the stacked slices
        G2 = torch.empty(Op, Kp, dtype=torch.float32, device=dev)
        for j in range(nb):
            K.linear_wgrad(V[j], xs[:, j * rbp:(j + 1) * rbp], G2[:, j * rbp:(j + 1) * rbp])
        gw = torch.empty_like(ops.w)
        _lib.check(L.sdmi_adda_unpack_wgrad(G2.data_ptr(), O, I, ops.rb, a_s.data_ptr(), gw.data_ptr(), st),
                   "sdmi_adda_unpack_wgrad")
        if ops.noise is not None:  # through the noise in code space (the range is differentiable)
            eps, rws, ns = ops.noise
            n = ops.w.numel()
            gw = K.latent_noise_bwd(None, 0, None, gw, eps, ops.codes, 1, 1, n, ns, rws, K.latent_noise_ws(n, dev),
                                    torch.empty_like(gw))
        # x_q = q se / se.detach(): the plain quantiser's backward on the gradient divided by the step
        LQ.scale(gw, q_w[0], q_w[1], True, gw)
        dw = torch.empty_like(ops.w)
        ds_w = torch.empty((), dtype=torch.float32, device=dev)
        LQ.quant_bwd(ops.w, gw, q_w[0], q_w[2], q_w[1], dw, ds_w)
        # data gradient in code space, one GEMM per row block, then the input quantiser
        G1 = torch.empty(M, Kp, dtype=torch.float32, device=dev)
        for j in range(nb):
            K.linear_dgrad(U[j], hi[:Op, j * rbp:(j + 1) * rbp], G1[:, j * rbp:(j + 1) * rbp])
        dx = torch.empty(xshape, dtype=torch.float32, device=dev)
        ds_in = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(L.sdmi_adda_in_bwd(ops.xf.data_ptr(), G1.data_ptr(), Bn, I, P, ops.rb, q_in[0].data_ptr(), q_in[1],
                                      input_bit, dac_bit, a_s.data_ptr(), dx.data_ptr(), LQ._ws(dev).data_ptr(),
                                      ds_in.data_ptr(), st), "sdmi_adda_in_bwd")
        return None, dx, dw, db, ds_in, ds_w, ds_out, dscale[0].reshape(as_shape), None


class _ADDAMixin(LQ._QNMixin):
    """State and methods shared by the two layers (the reference repeats them in each class)."""

    def _init_adda(self, weight_bit, input_bit, output_bit, noise_scale, dac_bit, adc_bit, adc_gain_1_scale,
                   adc_gain_range, adc_adjust_mode, input_quant, output_quant, weight_quant, gain_noise_scale,
                   offset_noise_scale, seed):
        self._init_qn(weight_bit, input_bit, output_bit, noise_scale, input_quant, output_quant, weight_quant,
                      gain_noise_scale, offset_noise_scale)
        self.dac_bit = dac_bit
        self.adc_bit = adc_bit
        self.adc_gain_1_scale = adc_gain_1_scale
        self._set_slices()
        self.adc_gain_min = float(adc_gain_range[0])
        self.adc_gain_max = float(adc_gain_range[1])
        self.adc_gain = nn.Parameter(torch.tensor(self.adc_gain_min))
        self.adc_adjust_mode = adc_adjust_mode
        self.seed = seed
        self.gain_reads = 0
        gen_adc_noise(self)

    def _set_slices(self):
        self.slice_bit = self.dac_bit - 1
        self.bit_slices = int(math.ceil((self.input_bit - 1) / self.slice_bit))

    def reset_step_cache(self):
        """Forget which steps were seen != 1 and that adc_gain was seen != adc_gain_min."""
        super().reset_step_cache()
        self.__dict__["_gain_seen"] = False

    def refresh_adc_params(self):
        self.adc_range = 2 ** (self.adc_bit - 1) - 1
        self.adc_scale = get_adc_scale(self, self.adc_gain, mode=self.adc_adjust_mode)

    def update_para(self, use_FP=False, weight_bit=None, input_bit=None, output_bit=None, noise_scale=None, adc_bit=None,
                    dac_bit=None, gain_noise_scale=None, offset_noise_scale=None, seed=None):
        old = {k: getattr(self, f"{k}_bit") for k in ("weight", "input", "output", "adc", "dac")}
        self.use_FP = use_FP
        for k, v in (("weight_bit", weight_bit), ("input_bit", input_bit), ("output_bit", output_bit),
                     ("adc_bit", adc_bit), ("dac_bit", dac_bit), ("noise_scale", noise_scale),
                     ("gain_noise_scale", gain_noise_scale), ("offset_noise_scale", offset_noise_scale), ("seed", seed)):
            if v is not None:
                setattr(self, k, v)
        gen_adc_noise(self)
        # update_adc_gain (layers_utils_adda.py:52-73): the gain follows the three ranges, in double on the host
        gain = self.adc_gain.data.item()
        if old["adc"] != self.adc_bit:
            gain *= 2 ** (self.adc_bit - old["adc"])
        if old["dac"] != self.dac_bit:
            gain /= 2 ** (self.dac_bit - old["dac"])
        if old["weight"] != self.weight_bit:
            gain /= 2 ** (self.weight_bit - old["weight"])
        self.adc_gain.data = torch.clamp(torch.tensor(gain, device=self.adc_gain.device), min=0.8 * self.adc_gain_min,
                                         max=1.2 * self.adc_gain_max)
        for k in ("weight", "input", "output"):  # update_step_size (layers_utils_lsq.py:11-28)
            new = getattr(self, f"{k}_bit")
            if new != old[k]:
                getattr(self, f"step_size_{k}").data /= 2 ** (new - old[k])
        self._set_slices()
        self.reset_step_cache()

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _check(self):
        for k in ("input", "weight", "output"):
            LQ._qp(getattr(self, f"{k}_bit"))
        if not (self.input_quant and self.weight_quant):
            raise NotImplementedError("layers_qn_lsq_adda_cim: the arrays take integer codes; input_quant and "
                                      "weight_quant must be on")
        if not (isinstance(self.dac_bit, int) and 2 <= self.dac_bit <= 9 and isinstance(self.adc_bit, int)
                and 2 <= self.adc_bit <= 16):
            raise ValueError(f"layers_qn_lsq_adda_cim: dac_bit {self.dac_bit!r} outside 2 .. 9 or adc_bit "
                             f"{self.adc_bit!r} outside 2 .. 16")
        if self.adc_adjust_mode not in ("gain", "current"):
            raise ValueError(f"layers_qn_lsq_adda_cim: adc_adjust_mode {self.adc_adjust_mode!r}")
        if getattr(self, "weight_mapping_info", None) is None:
            raise RuntimeError("layers_qn_lsq_adda_cim: the layer has no weight_mapping_info; call map_weight(model, "
                               "weight_block_size) (or the reference's map_weight_for_model) before the first forward")
        O = self.weight.shape[0]
        if (self.gain_noise_scale != 0 or self.offset_noise_scale != 0) and O > NOISE_ENTRIES:
            raise ValueError(f"layers_qn_lsq_adda_cim: ADC noise has {NOISE_ENTRIES} entries per layer; {O} output "
                             "columns cannot be noised")

    def _prepare(self, x):
        """The slices and the packed weight codes (with this forward's noise draw)."""
        conv = isinstance(self, nn.Conv2d)
        L = _lib.lib()
        st = K._stream()
        ops = _Operands()
        xf = ops.xf = LQ._cuda_f32(x, "the input")
        w = ops.w = LQ._cuda_f32(self.weight, "the weight")
        dev = xf.device
        if conv:
            if xf.dim() != 4 or xf.shape[1] != w.shape[1]:
                raise ValueError(f"layers_qn_lsq_adda_cim: input {tuple(xf.shape)} for a weight {tuple(w.shape)}")
            B, I, H, W = xf.shape
            O = w.shape[0]
            Bn, P, oshape = B, H * W, (B, O, H, W)
        else:
            O, I = w.shape
            if xf.shape[-1] != I:
                raise ValueError(f"layers_qn_lsq_adda_cim: input {tuple(xf.shape)} for a weight {tuple(w.shape)}")
            Bn, P, oshape = xf.numel() // I, 1, (*xf.shape[:-1], O)
        ops.dims = (Bn, I, O, P, oshape)
        rb = ops.rb = row_blocks(self.weight_mapping_info, I, O)
        g = ops.geo = geometry(Bn * P, O, I, rb, self.input_bit, self.dac_bit)
        self._ensure_step("input", xf)
        ops.q_in = (LQ._step_ptr(self.step_size_input), LQ._g(LQ._qp(self.input_bit), xf.numel()), LQ._qp(self.input_bit))
        ops.xs = torch.empty(g["L"] * g["Mp"] * g["Kp"], dtype=torch.bfloat16, device=dev)
        _lib.check(L.sdmi_adda_in_fwd(xf.data_ptr(), Bn, I, P, ops.q_in[0].data_ptr(), ops.q_in[1], self.input_bit,
                                      self.dac_bit, rb, ops.xs.data_ptr(), st), "sdmi_adda_in_fwd")
        self._ensure_step("weight", w)
        n = w.numel()
        ops.q_w = (LQ._step_ptr(self.step_size_weight), LQ._g(LQ._qp(self.weight_bit), n), LQ._qp(self.weight_bit))
        # w_int = fl(fl(q se) / se), the reference's q * se / se.detach(): in fp32 not always the integer q, so the operand
        # is always packed as a bf16 high and low part
        ops.codes = torch.empty_like(w)
        LQ.quant_fwd(w, ops.q_w[0], ops.q_w[2], ops.q_w[1], y=ops.codes)
        LQ.scale(ops.codes, ops.q_w[0], ops.q_w[1], True, ops.codes)
        ns = float(self.noise_scale)
        src, ops.noise = ops.codes, None
        ops.hi = torch.empty(g["Np"] * g["Kp"], dtype=torch.bfloat16, device=dev)
        ops.lo = torch.empty_like(ops.hi)
        if ns != 0:
            eps = torch.randn_like(w)
            rws = K.latent_range(ops.codes, K.latent_noise_ws(n, dev))
            src = K.latent_noise_fwd(ops.codes, eps, 1, 1, n, ns, rws, torch.empty_like(w))
            ops.noise = (eps, rws, ns)
        _lib.check(L.sdmi_adda_pack_w(src.data_ptr(), O, I, rb, ops.hi.data_ptr(), K._p(ops.lo), st), "sdmi_adda_pack_w")
        return ops

    def _gain_is_min(self):
        self.gain_reads += 1
        return bool(self.adc_gain.detach() == self.adc_gain_min)

    def _first_use_gain(self, ops):
        """init_adc_gain (layers_utils_adda.py:12-20) at the first mapping block, in dictionary order, at which
        adc_gain still equals adc_gain_min."""
        if self.__dict__["_gain_seen"]:
            return
        Bn, I, O, P, _ = ops.dims
        g = ops.geo
        M, nL, rbp = Bn * P, g["L"], g["rbp"]
        dev = ops.xf.device
        xs = ops.xs.view(nL, g["Mp"], g["Kp"])
        R = 2 ** (self.adc_bit - 1) - 1
        for info in self.weight_mapping_info.values():
            if not self._gain_is_min():
                break
            j, c0, cn = info["start_row"] // ops.rb, info["start_col"], info["col_num"]
            prod = torch.zeros(nL, M, LF._r8(cn), dtype=torch.float32, device=dev)
            part = torch.zeros_like(prod) if ops.lo is not None else prod
            for i in range(nL):
                a = xs[i, :M, j * rbp:(j + 1) * rbp]
                K.linear(a, ops.hi.view(g["Np"], g["Kp"])[c0:c0 + cn, j * rbp:(j + 1) * rbp], part[i])
                if ops.lo is not None:  # the weight's low part, added to the high part's product
                    K.linear(a, ops.lo.view(g["Np"], g["Kp"])[c0:c0 + cn, j * rbp:(j + 1) * rbp], prod[i], resid=part[i])
            top = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().sdmi_adda_absmax(prod.data_ptr(), prod.numel(), LQ._ws(dev).data_ptr(), top.data_ptr(),
                                                   K._stream()), "sdmi_adda_absmax")
            self.gain_reads += 1
            if bool(top != 0):
                gain = torch.clamp(R / top / self.adc_gain_1_scale, min=0.8 * self.adc_gain_min,
                                   max=1.2 * self.adc_gain_max)
                self.adc_gain.data.copy_(gain)
        self.__dict__["_gain_seen"] = not self._gain_is_min()

    def _adda_forward(self, x):
        if not x.is_cuda or not self.weight.is_cuda:
            raise RuntimeError(_CPU_MSG)
        if self.use_FP:
            return LF.conv2d(self, x) if isinstance(self, nn.Conv2d) else LF.linear(self, x)
        self._check()
        _lib.lib()
        with torch.no_grad():
            ops = self._prepare(x)
            self._first_use_gain(ops)
        self.refresh_adc_params()
        return _ADDALayer.apply(self, x, self.weight, self.bias, self.step_size_input, self.step_size_weight,
                                self.step_size_output, self.adc_scale, ops)


def _only_1x1(kernel_size, stride, padding, groups):
    two = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)  # noqa: E731
    if (two(kernel_size), two(stride), groups) != ((1, 1), (1, 1), 1) or isinstance(padding, str) or two(padding) != (0, 0):
        raise NotImplementedError(f"Conv2d_lsq_adda_cim on the HIP path is the 1x1 convolution only (kernel_size 1, "
                                  f"stride 1, padding 0, groups 1); got kernel_size={kernel_size}, stride={stride}, "
                                  f"padding={padding}, groups={groups}")


class Conv2d_lsq_adda_cim(_ADDAMixin, nn.Conv2d):
    """cim_layers/layers_qn_lsq_adda_cim.py:25-291 on the HIP path (module docstring), 1x1 only."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, groups, weight_bit, input_bit, output_bit,
                 noise_scale, dac_bit, adc_bit, adc_gain_1_scale, adc_gain_range, adc_adjust_mode="gain",
                 input_quant=True, output_quant=True, weight_quant=True, gain_noise_scale=0, offset_noise_scale=0, seed=0,
                 bias=True):
        _only_1x1(kernel_size, stride, padding, groups)
        nn.Conv2d.__init__(self, in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                           stride=stride, padding=padding, groups=groups, bias=bias)
        self.shape_info = None
        self._init_adda(weight_bit, input_bit, output_bit, noise_scale, dac_bit, adc_bit, adc_gain_1_scale,
                        adc_gain_range, adc_adjust_mode, input_quant, output_quant, weight_quant, gain_noise_scale,
                        offset_noise_scale, seed)

    def forward(self, x):
        return self._adda_forward(x)


class Linear_lsq_adda_cim(_ADDAMixin, nn.Linear):
    """cim_layers/layers_qn_lsq_adda_cim.py:294-522 on the HIP path (module docstring); an N-D input as nn.Linear."""

    def __init__(self, in_features, out_features, weight_bit, input_bit, output_bit, noise_scale, dac_bit, adc_bit,
                 adc_gain_1_scale, adc_gain_range, adc_adjust_mode="gain", input_quant=True, output_quant=True,
                 weight_quant=True, gain_noise_scale=0, offset_noise_scale=0, seed=0, bias=True):
        nn.Linear.__init__(self, in_features, out_features, bias)
        self._init_adda(weight_bit, input_bit, output_bit, noise_scale, dac_bit, adc_bit, adc_gain_1_scale,
                        adc_gain_range, adc_adjust_mode, input_quant, output_quant, weight_quant, gain_noise_scale,
                        offset_noise_scale, seed)

    def forward(self, x):
        return self._adda_forward(x)


# ---- mapping, conversion, registration ---------------------------------------------------------------------------------
def split_dict(rows, cols, weight_block_size):
    """The mapping of one [rows][cols] weight onto blocks of weight_block_size = (max rows, max columns): keys
    "{row_block}_{col_block}", row blocks outermost (cim_weight_mapper/weight_process.py:10-40)."""
    max_rows, max_cols = int(weight_block_size[0]), int(weight_block_size[1])
    out = {}
    for rblk in range(-(-rows // max_rows)):
        for cblk in range(-(-cols // max_cols)):
            out[f"{rblk}_{cblk}"] = {"start_row": rblk * max_rows, "start_col": cblk * max_cols,
                                     "row_num": min(max_rows, rows - rblk * max_rows),
                                     "col_num": min(max_cols, cols - cblk * max_cols)}
    return out


def map_weight(model, weight_block_size, assign_layers=None, exclude_layers=None):
    """weight_mapping_info (and `name`) on every ADC layer of `model`, as the reference's map_weight_for_model writes
    them before its array packing; returns {layer name: mapping}."""
    if exclude_layers is not None and assign_layers is not None:
        raise ValueError("Either 'excluded_layers' or 'assign_layers' should be provided, but not both.")
    done = {}
    for name, m in model.named_modules():
        if not isinstance(m, (Conv2d_lsq_adda_cim, Linear_lsq_adda_cim)):
            continue
        if (exclude_layers is not None and name in exclude_layers) or (assign_layers is not None
                                                                       and name not in assign_layers):
            continue
        m.weight_mapping_info = split_dict(m.weight[0].numel(), m.weight.shape[0], weight_block_size)
        m.name = name
        done[name] = m.weight_mapping_info
    return done


def convert(model, *, exclude=None, assign=None, **kw):
    """ProgressiveTrain.convert_to_layers(tar_layer_type='layers_qn_lsq_adda_cim') (progressive_qn_train.py:576-651):
    every nn.Conv2d / nn.Linear or LSQ layer of `model` (not in `exclude`; only those in `assign` when given) becomes an
    ADC layer holding the same weight / bias Parameter objects; the steps are copied from a layer that has them
    (copy_lsq_data). kw: the layers' constructor arguments. Returns the names of the replaced layers."""
    if exclude is not None and assign is not None:
        raise ValueError("Either 'exclude' or 'assign' should be provided, but not both.")
    todo = []
    for name, m in model.named_modules():
        if (exclude and name in exclude) or (assign and name not in assign):
            continue
        if type(m) in (nn.Conv2d, LQ.Conv2d_qn_lsq):
            new = Conv2d_lsq_adda_cim(in_channels=m.in_channels, out_channels=m.out_channels, kernel_size=m.kernel_size,
                                      stride=m.stride, padding=m.padding, groups=m.groups, bias=m.bias is not None, **kw)
        elif type(m) in (nn.Linear, LQ.Linear_qn_lsq):
            new = Linear_lsq_adda_cim(in_features=m.in_features, out_features=m.out_features, bias=m.bias is not None,
                                      **kw)
        else:
            continue
        new.weight = m.weight
        if m.bias is not None:
            new.bias = m.bias
        for attr in ("name", "layer_flag"):
            if hasattr(m, attr):
                setattr(new, attr, getattr(m, attr))
        dev = m.weight.device
        for k in ("input", "weight", "output"):
            p = getattr(new, f"step_size_{k}")
            p.data = getattr(m, f"step_size_{k}").data if hasattr(m, f"step_size_{k}") else p.data.to(dev)
        new.adc_gain.data = new.adc_gain.data.to(dev)
        new.gain_noise, new.offset_noise = new.gain_noise.to(dev), new.offset_noise.to(dev)
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
    convert_to_layers(tar_layer_type='layers_qn_lsq_adda_cim') picks them (it takes the first class whose module path
    holds the name) and its type checks (adda_layers, cim_layers, custom_layers, op_layers) know them."""
    conv, lin = (Conv2d_lsq_adda_cim,), (Linear_lsq_adda_cim,)
    for name, add in (("conv_layers", conv), ("adda_conv_layers", conv), ("cim_conv_layers", conv),
                      ("custom_conv_layers", conv), ("linear_layers", lin), ("adda_linear_layers", lin),
                      ("cim_linear_layers", lin), ("custom_linear_layers", lin), ("adda_layers", conv + lin),
                      ("cim_layers", lin + conv), ("custom_layers", lin + conv), ("op_layers", lin + conv)):
        cur = getattr(reg_dict, name, None)
        if cur is not None:
            setattr(reg_dict, name, add + tuple(c for c in cur if c not in add))
    return reg_dict
