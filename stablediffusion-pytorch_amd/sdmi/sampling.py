"""Captured sampling loops: the reference's samplers -- T x [model(x_t, t) -> LinearNoiseScheduler.sample_prev_timestep]
(tools/sample_ddpm_vqvae.py:29-52, tools/sample_ddpm_text_image_cond.py) and DDIMSampler.forward's
`steps` x [model(x_t, t, cond) -> DDIM update] (scheduler/linear_noise_scheduler.py:209-256) -- captured ONCE (as
one hipGraph per reverse step, default, or as sdmi.plan's native launch list: SDMI_SAMPLE_ISSUE=plan) and replayed
per step with no host work.

Everything a step needs lives on the device: the model's timestep is an int64 device scalar read by the
time-embedding kernel; the DDPM step kernel (sdmi_ddpm_prev) decrements it after the step, the DDIM step kernel
(sdmi_ddim_prev_dev) reads its (t, t_prev) pair from device tables through a device step index and moves both down;
the noise comes from the Philox kernel (sdmi_randn) keyed by (seed, device draw counter) that advances per replay;
x_t is updated in place. The reference instead builds t on the host, draws the noise with the host generator (DDPM:
on the CPU, scheduler :72) and syncs on `t == 0` every step.

A model that does not run on the fused engine (a swapped leaf, SURVEY.md §8(b), or sdmi_leaf_path = True) is
sampled stepwise through its own forward (`model(x, t, cond)`), with the same step kernels and noise.

Classifier-free guidance (every sampler of the reference: tools/sample_ddpm_text_cond.py:62-64, the generator
scripts' _GuidedWrapper) is part of the recorded step: one forward over the doubled batch [cond | uncond], the
combine kernel (sdmi_cfg_combine_nhwc in place of the UNet's layout kernel; sdmi_cfg_combine after the DiT's), the
scale a launch argument."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .module_glue import engine_path_ok
from .plan import StepPlan


def guidance_mode(scale):
    """What a classifier-free guidance scale asks of a step, as the reference's _GuidedWrapper decides it
    (batch_condition_image_generator_single.py:255-262): "uncond" (max(0, scale) == 0: the unconditional forward
    alone), "cond" (|scale - 1| < 1e-6: the conditional forward alone) or "guided" (both, combined -- every other
    scale, 0 < scale < 1 included)."""
    s = max(0.0, float(scale))
    if s == 0.0:
        return "uncond"
    if abs(s - 1.0) < 1e-6:
        return "cond"
    return "guided"


def check_uncond(cond_input, uncond_input):
    """The unconditional input of classifier-free guidance mirrors the conditional one: same keys, same shapes."""
    if uncond_input is None:
        return
    if not cond_input:
        raise ValueError("uncond_input given, but the model is sampled without conditions")
    if set(cond_input) != set(uncond_input):
        raise ValueError(f"uncond_input keys {sorted(uncond_input)} differ from cond_input keys {sorted(cond_input)}")
    for k, v in cond_input.items():
        u = uncond_input[k]
        if isinstance(v, torch.Tensor) and (not isinstance(u, torch.Tensor) or tuple(u.shape) != tuple(v.shape)):
            raise ValueError(f"uncond_input[{k!r}] has shape {tuple(getattr(u, 'shape', ()))}, cond_input[{k!r}] "
                             f"{tuple(v.shape)}")


def cat_conditions(cond_input, uncond_input, out=None, operands=False):
    """[cond | uncond] along the batch: the condition dict of one doubled-batch forward. out: a previous result,
    refilled in place (a recorded step keeps reading the same memory). operands: tensors in the form the engines read
    without a conversion (fp32; a uint8 class-map mask stays uint8)."""
    if out is None:
        out = {}
        for k, v in cond_input.items():
            if not isinstance(v, torch.Tensor):
                out[k] = v
                continue
            dt = v.dtype
            if operands and not (k == "image" and K.is_class_map(v)):
                dt = torch.float32
            out[k] = torch.empty((2 * v.shape[0],) + tuple(v.shape[1:]), dtype=dt, device=v.device)
    for k, v in cond_input.items():
        if isinstance(v, torch.Tensor):
            n = v.shape[0]
            out[k][:n].copy_(v)
            out[k][n:].copy_(uncond_input[k])
    return out


class _Loop:
    """Shared state of a captured loop: the model binding (fused engine, or a stepwise model call), x_t / noise /
    device-counter buffers and the recorded plan.

    Classifier-free guidance (uncond_input + guidance_scale, see guidance_mode): a guided step is ONE forward of
    batch 2B -- x_t in both halves of a (2B, C, H, W) buffer, the conditions [cond | uncond] concatenated once per
    run -- whose halves sdmi_cfg_combine(_nhwc) combines into the (B, C, H, W) eps; the step kernel then writes
    x_{t-1} into both halves (its second output pointer). "cond" / "uncond" run the plain batch-B step."""

    def __init__(self, model, shape, cond_input, seed, uncond_input=None, guidance_scale=1.0):
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the sampling loop runs on the MI355X HIP path only (move the model to cuda)")
        self.dev = dev
        self.model = model
        # the fused engine only when the model's forward would use it (no swapped / foreign leaves, no leaf override)
        self.fused = hasattr(model, "_sdmi") and engine_path_ok(model)
        self.eng = model._sdmi.ensure(dev) if self.fused else None
        B, C, H, W = shape
        self.shape = (B, C, H, W)
        check_uncond(cond_input, uncond_input)
        # with an unconditional input x_t is the first half of the doubled-batch buffer a guided step feeds the model
        self.x2 = torch.empty((2 * B, C, H, W), dtype=torch.float32, device=dev) if uncond_input is not None else None
        self.xt = self.x2[:B] if self.x2 is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        self.z = torch.empty_like(self.xt)
        self.eps = None  # the model output of the last step (a buffer of the recorded plan)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.offset = torch.zeros(1, dtype=torch.int64, device=dev)  # Philox draw counter (uint64 bits)
        self.seed = int(seed)
        self.cond = cond_input
        self.uncond = uncond_input
        self.cond2 = None  # [cond | uncond], filled once per run (guided mode)
        self._scale = float(guidance_scale)
        self.mode = self._mode_of(self._scale)
        self._bind()
        self.plan = None
        # captured issue: "graph" (default) -- the reverse step as ONE hipGraph launch (torch.cuda.CUDAGraph of the
        # eager step; one stream, since inference keeps the context branch inline); "plan" -- sdmi.plan's
        # native launch list re-issued per step. Both bit-identical to the stepwise loop; the graph removes the
        # per-launch host issue that bounds the small-batch step (scripts/sample_graph_probe.py)
        self.issue = os.environ.get("SDMI_SAMPLE_ISSUE", "graph")
        if self.issue not in ("graph", "plan"):
            raise ValueError(f"SDMI_SAMPLE_ISSUE={self.issue!r}: graph or plan")
        self.graph = None
        self.ctx_cache = None

    def _mode_of(self, scale):
        mode = guidance_mode(scale)
        if mode != "cond" and self.uncond is None:
            raise ValueError(f"guidance_scale={scale} needs uncond_input (only a scale of 1 samples without it)")
        return mode

    def _bind(self):
        """The condition dict the step's forward reads: cond, uncond, or (guided) the doubled-batch [cond | uncond]
        buffers that _refresh fills."""
        if self.mode == "guided":
            if self.cond2 is None:
                self.cond2 = cat_conditions(self.cond, self.uncond, operands=self.fused)
            self.active = self.cond2
        else:
            self.active = self.uncond if self.mode == "uncond" else self.cond
        c = self.active or {}
        self.text, self.mask, self.klass = c.get("text"), c.get("image"), c.get("class")

    @property
    def guidance_scale(self):
        return self._scale

    @guidance_scale.setter
    def guidance_scale(self, scale):
        """The scale is a launch argument of the recorded step: a new value drops the recording."""
        scale = float(scale)
        if scale == self._scale:
            return
        self.mode = self._mode_of(scale)
        self._scale = scale
        self._bind()
        self._drop_recording()

    def set_conditions(self, cond_input, uncond_input=None):
        """Other conditions (same batch) for the next runs; the recorded step read the old ones' memory and shapes, so
        it is dropped. A loop built without uncond_input has no doubled-batch buffer and stays unguided."""
        check_uncond(cond_input, uncond_input)
        if uncond_input is not None and self.x2 is None:
            raise ValueError("the loop was built without uncond_input: build a new loop for guided sampling")
        self.cond, self.uncond, self.cond2 = cond_input, uncond_input, None
        self.mode = self._mode_of(self._scale)
        self._bind()
        self._drop_recording()

    def _refresh(self):
        """Pack the current weights (plain kernel launches into the engine's fixed buffers, outside the plan): a loop
        reused after a training update or an EMA swap samples with the weights of the moment it runs. Parameters
        REPLACED rather than updated in place (load_state_dict(assign=True), .to(), ...) rebind the engine; a new
        engine or a re-allocated pack buffer drops the recorded graph / plan, which hold the old pointers."""
        if self.mode == "guided":  # [cond | uncond] once per run, into the buffers the recorded step reads
            cat_conditions(self.cond, self.uncond, out=self.cond2)
        if self.fused:
            eng = self.model._sdmi.ensure(self.dev)
            buf = getattr(getattr(eng, "pack", None), "buf", None)
            if eng is not self.eng:
                self.eng = eng
                self._drop_recording()
            self.eng.refresh_weights()
            nbuf = getattr(getattr(self.eng, "pack", None), "buf", None)
            if nbuf is not buf:  # refresh_weights re-finalised the pack into a new buffer
                self._drop_recording()
            # the context branch (text -> context_proj -> every cross-attention's k|v) is the same for every step of
            # the loop: computed once per run into fixed buffers (UNetEngine.context_cache) instead of per step
            if self.text is not None and hasattr(self.eng, "context_cache"):
                self.ctx_cache = self.eng.context_cache(self.text, self.ctx_cache)

    def _drop_recording(self):
        self.graph = None
        self.plan = None
        self.ctx_cache = None

    def _model_eps(self):
        B, C, H, W = self.shape
        guided = self.mode == "guided"
        x = self.x2 if guided else self.xt
        if self.fused:
            kw = {"ctx_cache": self.ctx_cache} if self.ctx_cache is not None else {}
            pred, _ = self.eng.forward(x, self.t, self.text, self.mask, need_backward=False, klass=self.klass, **kw)
            if guided:
                self.eps = self.eng.guided_to_nchw(pred, B, H, W, self._scale)
            else:
                self.eps = self.eng.pred_to_nchw(pred, B, H, W)
        else:
            with torch.no_grad():
                tt = self.t.expand(x.shape[0])
                out = self.model(x, tt) if self.active is None else self.model(x, tt, self.active)
            out = out.float().contiguous()
            if guided:  # one doubled-batch call (x_t in both halves, [cond | uncond]), then the combine kernel
                _lib.check(_lib.lib().sdmi_cfg_combine(out.data_ptr(), out[B:].data_ptr(), out.numel() // 2,
                                                       self._scale, out.data_ptr(), K._stream()), "sdmi_cfg_combine")
                out = out[:B]
            self.eps = out

    def _x_uncond(self):
        """Second output pointer of the step kernel: the unconditional half of a guided step's doubled input."""
        return self.x2[self.shape[0]:].data_ptr() if self.mode == "guided" else None

    def _set_x(self, x_T):
        self.xt.copy_(x_T)
        if self.mode == "guided":
            self.x2[self.shape[0]:].copy_(x_T)

    @staticmethod
    def fresh_draw():
        """A random 62-bit starting draw counter from torch's default generator: torch.manual_seed governs it, and runs
        started from different counters draw disjoint Philox streams (a run uses `steps` consecutive counters)."""
        return int(torch.randint(0, 1 << 62, (1,)).item())

    def _draw(self):
        _lib.check(_lib.lib().sdmi_randn(self.z.data_ptr(), self.xt.numel(), ctypes.c_ulonglong(self.seed),
                                         self.offset.data_ptr(), 1, K._stream()), "sdmi_randn")

    def _iterate(self, steps, captured):
        # the stepwise (foreign-leaf) path reads device scalars through torch ops: never recorded
        captured = captured and self.fused
        for _ in range(steps):
            if not captured:
                self._step()
            elif self.issue == "graph":
                if self.graph is None:  # the first step runs eagerly, then the step is captured (capture runs nothing)
                    self._step()
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph):
                        self._step()
                else:
                    self.graph.replay()
            elif self.plan is None:  # the first step is recorded while it runs
                self.plan = StepPlan(self._step, self.dev)
            else:
                self.plan.replay()


class DDPMSampleLoop(_Loop):
    def __init__(self, model, scheduler, shape, cond_input=None, seed=0, uncond_input=None, guidance_scale=1.0):
        """model: a drop-in denoiser module (models.unet_cond_base.Unet / unet_base.Unet / transformer.DIT) already
        on the GPU; scheduler: scheduler.linear_noise_scheduler.LinearNoiseScheduler; shape: (B, C, H, W) latents;
        cond_input: the model's condition dict (text / image / class), fixed for the whole loop; uncond_input +
        guidance_scale: classifier-free guidance (tools/sample_ddpm_text_cond.py:62-64), see _Loop."""
        super().__init__(model, shape, cond_input, seed, uncond_input, guidance_scale)
        self.T = scheduler.num_timesteps
        self.tab = scheduler.tables(self.dev)
        self.x0 = torch.empty_like(self.xt)

    def _step(self):
        self._model_eps()
        self._draw()
        tab = self.tab
        args = (self.xt.data_ptr(), self.eps.data_ptr(), self.z.data_ptr(), self.xt.numel(), self.t.data_ptr(),
                tab["betas"].data_ptr(), tab["alphas"].data_ptr(), tab["alpha_cum_prod"].data_ptr(),
                tab["sqrt_one_minus_alpha_cum_prod"].data_ptr(), self.xt.data_ptr())
        if self.mode == "guided":  # x_{t-1} into both halves of the doubled input
            _lib.check(_lib.lib().sdmi_ddpm_prev_dup(*args, self._x_uncond(), self.x0.data_ptr(), 1, K._stream()),
                       "sdmi_ddpm_prev_dup")
        else:
            _lib.check(_lib.lib().sdmi_ddpm_prev(*args, self.x0.data_ptr(), 1, K._stream()), "sdmi_ddpm_prev")

    def reset(self, x_T, t_start=None, draw=0):
        """Start a loop from x_T at timestep t_start (default T - 1) with the noise draw counter at `draw`."""
        self._set_x(x_T)
        self.t.fill_(self.T - 1 if t_start is None else int(t_start))
        self.offset.fill_(int(draw))

    def run(self, x_T, steps=None, captured=True, t_start=None):
        """`steps` (default T) reverse steps from x_T; returns (x_{t_end}, x0 prediction of the last step).
        captured=False issues every step eagerly (the stepwise reference loop, same kernels and order)."""
        self._refresh()
        self.reset(x_T, t_start)
        self._iterate(self.T if steps is None else int(steps), captured)
        return self.xt, self.x0


def ddim_time_steps(T, steps, method="linear"):
    """DDIMSampler.forward's timestep pairs (scheduler/linear_noise_scheduler.py:231-242): "linear" range(0, T, T //
    steps) or "quadratic" int32(linspace(0, sqrt(0.8 T), steps)^2), both + 1; previous = [0] + ts[:-1]."""
    if method == "linear":
        ts = np.asarray(list(range(0, T, T // steps)))
    elif method == "quadratic":
        ts = (np.linspace(0, np.sqrt(T * 0.8), steps) ** 2).astype(np.int32)
    else:
        raise NotImplementedError(f"sampling method {method} is not implemented!")
    ts = ts + 1
    return ts, np.concatenate([[0], ts[:-1]])


class DDIMSampleLoop(_Loop):
    """DDIMSampler.forward (reference :209-256) with the model, the DDIM update and the per-step noise
    (torch.randn_like at :200, here device Philox) recorded once and replayed `steps` times."""

    def __init__(self, model, alpha_t_bar, shape, cond_input=None, steps=50, method="linear", eta=0.0, seed=0,
                 uncond_input=None, guidance_scale=1.0):
        """alpha_t_bar: the sampler's fp32 cumulative-product table (DDIMSampler.alpha_t_bar, from linspace(beta));
        uncond_input + guidance_scale: classifier-free guidance (the generator scripts' _GuidedWrapper), see _Loop."""
        super().__init__(model, shape, cond_input, seed, uncond_input, guidance_scale)
        self.steps = int(steps)
        self.eta = float(eta)
        ts, tp = ddim_time_steps(len(alpha_t_bar), self.steps, method)
        # the reference's loop reads pairs i = steps - 1 .. 0 only (linear spacing can yield more when T % steps != 0)
        if len(ts) < self.steps:
            raise ValueError(f"{method} time steps: {len(ts)} pairs for steps={self.steps}")
        ts, tp = ts[:self.steps], tp[:self.steps]
        if int(ts.max()) >= len(alpha_t_bar):  # the reference would raise an IndexError in its gather
            raise IndexError(f"DDIM timestep {int(ts.max())} out of range for T={len(alpha_t_bar)}")
        self.ts = torch.as_tensor(ts, dtype=torch.int64).to(self.dev)
        self.tp = torch.as_tensor(tp, dtype=torch.int64).to(self.dev)
        self.abar = alpha_t_bar.to(device=self.dev, dtype=torch.float32).contiguous()
        self.idx = torch.zeros(1, dtype=torch.int64, device=self.dev)

    def _step(self):
        self._model_eps()
        self._draw()
        # elementwise and in place: x_{t-1} overwrites x_t (the next step's model input)
        args = (self.xt.data_ptr(), self.eps.data_ptr(), self.z.data_ptr(), self.xt.numel(), self.ts.data_ptr(),
                self.tp.data_ptr(), self.idx.data_ptr(), self.t.data_ptr(), self.abar.data_ptr(), self.eta,
                self.xt.data_ptr())
        if self.mode == "guided":  # ... and the unconditional half of the doubled input
            _lib.check(_lib.lib().sdmi_ddim_prev_dev_dup(*args, self._x_uncond(), 1, K._stream()),
                       "sdmi_ddim_prev_dev_dup")
        else:
            _lib.check(_lib.lib().sdmi_ddim_prev_dev(*args, 1, K._stream()), "sdmi_ddim_prev_dev")

    def reset(self, x_T, draw=0):
        self._set_x(x_T)
        self.idx.fill_(self.steps - 1)
        self.t.copy_(self.ts[self.steps - 1:self.steps])
        self.offset.fill_(int(draw))

    def run(self, x_T, captured=True, draw=0):
        """The whole reversed loop (i = steps - 1 .. 0) from x_T; returns x_0 (the loop's buffer). `draw` is the Philox
        draw counter the run starts at: runs from the same (seed, draw) repeat their noise exactly; fresh_draw() gives
        a run noise of its own."""
        self._refresh()
        self.reset(x_T, draw)
        self._iterate(self.steps, captured)
        return self.xt
