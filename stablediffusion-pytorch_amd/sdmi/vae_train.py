"""KL autoencoder training step (reference models/vae.py; the reference ships no trainer for it, so the loss is the
standard closed form) on the HIP kernels of libsdmi.so:

    encoder -> pre_quant_conv -> (mean, logvar) -> sample = mean + exp(0.5 logvar) eps -> post_quant_conv -> decoder
    loss = MSE(out, im) + kl_weight * KL,   KL = (1 / B) sum_b 0.5 sum_{c,h,w} (exp(logvar) + mean^2 - 1 - logvar)

Trunk, tape and backward schedule are sdmi.vqvae_train's (VAETrainEngine subclasses VQVAETrainEngine and replaces the
latent section alone); the latent interface is csrc/kl_latent.hip: sdmi_kl_sample (one launch: pre_quant_conv, the draw,
post_quant_conv fused into decoder_conv_in's bf16 operand; one more for the KL value) and sdmi_kl_bwd (two launches)."""
import torch

from . import kernels as K
from . import plan
from .vae_engine import check_kl_latent
from .vqvae_train import S_LOSS, AutoencoderTrainer, VQVAETrainEngine, noise_key  # noqa: F401


class VAETrainEngine(VQVAETrainEngine):
    """Forward + backward of models/vae.py VAE. Parameters / gradients: {state-dict key: fp32 CUDA tensor}."""

    def _check_latent(self):
        check_kl_latent(self.L)

    def _n_lat(self):
        return 2 * self.L["z"]

    def forward(self, x, need_backward=True, eps=None, want_kl=False):
        """x: (B, im_channels, H, W) fp32 image; eps: the standard-normal draw of latent_shape(B, H, W), or None (the
        decoder then sees the mean). Returns (reconstruction NHWC fp32 [B*H*W, 8], ctx); ctx["moments"] (B, 2z, h, w)
        is the reference's encoder_output, ctx["sample"] (B, z, h, w) the latent, ctx["kl"] (1,) the unweighted KL
        term under want_kl (one more launch)."""
        return self._forward(x, need_backward, dict(eps=eps, want_kl=want_kl))

    def _latent_fwd(self, z, q, tape, eps=None, want_kl=False):
        L, P = self.L, self.P
        B, h, w = q["B"], q["h"], q["w"]
        zc = L["z"]
        mom = torch.empty(B, 2 * zc, h, w, dtype=torch.float32, device=self.device)
        smp = torch.empty(B, zc, h, w, dtype=torch.float32, device=self.device)
        kl = torch.empty(1, dtype=torch.float32, device=self.device) if want_kl else None
        if eps is not None:
            if tuple(eps.shape) != tuple(smp.shape):
                raise ValueError("eps must be a standard-normal draw of latent_shape(B, H, W)")
            eps = plan.as_operand(eps)
        tape.label = "decoder_in"
        zin = self._new(B * h * w, 8)
        K.kl_sample(z, 8, P["pre_quant_conv.weight"], P["pre_quant_conv.bias"], eps, B, zc, h * w, mom, smp,
                    w_post=P["post_quant_conv.weight"], b_post=P["post_quant_conv.bias"], zin=zin, ld=8, kl=kl)
        q.update(z=z, moments=mom, sample=smp, eps=eps)
        tape.label = "quant"
        tape.append((self._bwd_quant, dict(q=q)))
        return zin, dict(moments=mom, sample=smp, eps=eps, kl=kl)

    def _bwd_quant(self, c, grads):
        """sdmi_kl_bwd: post_quant_conv dW/db, the gradient of the sample into mean and log-variance, the fused KL
        term and the outside gradients, pre_quant_conv dW/db and the gradient of encoder_conv_out's output."""
        q = c["q"]
        B, h, w = q["B"], q["h"], q["w"]
        P = self.P
        q["dz"] = dz = self._new(B * h * w, 8)
        K.kl_bwd(q["dzin"], 8, P["post_quant_conv.weight"], q["sample"], q["moments"], q["eps"], q["z"], 8,
                 P["pre_quant_conv.weight"], B, self.L["z"], h * w, kl_weight=self.kl_weight, loss_w=self.loss_w,
                 dsample_add=self.dsample_add, dmom_add=self.dmom_add, dh=dz, ld_out=8,
                 dw_post=self.g("post_quant_conv.weight"), db_post=self.g("post_quant_conv.bias"),
                 dw_pre=self.g("pre_quant_conv.weight"), db_pre=self.g("pre_quant_conv.bias"))

    def backward(self, ctx, dout, kl_weight=0.0, grads=None, on_progress=None, dsample=None, dmom=None, loss_w=None):
        """dout: NHWC bf16 [B*H*W, 8] = dL/d(reconstruction). kl_weight (times the device scalar loss_w when given)
        enters the fused KL term at the latent; dsample (B, z, h, w) / dmom (B, 2z, h, w), NCHW fp32, optional: outside
        gradients of the sample and of the moments (a caller's own loss on encoder_output). Every parameter gradient is
        fully overwritten."""
        self.kl_weight = float(kl_weight)
        self.dsample_add, self.dmom_add, self.loss_w = dsample, dmom, loss_w
        self._run_tape(ctx, dout, grads, on_progress)


class VAETrainer(AutoencoderTrainer):
    """One training step of the KL autoencoder: forward, recon MSE + kl_weight * KL (+ perceptual_weight * LPIPS with
    lpips_state, as in VQVAETrainer), backward, Adam(lr, betas=(0.5, 0.999)). Flat fp32 buffers; the step never
    synchronises with the host; N > 1 ranks average their gradients before Adam.

    eps is drawn on the device by sdmi_randn(key = noise_key(noise_seed, rank), offset), the offset a device counter
    owned by the trainer that advances with every draw, so every step -- and every replay of a recorded StepPlan --
    draws fresh, reproducible noise. kl_weight (settable attribute) is a launch argument: a recorded StepPlan keeps the
    value it was recorded with and must be recorded again after kl_weight changes, as n_scale in VQVAETrainer."""

    engine_cls = VAETrainEngine

    def __init__(self, cfg, state_dict, device, *, im_channels=3, lr=2e-5, betas=(0.5, 0.999), eps=1e-8,
                 kl_weight=5e-6, group=None, bucket_bytes=64 << 20, perceptual_weight=0.0, lpips_state=None,
                 noise_seed=0):
        super().__init__(cfg, state_dict, device, im_channels=im_channels, lr=lr, betas=betas, eps=eps, group=group,
                         bucket_bytes=bucket_bytes, perceptual_weight=perceptual_weight, lpips_state=lpips_state,
                         noise_seed=noise_seed, hp={})
        self.kl_weight = float(kl_weight)
        self.noise_offset = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.kl = None

    def _forward(self, im):
        eng = self.engine
        B, _, H, W = im.shape
        return eng.forward(im, eps=self._draw(eng.latent_shape(B, H, W)), want_kl=True)

    def _backward(self, ctx, dout):
        self.engine.backward(ctx, dout, self.kl_weight)

    def _keep(self, ctx, out):
        self.kl, self.eps, self.moments, self.sample = ctx["kl"], ctx["eps"], ctx["moments"], ctx["sample"]

    def losses(self):
        """Host dict of the last step's losses (synchronises): recon, kl (weighted), total and, with the LPIPS term,
        perceptual (weighted)."""
        rec = self.state[S_LOSS].item()
        kl = self.kl_weight * self.kl.item()
        d = dict(recon=rec, kl=kl, total=rec + kl)
        if self.lpips is not None:
            d["perceptual"] = self.lp_loss.item()
            d["total"] += d["perceptual"]
        return d
