"""Drop-in noise-robust VQVAE (reference models/vqvae_noise.py) on the MI355X HIP path.

The autoencoder train_vqvae_celebhq_noise_multi_GPU.py trains and every production caller of the reference loads:
models/vqvae.py with one more line between quantize() and decode() (vqvae_noise.py:155,177-183),

    out = add_noise(out, n_scale)        weight + (weight.max() - weight.min()) * n_scale * randn_like(weight)

Same constructor, module tree and state-dict keys as models.vqvae.VQVAE (it is a subclass); `encode(x, n_scale)`
(n_scale required, as in the reference), `decode(z)` and `forward(x, n_scale=0.0)` -> (out, z, losses). n_scale is a
Python float or a 0-dim tensor (the reference walks a torch.linspace). With n_scale != 0 the module draws
eps = randn of the latent's shape from torch's generator of the device, exactly once per call, so the reference's
RNG-draw sequence is kept; with n_scale == 0 nothing is drawn and every path is models.vqvae.VQVAE's. The range, the
noise and their backward -- the range is differentiable: n_scale * sum(g * eps) goes to the extremal elements of the
clean latent, split evenly among ties, the minimum's share negated -- are the kernels of csrc/latent_noise.hip. Training
`forward` under autograd runs the training engine as one autograd Function, as models.vqvae does; the returned z is the
noisy latent and a gradient on it enters the backward as the outside gradient of the latent.
"""
import torch

from models.blocks import DownBlock, MidBlock, UpBlock
from models.vqvae import VQVAE as _CleanVQVAE
from models.vqvae import VQVAEFunction
from sdmi import _lib
from sdmi import kernels as K
from sdmi import leaf as LF
from sdmi.module_glue import NO_INPUT_GRAD


def _scale(n_scale):
    """n_scale as a Python float (a 0-dim tensor is read once, like the reference's `n_scale == 0`)."""
    return float(n_scale.item()) if isinstance(n_scale, torch.Tensor) else float(n_scale)


class _AddNoise(torch.autograd.Function):
    """(weight, eps) -> weight + (max - min) n_scale eps over any contiguous cuda fp32 tensor, taken flat."""

    @staticmethod
    def forward(ctx, weight, eps, n_scale):
        z = weight.detach().float().contiguous()
        eps = eps.detach().float().contiguous()
        n = z.numel()
        rws = K.latent_range(z, K.latent_noise_ws(n, z.device))
        out = K.latent_noise_fwd(z, eps, 1, 1, n, n_scale, rws, torch.empty_like(z))
        ctx.saved = (z, eps, rws, n_scale)
        return out

    @staticmethod
    def backward(ctx, g):
        z, eps, rws, n_scale = ctx.saved
        n = z.numel()
        r = K.latent_noise_bwd(None, 0, None, g.float().contiguous(), eps, z, 1, 1, n, n_scale, rws,
                               K.latent_noise_ws(n, z.device), torch.empty_like(z))
        return r, None, None


def add_noise(weight, n_scale=0.074):
    """vqvae_noise.py:177-183 for a cuda fp32 tensor; differentiable in `weight` (through the range as well)."""
    ns = _scale(n_scale)
    if ns == 0:
        return weight
    if not weight.is_cuda:
        raise RuntimeError("add_noise runs on the MI355X HIP path only (move the tensor to cuda)")
    _lib.lib()
    return _AddNoise.apply(weight, torch.randn_like(weight), ns)


class VQVAENoiseFunction(torch.autograd.Function):
    """(x, *params) -> (reconstruction, noisy z_q, codebook_loss, commitment_loss) on the HIP training engine."""

    @staticmethod
    def forward(ctx, mod, n_scale, eps, x, *params):
        if ctx.needs_input_grad[3]:
            raise RuntimeError(NO_INPUT_GRAD)
        eng = mod._train_eng(x)
        B, C, H, W = x.shape
        out, c = eng.forward(x, n_scale=n_scale, eps=eps)
        ctx.mod, ctx.c, ctx.hw, ctx.packs_of = mod, c, (B, H, W), mod._packs_of
        vq = c["vq_loss"].reshape(())
        return eng.pred_to_nchw(out, B, H, W), c["z"], vq.clone(), vq.clone()

    @staticmethod
    def backward(ctx, dimg, dz, dcb, dcm):
        # the engine's context carries the noise: its quantiser backward runs sdmi_latent_noise_bwd first
        return (None, None) + VQVAEFunction.backward(ctx, dimg, dz, dcb, dcm)


class VQVAE(_CleanVQVAE):
    def _leaf(self):
        return getattr(self, "sdmi_leaf_path", False) or not LF.engine_ok(
            self, (VQVAE, _CleanVQVAE, DownBlock, MidBlock, UpBlock))

    def _latent_shape(self, x):
        f = 2 ** sum(1 for d in self.down_sample if d)
        return (x.shape[0], self.z_channels, x.shape[2] // f, x.shape[3] // f)

    def encode(self, x, n_scale):
        if self._leaf():
            zq, losses, _ = self._leaf_encode(x)
            return add_noise(zq, n_scale), losses
        ns = _scale(n_scale)
        if ns == 0:
            return super().encode(x)
        eps = torch.randn(self._latent_shape(x), dtype=torch.float32, device=x.device)
        with torch.no_grad():
            zq, loss, _ = self._eng(x).encode(x, n_scale=ns, eps=eps)
        return zq, {"codebook_loss": loss[0], "commitment_loss": loss[0]}

    def forward(self, x, n_scale=0.0):
        if self._leaf():
            z, losses = self.encode(x, n_scale)
            return self._leaf_decode(z), z, losses
        ns = _scale(n_scale)
        if torch.is_grad_enabled() and x.requires_grad:  # (before anything is packed or drawn)
            raise RuntimeError(NO_INPUT_GRAD)
        training = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if ns == 0 and training:
            return super().forward(x)  # models.vqvae's autograd Function: nothing is drawn
        if training:
            self._train_eng(x)  # (raises off the HIP path before anything is drawn)
            eps = torch.randn(self._latent_shape(x), dtype=torch.float32, device=x.device)
            out, z, cb, cm = VQVAENoiseFunction.apply(self, ns, eps, x, *self.parameters())
            return out, z, {"codebook_loss": cb, "commitment_loss": cm}
        z, quant_losses = self.encode(x, ns)
        return self.decode(z), z, quant_losses
