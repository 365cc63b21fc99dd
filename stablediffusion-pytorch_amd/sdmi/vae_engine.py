"""KL autoencoder encode / sample / decode (reference models/vae.py:88-115) as one schedule of gfx950 kernels.

The encoder and decoder trunks are sdmi.vqvae_engine's (same blocks, same state-dict keys); encoder_conv_out has 2z
output rows (the moments) and there is no codebook. The latent interface is one launch, sdmi_kl_sample
(csrc/kl_latent.hip): pre_quant_conv in fp32 on the encoder head's fp32 output, the split into mean and log-variance and
the reparameterised draw mean + exp(0.5 logvar) * eps -- the moments never pass through bf16. Forward only."""
import torch

from . import kernels as K
from . import plan
from .vqvae_engine import VQVAEEngine


def check_kl_latent(L):
    if 2 * L["z"] > 8:
        raise ValueError("z_channels > 4 (2 * z_channels > 8 moment channels) is not supported by sdmi_kl_sample")


class VAEEngine(VQVAEEngine):
    def _check_latent(self):
        check_kl_latent(self.L)

    def _n_lat(self):
        return 2 * self.L["z"]

    def encode(self, x, eps=None):
        """vae.py:88-101. x: (B, 3, H, W) fp32, eps: the standard-normal draw (B, z, h, w) fp32 or None (the sample is
        then the mean) -> (sample (B, z, h, w), moments (B, 2z, h, w)), NCHW fp32."""
        L, P = self.L, self.P
        B, zc = x.shape[0], L["z"]
        hz, h, w = self._encoder(x)
        mom = torch.empty(B, 2 * zc, h, w, dtype=torch.float32, device=self.device)
        smp = torch.empty(B, zc, h, w, dtype=torch.float32, device=self.device)
        if eps is not None:
            if tuple(eps.shape) != tuple(smp.shape):
                raise ValueError(f"eps must have the latent's shape {tuple(smp.shape)}")
            eps = plan.as_operand(eps)
        K.kl_sample(hz, 8, P["pre_quant_conv.weight"], P["pre_quant_conv.bias"], eps, B, zc, h * w, mom, smp)
        return smp, mom
