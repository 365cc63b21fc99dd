"""The KL autoencoder's training step as a composition of the unchanged oracle (oracle/vqvae_oracle.py):

    encode_pre_quant -> (mean, logvar) = chunk -> sample = mean + exp(0.5 logvar) * eps -> decode

with autograd (reference models/vae.py:88-120; the reference has no trainer for this model, the loss is the standard
closed form recon + kl_weight * KL). The oracle's trunk functions index the state dict by key and take their widths from
the tensors, so the 2z-row encoder_conv_out / pre_quant_conv of the KL model need nothing new.
tests/test_oracle_vae.py pins this to the reference's own step (tests/golden/vae_small.safetensors);
tests/test_vae_gpu.py holds the engines to it."""
import json
import os

import torch
import torch.nn.functional as F

from oracle import vqvae_oracle as VO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def param_shapes():
    """Ordered {state-dict key: shape} of the reference models.vae.VAE(3, SMALL_VQVAE), as its generator recorded it."""
    with open(os.path.join(GOLDEN, "vae_small_keys.json")) as fh:
        return {k: tuple(s) for k, s in json.load(fh)}


def kl_term(encoder_output):
    """KL = (1 / B) sum_b 0.5 sum_{c,h,w} (exp(logvar) + mean^2 - 1 - logvar)."""
    mean, logvar = torch.chunk(encoder_output, 2, dim=1)
    return torch.mean(0.5 * torch.sum(torch.exp(logvar) + mean ** 2 - 1 - logvar, dim=[1, 2, 3]))


def forward(sd, cfg, im, eps):
    """(reconstruction, encoder_output, sample); eps None: the sample is the mean."""
    enc = VO.encode_pre_quant(sd, cfg, im)
    mean, logvar = torch.chunk(enc, 2, dim=1)
    sample = mean if eps is None else mean + torch.exp(0.5 * logvar) * eps
    return VO.decode(sd, cfg, sample), enc, sample


def train_grads(sd, cfg, im, eps, kl_weight):
    """(losses {recon, kl (unweighted), total}, grads {key: tensor}, reconstruction, encoder_output, sample)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out, enc, sample = forward(p, cfg, im, eps)
    recon = F.mse_loss(out, im)
    kl = kl_term(enc)
    total = recon + kl_weight * kl
    total.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}
    losses = {"recon": recon.detach(), "kl": kl.detach(), "total": total.detach()}
    return losses, grads, out.detach(), enc.detach(), sample.detach()
