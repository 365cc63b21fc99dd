"""The noise-robust autoencoder's training step as a composition of the unchanged oracle (oracle/vqvae_oracle.py):

    encode_pre_quant -> quantize_train -> z = zq + (zq.max() - zq.min()) * n_scale * eps -> decode

with autograd (reference models/vqvae_noise.py:144-183 and the generator step of
train_vqvae_celebhq_noise_multi_GPU.py without LPIPS / GAN). tests/test_oracle_vqvae_noise.py pins it to the
reference's own step (tests/golden/vqvae_noise.safetensors); tests/test_vqvae_noise_gpu.py holds the engine to it."""
import torch
import torch.nn.functional as F

from oracle import vqvae_oracle as VO


def latent_range(zq, masks=None):
    """zq.max() - zq.min(). masks = (at_max, at_min), bool tensors of zq's shape: the value stays the true range, the
    gradient goes to the masked elements instead (evenly, the minimum's share negated) -- the extreme of x + (q - x)
    among pixels that share a code is decided by the last bit, so a bf16 path is held to the oracle at its own
    extremal positions, as it is at its own code indices."""
    w = zq.max() - zq.min()
    if masks is None:
        return w
    at_max, at_min = (m.to(zq.dtype) for m in masks)
    routed = (zq * at_max).sum() / at_max.sum() - (zq * at_min).sum() / at_min.sum()
    return routed + (w - routed).detach()


def train_grads(sd, cfg, im, n_scale, eps, codebook_weight=1.0, commitment_beta=0.2, indices=None, masks=None):
    """(losses {recon, codebook, commitment, total}, grads {key: tensor}, reconstruction, indices, clean zq, noisy z)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    zq, cb, cm, idx = VO.quantize_train(p, VO.encode_pre_quant(p, cfg, im), indices)
    z = zq + latent_range(zq, masks) * n_scale * eps
    out = VO.decode(p, cfg, z)
    recon = F.mse_loss(out, im)
    total = recon + codebook_weight * cb + commitment_beta * cm
    total.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}
    losses = {"recon": recon.detach(), "codebook": (codebook_weight * cb).detach(),
              "commitment": (commitment_beta * cm).detach(), "total": total.detach()}
    return losses, grads, out.detach(), idx, zq.detach(), z.detach()


def closed_form(z, g, eps, n_scale):
    """dL/dz of L = sum(g * (z + (z.max() - z.min()) * n_scale * eps)): g plus n_scale * sum(g * eps) at the maxima,
    divided evenly among them, minus the same at the minima (torch's tie rule for full reductions)."""
    S = (g * eps).sum()
    at_max, at_min = (z == z.max()).to(z.dtype), (z == z.min()).to(z.dtype)
    return g + n_scale * S * (at_max / at_max.sum() - at_min / at_min.sum())
