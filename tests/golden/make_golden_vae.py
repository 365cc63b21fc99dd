"""Generates tests/golden/vae_small.safetensors and tests/golden/vae_small_keys.json by importing the REFERENCE KL
autoencoder (models/vae.py) in THIS container. Only input / output tensors and the state-dict key / shape list are
committed; the weights regenerate from oracle.sd_oracle.deterministic_state over that list.

Run:  PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vae.py

One training step on the small config: model(im) after torch.manual_seed(77), loss = recon + 1e-4 * KL with
KL = (1 / B) sum_b 0.5 sum_{c,h,w} (exp(logvar) + mean^2 - 1 - logvar) (the reference has no trainer for this model; the
standard closed form). The forward draws nothing but encode's torch.randn(mean.shape) on the CPU generator, so eps is
recovered by reseeding and drawing that shape again."""
import json
import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get("SDMI_REFERENCE")
if REF and REF not in sys.path:
    sys.path.insert(1, REF)

from oracle import sd_oracle as O  # noqa: E402
from tests.golden.configs import SMALL_VQVAE  # noqa: E402
from tests.golden.make_golden_dit_vqvae import GRAD_KEYS_VQVAE  # noqa: E402

torch.set_num_threads(8)
KL_WEIGHT, DRAW_SEED, STATE_SEED, IMAGE_SEED = 1e-4, 77, 9, 60
GRAD_KEYS_VAE = tuple(GRAD_KEYS_VQVAE) + ("pre_quant_conv.weight", "pre_quant_conv.bias")


def kl_term(encoder_output):
    mean, logvar = torch.chunk(encoder_output, 2, dim=1)
    return torch.mean(0.5 * torch.sum(torch.exp(logvar) + mean ** 2 - 1 - logvar, dim=[1, 2, 3]))


def main():
    import models.vae as ref_vae
    cfg = SMALL_VQVAE
    model = ref_vae.VAE(im_channels=3, model_config=cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(O.deterministic_state(shapes, STATE_SEED))
    model.train()
    im = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(IMAGE_SEED)) * 2 - 1
    model.zero_grad()
    torch.manual_seed(DRAW_SEED)
    out, enc = model(im)
    mean, logvar = torch.chunk(enc.detach(), 2, dim=1)
    torch.manual_seed(DRAW_SEED)
    eps = torch.randn(mean.shape)
    sample = mean + torch.exp(0.5 * logvar) * eps
    with torch.no_grad():
        assert torch.equal(model.decode(sample), out), "the recovered eps is not the forward's draw"
    recon = torch.nn.functional.mse_loss(out, im)
    kl = kl_term(enc)
    (recon + KL_WEIGHT * kl).backward()
    f = {"im": im, "eps": eps, "encoder_output": enc.detach(), "sample": sample, "out": out.detach(),
         "recon": recon.detach().reshape(1), "kl": kl.detach().reshape(1),
         "grad_norms": torch.stack([p.grad.norm() if p.grad is not None else torch.zeros(())
                                    for _, p in model.named_parameters()])}
    for k, p in model.named_parameters():
        if k in GRAD_KEYS_VAE:
            f["grad." + k] = p.grad.detach().reshape(-1)[:8192].clone()
    path = os.path.join(HERE, "vae_small.safetensors")
    save_file({k: v.contiguous() for k, v in f.items()}, path)
    with open(os.path.join(HERE, "vae_small_keys.json"), "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps([k, list(s)]) for k, s in shapes.items()) + "\n]\n")
    print("fixture written to", path, os.path.getsize(path), "bytes;", len(shapes), "state-dict tensors; recon",
          float(recon), "kl", float(kl))


if __name__ == "__main__":
    main()
