"""Generates tests/golden/vqvae_noise.safetensors by importing the REFERENCE noise-robust autoencoder
(models/vqvae_noise.py, read-only at /root/reference) in THIS container. Only input / output tensors are committed;
the weights regenerate from oracle.sd_oracle.deterministic_state.

Run:  PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vqvae_noise.py

One generator step of train_vqvae_celebhq_noise_multi_GPU.py (without LPIPS / GAN) on the small config at
n_scale = 0.2: recon + 1.0 * codebook + 0.2 * commitment. The forward draws nothing but add_noise's randn_like, so
eps is recovered by reseeding torch's generator and drawing the latent's shape again."""
import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get("SDMI_REFERENCE", "/root/reference")
if REF not in sys.path:
    sys.path.insert(1, REF)

from oracle import sd_oracle as O  # noqa: E402
from oracle import vqvae_oracle as VO  # noqa: E402
from tests.golden.configs import SMALL_VQVAE  # noqa: E402
from tests.golden.make_golden_dit_vqvae import GRAD_KEYS_VQVAE  # noqa: E402

torch.set_num_threads(8)
N_SCALE, DRAW_SEED, STATE_SEED, IMAGE_SEED = 0.2, 77, 9, 60


def main():
    import models.vqvae_noise as ref_vq
    cfg = SMALL_VQVAE
    model = ref_vq.VQVAE(im_channels=3, model_config=cfg)
    shapes = VO.vqvae_param_shapes(cfg)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(shapes.keys()), [k for k in ref_sd if k not in shapes][:5]
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, v.shape, shapes[k])
    model.load_state_dict(O.deterministic_state(shapes, STATE_SEED))
    model.train()
    im = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(IMAGE_SEED)) * 2 - 1
    pre = {}
    h = model.pre_quant_conv.register_forward_hook(lambda m, i, o: pre.__setitem__("z", o.detach().clone()))
    model.zero_grad()
    torch.manual_seed(DRAW_SEED)
    out, z, ql = model(im, N_SCALE)
    h.remove()
    torch.manual_seed(DRAW_SEED)
    eps = torch.randn_like(z)
    recon = torch.nn.functional.mse_loss(out, im)
    cb, cm = 1.0 * ql["codebook_loss"], 0.2 * ql["commitment_loss"]
    (recon + cb + cm).backward()
    with torch.no_grad():
        zq, _, idx = model.quantize(pre["z"])
        assert torch.equal(z, zq + (zq.max() - zq.min()) * N_SCALE * eps), "the recovered eps is not the forward's draw"
    f = {"im": im, "eps": eps, "zq": zq, "z": z.detach(), "out": out.detach(), "indices": idx,
         "n_scale": torch.tensor([N_SCALE]), "recon": recon.detach().reshape(1), "codebook": cb.detach().reshape(1),
         "commitment": cm.detach().reshape(1),
         "grad_norms": torch.stack([p.grad.norm() if p.grad is not None else torch.zeros(())
                                    for _, p in model.named_parameters()])}
    for k, p in model.named_parameters():
        if k in GRAD_KEYS_VQVAE:
            f["grad." + k] = p.grad.detach().reshape(-1)[:8192].clone()
    path = os.path.join(HERE, "vqvae_noise.safetensors")
    save_file({k: v.contiguous() for k, v in f.items()}, path)
    print("fixture written to", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
