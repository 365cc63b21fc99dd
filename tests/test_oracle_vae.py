"""Pins tests/vae_oracle.py to the reference KL autoencoder's own step (tests/golden/vae_small.safetensors, written by
tests/golden/make_golden_vae.py from the reference models/vae.py): encoder_output, sample and reconstruction bit for bit,
the losses and the recorded gradient slices to 1e-5 relative; and the drop-in module's state-dict surface to the key /
shape list the generator recorded from the reference module."""
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import sd_oracle as O
from tests import vae_oracle as VAO
from tests.golden.configs import SMALL_VQVAE

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KL_WEIGHT = 1e-4


@pytest.fixture(scope="module")
def fixture():
    return load_file(os.path.join(G, "vae_small.safetensors"))


@pytest.fixture(scope="module")
def step(fixture):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = O.deterministic_state(VAO.param_shapes(), seed=9)
    return sd, VAO.train_grads(sd, SMALL_VQVAE, fixture["im"], fixture["eps"], KL_WEIGHT)


def test_recorded_surface():
    shapes = VAO.param_shapes()
    z = SMALL_VQVAE["z_channels"]
    assert len(shapes) == 128 and "embedding.weight" not in shapes
    assert shapes["pre_quant_conv.weight"] == (2 * z, 2 * z, 1, 1)
    assert shapes["encoder_conv_out.weight"] == (2 * z, SMALL_VQVAE["down_channels"][-1], 3, 3)
    assert shapes["post_quant_conv.weight"] == (z, z, 1, 1)


def test_module_state_dict_is_the_reference_surface():
    from models.vae import VAE
    sd = VAE(3, SMALL_VQVAE).state_dict()
    ref = VAO.param_shapes()
    assert list(sd) == list(ref)
    assert all(tuple(sd[k].shape) == ref[k] for k in sd)
    cfg = {k: v for k, v in SMALL_VQVAE.items() if k != "codebook_size"}
    assert list(VAE(3, cfg).state_dict()) == list(ref), "the module must not need codebook_size"


def test_forward_is_bitwise(step, fixture):
    _, (_, _, out, enc, sample) = step
    assert torch.equal(enc, fixture["encoder_output"])
    assert torch.equal(sample, fixture["sample"])
    assert torch.equal(out, fixture["out"])


def test_losses_and_gradients(step, fixture):
    sd, (losses, grads, _, _, _) = step
    for name in ("recon", "kl"):
        want = fixture[name].item()
        assert abs(losses[name].item() - want) <= 1e-5 * abs(want), (name, losses[name].item(), want)
    seen = 0
    for k in sd:
        key = "grad." + k
        if key in fixture:
            got, want = grads[k].reshape(-1)[:8192], fixture[key]
            assert float((got - want).norm()) <= 1e-5 * float(want.norm()), k
            seen += 1
    assert seen >= 20 and "grad.pre_quant_conv.weight" in fixture and "grad.pre_quant_conv.bias" in fixture
    norms = torch.stack([grads[k].norm() for k in sd])
    assert torch.allclose(norms, fixture["grad_norms"], rtol=1e-5, atol=1e-9)


def test_the_kl_weight_is_visible_in_the_gradients(step, fixture):
    """At kl_weight = 1e-4 the KL term moves pre_quant_conv.weight's gradient by tens of percent (at the 5e-6 default
    by about 2 %, below what a cosine threshold of 0.99 sees): the gradient tests use 1e-4."""
    sd, (_, grads, _, _, _) = step
    _, plain, _, _, _ = VAO.train_grads(sd, SMALL_VQVAE, fixture["im"], fixture["eps"], 0.0)
    k = "pre_quant_conv.weight"
    moved = float((grads[k] - plain[k]).norm() / plain[k].norm())
    assert moved > 0.2, moved
