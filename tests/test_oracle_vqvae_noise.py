"""Pins the oracle composition of the noise-robust autoencoder's training step (tests/noise_oracle.py: the unchanged
oracle/vqvae_oracle.py around z = zq + (max - min) n_scale eps, with autograd) against the reference's own step
(tests/golden/vqvae_noise.safetensors, written by tests/golden/make_golden_vqvae_noise.py from the reference
models/vqvae_noise.py). CPU only. Tolerances are those of tests/test_oracle_vqvae.py.

Also the closed-form gradient of the range term -- the tie rule included -- against torch autograd on planted ties."""
import inspect
import os

import pytest
import torch
from safetensors.torch import load_file

import models.vqvae_noise as MN
from oracle import sd_oracle as O
from oracle import vqvae_oracle as VO
from tests import noise_oracle as NO
from tests.golden.configs import SMALL_VQVAE

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def test_noise_train_step_against_the_reference():
    f = load_file(os.path.join(G, "vqvae_noise.safetensors"))
    assert os.path.getsize(os.path.join(G, "vqvae_noise.safetensors")) < 2 ** 20
    sd = O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=9)
    n_scale = float(f["n_scale"])
    assert n_scale == pytest.approx(0.2)
    losses, grads, out, idx, zq, z = NO.train_grads(sd, SMALL_VQVAE, f["im"], n_scale, f["eps"])
    assert torch.equal(idx, f["indices"])
    assert rel(zq, f["zq"]) <= 1e-5 and rel(z, f["z"]) <= 1e-5
    # the fixture's own noisy latent is the torch expression on its clean one, bit for bit
    assert torch.equal(f["z"], f["zq"] + (f["zq"].max() - f["zq"].min()) * n_scale * f["eps"])
    assert not torch.equal(f["z"], f["zq"])
    for k in ("recon", "codebook", "commitment"):
        assert rel(losses[k].reshape(1), f[k]) <= 1e-5, k
    assert rel(out, f["out"]) <= 1e-5
    norms = torch.stack([grads[k].norm() for k in sd])
    assert ((norms - f["grad_norms"]).abs() <= 1e-4 * f["grad_norms"] + 1e-9).all()
    checked = 0
    for k in sd:
        if "grad." + k in f:
            assert rel(grads[k].reshape(-1)[:8192], f["grad." + k]) <= 1e-4, k
            checked += 1
    assert checked >= 20


def test_masks_at_the_oracles_own_extremes_change_nothing():
    """Routing the range gradient through masks of the clean latent's own extremal positions is the plain range."""
    f = load_file(os.path.join(G, "vqvae_noise.safetensors"))
    sd = O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=9)
    zq = f["zq"]
    masks = (zq == zq.max(), zq == zq.min())
    a = NO.train_grads(sd, SMALL_VQVAE, f["im"], 0.2, f["eps"])
    b = NO.train_grads(sd, SMALL_VQVAE, f["im"], 0.2, f["eps"], masks=masks)
    assert rel(b[5], a[5]) <= 1e-6              # (routed + (w - routed) may round once more than w)
    for k in sd:
        assert rel(b[1][k], a[1][k]) <= 1e-5 or a[1][k].norm() == 0, k


def test_the_range_term_matters_in_the_fixture():
    """The spike n_scale * sum(g * eps) at the two extremes is a visible share of the latent gradient: a composition
    that detached the range would not meet the gradient tolerances above."""
    f = load_file(os.path.join(G, "vqvae_noise.safetensors"))
    sd = O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=9)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    zq = f["zq"].clone().requires_grad_(True)
    out = VO.decode(p, SMALL_VQVAE, zq + (zq.max() - zq.min()) * 0.2 * f["eps"])
    torch.nn.functional.mse_loss(out, f["im"]).backward()
    with_range = zq.grad.clone()
    zq.grad = None
    out = VO.decode(p, SMALL_VQVAE, zq + (zq.max() - zq.min()).detach() * 0.2 * f["eps"])
    torch.nn.functional.mse_loss(out, f["im"]).backward()
    spike = (with_range - zq.grad).norm() / with_range.norm()
    print(f"the range term carries {float(spike):.3f} of the latent gradient's norm")
    assert spike > 0.02
    assert torch.allclose(with_range, NO.closed_form(f["zq"], zq.grad, f["eps"], 0.2), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_closed_form_gradient_with_planted_ties(dtype):
    x = torch.tensor([1.0, 3.0, 3.0, -2.0, -2.0, -2.0, 0.0], requires_grad=True)
    (x.max() - x.min()).backward()
    assert torch.allclose(x.grad, torch.tensor([0, .5, .5, -1 / 3, -1 / 3, -1 / 3, 0]), atol=1.5e-8)
    gen = torch.Generator().manual_seed(4)
    for shape, ties in (((3, 5, 7), (2, 3)), ((2, 4, 16, 16), (4, 1)), ((1, 1, 9), (1, 1)), ((6,), (6, 6))):
        z0 = torch.randn(shape, generator=gen, dtype=dtype)
        flat = z0.reshape(-1)
        if ties == (6, 6):
            flat.fill_(0.75)                     # all equal: every element is both extremes and the range term cancels
        else:
            perm = torch.randperm(flat.numel(), generator=gen)
            flat[perm[:ties[0]]] = 5.0
            flat[perm[ties[0]:ties[0] + ties[1]]] = -5.0
        eps, g = (torch.randn(shape, generator=gen, dtype=dtype) for _ in range(2))
        z = z0.clone().requires_grad_(True)
        ((z + (z.max() - z.min()) * 0.2 * eps) * g).sum().backward()
        want = NO.closed_form(z0, g, eps, 0.2)
        tol = 1e-12 if dtype == torch.float64 else 2e-6
        assert torch.allclose(z.grad, want, rtol=tol, atol=tol * float(g.abs().max())), (shape, ties)
        if ties == (6, 6):
            assert torch.allclose(want, g, rtol=tol, atol=tol)


def test_module_surface():
    from models.vqvae import VQVAE as Clean
    Noisy, add_noise = MN.VQVAE, MN.add_noise
    m = Noisy(3, SMALL_VQVAE)
    assert isinstance(m, Clean) and list(m.state_dict()) == list(Clean(3, SMALL_VQVAE).state_dict())
    assert list(m.state_dict()) == list(VO.vqvae_param_shapes(SMALL_VQVAE))
    assert inspect.signature(m.encode).parameters["n_scale"].default is inspect.Parameter.empty
    assert inspect.signature(m.forward).parameters["n_scale"].default == 0.0
    assert inspect.signature(add_noise).parameters["n_scale"].default == 0.074
    with pytest.raises(TypeError):
        m.encode(torch.zeros(1, 3, 64, 64))
