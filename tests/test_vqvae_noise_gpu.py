"""The noise-robust VQVAE on the HIP path (models.vqvae_noise, sdmi.vqvae_train n_scale; reference
models/vqvae_noise.py and train_vqvae_celebhq_noise_multi_GPU.py:554-580 without LPIPS / GAN). SMALL_VQVAE, 64 x 64
images, B = 2.

* the module at n_scale = 0 is models.vqvae.VQVAE bit for bit and draws nothing;
* at n_scale = 0.2 the returned z is bitwise the torch expression on the module's own clean latent and the re-drawn
  randn_like (inference and training path, float and 0-dim tensor n_scale);
* add_noise on a (3, 5, 7) tensor with planted ties: the value bitwise, the gradient against torch autograd;
* the engine's gradients of every parameter against the composed oracle (tests/noise_oracle.py, pinned to the
  reference's own step by tests/test_oracle_vqvae_noise.py) given the engine's own code indices and its own extremal
  positions -- bf16 activations: per-parameter cosine >= 0.99, the global norm within 5 %, code agreement >= 0.8;
* VQVAETrainer(n_scale=0.2, noise_seed=3): the recorded plan replays the eager step bit-identically, consecutive steps
  draw different noise, the launch counts are the budget's, and the defaults launch what they always did;
* the module under the noise trainer's loop lines: two Adam steps, every parameter with a gradient moves."""
import ctypes
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import sd_oracle as O
from oracle import vqvae_oracle as VO
from tests import noise_matrix as NM
from tests import noise_oracle as NO
from tests.golden.configs import SMALL_VQVAE

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cos(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def fixture():
    return load_file(os.path.join(G, "vqvae_noise.safetensors"))


@pytest.fixture(scope="module")
def state():
    return O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=9)


def _models(state):
    from models.vqvae import VQVAE as Clean
    from models.vqvae_noise import VQVAE as Noisy
    clean, noisy = Clean(3, SMALL_VQVAE).cuda(), Noisy(3, SMALL_VQVAE).cuda()
    clean.load_state_dict(state)
    noisy.load_state_dict(state)
    return clean, noisy


def _expression(zq, n_scale, seed):
    """vqvae_noise.py:177-183 in torch on the device, after reseeding: the draw the module made."""
    torch.manual_seed(seed)
    return zq + (zq.max() - zq.min()) * n_scale * torch.randn_like(zq)


def test_module_at_zero_scale_is_the_clean_module(state, fixture):
    clean, noisy = _models(state)
    im = fixture["im"].cuda()
    torch.manual_seed(5)
    rng = torch.cuda.get_rng_state()
    with torch.no_grad():
        a = clean(im)
        b = noisy(im, 0.0)
        c = noisy(im)
        zb, lb = noisy.encode(im, torch.tensor(0.0))
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
        assert torch.equal(a[2]["codebook_loss"], x[2]["codebook_loss"])
    assert torch.equal(zb, a[1]) and torch.equal(lb["commitment_loss"], a[2]["commitment_loss"])
    clean.train()
    noisy.train()
    ta, tb = clean(im), noisy(im, 0.0)
    assert tb[0].requires_grad and torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1])
    assert torch.equal(ta[2]["codebook_loss"], tb[2]["codebook_loss"])
    assert torch.equal(torch.cuda.get_rng_state(), rng), "n_scale = 0 drew from the device generator"


def test_module_noise_is_the_torch_expression(state, fixture):
    clean, noisy = _models(state)
    im = fixture["im"].cuda()
    with torch.no_grad():
        zq, ql = clean.encode(im)
        torch.manual_seed(11)
        z, qn = noisy.encode(im, 0.2)
        want = _expression(zq, 0.2, 11)
        assert torch.equal(z, want) and not torch.equal(z, zq)
        assert torch.equal(qn["codebook_loss"], ql["codebook_loss"])      # the losses are the clean latent's
        # a 0-dim tensor n_scale (the reference iterates over a linspace), through forward
        ns = torch.linspace(0.0, 0.2, 3)[2]
        torch.manual_seed(12)
        out, z2, _ = noisy(im, ns)
        assert torch.equal(z2, _expression(zq, float(ns), 12))
        assert torch.equal(out, clean.decode(z2))
        # exactly one draw of the latent's shape per call
        torch.manual_seed(12)
        torch.randn_like(zq)
        after = torch.cuda.get_rng_state()
        torch.manual_seed(12)
        noisy(im, ns)
        assert torch.equal(torch.cuda.get_rng_state(), after)
    # the training path: one autograd Function; z is the noisy latent of ITS clean latent
    noisy.train()
    zq_t = noisy(im, 0.0)[1].detach()
    torch.manual_seed(13)
    out, z3, ql3 = noisy(im, 0.2)
    assert out.requires_grad and z3.requires_grad and ql3["codebook_loss"].requires_grad
    assert torch.equal(z3.detach(), _expression(zq_t, 0.2, 13))


def test_add_noise_value_and_gradient():
    """The value is bitwise the torch expression. The gradient is g + corr with corr = n_scale S / count at the
    extremes: our S and torch's each lie within K_S u T of the exact sum (T = sum |g eps|), so the two corr differ by at
    most n_scale 2 K_S u T (count >= 1), plus the roundings of the product, the quotient and the final add, 2^-22 (|g|
    + |corr|), plus -- where an element is both extremes and autograd adds and subtracts its two shares one after the
    other -- the rounding of that intermediate, 2^-22 n_scale T. Away from the extremes r is g bitwise."""
    from models.vqvae_noise import add_noise
    gen = torch.Generator().manual_seed(8)
    for ties in ((1, 1), (2, 3), (105, 105)):
        w0 = torch.randn(3, 5, 7, generator=gen)
        flat = w0.reshape(-1)
        if ties == (105, 105):
            flat.fill_(-1.25)
        else:
            perm = torch.randperm(105, generator=gen)
            flat[perm[:ties[0]]] = 5.0
            flat[perm[ties[0]:ties[0] + ties[1]]] = -5.0
        g = torch.randn(3, 5, 7, generator=gen).cuda()
        for ns in (0.074, 0.2):
            w = w0.clone().cuda().requires_grad_(True)
            torch.manual_seed(21)
            out = add_noise(w, ns) if ns != 0.074 else add_noise(w)
            torch.manual_seed(21)
            eps = torch.randn_like(w)
            wt = w0.clone().cuda().requires_grad_(True)
            ref = wt + (wt.max() - wt.min()) * ns * eps
            assert torch.equal(out.detach(), ref.detach()), (ties, ns)
            (out * g).sum().backward()
            (ref * g).sum().backward()
            T = float((g.double() * eps.double()).abs().sum())
            at_max, at_min = (w0 == w0.max()).cuda(), (w0 == w0.min()).cuda()
            assert (int(at_max.sum()), int(at_min.sum())) == ties
            corr = (wt.grad - g).abs().double()
            tol = ns * T * (2 * NM.K_S * NM.U24 + 2.0 ** -22) + 2.0 ** -22 * (g.abs().double() + corr)
            tol = torch.where(at_max | at_min, tol, torch.zeros_like(tol))      # elsewhere r == g bitwise
            err = (w.grad - wt.grad).abs().double()
            assert bool((err <= tol).all()), (ties, ns, float((err / tol.clamp_min(1e-300)).max()))
            assert ties[0] > 1 or int((w.grad != g).sum()) == 2        # the spike sits on the two extremes
    w = torch.ones(4, device="cuda")
    assert add_noise(w, 0) is w and add_noise(w, torch.tensor(0.0)) is w


def _trainer(state, **kw):
    from sdmi.vqvae_train import VQVAETrainer
    return VQVAETrainer(SMALL_VQVAE, {k: v.cuda() for k, v in state.items()}, "cuda", **kw)


def test_engine_gradients_vs_composed_oracle(state, fixture):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    tr = _trainer(state, n_scale=0.2, noise_seed=3)
    im = fixture["im"]
    tr.step(im.cuda())
    torch.cuda.synchronize()
    # the trainer's latent is the torch expression on its own clean latent and its own draw
    assert torch.equal(tr.z, tr.zq + (tr.zq.max() - tr.zq.min()) * 0.2 * tr.eps)
    idx, zq, eps = tr.indices.cpu(), tr.zq.cpu(), tr.eps.cpu()
    agree = (idx == fixture["indices"]).float().mean().item()
    assert agree >= 0.8, agree
    assert abs(float(eps.mean())) < 0.1 and abs(float(eps.std()) - 1.0) < 0.1
    # the oracle at the engine's code indices and at the engine's extremal positions
    masks = (zq == zq.max(), zq == zq.min())
    losses, grads, out, _, _, _ = NO.train_grads(state, SMALL_VQVAE, im, 0.2, eps, indices=idx, masks=masks)
    got = tr.losses()
    assert abs(got["recon"] - losses["recon"].item()) <= 2e-2 * losses["recon"].item()
    assert abs(got["codebook"] - losses["codebook"].item()) <= 5e-2 * losses["codebook"].item()
    worst = (1.0, None)
    for k in state:
        r, gk = grads[k], tr.store.g[k].cpu()
        assert torch.isfinite(gk).all(), k
        if r.norm() > 1e-6:
            worst = min(worst, (cos(gk, r), k))
    gn = torch.norm(torch.stack([tr.store.g[k].norm() for k in state])).item()
    rn = torch.norm(torch.stack([grads[k].norm() for k in state])).item()
    print(f"worst cosine {worst}, global norm {gn:.6f} vs {rn:.6f}, code agreement {agree:.3f}")
    assert worst[0] >= 0.99, worst
    assert abs(gn - rn) <= 0.05 * rn, (gn, rn)


def _kernels(plan):
    """The kernel names of a recorded StepPlan, in order."""
    from sdmi import _lib
    L = _lib.lib()
    n = ctypes.c_int()
    assert L.sdmi_plan_info(plan.handle, ctypes.byref(n), None) == 0
    kind, name, grid = ctypes.c_int(), ctypes.c_char_p(), (ctypes.c_int * 3)()
    out = []
    for i in range(n.value):
        assert L.sdmi_plan_op_info(plan.handle, i, ctypes.byref(kind), ctypes.byref(name), grid, None, None) == 0
        if kind.value == 0:
            out.append(name.value.decode(errors="replace") if name.value else "?")
    return out


def _count(names, fragment):
    return sum(fragment in n for n in names)


def test_noise_key_is_seed_plus_rank():
    from sdmi.vqvae_train import noise_key
    assert noise_key(3) == 3 and noise_key(3, 0) == 3 and noise_key(3, 5) == 8
    assert noise_key(2 ** 64 - 1, 2) == 1
    assert len({noise_key(7, r) for r in range(8)}) == 8


def test_trainer_plan_replay_matches_eager_and_draws_fresh_noise(state, fixture):
    from sdmi.plan import StepPlan
    from sdmi.vqvae_train import noise_key
    im = fixture["im"].cuda()
    a = _trainer(state, n_scale=0.2, noise_seed=3)
    b = _trainer(state, n_scale=0.2, noise_seed=3)
    assert a.noise_key == noise_key(3, 0) and a.n_scale == 0.2
    assert list(a.state_dict()) == list(state)
    a.step(im)
    b.step(im)
    e1 = b.eps.clone()
    plan = StepPlan(lambda: a.step(im))
    b.step(im)
    e2 = b.eps.clone()
    plan.replay()
    b.step(im)
    torch.cuda.synchronize()
    assert torch.equal(a.store.params, b.store.params)
    assert torch.equal(a.store.grads, b.store.grads)
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert torch.equal(a.eps, b.eps), "the replay did not draw the eager step's noise"
    assert not torch.equal(e1, e2) and not torch.equal(e2, b.eps), "consecutive steps drew the same noise"
    assert int(a.noise_offset) == 3 and int(b.noise_offset) == 3
    # another seed draws other noise
    c = _trainer(state, n_scale=0.2, noise_seed=4)
    c.step(im)
    assert not torch.equal(c.eps, e1)
    # the launch budget inside the step: sdmi_randn (the draw and the advance of its device offset) + range + one
    # forward launch in place of the pointwise, two backward
    names = _kernels(plan)
    d = _trainer(state)
    assert d.noise_offset is None and d.n_scale == 0.0
    d.step(im)
    base = _kernels(StepPlan(lambda: d.step(im)))
    assert d.noise_offset is None and d.eps is None
    assert _count(base, "latent_") == 0 and _count(base, "randn") == 0 and _count(base, "pointwise_in_kernel") == 1
    assert _count(names, "pointwise_in_kernel") == 0
    for fragment in ("latent_range_kernel", NM.fwd_name(1), "latent_noise_dot_kernel", "latent_noise_bwd_kernel"):
        assert _count(names, fragment) == 1, fragment
    assert _count(names, "randn_kernel") == 1 and _count(names, "advance_kernel") == 1
    assert _count(names, "latent_") == 4 and len(names) == len(base) + 5, (len(names), len(base))
    # n_scale is settable (the staged schedule); back at 0 the step is the default one
    a.n_scale = 0.0
    a.step(im)
    assert a.eps is None and int(a.noise_offset) == 3


def test_module_under_the_noise_trainer_loop(state, fixture):
    """train_vqvae_celebhq_noise_multi_GPU.py:554-580 without LPIPS / GAN: output, _, quantize_losses =
    vqvae(im, n_scale); recon + codebook_weight * codebook + commitment_beta * commitment; backward; Adam step."""
    _, model = _models(state)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=2e-5, betas=(0.5, 0.999))
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    im = fixture["im"].cuda()
    torch.manual_seed(3)
    for n_scale in torch.linspace(0.1, 0.2, 2):
        opt.zero_grad(set_to_none=True)
        output, _, quantize_losses = model(im, n_scale)
        recon_loss = torch.nn.functional.mse_loss(output, im)
        codebook_loss = 1.0 * quantize_losses["codebook_loss"]
        commitment_loss = 0.2 * quantize_losses["commitment_loss"]
        total_generator_loss = recon_loss + codebook_loss + commitment_loss
        total_generator_loss.backward()
        assert torch.isfinite(total_generator_loss)
        opt.step()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        has = p.grad != 0
        assert bool(has.any()), f"{k} has no gradient"
        moved = p.detach() != before[k]
        assert bool(moved.any()), f"{k} did not move"
        # element by element an Adam step may undo the one before it, to the bit, but rarely
        assert float(moved[has].float().mean()) >= 0.99, k


def test_leaf_path_goes_through_add_noise(state):
    """sdmi_leaf_path: encode -> add_noise (the autograd Function over the three kernels) -> decode, leaf by leaf. The
    noisy latent is the torch expression on the leaf path's own clean latent and its gradient reaches the encoder
    through the range as well."""
    _, model = _models(state)
    model.sdmi_leaf_path = True
    im = (torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    zq = model(im, 0.0)[1].detach()
    torch.manual_seed(17)
    out, z, ql = model(im, 0.2)
    assert torch.equal(z.detach(), _expression(zq, 0.2, 17))
    torch.manual_seed(17)
    eps = torch.randn_like(zq)
    # an upstream gradient correlated with eps, so that S = sum(g eps) is about n / 4 = 64 and the spike 0.2 S stands
    # well above the unit-variance rest
    g = torch.randn(z.shape, generator=torch.Generator().manual_seed(4)).cuda() + 0.25 * eps
    r = NO.closed_form(zq.double(), g.double(), eps.double(), 0.2).float()
    assert float((r - g).norm() / g.norm()) > 0.05, "the case cannot see the range term"

    def encoder_grad(latent, upstream):
        model.zero_grad()
        (latent * upstream).sum().backward()
        return dict(model.named_parameters())["pre_quant_conv.weight"].grad.clone()

    # the noisy latent under g pulls on the encoder as the clean latent does under the closed-form gradient r
    # (the leaf quantiser hands its latent gradient on in bf16: 2^-9 relative per element)
    got = encoder_grad(z, g)
    want = encoder_grad(model(im, 0.0)[1], r)
    plain = encoder_grad(model(im, 0.0)[1], g)
    assert float((got - want).norm() / want.norm()) <= 1e-2, (got, want)
    assert float((got - plain).norm() / want.norm()) > 0.03, "the range term did not reach the encoder"
