"""The KL autoencoder on the HIP path (models.vae, sdmi.vae_engine, sdmi.vae_train; reference models/vae.py).
SMALL_VQVAE, 64 x 64 images, B = 2; the reference's own step is tests/golden/vae_small.safetensors and the oracle
tests/vae_oracle.py (pinned to it by tests/test_oracle_vae.py).

* the module imports, registers the reference's 128 state-dict tensors, loads a state dict and raises off the GPU;
* encode draws torch.randn(mean.shape) on the CPU generator exactly once and leaves the device generator alone; the
  sample is the torch expression on the module's own encoder_output within the expf statement of tests/kl_matrix.py;
  decode(sample) is forward's reconstruction in eval mode;
* the moments against the reference's, to the VQVAE forward tolerance of the pre-quantisation latent (2e-2 rel. RMS);
* the training engine with the fused KL term at kl_weight = 1e-4 and the training module under the user's own torch
  KL loss (the dmom_add path), both against the oracle: per-parameter cosine >= 0.99, global norm within 5 %, recon
  within 2 %, KL within 5 % (the bounds of tests/test_vqvae_noise_gpu.py for this bf16 trunk);
* VAETrainer: a StepPlan replay is the eager step bit for bit, the draws are fresh and counted, the launch budget;
* the leaf path; wider latents raise."""
import ctypes
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import sd_oracle as O
from tests import kl_matrix as KM
from tests import vae_oracle as VAO
from tests.golden.configs import SMALL_VQVAE

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KL_WEIGHT, DRAW_SEED = 1e-4, 77


def cos(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def rrms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


@pytest.fixture(scope="module")
def fixture():
    return load_file(os.path.join(G, "vae_small.safetensors"))


@pytest.fixture(scope="module")
def state():
    return O.deterministic_state(VAO.param_shapes(), seed=9)


@pytest.fixture(scope="module")
def oracle(state, fixture):
    """The oracle's step with and without the KL term, computed once."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with_kl = VAO.train_grads(state, SMALL_VQVAE, fixture["im"], fixture["eps"], KL_WEIGHT)
    without = VAO.train_grads(state, SMALL_VQVAE, fixture["im"], fixture["eps"], 0.0)
    return with_kl, without


def _model(state):
    from models.vae import VAE
    m = VAE(3, SMALL_VQVAE)
    m.load_state_dict(state)
    return m.cuda()


def _kl(encoder_output):
    mean, logvar = torch.chunk(encoder_output, 2, dim=1)
    return torch.mean(0.5 * torch.sum(torch.exp(logvar) + mean ** 2 - 1 - logvar, dim=[1, 2, 3]))


def _held_to_oracle(got, losses_got, ref, what):
    losses, grads = ref[0], ref[1]
    rec, kl = losses["recon"].item(), losses["kl"].item()
    e_rec, e_kl = abs(losses_got["recon"] - rec) / rec, abs(losses_got["kl"] - kl) / kl
    worst = (1.0, None)
    for k, r in grads.items():
        gk = got[k].detach().cpu()
        assert torch.isfinite(gk).all(), k
        if r.norm() > 1e-6:
            worst = min(worst, (cos(gk, r), k))
    gn = torch.norm(torch.stack([got[k].detach().float().norm().cpu() for k in grads])).item()
    rn = torch.norm(torch.stack([grads[k].norm() for k in grads])).item()
    print(f"{what}: worst cosine {worst}, global norm {gn:.6f} vs {rn:.6f}, recon error {e_rec:.2e}, KL error {e_kl:.2e}")
    assert worst[0] >= 0.99, worst
    assert abs(gn - rn) <= 0.05 * rn, (gn, rn)
    assert e_rec <= 2e-2, (losses_got["recon"], rec)
    assert e_kl <= 5e-2, (losses_got["kl"], kl)


def test_import_and_surface(state):
    from models.vae import VAE
    m = VAE(3, SMALL_VQVAE)
    assert list(m.state_dict()) == list(VAO.param_shapes()) and len(m.state_dict()) == 128
    assert all(tuple(v.shape) == VAO.param_shapes()[k] for k, v in m.state_dict().items())
    m.load_state_dict(state)
    with pytest.raises(RuntimeError, match="HIP path only"):
        m.encode(torch.zeros(1, 3, 32, 32))
    wide = dict(SMALL_VQVAE, z_channels=8)
    with pytest.raises(ValueError, match="z_channels"):
        VAE(3, wide).cuda().encode(torch.zeros(1, 3, 32, 32, device="cuda"))


def test_encode_draws_once_on_the_cpu_generator(state, fixture):
    m = _model(state).eval()
    im = fixture["im"].cuda()
    torch.manual_seed(DRAW_SEED)                       # (seeds the device generator as well)
    dev_rng = torch.cuda.get_rng_state()
    sample, enc = m.encode(im)
    after = torch.get_rng_state()
    assert torch.equal(torch.cuda.get_rng_state(), dev_rng), "encode drew from the device generator"
    assert not sample.requires_grad and sample.shape == (2, 4, 16, 16) and enc.shape == (2, 8, 16, 16)
    torch.manual_seed(DRAW_SEED)
    eps = torch.randn(sample.shape)
    assert torch.equal(torch.get_rng_state(), after), "encode did not advance the CPU generator by exactly one draw"
    assert torch.equal(eps, fixture["eps"])
    mean, logvar = (t.cpu().double() for t in torch.chunk(enc, 2, dim=1))
    std = torch.exp(0.5 * logvar)
    want = mean + std * eps.double()
    # the kernel's std is within E_ULPS ulps of exp64; one rounding each for the product and the sum
    tol = (KM.E_ULPS + 1) * KM.ulp32(std) * eps.double().abs() + KM.ulp32(want)
    err = (sample.cpu().double() - want).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    with torch.no_grad():
        torch.manual_seed(DRAW_SEED)
        out, enc2 = m(im)
        assert torch.equal(enc2, enc) and torch.equal(m.decode(sample), out)
        # a second encode draws other noise: the generator moved on
        s2, _ = m.encode(im)
        assert not torch.equal(s2, sample)


def test_module_moments_vs_the_reference(state, fixture):
    m = _model(state).eval()
    torch.manual_seed(DRAW_SEED)
    with torch.no_grad():
        out, enc = m(fixture["im"].cuda())
    e_mom, e_out = rrms(enc, fixture["encoder_output"]), rrms(out, fixture["out"])
    print(f"moments rel RMS {e_mom:.3e}, reconstruction rel RMS {e_out:.3e}")
    assert e_mom <= 2e-2, e_mom


def test_training_engine_with_the_fused_kl_term(state, fixture, oracle):
    from sdmi import kernels as K
    from sdmi.vae_train import VAETrainEngine
    with_kl, without = oracle
    params = {k: v.cuda() for k, v in state.items()}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    eng = VAETrainEngine(SMALL_VQVAE, params, grads)
    eng.refresh_weights()
    im = fixture["im"].cuda()
    B, C, H, W = im.shape
    out, ctx = eng.forward(im, eps=fixture["eps"].cuda(), want_kl=True)
    dout, loss = eng.new_dpred(B, H, W), torch.zeros(1, device="cuda")
    K.mse(out, 8, im, B, C, H * W, 1.0, dout, loss)
    eng.backward(ctx, dout, KL_WEIGHT)
    torch.cuda.synchronize()
    _held_to_oracle(grads, dict(recon=loss.item(), kl=ctx["kl"].item()), with_kl, "fused KL")
    k = "pre_quant_conv.weight"
    g = grads[k].cpu()
    d_with, d_without = float((g - with_kl[1][k]).norm()), float((g - without[1][k]).norm())
    print(f"{k}: distance to the oracle with KL {d_with:.4e}, without {d_without:.4e}")
    assert d_with < d_without, "the fused KL term is not in the gradient"
    assert float(grads["post_quant_conv.weight"].abs().max()) > 0


def test_training_module_under_the_users_kl_loss(state, fixture, oracle):
    m = _model(state).train()
    im = fixture["im"].cuda()
    torch.manual_seed(DRAW_SEED)
    out, enc = m(im)
    assert out.requires_grad and enc.requires_grad
    recon = torch.nn.functional.mse_loss(out, im)
    kl = _kl(enc)
    (recon + KL_WEIGHT * kl).backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    _held_to_oracle(got, dict(recon=recon.item(), kl=kl.item()), oracle[0], "user KL")
    k = "pre_quant_conv.weight"
    g = got[k].cpu()
    assert float((g - oracle[0][1][k]).norm()) < float((g - oracle[1][1][k]).norm()), "dmom_add did not arrive"


def test_module_under_an_adam_loop(state, fixture):
    m = _model(state).train()
    opt = torch.optim.Adam(m.parameters(), lr=2e-5, betas=(0.5, 0.999))
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    im = fixture["im"].cuda()
    torch.manual_seed(3)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        out, enc = m(im)
        total = torch.nn.functional.mse_loss(out, im) + KL_WEIGHT * _kl(enc)
        total.backward()
        assert torch.isfinite(total)
        opt.step()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        has = p.grad != 0
        assert bool(has.any()), f"{k} has no gradient"
        moved = p.detach() != before[k]
        assert bool(moved.any()), f"{k} did not move"
        # element by element an Adam step may undo the one before it, to the bit, but rarely
        assert float(moved[has].float().mean()) >= 0.99, k


def _trainer(state, **kw):
    from sdmi.vae_train import VAETrainer
    return VAETrainer(SMALL_VQVAE, {k: v.cuda() for k, v in state.items()}, "cuda", **kw)


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


def test_trainer_plan_replay_matches_eager_and_the_launch_budget(state, fixture):
    from sdmi.plan import StepPlan
    from sdmi.vae_train import noise_key
    im = fixture["im"].cuda()
    a = _trainer(state, kl_weight=KL_WEIGHT, noise_seed=3)
    b = _trainer(state, kl_weight=KL_WEIGHT, noise_seed=3)
    assert a.noise_key == noise_key(3, 0) and a.kl_weight == KL_WEIGHT
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
    assert abs(float(e1.mean())) < 0.1 and abs(float(e1.std()) - 1.0) < 0.1
    c = _trainer(state, kl_weight=KL_WEIGHT, noise_seed=4)
    c.step(im)
    assert not torch.equal(c.eps, e1)
    # the losses, and the sample as the torch expression on the trainer's own moments and draw
    got = c.losses()
    assert set(got) == {"recon", "kl", "total"} and abs(got["total"] - got["recon"] - got["kl"]) <= 1e-6 * got["total"]
    assert abs(got["kl"] - KL_WEIGHT * float(_kl(c.moments))) <= 1e-3 * got["kl"]
    assert c.reconstruction().shape == im.shape
    names = _kernels(plan)
    for fragment in ("vq_", "pointwise_in", "latent_"):
        assert _count(names, fragment) == 0, fragment
    assert _count(names, "randn_kernel") == 1 and _count(names, "advance_kernel") == 1
    assert _count(names, "kl_sample") == 1 and _count(names, "kl_loss") <= 1 and _count(names, "kl_bwd") == 2
    print(f"recorded VAETrainer step: {len(names)} launches")


def test_leaf_path(state):
    m = _model(state)
    m.sdmi_leaf_path = True
    im = (torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    torch.manual_seed(17)
    out, enc = m(im)
    torch.manual_seed(17)
    sample, enc2 = m.encode(im)
    torch.manual_seed(17)
    eps = torch.randn(sample.shape)
    assert torch.equal(enc2, enc) and sample.requires_grad
    mean, logvar = (t.detach().cpu().double() for t in torch.chunk(enc, 2, dim=1))
    std = torch.exp(0.5 * logvar)
    want = mean + std * eps.double()
    tol = (KM.E_ULPS + 1) * KM.ulp32(std) * eps.double().abs() + KM.ulp32(want)
    assert bool(((sample.detach().cpu().double() - want).abs() <= tol).all())
    m.zero_grad()
    torch.nn.functional.mse_loss(out, im).backward()
    g = dict(m.named_parameters())["encoder_conv_in.weight"].grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
