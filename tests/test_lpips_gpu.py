"""LPIPS on the HIP path end to end (sdmi.lpips_engine, models.lpips, VQVAETrainer's LPIPS term) against the plain-torch
restatement of the metric on the CPU (tests/lpips_ref.py), with seeded weights.

Tolerances of the metric itself are measured, not fixed: the restatement run once more on the CPU at bf16 (weights and
activations) gives the reference's own bf16 error against fp32 -- e_val (relative error of val, the worst sample of
the batch: one sample's rounding error is a random draw, the worst one measures its scale) and e_cos (1 - cosine of an
input gradient). The HIP path rounds to bf16 once per layer like that run, at different points, hence the factor 3:
err_val <= 3 e_val, 1 - cos <= 3 e_cos; gradient norms within 5 %, the project's usual bound."""
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from oracle import sd_oracle as O
from oracle import vqvae_oracle as VO
from tests import lpips_ref as R
from tests.golden.configs import SMALL_VQVAE

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(2, 32, 32), (1, 40, 40), (2, 32, 48)]  # 40: the last pool floors 5 -> 2; 48: not square


def _module():
    from models.lpips import LPIPS
    m = LPIPS()
    m.load_state_dict(R.seeded_state())
    return m.cuda()


def _check(tag, val, grads, ref):
    """val (B,) and {0 / 1: input gradient} of mean_b val against the fp32 restatement, by the measured rule."""
    err = ((val.cpu() - ref["val"]).abs() / ref["val"].abs()).max().item()
    msg = f"{tag}: err_val {err:.3e} (e_val {ref['e_val']:.3e})"
    for side, g in grads.items():
        r, e_cos = ref[f"g{side}"], ref[f"e_cos{side}"]
        c, ratio = 1 - R.cos(g.cpu(), r), (g.norm().item() / r.norm().item())
        msg += f"; in{side}: 1-cos {c:.3e} (e_cos {e_cos:.3e}), norm ratio {ratio:.4f}"
    print(msg)
    assert err <= 3 * ref["e_val"], msg
    for side, g in grads.items():
        r = ref[f"g{side}"]
        assert torch.isfinite(g).all()
        assert 1 - R.cos(g.cpu(), r) <= 3 * ref[f"e_cos{side}"], msg
        assert abs(g.norm().item() - r.norm().item()) <= 0.05 * r.norm().item(), msg


@pytest.mark.parametrize("shape,which", [(SHAPES[0], "in0"), (SHAPES[1], "in0"), (SHAPES[2], "in0"),
                                         (SHAPES[0], "both"), (SHAPES[1], "in1")])
def test_module_vs_fp32_restatement(shape, which):
    ref = R.reference(*shape)
    m = _module()
    a = ref["out"].cuda().requires_grad_(which in ("in0", "both"))
    b = ref["im"].cuda().requires_grad_(which in ("in1", "both"))
    val = m(a, b)
    assert val.shape == (shape[0], 1, 1, 1)
    torch.mean(val).backward()
    grads = {s: t.grad for s, t in ((0, a), (1, b)) if t.requires_grad}
    assert (a.grad is None) == (which == "in1") and (b.grad is None) == (which == "in0")
    _check(f"module {shape} {which}", val.detach().reshape(-1), grads, ref)


def test_engine_matches_module_bitwise_and_serves_one_half_only():
    """The engine called directly (dval on the device, both halves) gives the module's numbers bit for bit, and the
    gradient of in0 does not depend on whether in1's was also asked for."""
    from sdmi.lpips_engine import LPIPSEngine
    shape = SHAPES[2]
    ref = R.reference(*shape)
    B = shape[0]
    eng = LPIPSEngine({k: v.cuda() for k, v in R.seeded_state().items()}, "cuda")
    a, b = ref["out"].cuda(), ref["im"].cuda()
    val, ctx = eng.forward(a, b)
    dval = torch.full((B,), 1.0 / B, device="cuda")
    g0, g1 = eng.backward(ctx, dval, want=(True, True))
    h0, none = eng.backward(ctx, None, want=(True, False), gscale=1.0 / B)
    assert none is None and torch.equal(g0, h0)
    _check(f"engine {shape}", val, {0: g0, 1: g1}, ref)
    m = _module()
    a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    v2 = m(a2, b2)
    torch.mean(v2).backward()
    assert torch.equal(v2.reshape(-1), val) and torch.equal(a2.grad, g0) and torch.equal(b2.grad, g1)
    v3, c3 = eng.forward(a, b, need_backward=False)
    assert c3 is None and torch.equal(v3, val)


def test_normalize_flag_and_small_images():
    """normalize maps [0, 1] images to [-1, 1] first (lpips.py:112-114): same value, twice the gradient."""
    ref = R.reference(*SHAPES[0])
    m = _module()
    a = ref["out"].cuda().requires_grad_(True)
    a01 = ((ref["out"] + 1) / 2).cuda().requires_grad_(True)
    b = ref["im"].cuda()
    v = m(a, b)
    v01 = m(a01, (b + 1) / 2, normalize=True)
    v.mean().backward()
    v01.mean().backward()
    assert torch.allclose(v01, v, rtol=3 * ref["e_val"], atol=0)
    assert R.cos(a01.grad, a.grad) >= 1 - 3 * ref["e_cos0"]
    assert abs(a01.grad.norm().item() - 2 * a.grad.norm().item()) <= 0.05 * 2 * a.grad.norm().item()
    with pytest.raises(ValueError, match="at least 16 x 16"):
        m(torch.zeros(1, 3, 12, 32, device="cuda"), torch.zeros(1, 3, 12, 32, device="cuda"))


def test_metric_properties():
    ref = R.reference(*SHAPES[0])
    m = _module()
    x = ref["out"].cuda().requires_grad_(True)
    v = m(x, x.detach().clone())
    v.sum().backward()
    assert (v == 0).all() and (x.grad == 0).all()
    a, b = ref["out"].cuda(), ref["im"].cuda()
    a1, a2 = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    v1, v2 = m(a1, b), m(a2, b)
    v1.mean().backward()
    v2.mean().backward()
    assert torch.equal(v1, v2) and torch.equal(a1.grad, a2.grad)
    assert (v1 > 0).all()


# ---- trainer ---------------------------------------------------------------------------------------------------------
def _trainer(seed=9, **kw):
    from sdmi.vqvae_train import VQVAETrainer
    sd = O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=seed)
    return VQVAETrainer(SMALL_VQVAE, {k: v.cuda() for k, v in sd.items()}, "cuda", **kw), sd


def _lpips_kw():
    return dict(perceptual_weight=1.0, lpips_state={k: v.cuda() for k, v in R.seeded_state().items()})


def test_default_trainer_holds_no_lpips_engine():
    tr, _ = _trainer()
    assert tr.lpips is None
    tr, _ = _trainer(perceptual_weight=0.0, lpips_state=R.seeded_state())
    assert tr.lpips is None
    with pytest.raises(ValueError, match="lpips_state"):
        _trainer(perceptual_weight=1.0)
    im = load_file(os.path.join(G, "vqvae_train.safetensors"))["s0.im"].cuda()
    tr.step(im)
    assert list(tr.losses()) == ["recon", "codebook", "commitment", "total"]


def test_trainer_with_lpips_vs_oracle():
    """Gradients of recon + codebook + 0.2 commitment + 1.0 mean(LPIPS(out, im)) against the oracle VQVAE (given the
    engine's own code choice) + the restatement, to the bounds of test_engine_gradients_vs_oracle. The perceptual
    loss is held to the 3 e_val rule on the trainer's own reconstruction: the rule measures the LPIPS arithmetic, so
    the HIP path, the fp32 restatement and the bf16 restatement all see the same two images."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    f = load_file(os.path.join(G, "vqvae_train.safetensors"))
    lsd = R.seeded_state()
    tr, sd = _trainer(**_lpips_kw())
    im = f["s0.im"]
    tr.step(im.cuda())
    torch.cuda.synchronize()
    idx = tr.indices.cpu()
    got = tr.losses()
    assert list(got) == ["recon", "codebook", "commitment", "total", "perceptual"]
    assert got["total"] == pytest.approx(got["recon"] + got["codebook"] + got["commitment"] + got["perceptual"])
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    zq, cb, cm, _ = VO.quantize_train(p, VO.encode_pre_quant(p, SMALL_VQVAE, im), idx)
    out = VO.decode(p, SMALL_VQVAE, zq)
    recon = F.mse_loss(out, im)
    perc = R.lpips(lsd, out, im).mean()
    (recon + cb + 0.2 * cm + 1.0 * perc).backward()
    assert abs(got["recon"] - recon.item()) <= 2e-2 * recon.item()
    mine = tr.reconstruction().cpu()
    v32 = R.lpips(lsd, mine, im).mean().item()
    v16 = R.lpips(lsd, mine, im, dtype=torch.bfloat16).mean().item()
    e_val = abs(v16 - v32) / v32
    err = abs(got["perceptual"] - v32) / v32
    print(f"trainer perceptual {got['perceptual']:.6f}, restatement on the same reconstruction {v32:.6f} "
          f"(err {err:.3e}, e_val {e_val:.3e}); on the oracle's reconstruction {perc.item():.6f}")
    worst = (1.0, None)
    for k in sd:
        r, gk = p[k].grad, tr.store.g[k].cpu()
        assert torch.isfinite(gk).all(), k
        if r is not None and r.norm() > 1e-6:
            worst = min(worst, (R.cos(gk, r), k))
    gn = torch.norm(torch.stack([tr.store.g[k].norm() for k in sd])).item()
    rn = torch.norm(torch.stack([p[k].grad.norm() for k in sd if p[k].grad is not None])).item()
    print(f"worst parameter-gradient cosine {worst}, global norm {gn:.5f} vs {rn:.5f}")
    assert worst[0] >= 0.99, worst
    assert abs(gn - rn) <= 0.05 * rn, (gn, rn)
    assert err <= 3 * e_val, (got["perceptual"], v32, e_val)


def test_lpips_step_plan_replay_matches_eager():
    from sdmi.plan import StepPlan
    f = load_file(os.path.join(G, "vqvae_train.safetensors"))
    im = f["s0.im"].cuda()
    a, _ = _trainer(**_lpips_kw())
    b, _ = _trainer(**_lpips_kw())
    a.step(im)
    b.step(im)
    plan = StepPlan(lambda: a.step(im))
    b.step(im)
    plan.replay()
    b.step(im)
    torch.cuda.synchronize()
    assert torch.equal(a.store.params, b.store.params)
    assert torch.equal(a.store.grads, b.store.grads)
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert torch.equal(a.lp_loss, b.lp_loss)


def test_reference_loop_on_the_modules_matches_native_trainer():
    """train_vqvae_celebhq.py:414-441 without the GAN term on the two drop-in modules: out, z, losses = vqvae(im);
    total = MSE + codebook + 0.2 commitment + 1.0 mean(lpips(out, im)); total.backward() -- the gradients equal the
    native trainer's to the bound of test_module_under_reference_trainer_loop."""
    from models.vqvae import VQVAE
    f = load_file(os.path.join(G, "vqvae_train.safetensors"))
    sd = O.deterministic_state(VO.vqvae_param_shapes(SMALL_VQVAE), seed=9)
    model = VQVAE(3, SMALL_VQVAE).cuda()
    model.load_state_dict(sd)
    model.train()
    lp = _module()
    im = f["s0.im"].cuda()
    output, z, ql = model(im)
    lpips_loss = torch.mean(lp(output, im))
    total = F.mse_loss(output, im) + 1.0 * ql["codebook_loss"] + 0.2 * ql["commitment_loss"] + 1.0 * lpips_loss
    total.backward()
    tr, _ = _trainer(**_lpips_kw())
    tr.step(im)
    # the same engine on the same reconstruction; only the mean over the two samples is formed in another place
    assert abs(lpips_loss.item() - tr.losses()["perceptual"]) <= 1e-5 * lpips_loss.item()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if tr.store.g[k].norm() > 1e-6:
            assert R.cos(p.grad, tr.store.g[k]) >= 0.999, k
