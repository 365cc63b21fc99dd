"""Classifier-free guidance in the captured DDPM / DDIM sampling loops (sdmi.sampling, DDIMSampler.forward's
guidance_scale; reference tools/sample_ddpm_text_cond.py:62-64 and the generator scripts' _GuidedWrapper):
* the combine kernels (sdmi_cfg_combine, sdmi_cfg_combine_nhwc) are bit-identical to torch's u + s * (c - u);
* a guided step is ONE doubled-batch forward [cond | uncond] + the combine, recorded (hipGraph / native plan) and
  bit-identical to the stepwise loop and to the reference composition built from the module's own forward;
* the guided prediction stays within the project's forward bound pushed through the combine, against the fp32 oracle;
* the launch budget: a guided step of batch B issues at most one launch more than an unguided step of batch 2B."""
import pytest
import torch

from oracle import sd_oracle as O
from oracle import dit_oracle as DO
from tests.golden.configs import SMALL_COND, SMALL_UNCOND, SMALL_CLASS_UNET, SMALL_CLASS_DIT

pytestmark = pytest.mark.gpu

SHAPE = (2, 4, 32, 32)
S = 3.0


def one_hot(cmap, n=18):
    return torch.nn.functional.one_hot(cmap.long().clamp(0, n), n + 1).movedim(-1, 1)[:, 1:].float()


def _unet(cfg, cond=True, seed=3):
    import models.unet_cond_base as mc
    import models.unet_base as mu
    m = (mc.Unet if cond else mu.Unet)(4, cfg)
    sd = O.deterministic_state(O.unet_param_shapes(cfg, base="cond" if cond else "uncond"), seed)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd


def _dit(cfg, seed=6):
    from models.transformer import DIT
    m = DIT(4, cfg)
    m.load_state_dict(O.deterministic_state(DO.dit_param_shapes(cfg), seed))
    return m.cuda().eval()


def _text_image(B=2, seed=9):
    """(x_T, cond, uncond) of the text + mask model: the unconditional input is one 'empty' text row for every sample
    and an all-zero mask (tools/sample_ddpm_text_image_cond.py:60-70)."""
    g = torch.Generator().manual_seed(seed)
    c = {"text": torch.randn(B, 77, 64, generator=g).cuda(),
         "image": one_hot(torch.randint(0, 19, (B, 64, 64), generator=g)).cuda()}
    u = {"text": torch.randn(1, 77, 64, generator=g).expand(B, 77, 64).contiguous().cuda(),
         "image": torch.zeros_like(c["image"])}
    xT = torch.randn(B, 4, 32, 32, generator=g).cuda()
    return xT, c, u


def _klass(B=2, seed=10):
    g = torch.Generator().manual_seed(seed)
    c = {"class": torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float().cuda()}
    u = {"class": c["class"] * 0}  # tools/sample_ddpm_class_cond.py:50-52
    xT = torch.randn(B, 4, 32, 32, generator=g).cuda()
    return xT, c, u


def _cat(c, u):
    # (contiguous: cat keeps the one-hot mask's channels-last strides, which a loop would copy per step -- a callout)
    return {k: torch.cat([c[k], u[k]]).contiguous() for k in c}


def _combine(e2, s):
    """The reference expression on a doubled-batch prediction, in torch on the CPU (three separately rounded ops)."""
    e2 = e2.detach().float().cpu()
    B = e2.shape[0] // 2
    return e2[B:] + s * (e2[:B] - e2[B:])


def _sched():
    from scheduler.linear_noise_scheduler import LinearNoiseScheduler
    return LinearNoiseScheduler(1000, 0.00085, 0.012)


@pytest.fixture(scope="module")
def cond_model():
    return _unet(SMALL_COND)


# ------------------------------------------------------------------------------------------------
# 1. the combine kernels, bitwise against torch on the CPU
# ------------------------------------------------------------------------------------------------
def _flat(c, u, scale, alias=False):
    from sdmi import _lib, kernels as K
    cd, ud = c.cuda(), u.cuda()
    out = cd if alias else torch.empty_like(cd)
    _lib.check(_lib.lib().sdmi_cfg_combine(cd.data_ptr(), ud.data_ptr(), cd.numel(), scale, out.data_ptr(),
                                           K._stream()), "sdmi_cfg_combine")
    torch.cuda.synchronize()
    return out.cpu()


# (the last size is past one pass of the largest grid, 4096 blocks of 256: the grid-stride loop takes a second turn)
@pytest.mark.parametrize("scale", [0.0, 1.5, 7.5])
@pytest.mark.parametrize("n", [1, 5, 255, 1027, 8192, 4096 * 256 + 77])
def test_combine_flat_bitwise(n, scale):
    g = torch.Generator().manual_seed(n)
    c, u = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref = u + scale * (c - u)
    assert torch.equal(_flat(c, u, scale), ref)


def test_combine_flat_in_place():
    g = torch.Generator().manual_seed(2)
    c, u = torch.randn(1027, generator=g), torch.randn(1027, generator=g)
    assert torch.equal(_flat(c, u, 7.5, alias=True), u + 7.5 * (c - u))


@pytest.mark.parametrize("f32", [1, 0])
@pytest.mark.parametrize("HW", [60, 1024])
@pytest.mark.parametrize("B", [1, 3])
def test_combine_nhwc_bitwise(B, HW, f32):
    from sdmi import _lib, kernels as K
    C, ld, scale = 4, 8, 7.5
    g = torch.Generator().manual_seed(B * HW)
    src = torch.randn(2 * B * HW, ld, generator=g).to(torch.float32 if f32 else torch.bfloat16)
    src[:, C:] = float("nan")  # the pad columns are never read
    halves = src[:, :C].float().reshape(2, B, HW, C).permute(0, 1, 3, 2)  # (cond | uncond, B, C, HW)
    ref = halves[1] + scale * (halves[0] - halves[1])
    sd = src.cuda()
    out = torch.empty(B, C, HW, device="cuda")
    _lib.check(_lib.lib().sdmi_cfg_combine_nhwc(sd.data_ptr(), f32, ld, B, C, HW, scale, out.data_ptr(), K._stream()),
               "sdmi_cfg_combine_nhwc")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------
# 2. captured equals eager
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("issue", ["graph", "plan"])
def test_guided_captured_loop_matches_stepwise(issue, monkeypatch, cond_model):
    monkeypatch.setenv("SDMI_SAMPLE_ISSUE", issue)
    from sdmi.sampling import DDPMSampleLoop
    model, _ = cond_model
    xT, c, u = _text_image()
    kw = dict(cond_input=c, seed=11, uncond_input=u, guidance_scale=S)
    cap = DDPMSampleLoop(model, _sched(), SHAPE, **kw)
    assert cap.issue == issue and cap.fused and cap.mode == "guided"
    xa, x0a = (v.clone() for v in cap.run(xT, steps=4, captured=True))
    assert cap.t.item() == 1000 - 1 - 4
    assert torch.equal(cap.x2[2:], cap.x2[:2])  # x_t reached both halves of the doubled input
    eag = DDPMSampleLoop(model, _sched(), SHAPE, **kw)
    xb, x0b = eag.run(xT, steps=4, captured=False)
    torch.cuda.synchronize()
    assert torch.isfinite(xa).all()
    assert torch.equal(xa, xb) and torch.equal(x0a, x0b)
    xc, x0c = cap.run(xT, steps=4, captured=True)
    assert torch.equal(xc, xa) and torch.equal(x0c, x0a)


# ------------------------------------------------------------------------------------------------
# 3. one step equals the reference composition
# ------------------------------------------------------------------------------------------------
def test_guided_step_is_the_reference_composition(cond_model):
    from sdmi.sampling import DDPMSampleLoop
    model, _ = cond_model
    xT, c, u = _text_image()
    sched = _sched()
    loop = DDPMSampleLoop(model, sched, SHAPE, cond_input=c, seed=2, uncond_input=u, guidance_scale=S)
    loop.run(xT, steps=1, captured=False)
    with torch.no_grad():
        e2 = model(torch.cat([xT, xT]), torch.tensor([999]).cuda(), _cat(c, u))
    g = _combine(e2, S)
    torch.cuda.synchronize()
    assert torch.equal(loop.eps.cpu(), g)
    prev, _ = sched.sample_prev_timestep(xT, g.cuda(), 999, z=loop.z)
    assert torch.equal(loop.xt, prev)
    assert not torch.equal(g, e2[:2].cpu())  # guidance has an effect


# ------------------------------------------------------------------------------------------------
# 4. against the fp32 oracle
# ------------------------------------------------------------------------------------------------
def test_guided_prediction_against_oracle(cond_model):
    """(a) MSE(loop.eps, oracle combine) <= (1 + 2 s)^2 * 1e-4: the forward bound (test_unet_gpu.py:67, per half) through
    the combine's triangle inequality, |g - g'| <= s |c - c'| + (1 + s) |u - u'|. (b) the doubled-batch forward is no
    worse than two batch-B forwards: its MSE is at most 1.25 x that of the combine of two separate module forwards
    (the two differ in fp32 split-K summation order only, far below the bf16 rounding both share)."""
    from sdmi.sampling import DDPMSampleLoop
    model, sd = cond_model
    xT, c, u = _text_image()
    t = torch.tensor([999, 999])
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    with torch.no_grad():
        rc = O.unet_forward(sd, SMALL_COND, xT.cpu(), t, cpu(c))
        ru = O.unet_forward(sd, SMALL_COND, xT.cpu(), t, cpu(u))
    ref = ru + S * (rc - ru)
    loop = DDPMSampleLoop(model, _sched(), SHAPE, cond_input=c, seed=2, uncond_input=u, guidance_scale=S)
    loop.run(xT, steps=1, captured=False)
    with torch.no_grad():
        ec, eu = model(xT, t.cuda(), c).cpu(), model(xT, t.cuda(), u).cpu()
    torch.cuda.synchronize()
    mse2 = ((loop.eps.cpu() - ref) ** 2).mean().item()
    mse1 = (((eu + S * (ec - eu)) - ref) ** 2).mean().item()
    msg = f"MSE vs the oracle: doubled-batch forward {mse2:.4e}, two batch-B forwards {mse1:.4e}"
    print(msg)
    assert mse2 <= (1 + 2 * S) ** 2 * 1e-4, msg
    assert mse2 <= 1.25 * mse1, msg


# ------------------------------------------------------------------------------------------------
# 5. the DDIM drop-in surface
# ------------------------------------------------------------------------------------------------
def test_ddim_sampler_guidance_scale(cond_model):
    from sdmi.sampling import DDIMSampleLoop
    from scheduler.linear_noise_scheduler import DDIMSampler
    model, _ = cond_model
    xT, c, u = _text_image(seed=12)
    sampler = DDIMSampler(model, (0.0001, 0.02), 1000)
    xs = sampler(xT, c, u, steps=5, eta=0.5, seed=5, guidance_scale=S)
    loop = DDIMSampleLoop(model, sampler.alpha_t_bar, SHAPE, c, steps=5, eta=0.5, seed=5, uncond_input=u,
                          guidance_scale=S)
    assert torch.isfinite(xs).all()
    assert torch.equal(xs, loop.run(xT))
    # eta = 0 uses no noise: the captured loop and the eager path (one doubled-batch module call + the combine) agree
    cap = sampler(xT, c, u, steps=5, eta=0.0, seed=5, guidance_scale=S)
    eag = sampler(xT, c, u, steps=5, eta=0.0, seed=5, guidance_scale=S, captured=False)
    assert torch.equal(cap, eag) and not torch.equal(cap, xs)
    plain = sampler(xT, c, u, steps=5, eta=0.5, seed=5)
    assert torch.equal(sampler(xT, c, u, steps=5, eta=0.5, seed=5, guidance_scale=1.0), plain)
    assert not torch.equal(plain, xs)
    assert torch.equal(sampler(xT, c, u, steps=5, eta=0.5, seed=5, guidance_scale=0.0),
                       sampler(xT, u, None, steps=5, eta=0.5, seed=5))


# ------------------------------------------------------------------------------------------------
# 6. class conditions, and the DiT token path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unet", "dit"])
def test_guided_class_conditional_models(kind):
    from sdmi.sampling import DDPMSampleLoop
    model = _unet(SMALL_CLASS_UNET, seed=5)[0] if kind == "unet" else _dit(SMALL_CLASS_DIT)
    xT, c, u = _klass()
    kw = dict(cond_input=c, seed=7, uncond_input=u, guidance_scale=S)
    cap = DDPMSampleLoop(model, _sched(), SHAPE, **kw)
    assert cap.fused
    xa, x0a = (v.clone() for v in cap.run(xT, steps=4, captured=True))
    eag = DDPMSampleLoop(model, _sched(), SHAPE, **kw)
    xb, x0b = eag.run(xT, steps=4, captured=False)
    torch.cuda.synchronize()
    assert torch.isfinite(xa).all()
    assert torch.equal(xa, xb) and torch.equal(x0a, x0b)
    one = DDPMSampleLoop(model, _sched(), SHAPE, **kw)
    one.run(xT, steps=1, captured=False)
    with torch.no_grad():
        e2 = model(torch.cat([xT, xT]), torch.tensor([999]).cuda(), _cat(c, u))
    g = _combine(e2, S)
    assert torch.equal(one.eps.cpu(), g)
    assert not torch.equal(g, e2[:2].cpu())


# ------------------------------------------------------------------------------------------------
# 7. launch budget
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unet", "dit"])
def test_guided_step_launch_budget(kind, monkeypatch, cond_model):
    """The native plan of a guided B = 2 step against an unguided B = 4 step (the same doubled-batch forward): at
    most one launch more, and no callout more."""
    monkeypatch.setenv("SDMI_SAMPLE_ISSUE", "plan")
    from sdmi.sampling import DDPMSampleLoop
    if kind == "unet":
        model = cond_model[0]
        xT, c, u = _text_image()
    else:
        model = _dit(SMALL_CLASS_DIT)
        xT, c, u = _klass()
    guided = DDPMSampleLoop(model, _sched(), SHAPE, cond_input=c, seed=1, uncond_input=u, guidance_scale=S)
    guided.run(xT, steps=2)
    plain = DDPMSampleLoop(model, _sched(), (4, 4, 32, 32), cond_input=_cat(c, u), seed=1)
    plain.run(torch.cat([xT, xT]), steps=2)
    _, lg, cg = guided.plan.info()
    _, lp, cp = plain.plan.info()
    assert lg <= lp + 1, (lg, lp)
    assert cg == cp, (cg, cp)


# ------------------------------------------------------------------------------------------------
# 8. errors
# ------------------------------------------------------------------------------------------------
def test_guidance_argument_errors(cond_model):
    from sdmi.sampling import DDPMSampleLoop
    xT, c, u = _text_image()
    plain, _ = _unet(SMALL_UNCOND, cond=False)
    with pytest.raises(ValueError):
        DDPMSampleLoop(plain, _sched(), SHAPE, uncond_input=u, guidance_scale=S)
    model, _ = cond_model
    with pytest.raises(ValueError):
        DDPMSampleLoop(model, _sched(), SHAPE, cond_input=c, uncond_input={"text": u["text"]}, guidance_scale=S)
    with pytest.raises(ValueError):
        DDPMSampleLoop(model, _sched(), SHAPE, cond_input=c, guidance_scale=S,
                       uncond_input={"text": u["text"][:, :40].contiguous(), "image": u["image"]})


# ------------------------------------------------------------------------------------------------
# 9. reuse
# ------------------------------------------------------------------------------------------------
def test_guided_loop_reuse(monkeypatch):
    """A guided loop reused after an in-place weight update samples with the new weights; a new guidance scale is a
    new launch argument, so the step is recorded again."""
    monkeypatch.setenv("SDMI_SAMPLE_ISSUE", "graph")
    from sdmi.sampling import DDPMSampleLoop
    model, _ = _unet(SMALL_COND)
    xT, c, u = _text_image()
    kw = dict(cond_input=c, seed=3, uncond_input=u)
    loop = DDPMSampleLoop(model, _sched(), SHAPE, guidance_scale=S, **kw)
    a = loop.run(xT, steps=3)[0].clone()
    with torch.no_grad():
        model.conv_out.weight.data.mul_(0.5)
    b = loop.run(xT, steps=3)[0].clone()
    assert not torch.equal(a, b)
    fresh = DDPMSampleLoop(model, _sched(), SHAPE, guidance_scale=S, **kw)
    assert torch.equal(fresh.run(xT, steps=3)[0], b)
    recorded = loop.graph
    assert recorded is not None
    loop.guidance_scale = 5.0
    assert loop.graph is None
    d = loop.run(xT, steps=3)[0].clone()
    assert loop.graph is not None and not torch.equal(d, b)
    fresh = DDPMSampleLoop(model, _sched(), SHAPE, guidance_scale=5.0, **kw)
    assert torch.equal(fresh.run(xT, steps=3)[0], d)
