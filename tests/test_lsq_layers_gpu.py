"""Conv2d_qn_lsq / Linear_qn_lsq (sdmi/layers_qn_lsq.py) on the GPU against the reference's own layers
(tests/golden/lsq_layers.safetensors, made by tests/golden/make_golden_lsq.py) and the hand restatement (tests/lsq_ref.py).

* y is torch.equal to the reference's: equal codes times the same step; the fixture keeps every quantiser input 1e-3 code
  units from a tie, so no share of mismatches is allowed.
* dx, dw, db meet the leaf path's standard (tests/test_leaf_gpu.py): error <= 2e-2 of the scale, cosine >= 0.999. The
  three step gradients lie within the derived bounds of tests/lsq_ref.py (d_pre rounded to bf16 is the one approximation).
* noise: weight_quant_noise is bitwise the torch expression on the re-drawn device noise, its gradient that of torch
  autograd (ties at the extreme codes included), noise_scale = 0 leaves the device generator untouched.
* the first forward initialises each step bitwise by the reference's formula, the second forward reads no step.
* use_FP=True is leaf.conv2d / leaf.linear bit for bit.
* whole model: the SMALL_COND UNet at B = 2, converted, runs forward and backward on the leaf path, every parameter and
  step gets a finite non-zero gradient (but a step whose quantiser inputs all sit exactly on its codes, where every term
  q - v is zero: see the test), two Adam steps move them, and its output agrees with the same model built from
  the restatement layers (WHOLE_MODEL_TOL, see there)."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from safetensors.torch import load_file

from tests import lsq_ref as R
from tests.golden.configs import SMALL_COND

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsq_layers.safetensors")
ALL = [(name, kind, geo, wbit) for name, kind, geo, _ in R.CASES for wbit in R.WEIGHT_BITS]
IDS = [f"{c[0]}-w{c[3]}" for c in ALL]
# Output error of the converted SMALL_COND UNet allowed against the restatement-layer model, as a share of the output
# scale. Measured on the CPU on the reference's own Unet with the restatement layers (weights 8 bit, features 8 bit, no
# noise, the test's inputs): fp32 against the same model with the conv / linear operands and d_pre rounded to bf16 gave
# MEASURED_WHOLE_MODEL (77 converted layers; the worst parameter-gradient cosine between the two was 0.9943); the tolerance
# is three times that. On an MI355X the converted model was 3.7e-2 from the restatement-layer model.
MEASURED_WHOLE_MODEL = 4.85e-2  # largest output difference over the largest output; its rms share was 1.08e-2
WHOLE_MODEL_TOL = 3 * MEASURED_WHOLE_MODEL


def cos(a, b):
    a, b = a.reshape(-1).double().cpu(), b.reshape(-1).double().cpu()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def rel(a, b):
    return ((a.cpu() - b.cpu()).abs().max() / (b.abs().max() + 1e-12)).item()


_FIX = {}


def load_case(name, wbit):
    if not _FIX:
        _FIX.update(load_file(FIXTURE))
    pre = f"{name}.w{wbit}."
    f = {k[len(pre):]: v for k, v in _FIX.items() if k.startswith(pre)}
    for k in ("s_in", "s_w", "s_out", "ds_in", "ds_w", "ds_out"):
        f[k] = f[k].reshape(())
    return f


def build(kind, geo, wbit, f=None, noise_scale=0.0, **flags):
    from sdmi import layers_qn_lsq as Q
    kw = dict(weight_bit=wbit, input_bit=R.FEATURE_BIT, output_bit=R.FEATURE_BIT, noise_scale=noise_scale, **flags)
    if kind == "conv":
        ci, co, k, s, p = geo
        m = Q.Conv2d_qn_lsq(ci, co, k, s, p, 1, bias=True, **kw)
    else:
        fi, fo, bias = geo
        m = Q.Linear_qn_lsq(fi, fo, bias=bias, **kw)
    m = m.cuda()
    if f is not None:
        with torch.no_grad():
            m.weight.copy_(f["w"])
            if m.bias is not None:
                m.bias.copy_(f["b"])
            for k, key in (("input", "s_in"), ("weight", "s_w"), ("output", "s_out")):
                getattr(m, f"step_size_{k}").copy_(f[key])
    return m


def run(m, x, dy):
    xg = x.clone().cuda().requires_grad_(True)
    m.zero_grad()
    y = m(xg)
    y.backward(dy.cuda())
    out = dict(y=y.detach().cpu(), dx=xg.grad.cpu(), dw=m.weight.grad.cpu())
    if m.bias is not None:
        out["db"] = m.bias.grad.cpu()
    for k, key in (("input", "ds_in"), ("weight", "ds_w"), ("output", "ds_out")):
        g = getattr(m, f"step_size_{k}").grad
        out[key] = None if g is None else float(g)
    return out


@pytest.mark.parametrize("name,kind,geo,wbit", ALL, ids=IDS)
def test_layer_against_the_reference(name, kind, geo, wbit):
    f = load_case(name, wbit)
    m = build(kind, geo, wbit, f)
    got = run(m, f["x"], f["dy"])
    assert got["y"].shape == f["y"].shape
    assert torch.equal(got["y"], f["y"]), f"{int((got['y'] != f['y']).sum())} of {f['y'].numel()} outputs differ"
    for k in ("dx", "dw", "db"):
        if k in f:
            print(f"{name} w{wbit} {k}: rel {rel(got[k], f[k]):.2e} cos {cos(got[k], f[k]):.6f}")
            assert got[k].shape == f[k].shape
            assert rel(got[k], f[k]) <= 2e-2 and cos(got[k], f[k]) >= 0.999, k
    assert torch.equal(got["dw"] == 0, f["dw"] == 0) and torch.equal(got["dx"] == 0, f["dx"] == 0)  # the clamp masks
    bounds = R.step_grad_bounds(kind, geo, f, wbit)
    for k, (ref, bound) in bounds.items():
        err = abs(got[k] - ref)
        print(f"{name} w{wbit} {k}: {got[k]:.6e} float64 {ref:.6e} error {err:.2e} bound {bound:.2e}")
        assert err <= bound, k
    # a second forward / backward repeats every bit
    again = run(m, f["x"], f["dy"])
    for k in got:
        assert (again[k] == got[k]) if not torch.is_tensor(got[k]) else torch.equal(again[k], got[k]), k


def _operands_are_codes(m, x, wbit):
    """Both GEMM operands of the last forward are integers (<= Qp): the packed weight view and the input codes."""
    from sdmi import leaf as LF
    pk = LF._PACKS[m.__dict__["_pack_src"]]["pk"]
    w = pk.view("f").float().cpu()
    assert bool((w == w.round()).all()) and float(w.abs().max()) <= R.qp_of(wbit)
    codes = m.__dict__["_codes"].cpu()
    assert bool((codes == codes.round()).all()) and float(codes.abs().max()) == R.qp_of(wbit)


def test_operands_are_integer_codes_without_noise():
    name, kind, geo, _ = R.CASES[0]
    for wbit in R.WEIGHT_BITS:
        f = load_case(name, wbit)
        m = build(kind, geo, wbit, f)
        with torch.no_grad():
            m(f["x"].cuda())
        _operands_are_codes(m, f["x"], wbit)


@pytest.mark.parametrize("flags", [dict(input_quant=False), dict(weight_quant=False), dict(output_quant=False),
                                   dict(input_quant=False, weight_quant=False, output_quant=False)],
                         ids=lambda d: "+".join(k for k in d))
@pytest.mark.parametrize("name,kind,geo,wbit", [ALL[0], ALL[3], ALL[7]], ids=[IDS[0], IDS[3], IDS[7]])
def test_quantisers_switched_off(name, kind, geo, wbit, flags):
    """An operand that is not quantised goes through bf16 like a plain leaf's: the leaf path's standard, not bitwise."""
    f = load_case(name, wbit)
    m = build(kind, geo, wbit, f, **flags)
    got = run(m, f["x"], f["dy"])
    quant = tuple(flags.get(k, True) for k in ("input_quant", "weight_quant", "output_quant"))
    ref = R.layer_grads(kind, geo, f, wbit, torch.float64, quant=quant)
    scale = float(ref["y"].abs().max())
    step = float(f["s_out"]) if quant[2] else 0.0  # a bf16 operand may move an output by one code
    assert float((got["y"].double() - ref["y"]).abs().max()) <= 2e-2 * scale + step
    for k in ("dx", "dw", "db"):
        if k in ref:
            assert cos(got[k], ref[k]) >= 0.999, k
    for k, on in zip(("ds_in", "ds_w", "ds_out"), quant):
        assert (got[k] is not None) == on, k
        if on:
            print(f"{name} w{wbit} {k}: {got[k]:.5e} float64 {float(ref[k]):.5e}")
            assert got[k] == got[k] and abs(got[k]) < float("inf"), k
    if quant[2]:
        _ds_out_within_operand_bound(kind, geo, f, ref, got, [not quant[0], not quant[1]])


def _ds_out_within_operand_bound(kind, geo, f, ref, got, rounded):
    """ds_out where GEMM operands are values rounded to bf16 (rounded: [x, w]), not integer codes: every pre-activation
    may move by 2^-9 |x| |w| per rounded operand through the same conv / linear, and ds_out by what
    lsq_ref.ds_out_operand_bound derives from that (code flips near ties and clamp crossings included). Nothing else
    enters: ds_out is formed before d_pre is rounded."""
    e = R.matmul_of(kind, geo)(ref["xq"].abs(), ref["wq"].abs(), None) * (R.BF16_REL * sum(rounded) * 1.01)
    bound = R.ds_out_operand_bound(ref["pre"], f["dy"], f["s_out"], e, R.FEATURE_BIT)
    print(f"ds_out {got['ds_out']:.5e} float64 {float(ref['ds_out']):.5e} operand bound {bound:.2e}")
    assert abs(got["ds_out"] - float(ref["ds_out"])) <= bound + 1e-6 * abs(float(ref["ds_out"]))


def test_weight_quant_noise_is_the_torch_expression():
    from sdmi import layers_qn_lsq as Q
    name, kind, geo, _ = R.CASES[1]
    for wbit, ns in ((8, 0.1), (4, 0.074)):
        f = load_case(name, wbit)
        m = build(kind, geo, wbit, f, noise_scale=ns)
        torch.manual_seed(11)
        w_qn, scale = Q.weight_quant_noise(m)
        assert scale == 1.0
        torch.manual_seed(11)
        eps = torch.randn_like(m.weight).cpu()
        w = f["w"].clone().requires_grad_(True)
        s = f["s_w"].clone().requires_grad_(True)
        w_q = R.quant_lsq(w, wbit, s)
        assert int((w_q == w_q.max()).sum()) > 1 and int((w_q == w_q.min()).sum()) > 1  # ties at the extreme codes
        ref = w_q + (w_q.max() - w_q.min()) * ns * eps
        assert torch.equal(w_qn.detach().cpu(), ref.detach())
        g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(12))
        m.zero_grad()
        w_qn.backward(g.cuda())
        ref.backward(g)
        # the sums behind the range gradient and ds run in another order than torch's: fp32 summation error only
        assert rel(m.weight.grad, w.grad) <= 1e-5 and cos(m.weight.grad, w.grad) >= 1 - 1e-9
        assert torch.equal(m.weight.grad.cpu() == 0, w.grad == 0)
        assert abs(float(m.step_size_weight.grad) - float(s.grad)) <= 1e-4 * abs(float(s.grad)) + 1e-6
    # no noise: no draw, the generator stays where it was; and add_noise is the vqvae_noise function
    m = build(kind, geo, 8, load_case(name, 8), noise_scale=0.0)
    state = torch.cuda.get_rng_state()
    Q.weight_quant_noise(m)
    m(load_case(name, 8)["x"].cuda())
    assert torch.equal(torch.cuda.get_rng_state(), state)
    m.noise_scale = 0.1
    m(load_case(name, 8)["x"].cuda())
    assert not torch.equal(torch.cuda.get_rng_state(), state)


@pytest.mark.parametrize("name,kind,geo,wbit", [ALL[0], ALL[2], ALL[6]], ids=[IDS[0], IDS[2], IDS[6]])
def test_layer_with_noise(name, kind, geo, wbit):
    """With noise the weight operand is fl(w_qn / se_w) rounded to bf16: the leaf path's standard against the float64
    restatement on the same draw; one draw per forward."""
    ns = 0.05
    f = load_case(name, wbit)
    m = build(kind, geo, wbit, f, noise_scale=ns)
    torch.manual_seed(21)
    got = run(m, f["x"], f["dy"])
    torch.manual_seed(21)
    eps = torch.randn_like(m.weight)
    after = torch.cuda.get_rng_state()
    torch.manual_seed(21)
    run(m, f["x"], f["dy"])
    assert torch.equal(torch.cuda.get_rng_state(), after)  # exactly one randn_like(weight) per forward
    ref = R.layer_grads(kind, geo, f, wbit, torch.float64, noise=(ns, eps.cpu().double()))
    scale = float(ref["y"].abs().max())
    assert float((got["y"].double() - ref["y"]).abs().max()) <= 2e-2 * scale + float(f["s_out"])
    for k in ("dx", "dw", "db"):
        if k in ref:
            assert cos(got[k], ref[k]) >= 0.999, k
    for k in ("ds_in", "ds_w", "ds_out"):
        print(f"{name} w{wbit} {k}: {got[k]:.5e} float64 {float(ref[k]):.5e}")
        assert got[k] == got[k] and abs(got[k]) < float("inf"), k
    _ds_out_within_operand_bound(kind, geo, f, ref, got, [False, True])


@pytest.mark.parametrize("name,kind,geo,wbit", [ALL[0], ALL[3], ALL[5], ALL[6], ALL[9]],
                         ids=[IDS[0], IDS[3], IDS[5], IDS[6], IDS[9]])
def test_noise_branch_step_gradients(name, kind, geo, wbit):
    """The backward's noise branch (scale by se_x, the latent-noise backward, the weight quantiser's backward) and the
    input quantiser behind a noisy weight, with the output quantiser off so that no code flip enters: ds_in and ds_w lie
    within the bounds lsq_ref.noise_step_grad_bounds derives from the two bf16 roundings, against the float64
    restatement on the same draw. A forgotten or doubled step factor misses them by the factor itself."""
    ns = 0.05
    f = load_case(name, wbit)
    m = build(kind, geo, wbit, f, noise_scale=ns, output_quant=False)
    torch.manual_seed(31)
    got = run(m, f["x"], f["dy"])
    torch.manual_seed(31)
    eps = torch.randn_like(m.weight).cpu()
    bounds, ref = R.noise_step_grad_bounds(kind, geo, f, wbit, ns, eps)
    assert got["ds_out"] is None
    for k, (want, bound) in bounds.items():
        err = abs(got[k] - want)
        print(f"{name} w{wbit} {k}: {got[k]:.6e} float64 {want:.6e} error {err:.2e} bound {bound:.2e}")
        assert err <= bound, k
    # a step factor is 1 / 50 or less: the ds_in bound (a few per cent of ds_in) always sees one; the ds_w bound is
    # printed above, it was 0.1 to 8 times |ds_w| on these cases
    assert bounds["ds_in"][1] < 0.5 * abs(bounds["ds_in"][0])
    for k in ("dx", "dw", "db"):
        if k in ref:
            assert cos(got[k], ref[k]) >= 0.999, k


def test_backward_after_a_later_forward_with_other_codes_raises():
    name, kind, geo, wbit = ALL[0]
    f = load_case(name, wbit)
    x = f["x"].cuda().requires_grad_(True)
    m = build(kind, geo, wbit, f)
    y1, y2 = m(x), m(x)  # the same codes twice: both backwards are right
    y1.backward(f["dy"].cuda())
    g1 = x.grad.clone()
    x.grad = None
    y2.backward(f["dy"].cuda())
    assert torch.equal(x.grad, g1)
    m.noise_scale = 0.1  # every forward draws: the first forward's codes are gone after the second
    y1, y2 = m(x), m(x)
    with pytest.raises(RuntimeError, match="other weight codes"):
        y1.backward(f["dy"].cuda())
    y2.backward(f["dy"].cuda())
    m.noise_scale = 0.0
    y1 = m(x)
    with torch.no_grad():
        m.weight.mul_(0.5)
    m(x)
    with pytest.raises(RuntimeError, match="other weight codes"):
        y1.backward(f["dy"].cuda())


@pytest.mark.parametrize("name,kind,geo,wbit", [ALL[0], ALL[3], ALL[9]], ids=[IDS[0], IDS[3], IDS[9]])
def test_first_forward_initialises_the_steps(name, kind, geo, wbit):
    f = load_case(name, wbit)
    m = build(kind, geo, wbit)
    with torch.no_grad():
        m.weight.copy_(f["w"])
        if m.bias is not None:
            m.bias.copy_(f["b"])
    assert m.step_reads == 0
    y = m(f["x"].cuda())
    fi = dict(x=f["x"], w=f["w"], b=f.get("b"))
    fi["s_in"], fi["s_w"] = R.init_step(f["x"], R.FEATURE_BIT), R.init_step(f["w"], wbit)
    pre = R.pre32(kind, geo, fi, wbit)
    s_out = R.init_step(pre, R.FEATURE_BIT)
    for k, want in (("input", fi["s_in"]), ("weight", fi["s_w"]), ("output", s_out)):
        assert torch.equal(getattr(m, f"step_size_{k}").detach().cpu(), want), k
    tm = R.terms(pre, torch.zeros_like(pre), s_out, R.FEATURE_BIT)
    assert torch.equal(y.detach().cpu(), tm["q"] * tm["se"])
    reads = m.step_reads
    assert reads == 6  # each step read once, initialised, and read back once
    y2 = m(f["x"].cuda())
    assert m.step_reads == reads, "the second forward read a step on the host"
    assert torch.equal(y2, y)
    m.reset_step_cache()
    m(f["x"].cuda())
    assert m.step_reads == reads + 3  # seen != 1: one read each, no initialisation
    for k, want in (("input", fi["s_in"]), ("weight", fi["s_w"]), ("output", s_out)):
        assert torch.equal(getattr(m, f"step_size_{k}").detach().cpu(), want), k
    # init_step_size, the exported function
    from sdmi import layers_qn_lsq as Q
    assert torch.equal(Q.init_step_size(f["x"].cuda(), R.FEATURE_BIT).cpu(), fi["s_in"])
    assert float(Q.init_step_size(torch.zeros(5, device="cuda"), 8)) == 1.0


def test_exported_quantiser_functions():
    from sdmi import layers_qn_lsq as Q
    c = R.quant_case(1025, 4, "soft")
    x = c["x"].cuda().requires_grad_(True)
    s = c["step"].cuda().requires_grad_(True)
    y, scale = Q.data_quant_lsq(x, 4, s)
    assert scale == 1.0
    y.backward(c["dy"].cuda())
    xr, sr = c["x"].clone().requires_grad_(True), c["step"].clone().requires_grad_(True)
    yr = R.quant_lsq(xr, 4, sr)
    yr.backward(c["dy"])
    assert torch.equal(y.detach().cpu(), yr.detach()) and torch.equal(x.grad.cpu(), xr.grad)
    tm = R.terms(c["x"], c["dy"], c["step"], 4)
    g = R.g32(4, 1025)
    assert s.grad.shape == s.shape and abs(float(s.grad) - R.ds64(tm["t"], g)) <= R.sum_bound(tm["t"], g)
    with pytest.raises(ValueError):
        Q.data_quant_lsq(x, 10, s)


@pytest.mark.parametrize("name,kind,geo,wbit", [ALL[0], ALL[2], ALL[6], ALL[8]], ids=[IDS[0], IDS[2], IDS[6], IDS[8]])
def test_use_fp_is_the_plain_leaf(name, kind, geo, wbit):
    from sdmi import leaf as LF
    f = load_case(name, wbit)
    m = build(kind, geo, wbit, f)
    m.update_para(use_FP=True)
    if kind == "conv":
        ci, co, k, s, p = geo
        plain, fn = nn.Conv2d(ci, co, k, s, p).cuda(), LF.conv2d
    else:
        plain, fn = nn.Linear(geo[0], geo[1], bias=geo[2]).cuda(), LF.linear
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("step_size")})
    got = run(m, f["x"], f["dy"])
    xg = f["x"].clone().cuda().requires_grad_(True)
    y = fn(plain, xg)
    y.backward(f["dy"].cuda())
    assert torch.equal(got["y"], y.detach().cpu()) and torch.equal(got["dx"], xg.grad.cpu())
    assert torch.equal(got["dw"], plain.weight.grad.cpu())
    if plain.bias is not None:
        assert torch.equal(got["db"], plain.bias.grad.cpu())
    assert got["ds_in"] is None and got["ds_w"] is None and got["ds_out"] is None


def test_limits():
    from sdmi import layers_qn_lsq as Q
    x = torch.randn(1, 4, 8, 8, device="cuda")
    kw = dict(weight_bit=8, input_bit=8, output_bit=8, noise_scale=0.0)
    with pytest.raises(NotImplementedError):
        Q.Conv2d_qn_lsq(4, 4, 3, 1, 1, 2, **kw).cuda()(x)  # groups
    with pytest.raises(NotImplementedError):
        Q.Conv2d_qn_lsq(4, 4, 3, 2, 1, 1, **kw).cuda()(x)  # a geometry leaf.conv2d does not run
    for bad in (dict(weight_bit=10), dict(input_bit=1), dict(output_bit=16)):
        with pytest.raises(ValueError):
            Q.Conv2d_qn_lsq(4, 4, 3, 1, 1, 1, **{**kw, **bad}).cuda()(x)
    m = Q.Linear_qn_lsq(4, 4, **{**kw, "weight_bit": 12}, weight_quant=False).cuda()  # an unused width is not checked
    m(torch.randn(3, 4, device="cuda"))


def _unet_inputs():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 32, 32, generator=g)
    t = torch.randint(0, 1000, (2,), generator=g)
    cmap = torch.randint(0, 19, (2, 64, 64), generator=g)
    # a soft mask: with an exact one-hot mask every input of cond_conv_in sits on a code (0 or Qp after the step's
    # initialisation), q - v is 0 everywhere and that step's gradient is exactly zero, in the reference as well
    mask = F.one_hot(cmap, 19).movedim(-1, 1)[:, 1:].float() * 0.8 + 0.2 * torch.rand(2, 18, 64, 64, generator=g)
    text = torch.randn(2, 77, SMALL_COND["condition_config"]["text_condition_config"]["text_embed_dim"], generator=g)
    return x, t, mask, text


def test_whole_model_converted():
    import models.unet_cond_base as mc
    from oracle import sd_oracle as O
    from sdmi import layers_qn_lsq as Q
    sd = O.deterministic_state(O.unet_param_shapes(SMALL_COND, base="cond"), 5)
    model = mc.Unet(4, SMALL_COND).cuda()
    model.load_state_dict(sd)
    twin = copy.deepcopy(model)
    names = Q.convert(model, weight_bit=8, input_bit=8, output_bit=8, noise_scale=0.0)
    assert names == R.convert_ref(twin, weight_bit=8, input_bit=8, output_bit=8, noise_scale=0.0) and len(names) > 20
    assert not model._sdmi_engine_ok()  # the converted model takes the leaf path
    x, t, mask, text = _unet_inputs()
    cond = {"image": mask.cuda(), "text": text.cuda()}
    out = model(x.cuda(), t.cuda(), cond)
    ref = twin(x.cuda(), t.cuda(), cond)
    err = rel(out.detach(), ref.detach())
    print(f"converted UNet against the restatement layers: {err:.3e} of the output scale (allowed {WHOLE_MODEL_TOL})")
    assert err <= WHOLE_MODEL_TOL
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    steps = [k for k in before if "step_size" in k]
    assert len(steps) == 3 * len(names)
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, a: seen.__setitem__(mod, a[0].detach().cpu()))
             for m in model.modules() if isinstance(m, (Q.Conv2d_qn_lsq, Q.Linear_qn_lsq))]
    for it in range(2):
        opt.zero_grad()
        loss = F.mse_loss(model(x.cuda(), t.cuda(), cond), noise)
        for h in hooks:
            h.remove()
        loss.backward()
        if it == 0:
            F.mse_loss(ref, noise).backward()
            zero = []
            for k, p in model.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
                if float(p.grad.abs().max()) == 0:
                    # only where the arithmetic itself gives zero: an input quantiser all of whose inputs sit exactly
                    # on its own codes (q - v = 0 in every term). downs.0.residual_input_conv.0 is one: its input is
                    # conv_in_concat's quantised output, and the step it initialises from that is the same grid; the
                    # reference's layer gives the same exact zero (measured on the CPU on its own Unet).
                    assert k.endswith("step_size_input"), f"{k}: zero gradient"
                    lay = model.get_submodule(k.rsplit(".", 1)[0])
                    tm = R.terms(seen[lay], torch.ones_like(seen[lay]), p.detach().cpu(), lay.input_bit)
                    assert bool((tm["t"] == 0).all()), f"{k}: zero gradient"
                    zero.append(k)
            print("steps with an exactly zero gradient (inputs on their own codes):", zero)
            assert len(zero) <= 2
            tw = dict(twin.named_parameters())
            worst = min((cos(p.grad, tw[k].grad), k) for k, p in model.named_parameters()
                        if "step_size" not in k and tw[k].grad.norm() > 1e-6)
            print("worst parameter-gradient cosine against the restatement layers:", worst)
            assert worst[0] >= 0.99, worst
        opt.step()
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert k in zero or not torch.equal(p.detach(), before[k]), f"{k} did not move"
    reads = sum(m.step_reads for m in model.modules() if hasattr(m, "step_reads"))
    model(x.cuda(), t.cuda(), cond)
    assert reads == sum(m.step_reads for m in model.modules() if hasattr(m, "step_reads"))
