"""CPU checks of the LSQ quantise-and-noise layers (sdmi/layers_qn_lsq.py): the fixture against the hand restatement
(tests/lsq_ref.py), the fixture's distance condition, the module surface, the derived bounds on the reference's own
result and on perturbed restatements, and the measurement behind K_LSQ.

Measured here (fixture of 10 cases): the reference's fp32 ds_in / ds_w lie at most 1e-3 of their bounds from the
float64 restatement. Its fp32 ds_out does NOT meet the summation-only bound of ds_out (up to 6 times the bound, 2.9e-6
against 4.6e-7): it subtracts two large sums (sum dy q - sum dy v, terms up to Qp times larger than dy (q - v)) and its
fp32 pre-activation is up to 1e-4 code units from the exact code form. The bound is the kernels' (per-element q - v on
the exact pre); test_ds_out_bound_is_for_the_per_element_form shows both facts."""
import os

import pytest
import torch
import torch.nn as nn
from safetensors.torch import load_file

from tests import lsq_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "lsq_layers.safetensors")
ALL = [(name, kind, geo, wbit) for name, kind, geo, _ in R.CASES for wbit in R.WEIGHT_BITS]
IDS = [f"{c[0]}-w{c[3]}" for c in ALL]


# The two (case, perturbation) pairs whose error stays inside the ds_w bound (0.57 and 0.80 of it): the bound pushes
# 2^-9 through absolute values, and on these cases that is 30 % and 8 times |ds_w|. The layer-level ds_w check of
# tests/test_lsq_layers_gpu.py cannot see these two errors on these two cases; it sees them on the other nine cases each,
# and the ds_in bound sees every perturbation on every case.
DS_W_BLIND = {("conv3", 4, "q_only", "ds_w"), ("conv4s2", 4, "no_mask", "ds_w")}


def load_case(name, wbit, path=FIXTURE, _cache={}):
    if path not in _cache:
        _cache[path] = load_file(path)
    pre = f"{name}.w{wbit}."
    f = {k[len(pre):]: v for k, v in _cache[path].items() if k.startswith(pre)}
    for k in ("s_in", "s_w", "s_out", "ds_in", "ds_w", "ds_out"):
        f[k] = f[k].reshape(())
    return f


@pytest.mark.parametrize("name,kind,geo,wbit", ALL, ids=IDS)
def test_fixture_equals_restatement(name, kind, geo, wbit):
    f = load_case(name, wbit)
    r = R.layer_grads(kind, geo, f, wbit, torch.float32)
    assert torch.equal(r["y"], f["y"])
    assert torch.equal(r["dx"], f["dx"])
    assert torch.equal(r["dw"] == 0, f["dw"] == 0)  # the weight quantiser's clamp mask
    assert int((f["dw"] == 0).sum()) > 0 and int((f["dx"] == 0).sum()) > 0  # the clamped branch is exercised
    # the HIP path's pre-activation formula reproduces the reference's codes, hence its y, bit for bit
    p = R.pre32(kind, geo, f, wbit)
    tm = R.terms(p, f["dy"], f["s_out"], R.FEATURE_BIT)
    assert torch.equal(tm["q"] * tm["se"], f["y"])


@pytest.mark.parametrize("name,kind,geo,wbit", ALL, ids=IDS)
def test_fixture_distance_condition(name, kind, geo, wbit):
    f = load_case(name, wbit)
    vx, vw, vp = R.quantiser_inputs64(kind, geo, f, wbit)
    for v, bit in ((vx, R.FEATURE_BIT), (vw, wbit), (vp, R.FEATURE_BIT)):
        assert R.tie_distance(v, bit) >= R.TIE_DISTANCE
        assert int((v.abs() > R.qp_of(bit)).sum()) > 0
    # the steps are the reference's initialisation times the factors
    assert torch.equal(f["s_in"], R.init_step(f["x"], R.FEATURE_BIT) * R.STEP_FACTORS["input"])
    assert torch.equal(f["s_w"], R.init_step(f["w"], wbit) * R.STEP_FACTORS["weight"])


@pytest.mark.parametrize("name,kind,geo,wbit", ALL, ids=IDS)
def test_step_gradient_bounds_hold_for_the_reference_and_catch_perturbations(name, kind, geo, wbit):
    f = load_case(name, wbit)
    B = R.step_grad_bounds(kind, geo, f, wbit)
    for k in ("ds_in", "ds_w"):
        ref, bound = B[k]
        print(f"{name} w{wbit} {k}: reference fp32 {float(f[k]):.6e} float64 {ref:.6e} bound {bound:.3e}")
        assert abs(float(f[k]) - ref) <= bound
    for pert in ("no_g", "no_mask", "q_only", "no_factor"):
        rp = R.layer_grads(kind, geo, f, wbit, torch.float64, perturb=pert)
        for k in ("ds_in", "ds_w"):
            ref, bound = B[k]
            ratio = abs(float(rp[k]) - ref) / bound
            print(f"{name} w{wbit} {pert} {k}: {ratio:.2f} bounds off")
            if (name, wbit, pert, k) in DS_W_BLIND:
                assert ratio <= 1, "no longer an exception: take it off DS_W_BLIND"
            else:
                assert ratio > 1, (pert, k)
    rp = R.layer_grads(kind, geo, f, wbit, torch.float64, perturb="no_factor")
    assert not torch.equal(rp["y"].float(), f["y"])


def _out_items(kind, f, wbit, geo):
    """The output quantiser's fp32 terms of a fixture case in lsq_out_bwd's order ([groups of 8 channels][pixels][8]),
    with q and g."""
    p = R.pre32(kind, geo, f, wbit)
    tm = R.terms(p, f["dy"], f["s_out"], R.FEATURE_BIT)
    C = p.shape[1] if kind == "conv" else p.shape[-1]
    tt = tm["t"].reshape(p.shape[0], C, -1).permute(0, 2, 1) if kind == "conv" else tm["t"]
    tt = tt.reshape(-1, C)
    pad = torch.zeros(tt.shape[0], (C + 7) // 8 * 8)
    pad[:, :C] = tt
    return pad.view(tt.shape[0], -1, 8).permute(1, 0, 2).contiguous(), tm, R.g32(R.FEATURE_BIT, p.numel())


@pytest.mark.parametrize("name,kind,geo,wbit", ALL, ids=IDS)
def test_ds_out_bound_is_for_the_per_element_form(name, kind, geo, wbit):
    f = load_case(name, wbit)
    ref, bound = R.step_grad_bounds(kind, geo, f, wbit)["ds_out"]
    items, tm, g = _out_items(kind, f, wbit, geo)
    assert abs(R.emulate_ds(items, g, "items") - ref) <= bound
    # dropping g, or the -v part, leaves the bound
    assert abs(R.emulate_ds(items, 1.0, "items") - ref) > bound
    assert abs(float((f["dy"] * tm["q"]).double().sum()) * g - ref) > bound
    print(f"{name} w{wbit} ds_out: reference fp32 off by {abs(float(f['ds_out']) - ref):.3e}, bound {bound:.3e}")


def test_k_lsq_is_measured():
    worst = 0.0
    for n in R.KERNEL_SIZES:
        for bit in R.KERNEL_BITS:
            for fam in R.STEP_FAMILIES:
                c = R.quant_case(n, bit, fam)
                t = R.terms(c["x"], c["dy"], c["step"], bit)["t"]
                g = R.g32(bit, n)
                T = R.U24 * g * float(t.double().abs().sum())
                for order, tt in (("flat", t),) + ((("items", _as_items(t)),) if n <= 1025 else ()):
                    worst = max(worst, abs(R.emulate_ds(tt, g, order) - R.ds64(t, g)) / T)
    for name, kind, geo, wbit in ALL:
        f = load_case(name, wbit)
        items, tm, g = _out_items(kind, f, wbit, geo)
        T = R.U24 * g * float(tm["t"].double().abs().sum())
        worst = max(worst, abs(R.emulate_ds(items, g, "items") - R.ds64(tm["t"], g)) / T)
    print("largest emulated ratio", worst)
    assert abs(worst - R.MEASURED) <= 0.005 * R.MEASURED + 1e-3
    assert 2 * worst <= R.K_LSQ <= 3 * worst
    # a perturbed sum leaves the bound: g dropped; q - v replaced by q
    c = R.quant_case(1025, 8, "soft")
    tm = R.terms(c["x"], c["dy"], c["step"], 8)
    g = R.g32(8, 1025)
    assert abs(R.emulate_ds(tm["t"], 1.0) - R.ds64(tm["t"], g)) > R.sum_bound(tm["t"], g)
    assert abs(R.emulate_ds(c["dy"] * tm["q"], g) - R.ds64(tm["t"], g)) > R.sum_bound(tm["t"], g)


def _as_items(t):
    n = t.numel()
    pad = torch.zeros((n + 7) // 8 * 8)
    pad[:n] = t
    return pad.view(1, -1, 8)  # one pixel row per 8 terms, a single channel group


def test_planted_ties_and_bounds():
    for bit in R.KERNEL_BITS:
        c = R.quant_case(63, bit, "dyadic")
        assert torch.equal(R.effective_step(c["step"], bit, 63), c["step"])
        tm = R.terms(c["x"], c["dy"], c["step"], bit)
        qp = R.qp_of(bit)
        want = [min(v, qp) for v in (0.0, 2.0, 2.0)]
        assert tm["q"][:3].tolist() == want and tm["q"][3:6].tolist() == [-w for w in want]
        assert tm["inside"][6:8].all() and not tm["inside"][8:10].any()
        assert tm["q"][10] == 0 and not torch.signbit(tm["q"][10])  # -0.0 gives +0, as round_pass does
        xr = c["x"].clone()
        assert torch.equal(R.quant_lsq(xr, bit, c["step"]).view(torch.int32), (tm["q"] * tm["se"]).view(torch.int32))


def test_init_step_rounding_order():
    x = torch.randn(5, 6, 7, generator=torch.Generator().manual_seed(0))
    s = R.init_step(x, 8)
    assert float(s) != float(x.abs().max() / 127)  # the two rounding orders differ on this input (8th digit)
    assert torch.equal(s, 1 / (1 / x.abs().max() * 127))
    assert float(R.init_step(torch.zeros(4), 8)) == 1.0


# ---- module surface ----------------------------------------------------------------------------------------------------
def _mods():
    from sdmi import layers_qn_lsq as Q
    c = Q.Conv2d_qn_lsq(4, 8, 3, 1, 1, 1, weight_bit=8, input_bit=8, output_bit=8, noise_scale=0.0)
    li = Q.Linear_qn_lsq(6, 5, weight_bit=4, input_bit=8, output_bit=8, noise_scale=0.1)
    return Q, c, li


def test_module_surface():
    Q, c, li = _mods()
    assert "layers_qn_lsq" in type(c).__module__.split(".")
    assert list(c.state_dict()) == ["weight", "bias", "step_size_input", "step_size_output", "step_size_weight"]
    assert list(li.state_dict()) == ["weight", "step_size_input", "step_size_output", "step_size_weight"]  # bias=False
    for m in (c, li):
        assert m.use_FP is False and m.input_quant and m.output_quant and m.weight_quant
        assert m.gain_noise_scale == 0 and m.offset_noise_scale == 0
        for k in ("input", "output", "weight"):
            p = getattr(m, f"step_size_{k}")
            assert isinstance(p, nn.Parameter) and p.dim() == 0 and float(p.detach()) == 1.0
    assert isinstance(c, nn.Conv2d) and isinstance(li, nn.Linear) and li.bias is None and c.bias is not None


def test_update_para_rescales_steps_and_forgets_the_cache():
    Q, c, _ = _mods()
    with torch.no_grad():
        c.step_size_weight.fill_(0.5)
        c.step_size_input.fill_(0.25)
    c._step_seen["weight"] = True
    c.update_para(weight_bit=4, noise_scale=0.05)
    assert c.weight_bit == 4 and c.noise_scale == 0.05 and c.use_FP is False
    assert float(c.step_size_weight) == 0.5 / 2 ** (4 - 8) and float(c.step_size_input) == 0.25
    assert not any(c._step_seen.values())
    c.update_para(use_FP=True, input_bit=6)
    assert c.use_FP and float(c.step_size_input) == 0.25 * 4
    c._step_seen["input"] = True
    c.load_state_dict(c.state_dict())
    assert not any(c._step_seen.values())
    c._step_seen["input"] = True
    c.reset_step_cache()
    assert not any(c._step_seen.values())


def test_convert_keeps_parameters_and_skips_subclasses():
    from sdmi import layers_qn_lsq as Q

    class MyConv(nn.Conv2d):
        pass

    model = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), MyConv(8, 8, 1), nn.Sequential(nn.Linear(8, 4, bias=False)),
                          nn.Linear(4, 2))
    w0, b0, w2 = model[0].weight, model[0].bias, model[2][0].weight
    names = Q.convert(model, weight_bit=4, input_bit=8, output_bit=8, noise_scale=0.1, exclude=["3"], output_quant=False)
    assert names == ["0", "2.0"]
    assert type(model[0]) is Q.Conv2d_qn_lsq and type(model[1]) is MyConv and type(model[2][0]) is Q.Linear_qn_lsq
    assert type(model[3]) is nn.Linear
    assert model[0].weight is w0 and model[0].bias is b0 and model[2][0].weight is w2 and model[2][0].bias is None
    assert model[0].weight_bit == 4 and model[0].noise_scale == 0.1 and model[0].output_quant is False
    assert (model[0].stride, model[0].padding, model[0].kernel_size) == ((1, 1), (1, 1), (3, 3))
    with torch.no_grad():
        model[0].step_size_weight.fill_(0.3)
    again = Q.convert(model, weight_bit=4, input_bit=8, output_bit=8, noise_scale=0.0)
    assert again == ["3"]  # a converted layer is no exact nn.Conv2d any more
    with pytest.raises(ValueError):
        Q.convert(model, weight_bit=4, input_bit=8, output_bit=8, noise_scale=0.0, exclude=["0"], assign=["0"])


def test_register_prepends_to_the_reference_tuples():
    from sdmi import layers_qn_lsq as Q

    class Other(nn.Conv2d):
        pass

    class Reg:  # a stand-in with cim_layers.register_dict's tuple names
        qn_linear_layers = (nn.Bilinear,)
        qn_conv_layers = (Other,)
        qn_layers = qn_linear_layers + qn_conv_layers
        custom_linear_layers = qn_linear_layers
        custom_conv_layers = qn_conv_layers
        custom_layers = custom_linear_layers + custom_conv_layers
        linear_layers = custom_linear_layers + (nn.Linear,)
        conv_layers = custom_conv_layers + (nn.Conv2d,)
        op_layers = linear_layers + conv_layers

    Q.register(Reg)
    Q.register(Reg)  # idempotent
    assert Reg.conv_layers == (Q.Conv2d_qn_lsq, Other, nn.Conv2d)
    assert Reg.linear_layers == (Q.Linear_qn_lsq, nn.Bilinear, nn.Linear)
    assert Reg.qn_conv_layers[0] is Q.Conv2d_qn_lsq and Reg.custom_linear_layers[0] is Q.Linear_qn_lsq
    assert Reg.qn_layers[:2] == (Q.Linear_qn_lsq, Q.Conv2d_qn_lsq) and Reg.custom_layers[:2] == Reg.qn_layers[:2]
    # convert_to_layers' selection rule picks them
    pick = next(cls for cls in Reg.conv_layers if "layers_qn_lsq" in cls.__module__.split("."))
    assert pick is Q.Conv2d_qn_lsq


def test_cpu_tensors_and_bad_arguments_raise():
    Q, c, li = _mods()
    with pytest.raises(RuntimeError):
        c(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError):
        li(torch.zeros(2, 6))
    with pytest.raises(RuntimeError):
        Q.data_quant_lsq(torch.zeros(4), 8, torch.tensor(0.1))
    with pytest.raises(RuntimeError):
        Q.weight_quant_noise(c)
    with pytest.raises(NotImplementedError):
        Q.data_quant_lsq(torch.zeros(4), 8, torch.tensor(0.1), isint=True)
    for bad in (1, 10, 0):
        with pytest.raises(ValueError):
            Q.data_quant_lsq(torch.zeros(4), bad, torch.tensor(0.1))
    assert Q.weight_quant_lsq is Q.data_quant_lsq and callable(Q.add_noise) and callable(Q.init_step_size)
