"""The ADC/DAC-aware CIM layers on the GPU against the reference's fixture (tests/golden/adda_layers.safetensors) and the
bounds of tests/adda_ref.py. Each case prints its figures before it asserts."""
from unittest import mock

import pytest
import torch

from tests import adda_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX, META = A.load_fixture()


def _layer(name, fresh=False):
    import sdmi.layers_qn_lsq_adda_cim as M
    c, f = A.CASES[name], FX[name]
    if c["kind"] == "conv":
        m = M.Conv2d_lsq_adda_cim(c["geo"][0], c["geo"][1], 1, 1, 0, 1, bias=True, **c["cfg"])
    else:
        m = M.Linear_lsq_adda_cim(c["geo"][0], c["geo"][1], bias=True, **c["cfg"])
    m = m.to(DEV)
    with torch.no_grad():
        m.weight.copy_(f["w"].reshape(m.weight.shape))
        m.bias.copy_(f["b"])
        if not fresh:
            for k, s in (("input", "s_in"), ("weight", "s_w"), ("output", "s_out")):
                getattr(m, f"step_size_{k}").data = f[s].to(DEV)
            m.adc_gain.data = f["gain"].to(DEV)
    for k in ("gain_noise", "offset_noise"):
        v = torch.zeros(1000)
        if k in f:
            v[:f[k].numel()] = f[k]
        setattr(m, k, v.to(DEV))
    M.map_weight(torch.nn.Sequential(m), c["blocks"])
    return m


def _run(name, fresh=False):
    c, f = A.CASES[name], FX[name]
    m = _layer(name, fresh)
    x = f["x"].to(DEV).requires_grad_(True)
    ctx = mock.patch("torch.randn_like", lambda t: f["eps"].to(t.device).reshape(t.shape)) if "eps" in f else mock.patch(
        "torch.is_tensor", torch.is_tensor)
    with ctx:
        y = m(x)
    y.backward(f["dy"].to(DEV))
    torch.cuda.synchronize()
    return m, x, y.detach().cpu()


@pytest.mark.parametrize("name", [n for n in A.CASES if n != "c8_wnoise"])
def test_layer_against_the_reference(name):
    c, f = A.CASES[name], FX[name]
    m, x, y = _run(name, fresh=c["fresh"])
    diff = int((y != f["y"]).sum())
    print(f"{name}: y differs from the reference's in {diff} of {y.numel()} elements")
    b, _ = A.grad_bounds(c, f)
    got = dict(dx=x.grad.cpu(), dw=m.weight.grad.cpu().reshape(f["w"].shape), db=m.bias.grad.cpu(),
               ds_in=m.step_size_input.grad.cpu(), ds_w=m.step_size_weight.grad.cpu(), ds_out=m.step_size_output.grad.cpu(),
               dgain=m.adc_gain.grad.cpu())
    fig = {}
    for k in ("dx", "dw", "db"):
        ref, bd = b[k]
        fig[k] = float(((got[k].double() - ref).abs() / bd.clamp_min(1e-300)).max())
    for k in ("ds_in", "ds_w", "ds_out", "dgain"):
        ref, bd = b[k]
        fig[k] = abs(float(got[k]) - ref) / bd
    print(f"{name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    if c["fresh"]:
        print(f"{name}: host reads: steps {m.step_reads}, gain {m.gain_reads}")
        # each step: read, found 1, initialised, read again; the gain: found at the minimum, the first block's maximum
        # read, found changed before the second block, and once more after the loop
        assert (m.step_reads, m.gain_reads) == (6, 4)
        for k, s in (("input", "s_in"), ("weight", "s_w"), ("output", "s_out")):
            assert torch.equal(getattr(m, f"step_size_{k}").detach().cpu(), f[s]), k
        assert torch.equal(m.adc_gain.detach().cpu(), f["gain"])
        reads = (m.step_reads, m.gain_reads)
        m(f["x"].to(DEV))
        assert (m.step_reads, m.gain_reads) == reads, "a second forward read a step or the gain on the host again"
    assert diff == 0, f"{name}: y differs in {diff} elements"
    assert all(v <= 1.0 for v in fig.values()), fig


def test_weight_noise_against_float64():
    c, f = A.CASES["c8_wnoise"], FX["c8_wnoise"]
    m, x, y = _run("c8_wnoise")
    r = A.layer_grads(c, f, torch.float64)
    near = A.near_tie(r["keep"], c["cfg"], f["map"])
    fed = torch.zeros_like(r["pre"], dtype=torch.bool)
    for (key, i), v in near.items():
        mp = f["map"][key]
        fed[..., mp["start_col"]:mp["start_col"] + mp["col_num"]] |= v
    bad = (y.double() != r["y"].float().double()) & ~fed
    print(f"c8_wnoise: y differs in {int((y.double() != r['y'].float().double()).sum())} elements, {int(bad.sum())} of them "
          f"not fed by an ADC input within tau of a tie; {int(fed.sum())} elements are fed by one")
    assert int(bad.sum()) == 0
    # gradients: the float64 restatement on the same eps; the data gradient multiplies the bf16 high part of w_qn alone
    b, _ = A.grad_bounds(c, f, w_rel=2.0 ** -8)
    got = dict(dx=x.grad.cpu(), dw=m.weight.grad.cpu(), db=m.bias.grad.cpu(), ds_in=m.step_size_input.grad.cpu(),
               ds_w=m.step_size_weight.grad.cpu(), dgain=m.adc_gain.grad.cpu())
    fig = {}
    for k, v in got.items():
        ref, bd = b[k]
        fig[k] = float(((v.double() - ref).abs() / bd.clamp_min(1e-300)).max()) if torch.is_tensor(ref) else \
            abs(float(v) - ref) / bd
    print("c8_wnoise: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert all(v <= 1.0 for v in fig.values()), fig


DIT_CFG = dict(weight_bit=4, input_bit=8, output_bit=8, noise_scale=0, dac_bit=5, adc_bit=8, adc_gain_1_scale=9.071428571,
               adc_gain_range=[1 / 64, 1 / 64], adc_adjust_mode="current")
DIT_BLOCKS = (64, 2048)  # the small DiT's widest layer has 384 rows: six row blocks there, one in most layers
# Gradient movement of the converted SMALL_DIT allowed against the same model on the restatement layers: the global
# relative error over all parameter gradients. Measured on the CPU on the restatement-layer model itself: fp32 against
# the same model with every layer's d_pre rounded to bf16 (the rounding the HIP path adds) moved the gradients by
# MEASURED_WHOLE_DIT; the tolerance is three times that. The outputs of the two models are compared bit for bit:
# every other leaf runs the same kernels in both.
MEASURED_WHOLE_DIT = 1.67e-3  # 155 parameter gradients, 26 converted layers, the test's inputs
WHOLE_DIT_TOL = 3 * MEASURED_WHOLE_DIT


def _dit_pair():
    import copy
    import sdmi.layers_qn_lsq_adda_cim as M
    from models.transformer import DIT
    from oracle import dit_oracle as DO, sd_oracle as O
    from tests.golden.configs import SMALL_DIT
    model = DIT(4, SMALL_DIT)
    model.load_state_dict(O.deterministic_state(DO.dit_param_shapes(SMALL_DIT), seed=5))
    model = model.to(DEV)
    twin = copy.deepcopy(model)
    names = M.convert(model, **DIT_CFG)
    assert names == A.convert_ref(twin, dict(DIT_CFG, gain_noise_scale=0, offset_noise_scale=0), DIT_BLOCKS)
    assert len(names) == 26 and set(M.map_weight(model, DIT_BLOCKS)) == set(names)
    g = torch.Generator().manual_seed(70)
    x0, noise, t = torch.randn(2, 4, 32, 32, generator=g), torch.randn(2, 4, 32, 32, generator=g), \
        torch.randint(0, 1000, (2,), generator=g)
    text = torch.randn(2, 77, 64, generator=g)
    mask = torch.nn.functional.one_hot(torch.randint(0, 19, (2, 64, 64), generator=g), 19).movedim(-1, 1)[:, 1:].float()
    mask = mask * 0.8 + 0.2 * torch.rand(2, 18, 64, 64, generator=g)  # a soft mask, as in tests/test_lsq_layers_gpu.py
    return model, twin, (x0.to(DEV), t.to(DEV), {"text": text.to(DEV), "image": mask.to(DEV)}), noise.to(DEV)


def test_whole_dit_converted():
    model, twin, (x0, t, cond), noise = _dit_pair()
    grads = []
    outs = []
    for net in (model, twin):
        out = net(x0, t, cond_input=cond)
        torch.nn.functional.mse_loss(out, noise).backward()
        outs.append(out.detach())
        grads.append({k: p.grad.detach().double() for k, p in net.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    assert grads[0].keys() == grads[1].keys() and sum("adc_gain" in k for k in grads[0]) == 26
    diff = int((outs[0] != outs[1]).sum())
    num = sum(float(((grads[0][k] - grads[1][k]) ** 2).sum()) for k in grads[0]) ** 0.5
    den = sum(float((grads[1][k] ** 2).sum()) for k in grads[1]) ** 0.5
    print(f"converted DiT against the restatement layers: output differs in {diff} of {outs[0].numel()} elements, "
          f"gradients move by {num / den:.3e} (allowed {WHOLE_DIT_TOL})")
    assert all(bool(torch.isfinite(v).all()) for v in grads[0].values())
    assert diff == 0
    assert num / den <= WHOLE_DIT_TOL


def test_use_fp_update_para_and_errors():
    import sdmi.layers_qn_lsq_adda_cim as M
    m = _layer("c2_small")
    f = FX["c2_small"]
    x = f["x"].to(DEV)
    m.update_para(use_FP=True)
    ref = torch.nn.functional.linear(f["x"], f["w"], f["b"])
    assert float((m(x).cpu() - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
    s_in, gain = float(m.step_size_input), float(m.adc_gain)
    m.update_para(input_bit=7, adc_bit=7)
    assert float(m.step_size_input) == s_in * 2 and float(m.adc_gain) == pytest.approx(gain / 2)
    assert m(x).shape == (2, 3, 40)
    del m.weight_mapping_info
    with pytest.raises(RuntimeError, match="weight_mapping_info"):
        m(x)
    big = M.Linear_lsq_adda_cim(16, 1001, bias=False, **dict(A.CASES["c6_adcnoise"]["cfg"])).to(DEV)
    M.map_weight(torch.nn.Sequential(big), (8, 2048))
    with pytest.raises(ValueError, match="1000"):
        big(torch.randn(2, 16, device=DEV))
