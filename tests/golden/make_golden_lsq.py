"""Generates tests/golden/lsq_layers.safetensors by running the REFERENCE's own Conv2d_qn_lsq / Linear_qn_lsq
(cim_layers/layers_qn_lsq.py) on the CPU. Data only: inputs, parameters, steps, dy, outputs and all gradients.

Run:  SDMI_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lsq.py

Cases (tests/lsq_ref.py CASES), each at weight bits 8 and 4 with features at 8 bit and noise_scale = 0. The steps are the
reference's own first-forward initialisation times 0.75 (input), 0.8 (weight), 0.7 (output): straight after the
initialisation the extreme element sits within 1e-6 code units of the clamp bound, where its mask bit is a coin toss
between two correct implementations; the factors move it away and put elements into the clamped branch. Seeds are walked
until, evaluated in float64, every quantiser input is at least 1e-3 code units from a rounding tie and from +-Qp.

A case has up to 8900 quantiser inputs, and n independent inputs all stay 1e-3 away from a tie with probability
(1 - 2e-3)^n: no seed would ever pass. So the elements of x and of the weight that lie within 2e-3 code units of a tie or of
+-Qp are first moved to 2e-3 from it (never the extreme element, which the factors put far outside the range, so the
reference's initialisation is unchanged); the walk is then over the pre-activation alone, 240 - 2880 outputs."""
import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get("SDMI_REFERENCE")
if not REF:
    raise SystemExit("set SDMI_REFERENCE to the reference checkout")
if REF not in sys.path:
    sys.path.insert(1, REF)

from tests import lsq_ref as R  # noqa: E402

torch.set_num_threads(8)
MAX_SEEDS = 4000


def build(ref, kind, geo, wbit):
    kw = dict(weight_bit=wbit, input_bit=R.FEATURE_BIT, output_bit=R.FEATURE_BIT, noise_scale=0)
    if kind == "conv":
        ci, co, k, s, p = geo
        return ref.Conv2d_qn_lsq(ci, co, k, s, p, 1, bias=True, **kw)
    fi, fo, bias = geo
    return ref.Linear_qn_lsq(fi, fo, bias=bias, **kw)


NUDGE = 2 * R.TIE_DISTANCE


def nudge(x, step, bit):
    """x with every element within NUDGE code units of a rounding tie (inside the range) or of +-Qp moved to NUDGE
    from it; evaluated in float64 against the effective step."""
    qp = R.qp_of(bit)
    se = R.effective_step(step.double(), bit, x.numel())
    v = x.double() / se
    tie = torch.floor(v) + 0.5
    d = v - tie
    side = torch.where(d >= 0, 1.0, -1.0).double()
    v2 = torch.where((d.abs() < NUDGE) & (v.abs() < qp), tie + side * NUDGE, v)
    b = v.abs() - qp
    sb = torch.where(b >= 0, 1.0, -1.0).double()
    v2 = torch.where(b.abs() < NUDGE, torch.sign(v) * (qp + sb * NUDGE), v2)
    return torch.where(v2 != v, (v2 * se).float(), x)


def one(ref, kind, geo, shape, wbit, seed):
    torch.manual_seed(seed)
    m = build(ref, kind, geo, wbit)
    x = torch.randn(shape)
    with torch.no_grad():
        want_in = R.init_step(x, R.FEATURE_BIT) * R.STEP_FACTORS["input"]
        want_w = R.init_step(m.weight, wbit) * R.STEP_FACTORS["weight"]
        x = nudge(x, want_in, R.FEATURE_BIT)
        m.weight.copy_(nudge(m.weight, want_w, wbit))
        R.quiet(m, x)  # the reference initialises its three steps here
        m.step_size_input.mul_(R.STEP_FACTORS["input"])
        m.step_size_weight.mul_(R.STEP_FACTORS["weight"])
        m.step_size_output.mul_(R.STEP_FACTORS["output"])
        assert torch.equal(m.step_size_input, want_in) and torch.equal(m.step_size_weight, want_w)
    f = dict(x=x, w=m.weight.detach().clone(), s_in=m.step_size_input.detach().clone(),
             s_w=m.step_size_weight.detach().clone(), s_out=m.step_size_output.detach().clone())
    if m.bias is not None:
        f["b"] = m.bias.detach().clone()
    vx, vw, vp = R.quantiser_inputs64(kind, geo, f, wbit)
    dist = min(R.tie_distance(vx, R.FEATURE_BIT), R.tie_distance(vw, wbit), R.tie_distance(vp, R.FEATURE_BIT))
    if dist < R.TIE_DISTANCE:
        return None, dist
    xr = x.clone().requires_grad_(True)
    y = R.quiet(m, xr)
    f["dy"] = torch.randn(y.shape)
    y.backward(f["dy"])
    f.update(y=y.detach(), dx=xr.grad, dw=m.weight.grad, ds_in=m.step_size_input.grad, ds_w=m.step_size_weight.grad,
             ds_out=m.step_size_output.grad)
    if m.bias is not None:
        f["db"] = m.bias.grad
    clamped = [int((v.abs() > R.qp_of(b)).sum()) for v, b in ((vx, R.FEATURE_BIT), (vw, wbit), (vp, R.FEATURE_BIT))]
    return f, (dist, clamped)


def main():
    import cim_layers.layers_qn_lsq as ref
    out = {}
    for name, kind, geo, shape in R.CASES:
        for wbit in R.WEIGHT_BITS:
            for seed in range(MAX_SEEDS):
                f, info = one(ref, kind, geo, shape, wbit, seed)
                if f is not None:
                    break
            else:
                raise SystemExit(f"{name} w{wbit}: no seed below {MAX_SEEDS} meets the distance condition")
            print(f"{name} w{wbit}: seed {seed}, distance {info[0]:.2e}, clamped (x, w, pre) {info[1]}")
            for k, v in f.items():
                out[f"{name}.w{wbit}.{k}"] = v.detach().reshape(-1).contiguous() if v.dim() == 0 else v.contiguous()
            out[f"{name}.w{wbit}.seed"] = torch.tensor([seed])
    path = os.path.join(HERE, "lsq_layers.safetensors")
    save_file(out, path)
    print("fixture written to", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
