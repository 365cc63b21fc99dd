"""Generates tests/golden/adda_layers.safetensors by running the REFERENCE's own Linear_lsq_adda_cim /
Conv2d_lsq_adda_cim (cim_layers/layers_qn_lsq_adda_cim.py) on the CPU. Data only: inputs, parameters, noise vectors, the
mapping as numbers, outputs and gradients, and the two classes' state-dict key lists (file metadata).

Run:  SDMI_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adda.py

Cases: tests/adda_ref.py CASES. To stay below the size of lsq_layers.safetensors
  * a weight is an int8 multiple k of 2^-10 (`w_k`; the 1300 x 96 weight is 125 KB that way, not 499 KB) and cases that
    vary one setting of another case share its x, weight and dy (`data`);
  * of dw every n-th row is recorded (tests/adda_ref.py dw_rows); the tests compare the other rows with the float64
    restatement, which the recorded rows tie to the reference;
  * of the 1000-entry ADC noise vectors the first `out_features` entries are recorded (the layer reads no others);
  * the weight noise `eps` is a draw rounded to fp16 and stored as fp16; the reference's randn_like is patched to
    return it.
Steps: the reference's own first-forward initialisation times 0.75 / a factor near 0.7 (weight_plan) / 0.7 as in make_golden_lsq.py, except in the
fresh case, which records the first forward itself (steps and gain before and after). Seeds are walked until, in float64,
every input of the three LSQ quantisers of every case of a group lies 1e-3 code units from a rounding tie and from +-Qp
(x is nudged first, as in make_golden_lsq.py; the weight's few distinct values are only checked) and, in the fresh
case, the clamp masks decided in fp32 and in float64 agree (the extreme element sits on the bound there).
One more condition (weight_plan): the weight's codes survive the reference's q * se / se.detach() in fp32 (fl(fl(q se) /
se) == q for every code in use). Where they do not, the reference's weight operand sits one ulp beside an integer, its
fp32 matmul is no longer exact and, where an ADC input then lands on a rounding tie (0.0375 x 40 = 1.5 in the 'gain'
case), its result depends on the BLAS's order of additions: no implementation could be held to it bit for bit. The
input's codes are NOT held to that: there the reference's floor() turns the ulp into a whole code, and the kernels follow it."""
import os
import sys
from unittest import mock

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

from tests import adda_ref as A  # noqa: E402
from tests import lsq_ref as LR  # noqa: E402
from tests.golden.make_golden_lsq import nudge  # noqa: E402

torch.set_num_threads(8)
MAX_SEEDS = 4000


def build(ref, case):
    cfg = case["cfg"]
    if case["kind"] == "conv":
        m = ref.Conv2d_lsq_adda_cim(case["geo"][0], case["geo"][1], 1, 1, 0, 1, bias=True, **cfg)
    else:
        m = ref.Linear_lsq_adda_cim(case["geo"][0], case["geo"][1], bias=True, **cfg)
    m.weight_mapping_info = A.split_dict(case["geo"][0], case["geo"][1], case["blocks"])
    return m


def weight_plan(case, natural, fresh):
    """(extreme k, step factor) of a weight whose kaiming extreme is `natural` grid units: the largest odd extreme (odd:
    at the fresh step max|w| / Qp the codes k Qp / top never sit on a tie) and the first factor of WEIGHT_FACTORS at which
    every code in use survives the reference's q * se / se.detach() in fp32 -- at the fresh step too when the group has a
    fresh case -- and every grid value lies 2e-3 code units from a rounding tie and from +-Qp. Cheap: no layer runs."""
    wb = case["cfg"]["weight_bit"]
    n = case["geo"][0] * case["geo"][1]
    q = torch.arange(-LR.qp_of(wb), LR.qp_of(wb) + 1).float()

    def survives(step):
        se = LR.effective_step(step, wb, n)
        return torch.equal(q * se / se, q)
    for top in range(natural - (1 - natural % 2), natural // 2, -2):
        r = torch.tensor([top * A.GRID])
        if fresh:  # at the fresh step the codes survive too, and fp32 and float64 agree on which side of Qp +-top lies
            s0, kk, qp = LR.init_step(r, wb), torch.tensor([-top, top]) * A.GRID, LR.qp_of(wb)
            v32, v64 = kk / LR.effective_step(s0, wb, n), kk.double() / LR.effective_step(s0.double(), wb, n)
            if not survives(s0) or not torch.equal(v32.abs() <= qp, v64.abs() <= qp):
                continue
        k = torch.arange(-top, top + 1).double() * A.GRID
        for wf in A.WEIGHT_FACTORS:
            step = LR.init_step(r, wb) * wf
            if survives(step) and LR.tie_distance(k / LR.effective_step(step.double(), wb, n), wb) >= 2 * A.TIE_DISTANCE:
                return top, wf
    raise SystemExit("no weight extreme / factor keeps the codes exact")


def data_for(ref, case, gen, fresh):
    """x, the weight on its grid, the bias, dy and the weight's step factor of a data-owning case."""
    torch.manual_seed(int(gen.initial_seed()))  # the layer's own initialisation draws from the global generator
    m = LR.quiet(build, ref, case)
    k = torch.round(m.weight.detach() / A.GRID).clamp(-127, 127)
    top, wf = weight_plan(case, int(round(case["geo"][0] ** -0.5 / A.GRID)), fresh)
    k = k.clamp(-top, top)
    k.view(-1)[0] = top  # the extreme is in the weight whatever the draw
    w = k * A.GRID
    x = torch.randn(case["shape"], generator=gen)
    oshape = (case["shape"][0], case["geo"][1], *case["shape"][2:]) if case["kind"] == "conv" else \
        (*case["shape"][:-1], case["geo"][1])
    return dict(x=x, w=w, w_k=k.to(torch.int8), b=m.bias.detach().clone(), dy=torch.randn(oshape, generator=gen)), wf


def run_case(ref, name, case, data, wf):
    """The reference layer of one case on `data`: the fixture entries, or (None, why)."""
    cfg = case["cfg"]
    ib, wb, ob = cfg["input_bit"], cfg["weight_bit"], cfg["output_bit"]
    m = LR.quiet(build, ref, case)
    with torch.no_grad():
        m.weight.copy_(data["w"])
        m.bias.copy_(data["b"])
    x = data["x"]
    f = dict(b=data["b"], dy=data["dy"])
    patches = []
    if cfg["noise_scale"] != 0:
        eps = torch.randn(data["w"].shape, generator=torch.Generator().manual_seed(77)).half()
        f["eps"] = eps
        patches.append(mock.patch("torch.randn_like", lambda t: eps.float().clone()))
    if cfg["gain_noise_scale"] != 0 or cfg["offset_noise_scale"] != 0:
        N = case["geo"][1]
        f["gain_noise"], f["offset_noise"] = m.gain_noise[:N].clone(), m.offset_noise[:N].clone()
    for p in patches:
        p.start()
    try:
        if case["fresh"]:
            f.update(s_in0=m.step_size_input.detach().clone(), gain0=m.adc_gain.detach().clone())
        else:
            with torch.no_grad():
                m.step_size_input.data = LR.init_step(x, ib) * A.STEP_FACTORS["input"]
                m.step_size_weight.data = LR.init_step(data["w"], wb) * wf
                m.adc_gain.data = torch.tensor(case["gain"] if case["gain"] is not None else 0.016)
                LR.quiet(m, x)  # the reference initialises the output step here
                m.step_size_output.mul_(A.STEP_FACTORS["output"])
        xr = x.clone().requires_grad_(True)
        y = LR.quiet(m, xr)
        y.backward(data["dy"])
    finally:
        for p in patches:
            p.stop()
    f.update(x=x, w=data["w"], s_in=m.step_size_input.detach().clone(), s_w=m.step_size_weight.detach().clone(),
             s_out=m.step_size_output.detach().clone(), gain=m.adc_gain.detach().clone())
    # conditions, in float64 at the steps the forward ran with
    d = torch.float64
    k32 = {}
    with torch.no_grad():
        A.layer_forward(case["kind"], x, f["w"], f["b"], [f[k] for k in ("s_in", "s_w", "s_out")], f["gain"], cfg,
                        m.weight_mapping_info, eps=f["eps"].float() if "eps" in f else None,
                        gain_noise=f.get("gain_noise"), offset_noise=f.get("offset_noise"), keep=k32)
    dec = {k: v for k, v in k32.items() if k != "A" or cfg["noise_scale"] == 0}  # fp32's discrete decisions
    keep = {}
    with torch.no_grad():
        _, pre = A.layer_forward(case["kind"], x.to(d), f["w"].to(d), f["b"].to(d), [f[k].to(d) for k in ("s_in", "s_w", "s_out")],
                                 f["gain"].to(d), cfg, m.weight_mapping_info, eps=f["eps"].to(d) if "eps" in f else None,
                                 gain_noise=f.get("gain_noise"), offset_noise=f.get("offset_noise"), keep=keep, decide=dec)
    if not torch.equal(k32["wq_v"], torch.round(k32["wq_v"])):
        return None, "weight round trip"
    vs = ((x.to(d) / LR.effective_step(f["s_in"].to(d), ib, x.numel()), ib, x),
          (f["w"].to(d) / LR.effective_step(f["s_w"].to(d), wb, f["w"].numel()), wb, f["w"]),
          (pre / LR.effective_step(f["s_out"].to(d), ob, pre.numel()), ob, None))
    if cfg["noise_scale"] != 0:
        vs = vs[:2]
    if case["fresh"]:  # the extreme element sits on +-Qp: rounding ties only, and the masks must agree with fp32
        for v, bit, t32 in vs:
            frac = (v - torch.floor(v) - 0.5).abs()
            if float(frac[v.abs() < LR.qp_of(bit) - 0.5].min()) < A.TIE_DISTANCE:
                return None, "tie"
        p32 = A.layer_forward(case["kind"], x, f["w"], f["b"], [f["s_in"], f["s_w"], f["s_out"]], f["gain"], cfg,
                              m.weight_mapping_info)[1].detach()
        for (v, bit, t32), s in zip(vs, ("s_in", "s_w", "s_out")):
            t32 = p32 if t32 is None else t32
            v32 = t32 / LR.effective_step(f[s], bit, t32.numel())
            qp = LR.qp_of(bit)
            if not torch.equal((v32 >= -qp) & (v32 <= qp), (v >= -qp) & (v <= qp)):
                return None, "mask"
    else:
        dist = min(LR.tie_distance(v, bit) for v, bit, _ in vs)
        if dist < A.TIE_DISTANCE:
            return None, f"distance {dist:.1e}"
    rows = A.dw_rows(name, case["geo"][1])
    f.update(y=y.detach(), dx=xr.grad, dw_rows=m.weight.grad[rows].clone(), db=m.bias.grad, ds_in=m.step_size_input.grad,
             ds_w=m.step_size_weight.grad, ds_out=m.step_size_output.grad, dgain=m.adc_gain.grad,
             mapping=torch.tensor([[v["start_row"], v["start_col"], v["row_num"], v["col_num"]]
                                   for v in m.weight_mapping_info.values()], dtype=torch.int32))
    info = dict(saturation=A.saturation(keep, cfg), keys=list(m.state_dict().keys()),
                map_keys=list(m.weight_mapping_info.keys()))
    return f, info


def main():
    import cim_layers.layers_qn_lsq_adda_cim as ref
    out, meta = {}, {}
    owners = [n for n, c in A.CASES.items() if c["data"] is None]
    for owner in owners:
        group = [owner] + [n for n, c in A.CASES.items() if c["data"] == owner]
        for seed in range(MAX_SEEDS):
            gen = torch.Generator().manual_seed(seed)
            case = A.CASES[owner]
            data, wf = data_for(ref, case, gen, any(A.CASES[n]["fresh"] for n in group))
            cfg = case["cfg"]
            # x off the ties of every step the group's cases use (the factor steps, and the fresh initialisation)
            for fac in (A.STEP_FACTORS["input"], 1.0):
                if fac == 1.0 and not any(A.CASES[n]["fresh"] for n in group):
                    continue
                keep_top = data["x"].abs().argmax()
                top = data["x"].view(-1)[keep_top].clone()
                data["x"] = nudge(data["x"], LR.init_step(data["x"], cfg["input_bit"]) * fac, cfg["input_bit"])
                data["x"].view(-1)[keep_top] = top
            res, why = {}, None
            for n in group:
                f, info = run_case(ref, n, A.CASES[n], data, wf)
                if f is None:
                    why = f"{n}: {info}"
                    break
                res[n] = (f, info)
            if why is None:
                break
        else:
            raise SystemExit(f"{owner}: no seed below {MAX_SEEDS} meets the conditions ({why})")
        for n, (f, info) in res.items():
            print(f"{n}: seed {seed}, weight factor {wf}, saturated {info['saturation']:.4f}, gain {float(f['gain']):.6f}")
            shared = ("x", "w", "b", "dy") if n != owner else ("w",)
            for k, v in f.items():
                if k in shared:
                    continue
                out[f"{n}.{k}"] = v.detach().reshape(-1).contiguous() if v.dim() == 0 else v.detach().contiguous()
            if n == owner:
                out[f"{n}.w_k"] = data["w_k"]
            out[f"{n}.seed"] = torch.tensor([seed])
            meta[f"{n}.map_keys"] = ",".join(info["map_keys"])
            meta[f"{A.CASES[n]['kind']}.state_dict_keys"] = ",".join(info["keys"])
    path = os.path.join(HERE, "adda_layers.safetensors")
    save_file(out, path, metadata=meta)
    print("fixture written to", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
