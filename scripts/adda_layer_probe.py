"""Forward + backward time of one ADC/DAC-aware CIM layer on the HIP path (sdmi.layers_qn_lsq_adda_cim) against a
hand-written torch restatement of the reference layer (tests/adda_ref.py RefLinear: the reference's elementwise
expressions and one fp32 torch.matmul per (array block, input slice)) on the same GPU. The linear shapes of the
reference's 9-layer DiT (hidden 288, 9 heads of 32, 256 tokens) at the stage's batch of 16, arrays of 576 x 2048:

  qkv      : 288 -> 864 on (16, 256, 288)     attn_out : 288 -> 288 on (16, 256, 288)
  ff_in    : 288 -> 1152 on (16, 256, 288)    ff_out   : 1152 -> 288 on (16, 256, 1152)   (two row blocks)
  adaln    : 288 -> 1728 on (16, 288)

at weights 4 bit, ADC 8 bit, (input, DAC) bits 8 / 5 and 5 / 5, weight noise 0 and 0.08. Both layers share weights and
already-initialised steps and gain. Every (shape, setting, path) is warmed up, then the two paths are alternated
`--rounds` times; one sample is a host clock around `--iters` forward + backward passes ending in a device synchronise.
Reported: ms per pass as median / min / max and the ratio of the medians, for every shape; no ratio is fixed beforehand.
Needs the MI355X: there is no fallback. Writes --out (default profiles/adda_layers.json)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]
import torch  # noqa: E402

SHAPES = (("qkv", 288, 864, (16, 256, 288)), ("attn_out", 288, 288, (16, 256, 288)), ("ff_in", 288, 1152, (16, 256, 288)),
          ("ff_out", 1152, 288, (16, 256, 1152)), ("adaln", 288, 1728, (16, 288)))
BLOCKS = (576, 2048)


def build_pair(fi, fo, cfg, dev):
    from sdmi import layers_qn_lsq_adda_cim as M
    from tests import adda_ref as A
    hip = M.Linear_lsq_adda_cim(fi, fo, bias=True, **cfg)
    ref = A.RefLinear(fi, fo, bias=True)
    ref._setup(dict(cfg, gain_noise_scale=0, offset_noise_scale=0), BLOCKS)
    hip, ref = hip.to(dev), ref.to(dev)
    M.map_weight(torch.nn.Sequential(hip), BLOCKS)
    return hip, ref


def one_pass(m, x, dy):
    x.grad = None
    for p in m.parameters():
        p.grad = None
    m(x).backward(dy)


def sample(m, x, dy, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        one_pass(m, x, dy)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adda_layers.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adda_layer_probe needs the MI355X (no GPU found; there is no fallback)")
    from sdmi import _build
    dev = torch.device("cuda", 0)
    result = {"_meta": {"unit": "ms per forward + backward of one layer", "batch": 16, "iters": a.iters,
                        "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                        "timing": "host clock around `iters` passes ending in a device synchronise, after a warm-up "
                                  "of both paths; the two paths alternated within one process",
                        "torch": "tests/adda_ref.py restatement of the reference layer, one fp32 matmul per (block, slice)",
                        "source_digest": _build.source_digest()}}
    for name, fi, fo, shape in SHAPES:
        g = torch.Generator().manual_seed(len(name))
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        for ib, db in ((8, 5), (5, 5)):
            for ns in (0.0, 0.08):
                cfg = dict(weight_bit=4, input_bit=ib, output_bit=8, noise_scale=ns, dac_bit=db, adc_bit=8,
                           adc_gain_1_scale=9.071428571, adc_gain_range=[1 / 64, 1 / 64], adc_adjust_mode="current")
                hip, ref = build_pair(fi, fo, cfg, dev)
                with torch.no_grad():
                    y = hip(x)  # initialises the steps and the gain
                    ref.load_state_dict(hip.state_dict())
                    yr = ref(x)
                dy = torch.randn(y.shape, generator=g).to(dev)
                same = float((y - yr).abs().max() / yr.abs().max()) if ns == 0 else None
                for m in (hip, ref):
                    for _ in range(3):
                        one_pass(m, x, dy)
                t = {"hip": [], "torch": []}
                for _ in range(a.rounds):
                    t["hip"].append(sample(hip, x, dy, a.iters))
                    t["torch"].append(sample(ref, x, dy, a.iters))
                row = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}
                row["torch_over_hip"] = row["torch"]["median"] / row["hip"]["median"]
                row["output_difference_share_of_scale"] = same
                key = f"{name}.in{ib}dac{db}.noise{ns}"
                result[key] = row
                print(key, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
