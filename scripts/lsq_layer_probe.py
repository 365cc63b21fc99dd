"""Forward + backward time of one LSQ quantise-and-noise layer on the HIP path (sdmi.layers_qn_lsq) against a hand-written
torch restatement of the reference layer (tests/lsq_ref.py RefConv2d / RefLinear: the reference's elementwise
expressions and an fp32 F.conv2d / F.linear) on the same GPU. Three shapes of the cond-UNet
(config/celebhq_text_image_cond.py) at B = 32:

  conv3x3  : 256 -> 256, k3 s1 p1 on 32 x 32   (a first-level resnet convolution)
  conv1x1  : 256 -> 384, k1 on 32 x 32         (a residual_input_conv)
  linear   : 512 -> 384 on (32, 77, 512)       (a text context_proj)

at weights 8 and 4 bit, features 8 bit, noise_scale 0 and 0.1. Both layers share weights and already-initialised
steps. Every (shape, setting, path) is warmed up, then the two paths are alternated `--rounds` times; one sample is a
host clock around `--iters` forward + backward passes (400: 0.1 to 0.8 s per sample) ending in a device synchronise.
Reported: ms per pass as median / min / max, and the ratio of the medians. Needs the MI355X: there is no fallback. Writes --out (default
profiles/lsq_layers.json)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]
import torch  # noqa: E402

SHAPES = (("conv3x3", "conv", (256, 256, 3, 1, 1), (32, 256, 32, 32)),
          ("conv1x1", "conv", (256, 384, 1, 1, 0), (32, 256, 32, 32)),
          ("linear", "linear", (512, 384, True), (32, 77, 512)))


def build_pair(kind, geo, wbit, ns, dev):
    from sdmi import layers_qn_lsq as Q
    from tests import lsq_ref as R
    kw = dict(weight_bit=wbit, input_bit=8, output_bit=8, noise_scale=ns)
    if kind == "conv":
        ci, co, k, s, p = geo
        hip = Q.Conv2d_qn_lsq(ci, co, k, s, p, 1, bias=True, **kw)
        ref = R.RefConv2d(ci, co, k, s, p, bias=True)
    else:
        fi, fo, bias = geo
        hip = Q.Linear_qn_lsq(fi, fo, bias=bias, **kw)
        ref = R.RefLinear(fi, fo, bias=bias)
    ref._setup(**kw)
    hip, ref = hip.to(dev), ref.to(dev)
    ref.load_state_dict(hip.state_dict())
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
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lsq_layers.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lsq_layer_probe needs the MI355X (no GPU found; there is no fallback)")
    from sdmi import _build
    dev = torch.device("cuda", 0)
    result = {"_meta": {"unit": "ms per forward + backward of one layer", "batch": 32, "iters": a.iters,
                        "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                        "timing": "host clock around `iters` passes ending in a device synchronise, after a warm-up "
                                  "of both paths; the two paths alternated within one process",
                        "torch": "tests/lsq_ref.py restatement of the reference layer, fp32 F.conv2d / F.linear",
                        "source_digest": _build.source_digest()}}
    for name, kind, geo, shape in SHAPES:
        g = torch.Generator().manual_seed(len(name))
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        for wbit in (8, 4):
            for ns in (0.0, 0.1):
                hip, ref = build_pair(kind, geo, wbit, ns, dev)
                with torch.no_grad():
                    y = hip(x)  # initialises the steps
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
                key = f"{name}.w{wbit}.noise{ns}"
                result[key] = row
                print(key, json.dumps(row))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
