"""What classifier-free guidance costs per reverse step: the full cond-UNet (config/celebhq_text_image_cond.py),
DDIM with 50 steps, B = 1 and B = 8, seeded inputs, three loops alternated within one process:

  unguided : the captured loop (DDIMSampler.forward, guidance_scale = 1);
  guided   : the captured guided loop (guidance_scale = 3: one doubled-batch forward + the combine kernel per step);
  wrapper  : what a user of the reference's generator scripts had before -- a _GuidedWrapper-style module handed to
             DDIMSampler (two module forwards plus torch arithmetic per step, issued eagerly);
  unguided_2B : the captured unguided loop at batch 2B (the same doubled-batch forward without the combine).

Every loop is warmed up at every shape, then timed `--rounds` times in turn (host clock around a whole 50-step run
that ends in a device synchronise); ms per step = run time / steps, reported as median / min / max over the rounds.
Needs the MI355X: there is no fallback. Writes --out (default profiles/cfg_sample.json)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]
import torch  # noqa: E402


class GuidedWrapper(torch.nn.Module):
    """The generator scripts' wrapper: two forwards of the wrapped model and the combine in torch."""

    def __init__(self, base, uncond, scale):
        super().__init__()
        self.base, self.uncond, self.scale = base, uncond, scale

    def forward(self, x, t, cond):
        c = self.base(x, t, cond)
        u = self.base(x, t, self.uncond)
        return u + self.scale * (c - u)


def inputs(B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    cmap = torch.randint(0, 19, (B, 512, 512), generator=g)
    mask = torch.nn.functional.one_hot(cmap, 19).movedim(-1, 1)[:, 1:].float().contiguous()
    c = {"text": torch.randn(B, 77, 512, generator=g).to(dev), "image": mask.to(dev)}
    u = {"text": torch.randn(1, 77, 512, generator=g).expand(B, 77, 512).contiguous().to(dev),
         "image": torch.zeros_like(c["image"])}
    return torch.randn(B, 4, 32, 32, generator=g).to(dev), c, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cfg_sample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cfg_sample_probe needs the MI355X (no GPU found; there is no fallback)")
    from oracle import sd_oracle as O
    from tests.golden.configs import full_cond_config
    from scheduler.linear_noise_scheduler import DDIMSampler
    from sdmi import _build
    import models.unet_cond_base as mc
    dev = torch.device("cuda", 0)
    cfg = full_cond_config()
    model = mc.Unet(4, cfg)
    model.load_state_dict(O.deterministic_state(O.unet_param_shapes(cfg), seed=2))
    model = model.to(dev).eval()
    result = {"_meta": {"config": "celebhq_text_image_cond (full cond-UNet)", "sampler": "ddim", "steps": a.steps,
                        "eta": 0.0, "guidance_scale": a.scale, "rounds": a.rounds, "unit": "ms per reverse step",
                        "timing": "host clock around a whole run ending in a device synchronise, after a warm-up "
                                  "run of every loop at every shape; loops alternated within one process",
                        "device": torch.cuda.get_device_name(0), "source_digest": _build.source_digest()}}
    for B in a.batches:
        xT, c, u = inputs(B, dev, 100 + B)
        c2 = {k: torch.cat([c[k], u[k]]) for k in c}
        x2 = torch.cat([xT, xT])
        # one sampler per loop: each keeps its own recorded loop across the rounds
        plain, guided, plain2 = (DDIMSampler(model, (0.0001, 0.02), 1000) for _ in range(3))
        wrapped = DDIMSampler(GuidedWrapper(model, u, a.scale), (0.0001, 0.02), 1000)
        kw = dict(steps=a.steps, eta=0.0, seed=1)
        loops = {"unguided": lambda: plain(xT, c, None, **kw),
                 "guided": lambda: guided(xT, c, u, guidance_scale=a.scale, **kw),
                 "wrapper": lambda: wrapped(xT, c, u, steps=a.steps, eta=0.0),
                 "unguided_2B": lambda: plain2(x2, c2, None, **kw)}
        outs = {}
        for name, fn in loops.items():  # warm-up: every shape, every recording
            outs[name] = fn().clone()
        torch.cuda.synchronize()
        ms = {name: [] for name in loops}
        for _ in range(a.rounds):
            for name, fn in loops.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
               for name, v in ms.items()}
        # the wrapper evaluates the same guided sampler through two batch-B forwards: the same bf16 forward in another
        # fp32 summation order (split counts are keyed by shape). One prediction differs by rounding; the 50-step
        # trajectories of this random-weight model then drift apart, so both are reported with their scales.
        d = (outs["guided"] - outs["wrapper"]).abs().max().item()
        row["guided_vs_wrapper_max_abs_diff"] = d
        row["guided_x0_max_abs"] = outs["guided"].abs().max().item()
        with torch.no_grad():
            t0 = torch.full((B,), 981, device=dev, dtype=torch.long)
            e2 = model(x2, torch.cat([t0, t0]), c2)
            e1 = wrapped.model(xT, t0, c)
        row["one_prediction_max_abs_diff"] = ((e2[B:] + a.scale * (e2[:B] - e2[B:])) - e1).abs().max().item()
        row["one_prediction_max_abs"] = e1.abs().max().item()
        row["guided_over_unguided"] = row["guided"]["median"] / row["unguided"]["median"]
        row["guided_over_wrapper"] = row["guided"]["median"] / row["wrapper"]["median"]
        result[f"B={B}"] = row
        print(f"B={B}: " + "  ".join(f"{n} {row[n]['median']:.3f} ms [{row[n]['min']:.3f}, {row[n]['max']:.3f}]"
                                     for n in loops) + f"  | guided / unguided {row['guided_over_unguided']:.2f}, "
              f"guided / wrapper {row['guided_over_wrapper']:.2f}, max |guided - wrapper| x_0 {d:.3e} of "
              f"{row['guided_x0_max_abs']:.3e}, one prediction {row['one_prediction_max_abs_diff']:.3e} of "
              f"{row['one_prediction_max_abs']:.3e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
