"""What the latent-range noise of the noise-robust VQVAE costs, on one build, within one process.

  step    the `vqvae-train` configuration of bench.py (celebhq autoencoder, 256 x 256, B = 8, recorded plan replayed)
          at n_scale = 0.2 against n_scale = 0: two trainers, each with its own recorded plan, alternated round by
          round; ms per step = the time of `--steps` replays ending in a device synchronise / steps.
  latent  on a latent of that shape (8, 4, 32, 32): out = z + (z.max() - z.min()) * n_scale * eps and the gradient of
          sum(out * g) with respect to z, as the torch expression with autograd (eager; about ten launches) against the
          kernels of csrc/latent_noise.hip (sdmi_latent_range + sdmi_latent_noise_fwd + sdmi_latent_noise_bwd: four
          launches, eps given in both cases); us per forward + backward over `--iters` iterations.

Every loop is warmed up before it is timed; the pairs are alternated `--rounds` times and reported as median / min /
max over the rounds. Needs the MI355X: there is no fallback. Writes --out (default profiles/vq_noise_train.json)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]
import torch  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vq_noise_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vq_noise_probe needs the MI355X (no GPU found; there is no fallback)")
    from models.vqvae import VQVAE
    from sdmi import _build
    from sdmi import kernels as K
    from sdmi.plan import StepPlan
    from sdmi.vqvae_train import VQVAETrainer
    from tests.golden.configs import vqvae_celebhq_config
    dev = torch.device("cuda", 0)
    cfg = vqvae_celebhq_config()
    torch.manual_seed(1111)
    init = VQVAE(3, cfg).state_dict()
    B = 8
    x = (torch.rand(B, 3, 256, 256, generator=torch.Generator().manual_seed(1111)) * 2 - 1).to(dev)
    result = {"_meta": {"config": "vqvae-train: celebhq autoencoder, 256x256, B=8, recon + codebook + commitment, Adam",
                        "n_scale": a.n_scale, "steps": a.steps, "iters": a.iters, "rounds": a.rounds,
                        "timing": "host clock around a window ending in a device synchronise, after a warm-up of "
                                  "every loop; the two sides of each pair alternated within one process",
                        "device": torch.cuda.get_device_name(0), "source_digest": _build.source_digest()}}
    # ---- the training step -------------------------------------------------------------------------------
    replay, launches, keep = {}, {}, []  # keep: a plan replays into its trainer's buffers
    for name, ns in (("clean", 0.0), ("noise", a.n_scale)):
        tr = VQVAETrainer(cfg, {k: v.to(dev) for k, v in init.items()}, dev, n_scale=ns, noise_seed=1)
        for _ in range(2):
            tr.step(x)
        plan = StepPlan(lambda tr=tr: tr.step(x), dev)
        for _ in range(3):
            plan.replay()
        replay[name], launches[name] = plan.replay, plan.info()[1]
        keep.append((tr, plan))
    ms = {name: [] for name in replay}
    for _ in range(a.rounds):
        for name, fn in replay.items():
            ms[name].append(timed(fn, a.steps) * 1e3)
    step = {name: summary(v) for name, v in ms.items()}
    step["launches"] = launches
    step["noise_minus_clean_ms"] = step["noise"]["median"] - step["clean"]["median"]
    step["noise_over_clean"] = step["noise"]["median"] / step["clean"]["median"]
    result["step_ms"] = step
    print(f"step: clean {step['clean']['median']:.3f} ms [{step['clean']['min']:.3f}, {step['clean']['max']:.3f}], "
          f"noise {step['noise']['median']:.3f} ms [{step['noise']['min']:.3f}, {step['noise']['max']:.3f}], "
          f"launches {launches}", flush=True)
    # ---- the latent alone --------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(7)
    z0, eps, g = (torch.randn(B, 4, 32, 32, generator=gen).to(dev) for _ in range(3))
    n = z0.numel()

    def torch_expr():
        z = z0.detach().requires_grad_(True)
        out = z + (z.max() - z.min()) * a.n_scale * eps
        (dz,) = torch.autograd.grad(out, z, g)
        return out, dz

    rws, ws = K.latent_noise_ws(n, dev), K.latent_noise_ws(n, dev)
    out_k, r_k = torch.empty_like(z0), torch.empty_like(z0)

    def kernels():
        K.latent_range(z0, rws)
        K.latent_noise_fwd(z0, eps, 1, 1, n, a.n_scale, rws, out_k)
        K.latent_noise_bwd(None, 0, None, g, eps, z0, 1, 1, n, a.n_scale, rws, ws, r_k)
        return out_k, r_k

    ot, dt = torch_expr()
    ok, dk = kernels()
    torch.cuda.synchronize()
    for fn in (torch_expr, kernels):
        timed(fn, 50)
    us = {"torch_autograd": [], "kernels": []}
    for _ in range(a.rounds):
        us["torch_autograd"].append(timed(torch_expr, a.iters) * 1e6)
        us["kernels"].append(timed(kernels, a.iters) * 1e6)
    lat = {name: summary(v) for name, v in us.items()}
    lat["shape"] = [B, 4, 32, 32]
    lat["out_bitwise_equal"] = bool(torch.equal(ot, ok))
    lat["grad_max_abs_diff"] = float((dt - dk).abs().max())
    lat["grad_max_abs"] = float(dt.abs().max())
    lat["torch_over_kernels"] = lat["torch_autograd"]["median"] / lat["kernels"]["median"]
    result["latent_us"] = lat
    print(f"latent: torch + autograd {lat['torch_autograd']['median']:.1f} us, kernels {lat['kernels']['median']:.1f} us "
          f"(issued eagerly through ctypes), out bitwise equal {lat['out_bitwise_equal']}, max |grad diff| "
          f"{lat['grad_max_abs_diff']:.3e} of {lat['grad_max_abs']:.3e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
