"""What the KL autoencoder costs beside the VQVAE, on one build, within one process.

  step    the `vqvae-train` configuration of bench.py (celebhq autoencoder, 256 x 256, B = 8, recorded plan replayed):
          sdmi.vae_train.VAETrainer (the KL model: 2z-row encoder head, no codebook) against this tree's
          sdmi.vqvae_train.VQVAETrainer, each with its own recorded plan, alternated round by round; ms per step = the
          time of `--steps` replays ending in a device synchronise / steps.
  latent  the two new entry points alone at the workload's latent (8, 4, 32, 32): sdmi_kl_sample (with the fused
          post_quant_conv and the KL value: two launches) and sdmi_kl_bwd (two launches), issued eagerly through ctypes;
          us per call over `--iters` iterations.
  codec   encode + decode of one (8, 3, 256, 256) batch through the two inference engines (eager issue); ms per pair.

Every loop is warmed up before it is timed; the sides are alternated `--rounds` times and reported as median / min / max
over the rounds. Needs the MI355X: there is no fallback. Writes --out (default profiles/vae_train.json)."""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vae_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_probe needs the MI355X (no GPU found; there is no fallback)")
    from models.vae import VAE
    from models.vqvae import VQVAE
    from sdmi import _build
    from sdmi import kernels as K
    from sdmi.plan import StepPlan
    from sdmi.vae_engine import VAEEngine
    from sdmi.vae_train import VAETrainer
    from sdmi.vqvae_engine import VQVAEEngine
    from sdmi.vqvae_train import VQVAETrainer
    from tests.golden.configs import vqvae_celebhq_config
    dev = torch.device("cuda", 0)
    cfg = vqvae_celebhq_config()
    torch.manual_seed(1111)
    init = {"vq": VQVAE(3, cfg).state_dict(), "kl": VAE(3, cfg).state_dict()}
    B = 8
    x = (torch.rand(B, 3, 256, 256, generator=torch.Generator().manual_seed(1111)) * 2 - 1).to(dev)
    result = {"_meta": {"config": "vqvae-train: celebhq autoencoder, 256x256, B=8, Adam; kl: recon + kl_weight * KL, vq: "
                                  "recon + codebook + commitment",
                        "steps": a.steps, "iters": a.iters, "rounds": a.rounds,
                        "timing": "host clock around a window ending in a device synchronise, after a warm-up of "
                                  "every loop; the sides alternated within one process",
                        "device": torch.cuda.get_device_name(0), "source_digest": _build.source_digest()}}
    # ---- the training step -------------------------------------------------------------------------------
    replay, launches, keep = {}, {}, []  # keep: a plan replays into its trainer's buffers
    for name, cls in (("vq", VQVAETrainer), ("kl", VAETrainer)):
        tr = cls(cfg, {k: v.to(dev) for k, v in init[name].items()}, dev, noise_seed=1)
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
    step["kl_minus_vq_ms"] = step["kl"]["median"] - step["vq"]["median"]
    step["kl_over_vq"] = step["kl"]["median"] / step["vq"]["median"]
    step["losses"] = {"kl": keep[1][0].losses(), "vq": keep[0][0].losses()}
    result["step_ms"] = step
    print(f"step: vq {step['vq']['median']:.3f} ms [{step['vq']['min']:.3f}, {step['vq']['max']:.3f}], "
          f"kl {step['kl']['median']:.3f} ms [{step['kl']['min']:.3f}, {step['kl']['max']:.3f}], launches {launches}",
          flush=True)
    # ---- the two entry points alone ----------------------------------------------------------------------
    z, hw = 4, 32 * 32
    P = B * hw
    gen = torch.Generator().manual_seed(7)
    h = torch.randn(P, 8, generator=gen).to(dev)
    w_pre, b_pre = (0.3 * torch.randn(8, 8, generator=gen)).to(dev), (0.1 * torch.randn(8, generator=gen)).to(dev)
    w_post, b_post = torch.randn(z, z, generator=gen).to(dev), torch.randn(z, generator=gen).to(dev)
    eps = torch.randn(B, z, 32, 32, generator=gen).to(dev)
    dzin = (1e-3 * torch.randn(P, 8, generator=gen)).to(torch.bfloat16).to(dev)
    mom, smp = torch.empty(B, 2 * z, 32, 32, device=dev), torch.empty(B, z, 32, 32, device=dev)
    zin, dh = torch.empty(P, 8, dtype=torch.bfloat16, device=dev), torch.empty(P, 8, dtype=torch.bfloat16, device=dev)
    kl = torch.empty(1, device=dev)
    gw = [torch.empty(n, device=dev) for n in (z * z, z, 64, 8)]

    def sample():
        K.kl_sample(h, 8, w_pre, b_pre, eps, B, z, hw, mom, smp, w_post=w_post, b_post=b_post, zin=zin, ld=8, kl=kl)

    def backward():
        K.kl_bwd(dzin, 8, w_post, smp, mom, eps, h, 8, w_pre, B, z, hw, kl_weight=5e-6, dh=dh, ld_out=8,
                 dw_post=gw[0], db_post=gw[1], dw_pre=gw[2], db_pre=gw[3])

    for fn in (sample, backward):
        timed(fn, 50)
    us = {"kl_sample": [], "kl_bwd": []}
    for _ in range(a.rounds):
        us["kl_sample"].append(timed(sample, a.iters) * 1e6)
        us["kl_bwd"].append(timed(backward, a.iters) * 1e6)
    lat = {name: summary(v) for name, v in us.items()}
    lat["shape"] = [B, z, 32, 32]
    lat["launches"] = {"kl_sample": 2, "kl_bwd": 2}
    result["latent_us"] = lat
    print(f"latent: sdmi_kl_sample {lat['kl_sample']['median']:.1f} us, sdmi_kl_bwd {lat['kl_bwd']['median']:.1f} us "
          "(two launches each, issued eagerly through ctypes with their workspace allocation)", flush=True)
    # ---- encode + decode ---------------------------------------------------------------------------------
    engines = {"vq": VQVAEEngine(cfg, {k: v.to(dev) for k, v in init["vq"].items()}),
               "kl": VAEEngine(cfg, {k: v.to(dev) for k, v in init["kl"].items()})}
    eps256 = torch.randn(B, z, 32, 32, generator=gen).to(dev)

    def codec(name):
        eng = engines[name]
        if name == "vq":
            return lambda: eng.decode(eng.encode(x)[0])
        return lambda: eng.decode(eng.encode(x, eps256)[0])

    with torch.no_grad():
        for eng in engines.values():
            eng.refresh_weights()
        fns = {name: codec(name) for name in engines}
        for fn in fns.values():
            timed(fn, 5)
        cms = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                cms[name].append(timed(fn, a.steps) * 1e3)
    cod = {name: summary(v) for name, v in cms.items()}
    cod["kl_over_vq"] = cod["kl"]["median"] / cod["vq"]["median"]
    result["encode_decode_ms"] = cod
    print(f"encode + decode: vq {cod['vq']['median']:.3f} ms, kl {cod['kl']['median']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
