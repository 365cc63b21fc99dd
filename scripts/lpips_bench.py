"""LPIPS timing at the VQVAE training shape (B = 8, 256 x 256, CelebHQ VQVAE config, seeded weights):
  * the LPIPS forward + backward alone (sdmi.lpips_engine: gradient to the reconstruction only), recorded plan replay,
    with a per-kernel table of one eager pass (sdmi.kernels.PROFILE events);
  * the full VQVAETrainer.step with and without the LPIPS term, recorded plans replayed alternately (A/B in one
    process, several rounds);
  * for comparison, the plain-torch restatement of the metric (tests/lpips_ref.py: F.conv2d / max_pool2d / normalize,
    i.e. MIOpen and torch kernels) under bf16 autocast on the same GPU, forward + backward to the reconstruction.
Times are device events around replays that end in a synchronise. Writes one JSON file (default
profiles/lpips_vqvae_train.json)."""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]
import torch  # noqa: E402

from sdmi import kernels as K  # noqa: E402
from sdmi.lpips_engine import LPIPSEngine  # noqa: E402
from sdmi.plan import StepPlan  # noqa: E402
from sdmi.vqvae_train import VQVAETrainer  # noqa: E402
from tests import lpips_ref as R  # noqa: E402
from tests.golden.configs import vqvae_celebhq_config  # noqa: E402


def timed(fn, iters, warm=3):
    """ms per call: device events around `iters` calls, after `warm` untimed ones."""
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel_table(step):
    """Per-kernel device time of one eager pass: {tag + shape: [launches, ms]} from the per-launch events."""
    K.PROFILE = []
    step()
    torch.cuda.synchronize()
    rows = {}
    for tag, flops, e0, e1, info in K.PROFILE:
        key = f"{tag} {info.split(' variant=')[0]}"
        r = rows.setdefault(key, [0, 0.0, 0.0])
        r[0] += 1
        r[1] += e0.elapsed_time(e1)
        r[2] += flops
    K.PROFILE = None
    return {k: dict(launches=v[0], ms=round(v[1], 4), tflops=round(v[2] / v[1] / 1e9, 1) if v[2] else None)
            for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_vqvae_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timings need the MI355X"
    dev, B, S = torch.device("cuda", 0), args.batch, args.size
    g = torch.Generator().manual_seed(1111)
    im = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    lsd = {k: v.to(dev) for k, v in R.seeded_state().items()}
    res = dict(batch=B, size=S, iters=args.iters, device=torch.cuda.get_device_name(0))

    # ---- LPIPS alone: the trainer's call (NHWC fp32 reconstruction, gradient added into the bf16 dpred buffer) ----
    eng = LPIPSEngine(lsd, dev)
    recon = torch.zeros(B * S * S, 8, device=dev)
    recon[:, :3] = (im + 0.3 * torch.randn(im.shape, generator=g).to(dev)).permute(0, 2, 3, 1).reshape(-1, 3)
    dpred = torch.zeros(B * S * S, 8, dtype=torch.bfloat16, device=dev)

    def lpips_step():
        val, ctx = eng.forward(recon, im, nhwc=(True, False), shape=(B, S, S))
        eng.backward(ctx, None, want=(True, False), gscale=1.0 / B, acc=dpred)

    def lpips_fwd():
        eng.forward(recon, im, nhwc=(True, False), shape=(B, S, S), need_backward=False)

    lpips_step()
    p_all, p_fwd = StepPlan(lpips_step, dev), StepPlan(lpips_fwd, dev)
    res["lpips_fwd_bwd_ms"] = [round(timed(p_all.replay, args.iters), 4) for _ in range(args.rounds)]
    res["lpips_fwd_ms"] = [round(timed(p_fwd.replay, args.iters), 4) for _ in range(args.rounds)]
    res["lpips_kernels"] = kernel_table(lpips_step)
    print("lpips fwd+bwd ms", res["lpips_fwd_bwd_ms"], "fwd ms", res["lpips_fwd_ms"], flush=True)
    del p_all, p_fwd

    # ---- the torch restatement under bf16 autocast (MIOpen convolutions), same images, gradient to `out` ----
    out_img = recon[:, :3].reshape(B, S, S, 3).permute(0, 3, 1, 2).contiguous()

    def torch_step():
        a = out_img.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            v = R.lpips(lsd, a, im)
        v.mean().backward()

    res["torch_autocast_fwd_bwd_ms"] = [round(timed(torch_step, args.iters, warm=5), 4) for _ in range(args.rounds)]
    print("torch bf16-autocast restatement fwd+bwd ms", res["torch_autocast_fwd_bwd_ms"], flush=True)

    # ---- full trainer step with / without LPIPS, alternating ----
    cfg = vqvae_celebhq_config()
    from models.vqvae import VQVAE
    torch.manual_seed(1111)
    init = {k: v.to(dev) for k, v in VQVAE(3, cfg).state_dict().items()}
    plans = {}
    for name, kw in (("without", {}), ("with", dict(perceptual_weight=1.0, lpips_state=lsd))):
        tr = VQVAETrainer(cfg, {k: v.clone() for k, v in init.items()}, dev, **kw)
        for _ in range(2):
            tr.step(im)
        plans[name] = (StepPlan(lambda tr=tr: tr.step(im), dev), tr)
    res["step_ms"] = {"without": [], "with": []}
    for _ in range(args.rounds):
        for name in ("without", "with"):
            res["step_ms"][name].append(round(timed(plans[name][0].replay, args.iters), 4))
    res["losses_with"] = plans["with"][1].losses()
    print("trainer step ms", res["step_ms"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "lpips_kernels"}))


if __name__ == "__main__":
    main()
