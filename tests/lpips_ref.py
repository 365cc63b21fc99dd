"""Shared by the LPIPS tests: seeded weights for the LPIPS module tree (the pretrained VGG16 is 59 MB, not a fixture)
and a plain-torch restatement of the metric (reference models/lpips.py:110-140) that runs at any dtype on the CPU.

Seeding: conv w ~ N(0, 2 / (9 cin)) (He), b ~ N(0, 0.05^2), lin_k = |N(0, 1)| / C. With it the fp32 restatement has no
all-zero feature pixel at any tap for 32x32, 40x40 and 32x48 inputs, so the zero-vector case is tested at kernel
level (tests/test_lpips_kernels_gpu.py)."""
import functools

import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def state_keys():
    """[(key, shape)] of the reference LPIPS module's state dict, in its order (38 entries)."""
    out = [("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))]
    cin = 3
    for s, idxs in enumerate(SLICES):
        for i in idxs:
            out += [(f"net.slice{s + 1}.{i}.weight", (CHANNELS[s], cin, 3, 3)),
                    (f"net.slice{s + 1}.{i}.bias", (CHANNELS[s],))]
            cin = CHANNELS[s]
    out += [(f"lin{k}.model.1.weight", (1, c, 1, 1)) for k, c in enumerate(CHANNELS)]
    out += [(f"lins.{k}.model.1.weight", (1, c, 1, 1)) for k, c in enumerate(CHANNELS)]
    return out


@functools.lru_cache(maxsize=None)
def seeded_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_keys():
        if key == "scaling_layer.shift":
            sd[key] = torch.tensor(SHIFT).view(shape)
        elif key == "scaling_layer.scale":
            sd[key] = torch.tensor(SCALE).view(shape)
        elif key.startswith("net.") and key.endswith(".weight"):
            sd[key] = torch.randn(shape, generator=g) * (2.0 / (9 * shape[1])) ** 0.5
        elif key.startswith("net."):
            sd[key] = torch.randn(shape, generator=g) * 0.05
        elif key.startswith("lin") and not key.startswith("lins"):
            sd[key] = torch.randn(shape, generator=g).abs() / shape[1]
        else:  # lins.k is lin{k} registered a second time
            sd[key] = sd[key.replace("lins.", "lin")]
    return sd


def features(sd, x, dtype):
    """The five taps (relu1_2, 2_2, 3_3, 4_3, 5_3) of the scaled image x."""
    taps, h = [], x
    for s, idxs in enumerate(SLICES):
        if s:
            h = F.max_pool2d(h, 2, 2)
        for i in idxs:
            h = F.relu(F.conv2d(h, sd[f"net.slice{s + 1}.{i}.weight"].to(dtype),
                                sd[f"net.slice{s + 1}.{i}.bias"].to(dtype), padding=1))
        taps.append(h)
    return taps


def lpips(sd, in0, in1, normalize=False, dtype=torch.float32):
    """val (B,) in fp32 with weights and activations at `dtype`."""
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    x0, x1 = ((t - shift) / scale for t in (in0, in1))
    f0, f1 = features(sd, x0.to(dtype), dtype), features(sd, x1.to(dtype), dtype)
    val = 0
    for k in range(5):
        d = (F.normalize(f0[k], dim=1) - F.normalize(f1[k], dim=1)) ** 2
        val = val + F.conv2d(d, sd[f"lin{k}.model.1.weight"].to(dtype)).float().mean([2, 3]).reshape(-1)
    return val


def images(B, H, W, seed):
    """im in [-1, 1] and out = clamp(im + 0.3 randn)."""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    out = (im + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    return out, im


def cos(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


@functools.lru_cache(maxsize=None)
def reference(B, H, W, seed=1):
    """fp32 restatement on the CPU with dval = 1 / B per sample (the mean), and the same at bf16: the reference's own
    bf16 error e_val (relative, worst sample) and e_cos (1 - cosine of each input gradient against fp32)."""
    sd = seeded_state()
    out, im = images(B, H, W, seed)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        a, b = out.clone().requires_grad_(True), im.clone().requires_grad_(True)
        val = lpips(sd, a, b, dtype=dtype)
        val.mean().backward()
        res[dtype] = (val.detach(), a.grad, b.grad)
    v32, g0, g1 = res[torch.float32]
    v16, h0, h1 = res[torch.bfloat16]
    e_val = ((v16 - v32).abs() / v32.abs()).max().item()
    return dict(out=out, im=im, val=v32, g0=g0, g1=g1, e_val=e_val, e_cos0=1 - cos(h0, g0), e_cos1=1 - cos(h1, g1))
