"""LPIPS perceptual distance (reference models/lpips.py: frozen VGG16 features, five taps, unit-normalised squared
difference through the learned 1x1 `lin` weights, spatial mean) on the HIP kernels of libsdmi.so.

    scale + pack both images into one 2B-row NHWC bf16 batch (sdmi_lpips_prep)
    -> 13 x [3x3 implicit-GEMM conv + bias + ReLU epilogue]  with sdmi_maxpool2_fwd between the five slices
    -> after relu1_2 / 2_2 / 3_3 / 4_3 / 5_3: sdmi_lpips_dist_fwd adds the tap's mean distance into val (B,)

The backward runs the data-gradient chain only over the image(s) that need a gradient: per tap sdmi_lpips_dist_bwd
(its own term + the gradient arriving from the next slice, through the tap's ReLU), the flipped-tap data-gradient
GEMMs with the ReLU-gradient epilogue (act 3 on the saved activation), sdmi_maxpool2_bwd, and sdmi_lpips_image_grad
out of the 8-channel gradient of the scaled image. The weights are frozen: there are no weight gradients, and the bf16
GEMM layouts are packed once. Nothing synchronises with the host; every launch records into sdmi.plan.StepPlan.
The GEMM shapes have no rows in sdmi/tuned_gemm.json (the split heuristic serves them)."""
import torch

from . import _lib
from . import kernels as K
from . import plan
from .unet_engine import PackPlan, UNetEngine

# torchvision vgg16.features indices of the convolutions of the five slices (reference lpips.py:31-40) and their widths
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHANNELS = (64, 128, 256, 512, 512)
MIN_SIDE = 16  # four floor-mode 2x2 pools


def conv_keys():
    """[(state-dict prefix, cin, cout)] of the 13 convolutions in forward order."""
    out, cin = [], 3
    for s, idxs in enumerate(SLICES):
        for i in idxs:
            out.append((f"net.slice{s + 1}.{i}", cin, CHANNELS[s]))
            cin = CHANNELS[s]
    return out


def state_shapes():
    """State-dict keys and shapes of the LPIPS module tree (reference models/lpips.py), in its order."""
    shapes = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for key, cin, cout in conv_keys():
        shapes[key + ".weight"] = (cout, cin, 3, 3)
        shapes[key + ".bias"] = (cout,)
    for prefix in ("lin{}", "lins.{}"):
        for k, c in enumerate(CHANNELS):
            shapes[prefix.format(k) + ".model.1.weight"] = (1, c, 1, 1)
    return shapes


class LPIPSEngine:
    """state_dict: the LPIPS module's (scaling_layer.*, net.slice*.N.{weight,bias}, lin{k}.model.1.weight)."""

    def __init__(self, state_dict, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the sdmi LPIPS runs on the MI355X HIP path only (move the model and inputs to cuda)")
        _lib.lib()

        def dev(k):
            return state_dict[k].detach().to(self.device, torch.float32).contiguous()

        self.convs = conv_keys()
        self.P = {}
        for key, cin, cout in self.convs:
            for leaf, shape in ((".weight", (cout, cin, 3, 3)), (".bias", (cout,))):
                t = dev(key + leaf)
                if tuple(t.shape) != shape:
                    raise ValueError(f"{key + leaf}: shape {tuple(t.shape)}, expected {shape}")
                self.P[key + leaf] = t
        self.lin = [dev(f"lin{k}.model.1.weight").reshape(-1) for k in range(5)]
        for k, c in enumerate(CHANNELS):
            if self.lin[k].numel() != c:
                raise ValueError(f"lin{k}.model.1.weight: {self.lin[k].numel()} weights, expected {c}")
        self.shift = dev("scaling_layer.shift").reshape(-1)
        self.scale = dev("scaling_layer.scale").reshape(-1)
        pk = PackPlan(self.device)
        for key, cin, cout in self.convs:  # key#f [cout][9*cin] and key#d [cin][9*cout]; conv1_1's cin padded to 8
            UNetEngine._pk_conv(self, pk, key, ipad=8 if cin == 3 else None)
        pk.finalize()
        pk.run()  # frozen weights: packed once
        self.pack = pk

    def W(self, name):
        return self.pack.view(name)

    def _new(self, rows, C, dtype=torch.bfloat16):
        return torch.empty(rows, C, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------------------------------
    def forward(self, in0, in1, normalize=False, need_backward=True, nhwc=(False, False), shape=None):
        """in0 / in1: (B, 3, H, W) fp32 images, or with nhwc[i] the training engine's NHWC fp32 [B*H*W, 8]
        reconstruction (shape = (B, H, W) then). Returns (val (B,) fp32, ctx)."""
        if shape is None:
            src = in1 if nhwc[0] else in0
            shape = (src.shape[0], src.shape[2], src.shape[3])
        B, H, W = shape
        for t, flat in zip((in0, in1), nhwc):
            want = (B * H * W, 8) if flat else (B, 3, H, W)
            if tuple(t.shape) != want:
                raise ValueError(f"LPIPS input of shape {tuple(t.shape)}, expected {want}")
        if min(H, W) < MIN_SIDE:
            raise ValueError(f"LPIPS needs images of at least {MIN_SIDE} x {MIN_SIDE} (four 2x2 pools), got {H} x {W}")
        in0, in1 = plan.as_operand(in0), plan.as_operand(in1)
        phase, K.PHASE = K.PHASE, "fwd"
        N = 2 * B
        x = self._new(N * H * W, 8)
        K.lpips_prep(in0, nhwc[0], in1, nhwc[1], B, H, W, self.shift, self.scale, normalize, x)
        val = torch.empty(B, dtype=torch.float32, device=self.device)
        cur, h, w = x, H, W
        layers, taps, it = [], [], iter(self.convs)
        for s, idxs in enumerate(SLICES):
            if s:
                pooled = self._new(N * (h // 2) * (w // 2), CHANNELS[s - 1])
                K.maxpool2_fwd(cur, N, h, w, CHANNELS[s - 1], pooled)
                cur, h, w = pooled, h // 2, w // 2
            for _ in idxs:
                key, cin, cout = next(it)
                cp = 8 if cin == 3 else cin
                y = self._new(N * h * w, cout)
                K.conv_fwd(cur, N, h, w, cp, cp, self.W(key + "#f"), cout, 3, 3, 1, 1, y, cout,
                           bias=self.P[key + ".bias"], act=2)
                layers.append((key, cur, s))  # the conv's input: the ReLU mask of its data gradient
                cur = y
            rn = torch.empty(N * h * w, dtype=torch.float32, device=self.device) if need_backward else None
            K.lpips_dist_fwd(cur, self.lin[s], B, h * w, CHANNELS[s], val, s > 0, rn)
            taps.append((cur, rn, h, w))
        K.PHASE = phase
        ctx = dict(B=B, H=H, W=W, normalize=normalize, layers=layers, taps=taps) if need_backward else None
        return val, ctx

    def backward(self, ctx, dval=None, want=(True, False), gscale=1.0, acc=None, mse=None):
        """dval: device fp32 (B,) = dL/dval (None: ones), times the host factor gscale. Returns (g0, g1): the
        (B, 3, H, W) fp32 gradient of each wanted image, None for the others. acc (NHWC bf16 [B*H*W, 8], optional): the
        gradient of image 0 is added into its channels 0..2 instead of being returned -- or, with mse = (pred NHWC fp32,
        target NCHW fp32), acc is written whole: the MSE gradient of (pred, target) plus the gradient of image 0,
        summed in fp32 and rounded to bf16 once (the trainer's reconstruction gradient)."""
        B, H, W = ctx["B"], ctx["H"], ctx["W"]
        if dval is not None:
            dval = plan.as_operand(dval.reshape(-1))
        phase, K.PHASE = K.PHASE, "bwd"
        out = [None, None]
        for side in (0, 1):
            if not want[side]:
                continue
            d = self._backward_side(ctx, dval, gscale, side)
            if side == 0 and acc is not None:
                K.lpips_image_grad(d, B, H, W, self.scale, ctx["normalize"], acc_nhwc=acc, mse=mse)
            else:
                out[side] = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
                K.lpips_image_grad(d, B, H, W, self.scale, ctx["normalize"], out_nchw=out[side])
        K.PHASE = phase
        return tuple(out)

    def _backward_side(self, ctx, dval, gscale, side):
        """The 8-channel NHWC bf16 gradient of the scaled image `side` (B*H*W rows)."""
        B, layers, taps = ctx["B"], ctx["layers"], ctx["taps"]

        def half(t, P):  # the rows of image `side` of a 2B-image activation
            return t[side * B * P:(side + 1) * B * P]

        arriving = None  # gradient of the tap from the next slice (pool backward), B*P rows
        for s in reversed(range(5)):
            f, rn, h, w = taps[s]
            P, C = h * w, CHANNELS[s]
            dy = self._new(B * P, C)
            K.lpips_dist_bwd(f, self.lin[s], rn, B, P, C, side, dy, g=dval, gscale=gscale, addend=arriving)
            convs = [(key, x) for key, x, sl in layers if sl == s]
            for j in range(len(convs) - 1, -1, -1):
                key, x = convs[j]
                cin = x.shape[1]  # 8 at conv1_1
                dx = self._new(B * P, cin)
                # a slice's first conv reads the pool output (the image at slice 1): no ReLU of its own to go through
                K.conv_fwd(dy, B, h, w, C, C, self.W(key + "#d"), cin, 3, 3, 1, 1, dx, cin,
                           act=3 if j else 0, aux=half(x, P) if j else None)
                dy = dx
            if s:
                fp, _, hp, wp = taps[s - 1]
                arriving = self._new(B * hp * wp, CHANNELS[s - 1])
                K.maxpool2_bwd(half(fp, hp * wp), dy, B, hp, wp, CHANNELS[s - 1], arriving)
        return dy
