"""Drop-in LPIPS perceptual metric (reference models/lpips.py:16-168) on the MI355X HIP path.

Same classes, module tree and state-dict keys as the reference (scaling_layer buffers, net.slice1..5 holding the VGG16
convolutions under their torchvision `features` indices, lin0..lin4 and the same five again as lins.0..4), so
`lpips_model = LPIPS().eval().to(device)` and `torch.mean(lpips_model(output, im))` in train_vqvae_celebhq.py run
unchanged. The forward is one autograd Function over sdmi.lpips_engine.LPIPSEngine and gives gradients to whichever of
the two images require them.

This module needs no torchvision and never touches the network. The pretrained weights are an input:
`load_state_dict()` of a full LPIPS state dict, or the constructor keywords `vgg_weights=` (a torchvision vgg16
state-dict file, keys `features.N.{weight,bias}`) and `lin_weights=` (the LPIPS v0.1 `vgg.pth` file, keys
`lin{k}.model.1.weight`). Without them the module keeps its seeded initialisation and warns once.
"""
import warnings

import torch
import torch.nn as nn

from sdmi import _lib
from sdmi.module_glue import TAPE_FREED
from sdmi.lpips_engine import CHANNELS, SLICES, LPIPSEngine

_CPU_ERROR = "the sdmi LPIPS runs on the MI355X HIP path only (move the model and inputs to cuda)"
_warned = False


def spatial_average(in_tens, keepdim=True):
    return in_tens.mean([2, 3], keepdim=keepdim)


class ScalingLayer(nn.Module):
    """(x - shift) / scale with the LPIPS constants for images in [-1, 1]."""

    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor([.458, .448, .450]).view(1, 3, 1, 1))

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class NetLinLayer(nn.Module):
    """The 1x1 convolution of one tap ([Dropout,] Conv2d(chn_in, chn_out, 1, bias=False) as `model`)."""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers.append(nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


class vgg16(nn.Module):
    """The VGG16 feature layers up to relu5_3 as slice1..slice5, every layer under its torchvision `features` index.
    `pretrained` is accepted for signature compatibility only: nothing is downloaded, the weights are loaded by the
    caller (LPIPS(vgg_weights=...) or load_state_dict)."""

    def __init__(self, requires_grad=False, pretrained=True):
        super().__init__()
        self.N_slices = len(SLICES)
        cin, index = 3, 0
        for s, convs in enumerate(SLICES):
            seq = nn.Sequential()
            if s:
                seq.add_module(str(index), nn.MaxPool2d(kernel_size=2, stride=2))
                index += 1
            for _ in convs:
                seq.add_module(str(index), nn.Conv2d(cin, CHANNELS[s], kernel_size=3, padding=1))
                seq.add_module(str(index + 1), nn.ReLU(inplace=True))
                cin, index = CHANNELS[s], index + 2
            setattr(self, f"slice{s + 1}", seq)
        if not requires_grad:
            for p in self.parameters():
                p.requires_grad = False


class LPIPSFunction(torch.autograd.Function):
    """(in0, in1) -> val (B, 1, 1, 1) on the HIP engine; gradients for the images that require them."""

    @staticmethod
    def forward(ctx, eng, normalize, in0, in1):
        need = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        val, c = eng.forward(in0, in1, normalize=normalize, need_backward=any(need))
        ctx.eng, ctx.c, ctx.need = eng, c, need
        return val.view(-1, 1, 1, 1)

    @staticmethod
    def backward(ctx, dval):
        if ctx.c is None:
            raise RuntimeError(TAPE_FREED)
        g0, g1 = ctx.eng.backward(ctx.c, dval.float().contiguous(), want=ctx.need)
        ctx.c = None
        return None, None, g0, g1


class LPIPS(nn.Module):
    def __init__(self, net="vgg", version="0.1", use_dropout=True, vgg_weights=None, lin_weights=None):
        super().__init__()
        if net != "vgg":
            raise ValueError("only net='vgg' is implemented (the reference uses no other)")
        self.version = version
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHANNELS)
        self.L = len(self.chns)
        self.net = vgg16(pretrained=False, requires_grad=False)
        for k, c in enumerate(self.chns):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(self.L)])
        for k in range(self.L):  # a distance needs non-negative weights; the trained ones are
            getattr(self, f"lin{k}").model[-1].weight.data.abs_()
        self._loaded = False
        if vgg_weights is not None:
            self.load_vgg_weights(vgg_weights)
        if lin_weights is not None:
            self.load_lin_weights(lin_weights)
        self._loaded = vgg_weights is not None and lin_weights is not None
        self.eval()
        for p in self.parameters():
            p.requires_grad = False
        self._engine, self._sig = None, None

    # ---- weights: local files or load_state_dict only ---------------------------------------------------------
    def load_vgg_weights(self, path):
        """A torchvision vgg16 state-dict file: features.N.{weight,bias} -> net.slice{s}.N.{weight,bias}."""
        sd = torch.load(path, map_location="cpu")
        own = {}
        for s, convs in enumerate(SLICES):
            for i in convs:
                for leaf in ("weight", "bias"):
                    own[f"net.slice{s + 1}.{i}.{leaf}"] = sd[f"features.{i}.{leaf}"]
        missing, unexpected = nn.Module.load_state_dict(self, own, strict=False)
        assert not unexpected, unexpected

    def load_lin_weights(self, path):
        """The LPIPS v0.1 vgg.pth layout: lin{k}.model.1.weight (1, C, 1, 1)."""
        sd = torch.load(path, map_location="cpu")
        own = {f"lin{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(self.L)}
        nn.Module.load_state_dict(self, own, strict=False)

    def load_state_dict(self, state_dict, strict=True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self._loaded = True
        return r

    def _eng(self, t):
        global _warned
        if self.training and any(isinstance(m, nn.Dropout) for m in self.modules()):
            raise RuntimeError("LPIPS is a frozen metric: its forward was called in training mode with dropout active; "
                               "call .eval() on it (the reference does, lpips.py:105)")
        if any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("LPIPS is a frozen metric: some of its parameters require grad; call "
                               ".requires_grad_(False) on it (the reference freezes them, lpips.py:106-107)")
        if not t.is_cuda:
            raise RuntimeError(_CPU_ERROR)
        _lib.lib()
        if not self._loaded and not _warned:
            _warned = True
            warnings.warn("LPIPS runs on its seeded initialisation: no pretrained weights were given "
                          "(vgg_weights= / lin_weights= or load_state_dict)")
        sd = self.state_dict()
        sig = tuple((v.data_ptr(), v._version) for v in sd.values())
        if self._engine is None or sig != self._sig:
            self._engine = LPIPSEngine(sd, t.device)
            self._sig = sig
        return self._engine

    def forward(self, in0, in1, normalize=False):
        eng = self._eng(in0 if in1.is_cuda else in1)  # frozen / eval checks first, then the device of both inputs
        return LPIPSFunction.apply(eng, bool(normalize), in0, in1)
