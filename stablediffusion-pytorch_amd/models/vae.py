"""Drop-in KL autoencoder (reference models/vae.py:6-120) on the MI355X HIP path.

Same constructor fields, assertions, module tree and state-dict keys as the reference (models.vqvae's trunk with a 2z-row
encoder_conv_out, a (2z, 2z, 1, 1) pre_quant_conv and no embedding; `codebook_size` in the config is ignored), so every
caller that binds an autoencoder to `vae` and does `im, _ = vae.encode(im)` / `vae.decode(xt)` runs unchanged:

    encode(x)  -> (sample, encoder_output)     encoder_output = pre_quant_conv(...) (B, 2z, h, w), mean | logvar
    decode(z)  -> reconstruction
    forward(x) -> (out, encoder_output)

The draw is the reference's (vae.py:100): torch.randn(mean.shape) on the CPU default generator, moved to the device,
exactly once per encode, so a reseeded reference and this module see the same eps. Inference runs sdmi.vae_engine under
no_grad. forward(x) with autograd enabled runs the training engine (sdmi.vae_train) as one autograd Function that
returns (reconstruction, encoder_output): a gradient on encoder_output -- the user's own torch KL loss on
torch.chunk(encoder_output, 2, 1) -- enters sdmi_kl_bwd as the outside gradient of the moments. encode() outside forward
is not differentiable on the engine path.
"""
import torch
import torch.nn as nn

from models.blocks import DownBlock, MidBlock, UpBlock
from sdmi import _lib
from sdmi import kernels as K
from sdmi import leaf as LF
from sdmi.module_glue import NO_INPUT_GRAD, check_tape
from sdmi.vae_engine import VAEEngine
from sdmi.vae_train import VAETrainEngine

_OFF_GPU = "the sdmi VAE runs on the MI355X HIP path only (move the model and inputs to cuda)"


class _KLSample(torch.autograd.Function):
    """(moments (B, 2z, h, w), eps (B, z, h, w)) -> mean + exp(0.5 logvar) eps over the two kernels of
    csrc/kl_latent.hip (the pre-conv of sdmi_kl_sample is the identity here: 1 * m + 0 is m)."""

    @staticmethod
    def forward(ctx, moments, eps):
        B, M, h, w = moments.shape
        z = M // 2
        mom = moments.detach().float().contiguous()
        eps = eps.detach().float().contiguous()
        rows = mom.permute(0, 2, 3, 1).reshape(B * h * w, M).contiguous()
        eye = torch.eye(M, dtype=torch.float32, device=mom.device)
        smp = torch.empty(B, z, h, w, dtype=torch.float32, device=mom.device)
        K.kl_sample(rows, M, eye, None, eps, B, z, h * w, torch.empty_like(mom), smp)
        ctx.saved = (mom, eps, (B, z, h * w))
        return smp

    @staticmethod
    def backward(ctx, g):
        mom, eps, (B, z, HW) = ctx.saved
        dmom = torch.empty_like(mom)
        K.kl_bwd(None, 0, None, None, mom, eps, None, 0, None, B, z, HW, dsample_add=g.float().contiguous(), dmom=dmom)
        return dmom, None


class VAEFunction(torch.autograd.Function):
    """(eps, x, *params) -> (reconstruction, encoder_output) on the HIP training engine."""

    @staticmethod
    def forward(ctx, mod, eps, x, *params):
        if ctx.needs_input_grad[2]:
            raise RuntimeError(NO_INPUT_GRAD)
        eng = mod._train_eng(x)
        B, C, H, W = x.shape
        out, c = eng.forward(x, eps=eps)
        ctx.mod, ctx.c, ctx.hw, ctx.packs_of = mod, c, (B, H, W), mod._packs_of
        return eng.pred_to_nchw(out, B, H, W), c["moments"]

    @staticmethod
    def backward(ctx, dimg, dmom):
        mod = ctx.mod
        check_tape(ctx.c, ctx.packs_of, mod._packs_of)
        eng = mod._tengine
        B, H, W = ctx.hw
        dout = (eng.dpred_from_nchw(dimg.float().contiguous()) if dimg is not None
                else torch.zeros(B * H * W, 8, dtype=torch.bfloat16, device=eng.device))
        names = [k for k, _ in mod.named_parameters()]
        params = dict(mod.named_parameters())
        grads = {k: torch.empty_like(params[k]) for k in names}
        eng.backward(ctx.c, dout, 0.0, grads=grads, dmom=dmom.float().contiguous() if dmom is not None else None)
        ctx.c = None
        return (None, None, None) + tuple(grads[k] for k in names)


class VAE(nn.Module):
    def __init__(self, im_channels, model_config):
        super().__init__()
        cfg = model_config
        self.im_channels = im_channels
        self.down_channels = cfg["down_channels"]
        self.mid_channels = cfg["mid_channels"]
        self.down_sample = cfg["down_sample"]
        self.num_down_layers = cfg["num_down_layers"]
        self.num_mid_layers = cfg["num_mid_layers"]
        self.num_up_layers = cfg["num_up_layers"]
        self.attns = cfg["attn_down"]
        self.z_channels = cfg["z_channels"]
        self.norm_channels = cfg["norm_channels"]
        self.num_heads = cfg["num_heads"]
        assert self.mid_channels[0] == self.down_channels[-1]
        assert self.mid_channels[-1] == self.down_channels[-1]
        assert len(self.down_sample) == len(self.down_channels) - 1
        assert len(self.attns) == len(self.down_channels) - 1
        self.up_sample = list(reversed(self.down_sample))
        dc, mc = self.down_channels, self.mid_channels
        self.encoder_conv_in = nn.Conv2d(im_channels, dc[0], kernel_size=3, padding=(1, 1))
        self.encoder_layers = nn.ModuleList([
            DownBlock(dc[i], dc[i + 1], t_emb_dim=None, down_sample=self.down_sample[i], num_heads=self.num_heads,
                      num_layers=self.num_down_layers, attn=self.attns[i], norm_channels=self.norm_channels)
            for i in range(len(dc) - 1)])
        self.encoder_mids = nn.ModuleList([
            MidBlock(mc[i], mc[i + 1], t_emb_dim=None, num_heads=self.num_heads, num_layers=self.num_mid_layers,
                     norm_channels=self.norm_channels)
            for i in range(len(mc) - 1)])
        self.encoder_norm_out = nn.GroupNorm(self.norm_channels, dc[-1])
        self.encoder_conv_out = nn.Conv2d(dc[-1], 2 * self.z_channels, kernel_size=3, padding=1)
        self.pre_quant_conv = nn.Conv2d(2 * self.z_channels, 2 * self.z_channels, kernel_size=1)
        self.post_quant_conv = nn.Conv2d(self.z_channels, self.z_channels, kernel_size=1)
        self.decoder_conv_in = nn.Conv2d(self.z_channels, mc[-1], kernel_size=3, padding=(1, 1))
        self.decoder_mids = nn.ModuleList([
            MidBlock(mc[i], mc[i - 1], t_emb_dim=None, num_heads=self.num_heads, num_layers=self.num_mid_layers,
                     norm_channels=self.norm_channels)
            for i in reversed(range(1, len(mc)))])
        self.decoder_layers = nn.ModuleList([
            UpBlock(dc[i], dc[i - 1], t_emb_dim=None, up_sample=self.down_sample[i - 1], num_heads=self.num_heads,
                    num_layers=self.num_up_layers, attn=self.attns[i - 1], norm_channels=self.norm_channels)
            for i in reversed(range(1, len(dc)))])
        self.decoder_norm_out = nn.GroupNorm(self.norm_channels, dc[0])
        self.decoder_conv_out = nn.Conv2d(dc[0], im_channels, kernel_size=3, padding=1)
        self._engine = None
        self._ptrs = None

    def model_config_dict(self):
        return {"down_channels": self.down_channels, "mid_channels": self.mid_channels,
                "down_sample": self.down_sample, "attn_down": self.attns, "num_down_layers": self.num_down_layers,
                "num_mid_layers": self.num_mid_layers, "num_up_layers": self.num_up_layers,
                "z_channels": self.z_channels, "norm_channels": self.norm_channels, "num_heads": self.num_heads}

    def _eng(self, t):
        if not t.is_cuda:
            raise RuntimeError(_OFF_GPU)
        _lib.lib()
        params = dict(self.named_parameters())
        ptrs = [p.data_ptr() for p in params.values()]
        if self._engine is None or ptrs != self._ptrs:
            self._engine = VAEEngine(self.model_config_dict(), {k: v.detach() for k, v in params.items()},
                                     im_channels=self.im_channels)
            self._ptrs = ptrs
        self._engine.refresh_weights()  # bf16 GEMM-layout copies of the (possibly updated) fp32 weights
        return self._engine

    def _train_eng(self, t):
        if not t.is_cuda:
            raise RuntimeError(_OFF_GPU)
        _lib.lib()
        params = dict(self.named_parameters())
        ptrs = [p.data_ptr() for p in params.values()]
        if getattr(self, "_tengine", None) is None or ptrs != self._tptrs:
            self._tengine = VAETrainEngine(self.model_config_dict(), {k: v.detach() for k, v in params.items()},
                                           im_channels=self.im_channels)
            self._tptrs = ptrs
        self._tengine.refresh_weights()
        # what a later backward checks its own forward's record against (`.data` writes keep the versions)
        self._packs_of = (self._tengine, tuple(p._version for p in params.values()))
        return self._tengine

    def _leaf(self):
        """Leaf-by-leaf path (sdmi.leaf): a swapped leaf or sdmi_leaf_path = True."""
        return getattr(self, "sdmi_leaf_path", False) or not LF.engine_ok(self, (VAE, DownBlock, MidBlock, UpBlock))

    def _latent_shape(self, x):
        f = 2 ** sum(1 for d in self.down_sample if d)
        return (x.shape[0], self.z_channels, x.shape[2] // f, x.shape[3] // f)

    def _draw(self, x):
        """vae.py:100: the CPU default generator, one draw of the mean's shape, moved to the device."""
        return torch.randn(self._latent_shape(x)).to(device=x.device)

    def _leaf_encode(self, x):
        if not x.is_cuda:
            raise RuntimeError(_OFF_GPU)
        out = LF.call(self.encoder_conv_in, x)
        for down in self.encoder_layers:
            out = down(out)
        for mid in self.encoder_mids:
            out = mid(out)
        out = LF.call(nn.Sequential(self.encoder_norm_out, nn.SiLU()), out)
        out = LF.call(self.pre_quant_conv, LF.call(self.encoder_conv_out, out))
        return _KLSample.apply(out, self._draw(x)), out

    def _leaf_decode(self, z):
        out = LF.call(self.decoder_conv_in, LF.call(self.post_quant_conv, z))
        for mid in self.decoder_mids:
            out = mid(out)
        for up in self.decoder_layers:
            out = up(out)
        out = LF.call(nn.Sequential(self.decoder_norm_out, nn.SiLU()), out)
        return LF.call(self.decoder_conv_out, out)

    def encode(self, x):
        if self._leaf():
            return self._leaf_encode(x)
        eng = self._eng(x)  # (raises off the HIP path before anything is drawn)
        eps = self._draw(x)
        with torch.no_grad():
            return eng.encode(x, eps)

    def decode(self, z):
        if self._leaf():
            return self._leaf_decode(z)
        with torch.no_grad():
            return self._eng(z).decode(z)

    def forward(self, x):
        if self._leaf():
            z, encoder_output = self._leaf_encode(x)
            return self._leaf_decode(z), encoder_output
        if torch.is_grad_enabled() and x.requires_grad:  # (before anything is packed or drawn)
            raise RuntimeError(NO_INPUT_GRAD)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            self._train_eng(x)  # (raises off the HIP path before anything is drawn)
            return VAEFunction.apply(self, self._draw(x), x, *self.parameters())
        z, encoder_output = self.encode(x)
        return self.decode(z), encoder_output
