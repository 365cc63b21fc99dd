"""Shared cases of the autograd-contract tests (tests/test_autograd_contract_gpu.py, tests/test_autograd_contract_cpu.py).

One Case per drop-in module with a fused autograd path: its weights, two batches `a` and `b` (different image, timestep
and conditioning), the loss a caller would write on the module's outputs, and the fp32 CPU oracle's gradient of that
loss. The combined loss of the two-forward tests is W_A * loss(a) + W_B * loss(b); the weights differ so that no failure
mode (one gradient counted twice, one gradient lost) looks like the true sum. Nothing here needs a GPU at import.

Oracle results are computed once per (case, batch, weight) and shared: tests must not write into them."""
import os

import torch
import torch.nn.functional as F

from oracle import dit_oracle as DO
from oracle import sd_oracle as O
from oracle import vqvae_oracle as VO
from tests import noise_oracle as NO
from tests import vae_oracle as VAO
from tests.golden.configs import SMALL_COND, SMALL_DIT, SMALL_UNCOND, SMALL_VQVAE

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 2
SEEDS = {"a": 3, "b": 4}        # generator seed of each batch
WEIGHTS = {"a": 4.0, "b": 1.0}  # its weight in the combined loss
N_SCALE = 0.2                   # the noise-robust VQVAE's latent noise (tests/test_vqvae_noise_gpu.py)
KL_WEIGHT = 1e-4                # the KL autoencoder's loss weight (tests/test_vae_gpu.py)
DRAW_SEED = 100                 # + the batch seed: torch.manual_seed before a forward that draws eps
COS_MIN, NORM_TOL = 0.99, 0.05  # one backward against the oracle: test_unet_gpu / test_dit_gpu / test_vqvae_train_gpu /
#                                 test_vae_gpu all hold per-tensor cosine >= 0.99 (oracle norm > 1e-6), global norm 5 %
LEAF_COS_MIN = 0.999            # tests/test_leaf_gpu.py _check: a leaf's data gradient against torch's


def one_hot(cmap, n=18):
    return F.one_hot(cmap.long().clamp(0, n), n + 1).movedim(-1, 1)[:, 1:].float()


def cos(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def against(got, ref):
    """(global norm of got / global norm of ref, worst per-tensor cosine over tensors whose ref norm exceeds 1e-6, its
    key): the two figures every gradient-vs-oracle test of this suite bounds."""
    worst = (1.0, "")
    gsq = rsq = 0.0
    for k, r in ref.items():
        g = got[k].detach().double().cpu()
        gsq += float((g * g).sum())
        rsq += float((r.double() * r.double()).sum())
        if r.norm() > 1e-6:
            worst = min(worst, (cos(g, r), k))
    return (gsq / rsq) ** 0.5, worst[0], worst[1]


def within(ratio, worst):
    return abs(ratio - 1.0) <= NORM_TOL and worst >= COS_MIN


def combine(ga, gb):
    """The true gradient of the combined loss: one fp32 add per element (bitwise what autograd's accumulation gives,
    in either order)."""
    return {k: ga[k] + gb[k] for k in ga}


def failure_modes(ga, gb):
    """What the known defects make of a two-forward gradient: one of the two counted twice (the second backward
    overwrote the first's views before they were accumulated) or one of the two alone."""
    return {"2g_a": {k: 2 * v for k, v in ga.items()}, "2g_b": {k: 2 * v for k, v in gb.items()},
            "g_a": dict(ga), "g_b": dict(gb)}


class Case:
    """name: the test id. holder: the module keeps an EngineHolder (flat gradient buffer, staged backward)."""
    holder = False
    staged = None

    def __init__(self, name):
        self.name = name
        self._state = None
        self._batches = {}
        self._oracle = {}

    def __repr__(self):
        return self.name

    def state(self):
        if self._state is None:
            self._state = self._make_state()
        return self._state

    def batch(self, which):
        if which not in self._batches:
            self._batches[which] = self._make_batch(SEEDS[which])
        return self._batches[which]

    def build(self):
        """A fresh module on the GPU with the case's weights."""
        m = self._module()
        m.load_state_dict(self.state())
        m = m.cuda()
        if self.staged is not None:
            m.sdmi_staged_backward = self.staged
        return m

    def loss(self, model, which, x=None):
        """WEIGHTS[which] * the caller's loss of batch `which` (x: a GPU input to use instead of the batch's own)."""
        b = self.batch(which)
        x = b["x"].cuda() if x is None else x
        return WEIGHTS[which] * self._loss(model, b, x, SEEDS[which])

    def oracle(self, which, aux=None, key=None):
        """({key: gradient}, input gradient) of WEIGHTS[which] * loss on the CPU oracle, fp32. aux: what a bf16 path is
        held to the oracle AT (its own code indices, extremal positions and device draw); key names it for the cache."""
        if (which, key) not in self._oracle:
            torch.set_num_threads(min(16, os.cpu_count() or 1))
            b = self.batch(which)
            p = {k: v.detach().clone().requires_grad_(True) for k, v in self.state().items()}
            x = b["x"].clone().requires_grad_(True)
            (WEIGHTS[which] * self._oracle_loss(p, b, x, SEEDS[which], aux)).backward()
            grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}
            self._oracle[(which, key)] = (grads, x.grad.detach())
        return self._oracle[(which, key)]

    def aux(self, model, which):
        return None

    def frozen(self, name, rule):
        """The frozen-subset rules. "half": about half of the parameters, whole blocks among them; "tail": everything
        but one late block, so that the parameters whose gradients a backward finishes last are all frozen."""
        raise NotImplementedError


class Denoiser(Case):
    holder = True

    def __init__(self, name, base, cfg, staged=None, seed=1):
        super().__init__(name)
        self.base, self.cfg, self.staged, self.seed = base, cfg, staged, seed

    def _make_state(self):
        if self.base == "dit":
            return O.deterministic_state(DO.dit_param_shapes(self.cfg), seed=self.seed)
        return O.deterministic_state(O.unet_param_shapes(self.cfg, base=self.base), seed=self.seed)

    def _module(self):
        if self.base == "dit":
            from models.transformer import DIT
            return DIT(4, self.cfg)
        import models.unet_base as mu
        import models.unet_cond_base as mc
        return (mc.Unet if self.base == "cond" else mu.Unet)(4, self.cfg)

    def _make_batch(self, seed):
        g = torch.Generator().manual_seed(seed)
        b = {"x": torch.randn(B, 4, 32, 32, generator=g), "t": torch.randint(0, 1000, (B,), generator=g), "cond": None}
        if self.base != "uncond":
            dim = self.cfg["condition_config"]["text_condition_config"]["text_embed_dim"]
            b["cond"] = {"text": torch.randn(B, 77, dim, generator=g),
                         "image": one_hot(torch.randint(0, 19, (B, 64, 64), generator=g))}
        b["target"] = torch.randn(B, 4, 32, 32, generator=g)
        return b

    def _loss(self, model, b, x, seed):
        if self.base == "uncond":
            out = model(x, b["t"].cuda())
        else:
            out = model(x, b["t"].cuda(), cond_input={k: v.cuda() for k, v in b["cond"].items()})
        return F.mse_loss(out, b["target"].cuda())

    def _oracle_loss(self, p, b, x, seed, aux):
        if self.base == "dit":
            out = DO.dit_forward(p, self.cfg, x, b["t"], b["cond"])
        else:
            out = O.unet_forward(p, self.cfg, x, b["t"], b["cond"])
        return F.mse_loss(out, b["target"])

    def frozen(self, name, rule):
        if self.base == "dit":
            if rule == "tail":
                return not name.startswith("transformer_layers.1.")
            return "attn_block" in name or name.startswith("proj_out")
        if rule == "tail":
            return not name.startswith("ups.")
        # every t_emb_layers and attention parameter, and the whole of the up blocks and the head (under the staged
        # backward those are whole segments)
        return ("t_emb_layers" in name or "attention" in name or name.startswith("ups.")
                or name.startswith(("norm_out", "conv_out")))


class Autoencoder(Case):
    """kind: "vqvae" (models.vqvae), "vqvae_noise" (models.vqvae_noise at N_SCALE) or "vae" (models.vae). The batches
    are the two images of the reference's own training fixture (64 x 64, B = 2)."""

    def __init__(self, name, kind, seed=9):
        super().__init__(name)
        self.kind, self.seed, self.cfg = kind, seed, SMALL_VQVAE

    def _make_state(self):
        shapes = VAO.param_shapes() if self.kind == "vae" else VO.vqvae_param_shapes(self.cfg)
        return O.deterministic_state(shapes, seed=self.seed)

    def _module(self):
        if self.kind == "vae":
            from models.vae import VAE
            return VAE(3, self.cfg)
        if self.kind == "vqvae_noise":
            from models.vqvae_noise import VQVAE as Noisy
            return Noisy(3, self.cfg)
        from models.vqvae import VQVAE
        return VQVAE(3, self.cfg)

    def _make_batch(self, seed):
        from safetensors.torch import load_file
        f = load_file(os.path.join(G, "vqvae_train.safetensors"))
        im = f["s0.im" if seed == SEEDS["a"] else "s1.im"]
        return {"x": im, "target": im.clone()}

    @staticmethod
    def kl(encoder_output):
        return VAO.kl_term(encoder_output)

    def _loss(self, model, b, x, seed):
        target = b["target"].cuda()
        torch.manual_seed(DRAW_SEED + seed)  # the one draw of the forward: device generator (noise), CPU generator (KL)
        if self.kind == "vae":
            out, enc = model(x)
            return F.mse_loss(out, target) + KL_WEIGHT * self.kl(enc)
        out, z, ql = model(x, N_SCALE) if self.kind == "vqvae_noise" else model(x)
        return F.mse_loss(out, target) + 1.0 * ql["codebook_loss"] + 0.2 * ql["commitment_loss"]

    def latent_shape(self):
        return (B, self.cfg["z_channels"], 16, 16)

    def _oracle_loss(self, p, b, x, seed, aux):
        aux = aux or {}
        pre = VO.encode_pre_quant(p, self.cfg, x)
        if self.kind == "vae":
            torch.manual_seed(DRAW_SEED + seed)
            eps = torch.randn(self.latent_shape())  # models/vae.py draws on the CPU default generator
            mean, logvar = torch.chunk(pre, 2, dim=1)
            out = VO.decode(p, self.cfg, mean + torch.exp(0.5 * logvar) * eps)
            return F.mse_loss(out, b["target"]) + KL_WEIGHT * self.kl(pre)
        zq, cb, cm, _ = VO.quantize_train(p, pre, aux.get("indices"))
        if self.kind == "vqvae_noise":
            eps = aux.get("eps")
            if eps is None:  # (CPU-only use: any fixed standard-normal draw)
                eps = torch.randn(self.latent_shape(), generator=torch.Generator().manual_seed(DRAW_SEED + seed))
            zq = zq + NO.latent_range(zq, aux.get("masks")) * N_SCALE * eps
        out = VO.decode(p, self.cfg, zq)
        return F.mse_loss(out, b["target"]) + 1.0 * cb + 0.2 * cm

    def aux(self, model, which):
        """The code indices (and, with noise, the extremal positions of the clean latent and the device draw) of the
        module's own forward of batch `which`: the quantiser's argmin and the range's arg-extremes are decided by the
        last bit, so a bf16 path is held to the oracle at its own choices (tests/test_vqvae_noise_gpu.py)."""
        if self.kind == "vae":
            return None
        x = self.batch(which)["x"].cuda()
        with torch.no_grad():
            if model._leaf():
                zq, _, idx = model._leaf_encode(x)
            else:
                _, c = model._train_eng(x).forward(x, need_backward=False)
                zq, idx = c["zq"], c["indices"]
        out = {"indices": idx.cpu()}
        if self.kind == "vqvae_noise":
            zq = zq.cpu()
            torch.manual_seed(DRAW_SEED + SEEDS[which])
            out["eps"] = torch.randn(self.latent_shape(), dtype=torch.float32, device="cuda").cpu()
            out["masks"] = (zq == zq.max(), zq == zq.min())
        return out

    def frozen(self, name, rule):
        if rule == "tail":
            return not name.startswith("decoder_")
        return "attention" in name or name.startswith("decoder_")


CASES = [
    Denoiser("cond", "cond", SMALL_COND, staged=False),
    Denoiser("cond_staged", "cond", SMALL_COND, staged=True),
    Denoiser("uncond", "uncond", SMALL_UNCOND, staged=False),
    Denoiser("dit", "dit", SMALL_DIT, staged=False, seed=4),
    Autoencoder("vqvae", "vqvae"),
    Autoencoder("vqvae_noise", "vqvae_noise"),
    Autoencoder("vae", "vae"),
]
BY_NAME = {c.name: c for c in CASES}
# the distinct networks (the staged case shares the cond UNet's weights, batches and oracle)
ORACLE_CASES = [c for c in CASES if c.name != "cond_staged"]
