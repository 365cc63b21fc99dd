"""Host-side surface of the LPIPS drop-in (models/lpips.py) and of the trainer's LPIPS keywords; no kernel runs here.
(tests/test_cabi_cpu.py checks that every sdmi_lpips_* / sdmi_maxpool2_* declaration is exported and bound.)"""
import inspect
import sys

import pytest
import torch

from tests import lpips_ref as R


def test_module_imports_without_torchvision(monkeypatch):
    monkeypatch.setitem(sys.modules, "torchvision", None)  # `import torchvision` now raises ImportError
    monkeypatch.delitem(sys.modules, "models.lpips", raising=False)
    import models.lpips as ML
    assert all(hasattr(ML, n) for n in ("LPIPS", "vgg16", "ScalingLayer", "NetLinLayer", "spatial_average"))
    with _no_network():
        ML.LPIPS()


class _no_network:
    """Any attempt to open a socket while the module is built fails the test."""

    def __enter__(self):
        import socket
        self._orig = socket.socket.connect

        def refuse(*a, **kw):
            raise AssertionError("models.lpips tried to reach the network")

        socket.socket.connect = refuse

    def __exit__(self, *a):
        import socket
        socket.socket.connect = self._orig


def test_state_dict_keys_and_shapes_match_the_reference_layout():
    from models.lpips import LPIPS
    m = LPIPS()
    sd = m.state_dict()
    want = R.state_keys()
    assert len(want) == 38
    assert list(sd) == [k for k, _ in want]
    assert all(tuple(sd[k].shape) == s for k, s in want)
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    assert torch.equal(sd["scaling_layer.shift"].reshape(-1), torch.tensor(R.SHIFT))
    assert torch.equal(sd["scaling_layer.scale"].reshape(-1), torch.tensor(R.SCALE))
    assert sd["lins.3.model.1.weight"].data_ptr() == sd["lin3.model.1.weight"].data_ptr()  # registered twice
    m.load_state_dict(R.seeded_state())  # strict
    assert torch.equal(getattr(m.net.slice3, "12").weight, R.seeded_state()["net.slice3.12.weight"])
    assert LPIPS(use_dropout=False).state_dict().keys() != sd.keys()  # no Dropout: the conv is model.0, as torch gives


def test_weight_files_are_remapped(tmp_path):
    from models.lpips import LPIPS
    sd = R.seeded_state()
    vgg = {}
    for k, v in sd.items():
        if k.startswith("net."):
            _, _, i, leaf = k.split(".")
            vgg[f"features.{i}.{leaf}"] = v
    vgg["classifier.0.weight"] = torch.zeros(2, 2)  # the rest of a torchvision file is ignored
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin") and not k.startswith("lins")}, tmp_path / "vgg.pth")
    m = LPIPS(vgg_weights=str(tmp_path / "vgg16.pth"), lin_weights=str(tmp_path / "vgg.pth"))
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_cpu_tensors_raise():
    from models.lpips import LPIPS
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="runs on the MI355X HIP path only"):
        LPIPS()(x, x)


def test_training_mode_or_trainable_parameters_raise():
    from models.lpips import LPIPS
    x = torch.zeros(1, 3, 32, 32)
    m = LPIPS()
    m.train()
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m(x, x)
    m.eval()
    m.lin2.model[1].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"requires_grad_\(False\)"):
        m(x, x)


def test_trainer_keywords_and_default_losses_keys():
    from sdmi.vqvae_train import S_LOSS, VQVAETrainer
    sig = inspect.signature(VQVAETrainer.__init__).parameters
    assert sig["perceptual_weight"].default == 0.0 and sig["lpips_state"].default is None
    tr = VQVAETrainer.__new__(VQVAETrainer)  # the state losses() reads, as a default-built trainer leaves it
    tr.state = torch.zeros(8)
    tr.state[S_LOSS] = 0.25
    tr.vq_loss = torch.tensor([0.5])
    tr.hp = dict(cw=1.0, beta=0.2)
    tr.lpips = None
    got = tr.losses()
    assert list(got) == ["recon", "codebook", "commitment", "total"]
    assert got["total"] == pytest.approx(0.25 + 1.2 * 0.5)
