"""Classifier-free guidance, host side (no GPU): the mode a guidance scale selects follows the reference's
_GuidedWrapper (batch_condition_image_generator_single.py:255-262), and the combine entry points of the C ABI refuse
null / empty arguments before any launch."""
import ctypes

import pytest


@pytest.mark.parametrize("scale,mode", [(-1, "uncond"), (0, "uncond"), (0.5, "guided"), (1, "cond"),
                                        (1 + 5e-7, "cond"), (3, "guided")])
def test_guidance_mode_follows_reference_wrapper(scale, mode):
    from sdmi.sampling import guidance_mode
    assert guidance_mode(scale) == mode


def test_uncond_input_must_mirror_cond_input():
    import torch
    from sdmi.sampling import check_uncond
    c = {"text": torch.zeros(2, 7, 8), "class": torch.zeros(2, 10)}
    check_uncond(c, None)
    check_uncond(c, {k: v.clone() for k, v in c.items()})
    with pytest.raises(ValueError):
        check_uncond(None, c)
    with pytest.raises(ValueError):
        check_uncond(c, {"text": c["text"]})
    with pytest.raises(ValueError):
        check_uncond(c, {"text": c["text"], "class": torch.zeros(2, 11)})


def test_combine_entry_points_refuse_null_arguments():
    from sdmi import _lib
    L = _lib.lib()
    host = ctypes.create_string_buffer(64)  # never dereferenced: every call below returns before a launch
    p = ctypes.addressof(host)
    assert L.sdmi_cfg_combine(None, None, 16, 1.5, None, None) == -1
    assert L.sdmi_cfg_combine(None, p, 16, 1.5, p, None) == -1
    assert L.sdmi_cfg_combine(p, None, 16, 1.5, p, None) == -1
    assert L.sdmi_cfg_combine(p, p, 16, 1.5, None, None) == -1
    assert L.sdmi_cfg_combine(p, p, 0, 1.5, p, None) == -1
    assert L.sdmi_cfg_combine_nhwc(None, 1, 8, 1, 4, 16, 1.5, None, None) == -1
    assert L.sdmi_cfg_combine_nhwc(None, 1, 8, 1, 4, 16, 1.5, p, None) == -1
    assert L.sdmi_cfg_combine_nhwc(p, 1, 8, 1, 4, 16, 1.5, None, None) == -1
    assert L.sdmi_cfg_combine_nhwc(p, 1, 8, 0, 4, 16, 1.5, p, None) == -1
    assert L.sdmi_cfg_combine_nhwc(p, 1, 2, 1, 4, 16, 1.5, p, None) == -1  # row stride below the channel count
