"""The entry checks of cwdm_unet_forward / cwdm_unet_forward_step without a GPU: each
returns its code (and message) before anything touches the device, so dummy non-null
pointers are enough and nothing is dereferenced."""
import ctypes

import pytest

from cwdm_hip import _lib

PTR = 0x1000   # a non-null address no check reads through


def _plan(L, levels=2, use_freq=0):
    cfg = _lib.UNetConfig(in_channels=16,model_channels=32, out_channels=8, num_res_blocks=1, num_levels=levels,
                          num_groups=8, dtype=_lib.CWDM_BF16, resblock_updown=1, use_freq=use_freq)
    for i in range(levels):
        cfg.channel_mult[i] = 1
    plan = _lib.vp()
    assert L.cwdm_unet_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0, L.cwdm_last_error()
    return plan


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def plans(L):
    made = {"unet2": _plan(L, 2), "unet3": _plan(L, 3), "wav2": _plan(L, 2, use_freq=1)}
    yield made
    for p in made.values():
        L.cwdm_unet_destroy(p)


def _forward(L, plan, B=1, D=16, H=16, W=16, ws_bytes=1 << 40, **null):
    a = {k: PTR for k in ("packed", "x", "t", "out", "ws")}
    a.update(null)
    return L.cwdm_unet_forward(plan, a["packed"], a["x"], a["t"], a["out"], B, D, H, W, a["ws"], ws_bytes, None)


@pytest.mark.parametrize("which", ["plan", "packed", "x", "t", "out", "ws"])
def test_null_argument_is_invalid(L, plans, which):
    if which == "plan":
        assert _forward(L, None) == _lib.E_INVALID
    else:
        assert _forward(L, plans["unet2"], **{which: None}) == _lib.E_INVALID
    assert b"null pointer" in L.cwdm_last_error()


def test_empty_batch_is_a_shape_error(L, plans):
    assert _forward(L, plans["unet2"], B=0) == _lib.E_SHAPE


@pytest.mark.parametrize("name,div", [("unet2", 2), ("unet3", 4), ("wav2", 4)])
def test_grid_edges_must_divide_by_the_level_count(L, plans, name, div):
    """2^(levels - 1) for UNetModel, 2^levels with use_freq: every edge, one at a time."""
    good = 4 * div
    assert L.cwdm_unet_workspace_bytes(plans[name], 1, good, good, good) > 0
    for axis in ("D", "H", "W"):
        edges = {"D": good, "H": good, "W": good, axis: good + div // 2}
        assert _forward(L, plans[name], **edges) == _lib.E_SHAPE, (name, axis)
        assert f"divisible by {div}".encode() in L.cwdm_last_error()


def test_workspace_one_byte_short_names_the_size_it_needs(L, plans):
    need = L.cwdm_unet_workspace_bytes(plans["unet2"], 2, 16, 16, 16)
    assert need > 0
    assert _forward(L, plans["unet2"], B=2, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert f"need {need} bytes".encode() in L.cwdm_last_error()


def test_forward_step_grid_must_be_the_steps(L, plans):
    def step(**kw):
        st = _lib.SamplerArgs(model_out=PTR, B=1, d=16, h=16, w=16, levels=1)
        for k, v in kw.items():
            setattr(st, k, v)
        return L.cwdm_unet_forward_step(plans["unet2"], PTR, PTR, PTR, ctypes.byref(st), 1, 16, 16, 16, PTR, 1 << 40,
                                        None, None)
    for kw in ({"d": 8}, {"h": 32}, {"w": 8}, {"B": 2}):
        assert step(**kw) == _lib.E_SHAPE, kw
        assert b"the step's grid must be the forward's" in L.cwdm_last_error()
    assert step(model_out=None) == _lib.E_INVALID
