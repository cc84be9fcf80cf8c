"""additive_skips=True without a GPU: the plan's parameter contract against the
restatement's own list (tests/additive_oracle.py), the model's state_dict, and
the refusals that stay (plan creation and state_dict handling need no device)."""
import ctypes

import pytest
import torch

import additive_oracle as ao
from oracle import unet as ou
from test_abi_cpu import CFGS

TINY = CFGS[1]


def _groups(cfg):
    return 32 if cfg["model_channels"] >= 64 else 8


def _plan(cfg, dtype, **kw):
    from cwdm_hip.unet_runtime import UNetPlan
    return UNetPlan(cfg["in_channels"], cfg["model_channels"], cfg["out_channels"], cfg["num_res_blocks"],
                    cfg["channel_mult"], _groups(cfg), dtype, **kw)


def _model(cfg, cls=None, **kw):
    from guided_diffusion.unet import UNetModel
    return (cls or UNetModel)(image_size=64, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                              out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                              attention_resolutions=(), channel_mult=cfg["channel_mult"], dims=3,
                              resblock_updown=True, bottleneck_attention=False, resample_2d=False,
                              num_groups=_groups(cfg), **kw)


def test_restatement_worked_example():
    """model_channels=32, channel_mult=(1, 2), num_res_blocks=1: the skip stack is
    [32, 32, 32, 64], output_blocks.0.0 is 64 -> 32 with a 1x1 skip, the rest 32 -> 32."""
    dec = [(b["prefix"], b["cin"], b["cout"], b.get("updown")) for b in ao.topology(**TINY)
           if b["prefix"].startswith("output_blocks")]
    assert dec == [("output_blocks.0.0", 64, 32, None), ("output_blocks.1.0", 32, 32, None),
                   ("output_blocks.1.1", 32, 32, "up"), ("output_blocks.2.0", 32, 32, None),
                   ("output_blocks.3.0", 32, 32, None)]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plan_param_contract_and_flops(cfg, dtype):
    plan = _plan(cfg, dtype, additive_skips=True)
    want = ao.param_shapes(**cfg)
    assert [(n, tuple(s)) for n, s in plan.param_specs] == [(n, tuple(s)) for n, s in want]
    # encoder, middle block and head are the concatenating model's; only decoder parameters differ
    # (every .0 block's input width, and the widths downstream of a mid_ch that is not the level's)
    cat = dict(ou.param_shapes(**cfg))
    differ = [n for n, s in want if n not in cat or tuple(cat[n]) != tuple(s)]
    assert differ and all(n.startswith("output_blocks.") for n in differ), differ
    assert all(n in dict(want) or n.startswith("output_blocks.") for n in cat)
    if cfg is TINY:
        got = dict(plan.param_specs)
        assert got["output_blocks.0.0.in_layers.2.weight"] == (32, 64, 3, 3, 3)
        assert "output_blocks.0.0.skip_connection.weight" in got
    assert 0 < plan.flops(1, 32, 32, 32) < _plan(cfg, dtype).flops(1, 32, 32, 32)
    # the backward's segments still tile the flat gradient
    assert sum(plan.segment_range(s)[1] for s in range(plan.num_segments)) == plan.grad_numel
    assert plan.workspace_bytes(1, 32, 32, 32) > 0 and plan.grad_workspace_bytes(1, 32, 32, 32) > 0
    assert plan.train_workspace_bytes(1, 32, 32, 32) >= plan.workspace_bytes(1, 32, 32, 32)


def test_plan_param_contract_resblock_updown_false():
    """The flag composes with the Downsample / Upsample conv layers: the Upsample keeps mid_ch."""
    cfg = CFGS[0]
    plan = _plan(cfg, "bf16", resblock_updown=False, additive_skips=True)
    want = ao.param_shapes(resblock_updown=False, **cfg)
    assert [(n, tuple(s)) for n, s in plan.param_specs] == [(n, tuple(s)) for n, s in want]
    assert "output_blocks.2.1.conv.weight" in dict(want)


def test_model_constructs_and_loads_additive_state_dict():
    m = _model(TINY, additive_skips=True)
    P = ao.random_params(seed=3, **TINY)
    assert [(n, tuple(v.shape)) for n, v in m.state_dict().items()] == [(n, tuple(v.shape)) for n, v in P.items()]
    m.load_state_dict(P)
    assert torch.equal(m.state_dict()["output_blocks.0.0.skip_connection.weight"],
                       P["output_blocks.0.0.skip_connection.weight"])
    with pytest.raises(RuntimeError, match="ROCm device"):   # no CPU fallback
        m(torch.zeros(1, 32, 16, 16, 16), torch.zeros(1))


def test_concatenating_state_dict_is_rejected():
    m = _model(TINY, additive_skips=True)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(ou.random_params(seed=3, **TINY))
    # and the other way round
    with pytest.raises(RuntimeError, match="size mismatch"):
        _model(TINY).load_state_dict(ao.random_params(seed=3, **TINY))


def test_script_util_forwards_the_flag():
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8)
    keys = script_util.model_and_diffusion_defaults().keys()
    kw = {k: args[k] for k in keys}
    kw["additive_skips"] = True
    model, _ = script_util.create_model_and_diffusion(**kw)
    assert model.additive_skips
    assert model.state_dict()["output_blocks.0.0.in_layers.2.weight"].shape == (32, 64, 3, 3, 3)


def test_wavunet_still_raises():
    from guided_diffusion.wunet import WavUNetModel
    with pytest.raises(NotImplementedError, match="additive_skips"):
        _model(dict(TINY, num_res_blocks=2), cls=WavUNetModel, additive_skips=True)


def test_plan_rejects_additive_skips_with_use_freq():
    from cwdm_hip import _lib
    cfg = _lib.UNetConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels, cfg.num_res_blocks, cfg.num_levels = 32, 32, 8, 2, 2
    cfg.channel_mult[0], cfg.channel_mult[1] = 1, 2
    cfg.num_groups, cfg.dtype, cfg.resblock_updown = 8, _lib.CWDM_F32, 1
    cfg.use_freq, cfg.additive_skips = 1, 1
    h = ctypes.c_void_p()
    assert _lib.lib().cwdm_unet_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.E_UNSUPPORTED
    assert b"additive_skips" in _lib.lib().cwdm_last_error()
    assert not h.value
    cfg.additive_skips = 0   # the same config without the flag is the WavUNetModel plan
    assert _lib.lib().cwdm_unet_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    _lib.lib().cwdm_unet_destroy(h)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_default_is_the_concatenating_plan(dtype):
    cfg = CFGS[0]
    a, b = _plan(cfg, dtype), _plan(cfg, dtype, additive_skips=False)
    assert a.param_specs == b.param_specs == [(n, tuple(s)) for n, s in ou.param_shapes(**cfg)]
    assert a.packed_bytes == b.packed_bytes
    assert a.workspace_bytes(1, 64, 64, 64) == b.workspace_bytes(1, 64, 64, 64)
    assert a.train_workspace_bytes(1, 64, 64, 64) == b.train_workspace_bytes(1, 64, 64, 64)
    assert a.grad_workspace_bytes(1, 64, 64, 64) == b.grad_workspace_bytes(1, 64, 64, 64)
