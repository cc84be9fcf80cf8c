"""8 + 8x input channels (0..4 condition volumes) without a device: the plans create in every compute dtype
with the reference's parameter contract, what is refused stays refused, the configurations that worked before
keep their sizes (tests/golden/cond_count_sizes.json, recorded with tools/record_plan_sizes.py from the
library of the commit before), and mode='default' reaches the kernels."""
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN
from oracle import cases, unet as ou

TINY = dict(cases.C1_CFG)
PROD = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
MODELS = {"tiny": (TINY, cases.C1_GROUPS), "prod": (PROD, 32)}


def _plan(cfg, groups, in_channels, dtype, **kw):
    from cwdm_hip.unet_runtime import UNetPlan
    return UNetPlan(in_channels, cfg["model_channels"], cfg["out_channels"], cfg["num_res_blocks"],
                    cfg["channel_mult"], groups, dtype, **kw)


@pytest.mark.parametrize("model", ["tiny", "prod"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("cin", [8, 16, 24, 32, 40])
def test_plans_create_with_the_reference_parameters(cin, dtype, model):
    cfg, groups = MODELS[model]
    plan = _plan(cfg, groups, cin, dtype)
    want = ou.param_shapes(**dict(cfg, in_channels=cin))
    assert [(n, tuple(s)) for n, s in plan.param_specs] == [(n, tuple(s)) for n, s in want]
    assert dict(plan.param_specs)["input_blocks.0.0.weight"] == (cfg["model_channels"], cin, 3, 3, 3)
    n = sum(math.prod(s) for _, s in want)
    assert plan.grad_numel == n
    # the backward's segments tile exactly the parameters: no padded column reaches the flat gradient
    assert sum(plan.segment_range(s)[1] for s in range(plan.num_segments)) == n
    assert plan.packed_bytes > 0 and plan.workspace_bytes(1, 16, 16, 16) > 0
    assert plan.grad_workspace_bytes(1, 16, 16, 16) > 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("cin", [8, 24, 40])
def test_flops_count_the_real_input_channels(cin, dtype):
    """cwdm_unet_flops / cwdm_unet_backward_flops of a padded plan: the fp32 plan's (whose chunk is 8, so it pads
    nothing), i.e. linear in in_channels through conv_in alone."""
    cfg, groups = MODELS["tiny"]
    grid = (2, 16, 16, 16)
    padded, plain = _plan(cfg, groups, cin, dtype), _plan(cfg, groups, cin, "fp32")
    assert padded.flops(*grid) == plain.flops(*grid)
    assert padded.backward_flops(*grid) == plain.backward_flops(*grid)
    f16, f32 = _plan(cfg, groups, 16, dtype).flops(*grid), _plan(cfg, groups, 32, dtype).flops(*grid)
    conv_in_per_channel = 2.0 * 2 * 16 ** 3 * cfg["model_channels"] * 27
    assert f32 - f16 == 16 * conv_in_per_channel
    assert padded.flops(*grid) == f16 + (cin - 16) * conv_in_per_channel


def test_padded_plan_grows_only_by_the_staged_input():
    """in_channels=24 in bf16 runs conv_in on 32 channels: its packed weights are the 32-channel plan's, and its
    workspace is that plan's plus the staged copy of x (one 256-byte-aligned tensor)."""
    cfg, groups = MODELS["tiny"]
    p24, p32 = _plan(cfg, groups, 24, "bf16"), _plan(cfg, groups, 32, "bf16")
    assert p24.packed_bytes == p32.packed_bytes
    B, D, H, W = 2, 16, 16, 16
    staged = B * D * H * W * 32 * 2
    assert staged % 256 == 0
    assert p24.workspace_bytes(B, D, H, W) == p32.workspace_bytes(B, D, H, W) + staged
    assert p24.train_workspace_bytes(B, D, H, W) == p32.train_workspace_bytes(B, D, H, W) + staged


def test_refusals():
    from cwdm_hip._lib import CwdmError
    cfg, groups = MODELS["tiny"]
    for dtype in ("fp32", "bf16", "fp16"):
        with pytest.raises(CwdmError, match="multiple of 8"):
            _plan(cfg, groups, 12, dtype)
    # WavUNetModel's pyramid reads the input tensor itself: the chunk rule stays
    wav = dict(cfg, num_res_blocks=2)
    with pytest.raises(CwdmError, match="multiple of 16"):
        _plan(wav, groups, 8, "bf16", use_freq=True)
    with pytest.raises(CwdmError, match="multiple of 16"):
        _plan(wav, groups, 24, "fp16", use_freq=True)
    _plan(wav, groups, 8, "fp32", use_freq=True)
    _plan(wav, groups, 16, "bf16", use_freq=True)


def _golden():
    with open(os.path.join(GOLDEN, "cond_count_sizes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("key", sorted(_golden()))
def test_aligned_configurations_keep_their_sizes(key):
    """in_channels 16 and 32: packed bytes, the three workspace sizes and the FLOPs are those of the commit
    before (which built these plans already)."""
    want = _golden()[key]
    model, cin, dtype = key.split("/")
    cfg, groups = MODELS[model]
    plan = _plan(cfg, groups, int(cin[2:]), dtype)
    assert plan.packed_bytes == want["packed_bytes"]
    assert plan.packed_bwd_bytes == want["packed_bwd_bytes"]
    assert plan.num_segments == want["num_segments"]
    for g, rec in want["grids"].items():
        grid = tuple(int(v) for v in g.split("x"))
        got = {"workspace_bytes": plan.workspace_bytes(*grid), "train_workspace_bytes": plan.train_workspace_bytes(*grid),
               "grad_workspace_bytes": plan.grad_workspace_bytes(*grid), "flops": plan.flops(*grid),
               "backward_flops": plan.backward_flops(*grid)}
        assert got == rec, (key, g)


def test_unet_model_and_factory_take_any_member_of_the_family():
    from guided_diffusion import script_util
    for cin, mode in ((8, "default"), (16, "i2i"), (24, "i2i"), (40, "i2i")):
        args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                             in_channels=cin, mode=mode)
        keys = script_util.model_and_diffusion_defaults().keys()
        model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype="bf16")
        assert diffusion.mode == mode and model.in_channels == cin
        assert model.state_dict()["input_blocks.0.0.weight"].shape == (32, cin, 3, 3, 3)
        assert model.plan.in_channels == cin   # the bf16 plan creates


def _default_model_and_diffusion(cin=8):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         in_channels=cin, mode="default" if cin == 8 else "i2i")
    keys = script_util.model_and_diffusion_defaults().keys()
    return script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype="bf16")


def test_training_losses_default_mode_reaches_the_kernels():
    """mode='default' and the generic condition dict on CPU tensors stop at the kernels ("no CPU fallback"), not
    at a NotImplementedError; a mode the engine does not have still says so."""
    model, diffusion = _default_model_and_diffusion()
    x = torch.rand(1, 1, 16, 16, 16)
    t = torch.tensor([3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diffusion.training_losses(model, x, t, mode="default")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diffusion.training_losses(model, {"target": x, "cond": [x]}, t, mode="i2i")
    with pytest.raises(NotImplementedError):
        diffusion.training_losses(model, x, t, mode="segmentation")
