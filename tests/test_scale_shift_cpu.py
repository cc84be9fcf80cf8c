"""use_scale_shift_norm=True without a GPU: the state_dict contract (names and
shapes written out here, not taken from the plan), the parameter count, the
refusals that stay, and that nothing moved for a model with the flag off (plan
creation and state_dict handling need no device)."""
import ctypes
import math

import pytest
import torch

import scale_shift_oracle as sso
from oracle import unet as ou
from test_abi_cpu import CFGS

PROD, TINY = CFGS[0], CFGS[1]


def _groups(cfg):
    return 32 if cfg["model_channels"] >= 64 else 8


def _plan(cfg, dtype="fp32", **kw):
    from cwdm_hip.unet_runtime import UNetPlan
    return UNetPlan(cfg["in_channels"], cfg["model_channels"], cfg["out_channels"], cfg["num_res_blocks"],
                    cfg["channel_mult"], _groups(cfg), dtype, **kw)


def _model(cfg, cls=None, **kw):
    from guided_diffusion.unet import UNetModel
    kw.setdefault("use_scale_shift_norm", True)
    kw.setdefault("bottleneck_attention", False)
    return (cls or UNetModel)(image_size=64, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                              out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                              attention_resolutions=(), channel_mult=cfg["channel_mult"], dims=3,
                              resblock_updown=True, resample_2d=False, num_groups=_groups(cfg), **kw)


def _res_names(p, ci, co, E):
    out = [(p + ".in_layers.0.weight", (ci,)), (p + ".in_layers.0.bias", (ci,)),
           (p + ".in_layers.2.weight", (co, ci, 3, 3, 3)), (p + ".in_layers.2.bias", (co,)),
           (p + ".emb_layers.1.weight", (2 * co, E)), (p + ".emb_layers.1.bias", (2 * co,)),
           (p + ".out_layers.0.weight", (co,)), (p + ".out_layers.0.bias", (co,)),
           (p + ".out_layers.3.weight", (co, co, 3, 3, 3)), (p + ".out_layers.3.bias", (co,))]
    if ci != co:
        out += [(p + ".skip_connection.weight", (co, ci, 1, 1, 1)), (p + ".skip_connection.bias", (co,))]
    return out


def _c1_names():
    """cases.C1_CFG (32 channels, mult (1, 2), one ResBlock per level), every entry written out."""
    E = 128
    out = [("time_embed.0.weight", (E, 32)), ("time_embed.0.bias", (E,)),
           ("time_embed.2.weight", (E, E)), ("time_embed.2.bias", (E,)),
           ("input_blocks.0.0.weight", (32, 32, 3, 3, 3)), ("input_blocks.0.0.bias", (32,))]
    out += _res_names("input_blocks.1.0", 32, 32, E)
    out += _res_names("input_blocks.2.0", 32, 32, E)       # the down block
    out += _res_names("input_blocks.3.0", 32, 64, E)
    out += _res_names("middle_block.0", 64, 64, E)
    out += _res_names("middle_block.1", 64, 64, E)
    out += _res_names("output_blocks.0.0", 128, 64, E)
    out += _res_names("output_blocks.1.0", 96, 64, E)
    out += _res_names("output_blocks.1.1", 64, 64, E)      # the up block
    out += _res_names("output_blocks.2.0", 96, 32, E)
    out += _res_names("output_blocks.3.0", 64, 32, E)
    out += [("out.0.weight", (32,)), ("out.0.bias", (32,)), ("out.2.weight", (8, 32, 3, 3, 3)), ("out.2.bias", (8,))]
    return out


def _prod_names():
    """The production config (64 channels, mult (1, 2, 2, 4, 4), two ResBlocks per level), every block written out
    as (prefix, C_in, C_out)."""
    E = 256
    out = [("time_embed.0.weight", (E, 64)), ("time_embed.0.bias", (E,)),
           ("time_embed.2.weight", (E, E)), ("time_embed.2.bias", (E,)),
           ("input_blocks.0.0.weight", (64, 32, 3, 3, 3)), ("input_blocks.0.0.bias", (64,))]
    blocks = [
        ("input_blocks.1.0", 64, 64), ("input_blocks.2.0", 64, 64), ("input_blocks.3.0", 64, 64),          # .3: down
        ("input_blocks.4.0", 64, 128), ("input_blocks.5.0", 128, 128), ("input_blocks.6.0", 128, 128),     # .6: down
        ("input_blocks.7.0", 128, 128), ("input_blocks.8.0", 128, 128), ("input_blocks.9.0", 128, 128),    # .9: down
        ("input_blocks.10.0", 128, 256), ("input_blocks.11.0", 256, 256), ("input_blocks.12.0", 256, 256),  # .12: down
        ("input_blocks.13.0", 256, 256), ("input_blocks.14.0", 256, 256),
        ("middle_block.0", 256, 256), ("middle_block.1", 256, 256),
        ("output_blocks.0.0", 512, 256), ("output_blocks.1.0", 512, 256), ("output_blocks.2.0", 512, 256),
        ("output_blocks.2.1", 256, 256),                                                                   # up
        ("output_blocks.3.0", 512, 256), ("output_blocks.4.0", 512, 256), ("output_blocks.5.0", 384, 256),
        ("output_blocks.5.1", 256, 256),                                                                   # up
        ("output_blocks.6.0", 384, 128), ("output_blocks.7.0", 256, 128), ("output_blocks.8.0", 256, 128),
        ("output_blocks.8.1", 128, 128),                                                                   # up
        ("output_blocks.9.0", 256, 128), ("output_blocks.10.0", 256, 128), ("output_blocks.11.0", 192, 128),
        ("output_blocks.11.1", 128, 128),                                                                  # up
        ("output_blocks.12.0", 192, 64), ("output_blocks.13.0", 128, 64), ("output_blocks.14.0", 128, 64),
    ]
    for p, ci, co in blocks:
        out += _res_names(p, ci, co, E)
    out += [("out.0.weight", (64,)), ("out.0.bias", (64,)), ("out.2.weight", (8, 64, 3, 3, 3)), ("out.2.bias", (8,))]
    return out


@pytest.mark.parametrize("cfg,names", [(TINY, _c1_names), (PROD, _prod_names)], ids=["c1", "production"])
def test_state_dict_written_out(cfg, names):
    sd = [(n, tuple(v.shape)) for n, v in _model(cfg).state_dict().items()]
    assert sd == names()
    assert sd == [(n, tuple(s)) for n, s in sso.param_shapes(**cfg)]


@pytest.mark.parametrize("cfg", [TINY, PROD], ids=["c1", "production"])
def test_only_the_emb_layers_differ_from_the_plain_model(cfg):
    sd = [(n, tuple(v.shape)) for n, v in _model(cfg).state_dict().items()]
    plain = [(n, tuple(s)) for n, s in ou.param_shapes(**cfg)]
    E = 4 * cfg["model_channels"]
    assert [n for n, _ in sd] == [n for n, _ in plain]
    n_emb = 0
    for (n, s), (_, sp) in zip(sd, plain):
        if n.endswith(".emb_layers.1.weight"):
            assert s == (2 * sp[0], E) and sp[1] == E, n
            n_emb += 1
        elif n.endswith(".emb_layers.1.bias"):
            assert s == (2 * sp[0],), n
        else:
            assert s == sp, n
    assert n_emb == sum(1 for b in ou.topology(**cfg) if b["kind"] == "res")
    assert sd == [(n, tuple(s)) for n, s in sso.param_shapes(**cfg)]
    # with the skips averaged or the bottleneck attention, the restatement lists the model's contract too
    for opts in (dict(additive_skips=True), dict(bottleneck_attention=True)):
        got = [(n, tuple(v.shape)) for n, v in _model(cfg, **opts).state_dict().items()]
        assert got == [(n, tuple(s)) for n, s in sso.param_shapes(**opts, **cfg)], opts


def test_production_parameter_count():
    """Each ResBlock's emb_layers.1 gains C_out rows of E + 1 numbers: the plain model's 81,511,048
    plus (E + 1) times the sum of the ResBlocks' output channels."""
    E = 256
    # encoder: 2 blocks per level + a down block (levels 0-3); middle: 2; decoder: 3 per level + an up block (levels 4-1)
    enc = 2 * (64 + 128 + 128 + 256 + 256) + (64 + 128 + 128 + 256)
    mid = 2 * 256
    dec = 3 * (256 + 256 + 128 + 128 + 64) + (256 + 256 + 128 + 128)
    couts = enc + mid + dec
    assert couts == sum(b["cout"] for b in ou.topology(**PROD) if b["kind"] == "res")
    n = sum(p.numel() for p in _model(PROD).parameters())
    assert n == 81_511_048 + (E + 1) * couts
    assert sum(math.prod(s) for _, s in _plan(PROD, "bf16", use_scale_shift_norm=True).param_specs) == n


def test_load_state_dict_round_trip():
    m = _model(TINY)
    sd0 = m.state_dict()
    # reference init: out_layers.3 zero (zero_module), the norms at ones / zeros, emb_layers drawn
    assert not sd0["middle_block.0.out_layers.3.weight"].any()
    assert bool((sd0["middle_block.0.out_layers.0.weight"] == 1).all())
    assert sd0["middle_block.0.emb_layers.1.weight"].abs().max() > 0
    assert sd0["middle_block.0.emb_layers.1.weight"].abs().max() <= 1 / math.sqrt(128)
    P = sso.random_params(seed=3, **TINY)
    m.load_state_dict(P)
    back = m.state_dict()
    assert list(back) == list(P)
    for k in P:
        assert torch.equal(back[k], P[k]), k
    m2 = _model(TINY)
    m2.load_state_dict(back)
    assert torch.equal(m2.flat_params, m.flat_params)
    with pytest.raises(RuntimeError, match="emb_layers"):   # a checkpoint without FiLM does not load
        m.load_state_dict(ou.random_params(seed=3, **TINY))
    with pytest.raises(RuntimeError, match="emb_layers"):   # ... nor a FiLM checkpoint into the plain model
        _model(TINY, use_scale_shift_norm=False).load_state_dict(P)
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU fallback
        m(torch.zeros(1, 32, 16, 16, 16), torch.zeros(1))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_flag_off_plans_are_the_default_plans(dtype):
    """Passing the flag as off is the same as not passing it, in every size the plan reports.  Both plans come
    from this tree: that the default plan itself did not move is held by the parameter list compared with
    oracle.unet.param_shapes here and by the recorded sizes of tests/golden/route_sizes.json."""
    grid = (1, 32, 32, 32)
    for cfg in (TINY, PROD):
        plan = _plan(cfg, dtype)
        off = _plan(cfg, dtype, use_scale_shift_norm=False)
        assert plan.param_specs == [(n, tuple(s)) for n, s in ou.param_shapes(**cfg)]
        assert off.param_specs == plan.param_specs and off.packed_bytes == plan.packed_bytes
        assert off.packed_bwd_bytes == plan.packed_bwd_bytes
        assert off.workspace_bytes(*grid) == plan.workspace_bytes(*grid)
        assert off.train_workspace_bytes(*grid) == plan.train_workspace_bytes(*grid)
        assert off.grad_workspace_bytes(*grid) == plan.grad_workspace_bytes(*grid)
        assert off.flops(*grid) == plan.flops(*grid) and off.backward_flops(*grid) == plan.backward_flops(*grid)
        assert off.num_segments == plan.num_segments
        # the flag adds parameters and embedding rows, but no conv, no segment and no FLOPs
        on = _plan(cfg, dtype, use_scale_shift_norm=True)
        assert on.flops(*grid) == plan.flops(*grid) and on.num_segments == plan.num_segments
        assert on.grad_numel > plan.grad_numel and on.packed_bytes > plan.packed_bytes
    assert "middle_block.1.emb_layers.1.weight" in _model(TINY, use_scale_shift_norm=False).state_dict()
    assert _model(TINY, use_scale_shift_norm=False).state_dict()["middle_block.1.emb_layers.1.weight"].shape == (64, 128)


def test_segments_cover_the_flat_gradient_once():
    plan = _plan(TINY, "bf16", use_scale_shift_norm=True)
    cover = torch.zeros(plan.grad_numel, dtype=torch.int32)
    for s in range(plan.num_segments):
        off, n = plan.segment_range(s)
        cover[off:off + n] += 1
    assert bool((cover == 1).all())
    assert plan.grad_numel == sum(math.prod(s) for _, s in _c1_names())


def test_wavunet_still_raises():
    from guided_diffusion.wunet import WavUNetModel
    with pytest.raises(NotImplementedError, match="use_scale_shift_norm"):
        _model(dict(TINY, num_res_blocks=2), cls=WavUNetModel, use_freq=True)


def test_script_util_builds_the_film_model():
    from guided_diffusion import script_util
    m = script_util.create_model(image_size=128, num_channels=32, num_res_blocks=1, channel_mult="1,2",
                                 attention_resolutions="", dims=3, num_groups=8, in_channels=32, out_channels=8,
                                 bottleneck_attention=False, resblock_updown=True, resample_2d=False,
                                 use_scale_shift_norm=True)
    assert m.use_scale_shift_norm
    assert m.state_dict()["middle_block.0.emb_layers.1.weight"].shape == (128, 128)
    assert m.state_dict()["input_blocks.1.0.emb_layers.1.bias"].shape == (64,)
    # the factory default of the flag builds, given the other switches of the run.sh family
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8)
    args["use_scale_shift_norm"] = script_util.model_and_diffusion_defaults()["use_scale_shift_norm"]
    assert args["use_scale_shift_norm"] is True
    keys = script_util.model_and_diffusion_defaults().keys()
    model, _ = script_util.create_model_and_diffusion(**{k: args[k] for k in keys})
    assert model.use_scale_shift_norm


def test_plan_refuses_the_flag_with_use_freq():
    from cwdm_hip import _lib
    cfg = _lib.UNetConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels, cfg.num_res_blocks, cfg.num_levels = 32, 32, 8, 2, 2
    cfg.channel_mult[0], cfg.channel_mult[1] = 1, 2
    cfg.num_groups, cfg.dtype, cfg.resblock_updown = 8, _lib.CWDM_F32, 1

    def create():
        h = ctypes.c_void_p()
        rc = _lib.lib().cwdm_unet_create(ctypes.byref(cfg), ctypes.byref(h))
        msg = _lib.lib().cwdm_last_error() if rc else b""
        if h.value:
            _lib.lib().cwdm_unet_destroy(h)
        return rc, msg
    cfg.use_freq, cfg.use_scale_shift_norm = 1, 0
    assert create()[0] == 0
    cfg.use_freq, cfg.use_scale_shift_norm = 0, 1
    assert create()[0] == 0
    cfg.use_freq, cfg.use_scale_shift_norm = 1, 1
    rc, msg = create()
    assert rc == _lib.E_UNSUPPORTED and b"use_scale_shift_norm" in msg and b"use_freq" in msg
