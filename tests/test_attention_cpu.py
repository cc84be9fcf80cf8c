"""bottleneck_attention=True without a GPU: the state_dict contract (names written
out here, not taken from the plan), parameter counts, the refusals that stay, the
plan's gradient segments and FLOPs, and that nothing moved for the model without
attention (plan creation and state_dict handling need no device)."""
import ctypes
import math

import pytest
import torch

import attention_oracle as ato
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
    kw.setdefault("bottleneck_attention", True)
    return (cls or UNetModel)(image_size=64, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                              out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                              attention_resolutions=(), channel_mult=cfg["channel_mult"], dims=3,
                              resblock_updown=True, resample_2d=False, num_groups=_groups(cfg), **kw)


def _attn_names(C):
    return [("middle_block.1.norm.weight", (C,)), ("middle_block.1.norm.bias", (C,)),
            ("middle_block.1.qkv.weight", (3 * C, C, 1)), ("middle_block.1.qkv.bias", (3 * C,)),
            ("middle_block.1.proj_out.weight", (C, C, 1)), ("middle_block.1.proj_out.bias", (C,))]


def _res_names(p, C, E):
    return [(p + ".in_layers.0.weight", (C,)), (p + ".in_layers.0.bias", (C,)),
            (p + ".in_layers.2.weight", (C, C, 3, 3, 3)), (p + ".in_layers.2.bias", (C,)),
            (p + ".emb_layers.1.weight", (C, E)), (p + ".emb_layers.1.bias", (C,)),
            (p + ".out_layers.0.weight", (C,)), (p + ".out_layers.0.bias", (C,)),
            (p + ".out_layers.3.weight", (C, C, 3, 3, 3)), (p + ".out_layers.3.bias", (C,))]


@pytest.mark.parametrize("cfg,C", [(TINY, 64), (PROD, 256)], ids=["c1", "production"])
def test_state_dict_names_and_shapes(cfg, C):
    sd = [(n, tuple(v.shape)) for n, v in _model(cfg).state_dict().items()]
    E = 4 * cfg["model_channels"]
    middle = [e for e in sd if e[0].startswith("middle_block.")]
    assert middle == _res_names("middle_block.0", C, E) + _attn_names(C) + _res_names("middle_block.2", C, E)
    # everything outside the middle block is the model without attention, in its order
    plain = [(n, tuple(s)) for n, s in ou.param_shapes(**cfg)]
    assert [e for e in sd if not e[0].startswith("middle_block.")] == \
        [e for e in plain if not e[0].startswith("middle_block.")]
    first = next(i for i, e in enumerate(sd) if e[0].startswith("middle_block."))
    assert sd[first - 1][0].startswith("input_blocks.") and sd[first + len(middle)][0].startswith("output_blocks.0.")
    # the restatement the GPU tests compare against lists the same contract
    assert sd == [(n, tuple(s)) for n, s in ato.param_shapes(**cfg)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_model_without_attention_keeps_its_names(dtype):
    for cfg in (TINY, PROD):
        plan = _plan(cfg, dtype)
        assert plan.param_specs == [(n, tuple(s)) for n, s in ou.param_shapes(**cfg)]
        off = _plan(cfg, dtype, bottleneck_attention=False, num_heads=4, use_new_attention_order=True)
        assert off.param_specs == plan.param_specs and off.packed_bytes == plan.packed_bytes
        assert off.workspace_bytes(1, 32, 32, 32) == plan.workspace_bytes(1, 32, 32, 32)
        assert off.train_workspace_bytes(1, 32, 32, 32) == plan.train_workspace_bytes(1, 32, 32, 32)
        assert off.grad_workspace_bytes(1, 32, 32, 32) == plan.grad_workspace_bytes(1, 32, 32, 32)
        assert off.flops(1, 32, 32, 32) == plan.flops(1, 32, 32, 32)
    sd = _model(TINY, bottleneck_attention=False).state_dict()
    assert "middle_block.1.in_layers.2.weight" in sd and "middle_block.2.in_layers.2.weight" not in sd


def test_production_parameter_count():
    C = 256
    n = sum(p.numel() for p in _model(PROD).parameters())
    assert n == 81_511_048 + (2 * C + 3 * C * C + 3 * C + C * C + C) == 81_774_728
    assert sum(math.prod(s) for _, s in _plan(PROD, "bf16", bottleneck_attention=True).param_specs) == n


@pytest.mark.parametrize("new_order", [False, True])
def test_load_state_dict_round_trip_and_init(new_order):
    m = _model(TINY, num_heads=4, use_new_attention_order=new_order)
    sd0 = m.state_dict()
    # reference init: proj_out zero (zero_module), the norm at ones / zeros, qkv drawn
    assert not sd0["middle_block.1.proj_out.weight"].any() and not sd0["middle_block.1.proj_out.bias"].any()
    assert bool((sd0["middle_block.1.norm.weight"] == 1).all()) and not sd0["middle_block.1.norm.bias"].any()
    assert sd0["middle_block.1.qkv.weight"].abs().max() > 0
    P = ato.random_params(seed=3, **TINY)
    m.load_state_dict(P)
    back = m.state_dict()
    assert list(back) == list(P)
    for k in P:
        assert torch.equal(back[k], P[k]), k
    m2 = _model(TINY, num_heads=4, use_new_attention_order=new_order)
    m2.load_state_dict(back)
    assert torch.equal(m2.flat_params, m.flat_params)
    with pytest.raises(RuntimeError):   # a checkpoint without the block does not load
        m.load_state_dict(ou.random_params(seed=3, **TINY))
    with pytest.raises(RuntimeError, match="ROCm device"):   # no CPU fallback
        m(torch.zeros(1, 32, 16, 16, 16), torch.zeros(1))


def test_per_level_attention_still_raises():
    from guided_diffusion.unet import UNetModel
    with pytest.raises(NotImplementedError, match="attention blocks"):
        UNetModel(image_size=64, in_channels=32, model_channels=32, out_channels=8, num_res_blocks=1,
                  attention_resolutions=(4,), channel_mult=(1, 2), dims=3, resblock_updown=True,
                  bottleneck_attention=True, resample_2d=False, num_groups=8)


def test_wavunet_still_raises():
    from guided_diffusion.wunet import WavUNetModel
    with pytest.raises(NotImplementedError, match="bottleneck_attention"):
        _model(dict(TINY, num_res_blocks=2), cls=WavUNetModel, use_freq=True)


def test_script_util_builds_the_attention_model():
    from guided_diffusion import script_util
    m = script_util.create_model(image_size=128, num_channels=32, num_res_blocks=1, channel_mult="1,2",
                                 attention_resolutions="", dims=3, num_groups=8, in_channels=32, out_channels=8,
                                 bottleneck_attention=True, resblock_updown=True, resample_2d=False, num_heads=2,
                                 use_new_attention_order=True)
    assert m.bottleneck_attention and m.num_heads == 2 and m.use_new_attention_order
    assert m.state_dict()["middle_block.1.qkv.weight"].shape == (192, 64, 1)


def _create(num_heads=0, num_head_channels=0, use_freq=0, mult=(1, 2), mc=32, groups=8):
    from cwdm_hip import _lib
    cfg = _lib.UNetConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels, cfg.num_res_blocks, cfg.num_levels = 32, mc, 8, 2, len(mult)
    for i, v in enumerate(mult):
        cfg.channel_mult[i] = v
    cfg.num_groups, cfg.dtype, cfg.resblock_updown, cfg.use_freq = groups, _lib.CWDM_F32, 1, use_freq
    cfg.bottleneck_attention, cfg.num_heads, cfg.num_head_channels = 1, num_heads, num_head_channels
    h = ctypes.c_void_p()
    rc = _lib.lib().cwdm_unet_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().cwdm_last_error() if rc else b""
    if h.value:
        _lib.lib().cwdm_unet_destroy(h)
    return rc, msg


def test_create_refusals():
    from cwdm_hip import _lib
    assert _create()[0] == 0                              # num_heads 0 reads as 1: ch = C = 64
    assert _create(num_heads=4)[0] == 0                   # ch = 16
    rc, msg = _create(num_head_channels=24, mult=(1, 3))  # C = 96 = 4 * 24: ch = 24 is no multiple of 16
    assert rc == _lib.E_UNSUPPORTED and b"multiple of 16" in msg
    rc, msg = _create(num_heads=3)                        # C % heads != 0
    assert rc == _lib.E_UNSUPPORTED and b"not divisible" in msg
    rc, msg = _create(num_head_channels=48)               # 64 % 48 != 0
    assert rc == _lib.E_UNSUPPORTED and b"not divisible" in msg
    rc, msg = _create(mult=(1, 8), mc=64, groups=32)      # one head of 512 channels
    assert rc == _lib.E_UNSUPPORTED and b"256" in msg
    assert _create(mult=(1, 8), mc=64, groups=32, num_heads=2)[0] == 0
    rc, msg = _create(use_freq=1)
    assert rc == _lib.E_UNSUPPORTED and b"use_freq" in msg


@pytest.mark.parametrize("cfg", [TINY, PROD], ids=["c1", "production"])
def test_segments_cover_the_flat_gradient_once(cfg):
    plan = _plan(cfg, "bf16", bottleneck_attention=True, num_heads=4)
    base = _plan(cfg, "bf16")
    assert plan.num_segments == base.num_segments + 1
    cover = torch.zeros(plan.grad_numel, dtype=torch.int32)
    ranges = [plan.segment_range(s) for s in range(plan.num_segments)]
    for off, n in ranges:
        cover[off:off + n] += 1
    assert bool((cover == 1).all())
    # one segment is exactly the block's parameters
    C = cfg["channel_mult"][-1] * cfg["model_channels"]
    names = [n for n, _ in plan.param_specs]
    offs = [0]
    for _, s in plan.param_specs:
        offs.append(offs[-1] + math.prod(s))
    first = names.index("middle_block.1.norm.weight")
    assert (offs[first], 4 * C * C + 6 * C) in ranges
    assert plan.train_workspace_bytes(1, 32, 32, 32) > plan.workspace_bytes(1, 32, 32, 32) > \
        base.workspace_bytes(1, 32, 32, 32)
    assert plan.grad_workspace_bytes(1, 32, 32, 32) > base.grad_workspace_bytes(1, 32, 32, 32)


@pytest.mark.parametrize("grid", [(1, 128, 128, 128), (2, 112, 112, 80), (1, 16, 16, 32)])
def test_flops_delta_is_the_closed_form(grid):
    B, D, H, W = grid
    C = 256
    T = (D // 16) * (H // 16) * (W // 16)
    for heads in (1, 4):
        got = _plan(PROD, "bf16", bottleneck_attention=True, num_heads=heads).flops(*grid) - \
            _plan(PROD, "bf16").flops(*grid)
        # 2 MAC each: qkv (T x 3C x C), proj (T x C x C), q k^T and P v (T x T x C each, over all heads)
        want = 2.0 * B * (T * 3 * C * C + T * C * C + 2 * T * T * C)
        assert abs(got - want) <= 1e-9 * want, (heads, got, want)


def test_conv_routes_of_existing_descs_are_unchanged():
    """The attention unit adds no conv route: the documented lone-conv routes hold (the rules of
    test_conv_route_cpu, asked through the same helper), and a plan's convs are sized as before --
    the attention plan's workspace is the plain plan's plus exactly its own two regions."""
    import test_conv_route_cpu as rc
    from cwdm_hip import _lib
    _lib.lib()
    L = rc.rec.load(_lib.LIB_PATH)
    r = rc.route(L, edge=128, cin=64, cout=64, gn=1)
    assert (r["kernel"], r["gn"], r["ksplit"], r["aa_units"]) == (rc.V5, rc.GN_APPLY, 1, 0), r
    r = rc.route(L, edge=32, cin=128, cout=128)
    assert (r["kernel"], r["gn"], r["ksplit"]) == (rc.V4, rc.GN_NONE, 1), r
    r = rc.route(L, edge=16, cin=256, cout=256)
    assert (r["kernel"], r["ksplit"]) == (rc.SMALL_GRID, 1), r
    r = rc.route(L, edge=8, cin=256, cout=256)
    assert r["kernel"] == rc.SMALL_GRID and r["ksplit"] > 1, r
    assert rc.route(L, edge=32, cin=128, cout=128, gn=1, ws=0)["kernel"] == rc.BRICK

    def up(n):
        return (n + 255) // 256 * 256
    for dtype, es in (("bf16", 2), ("fp32", 4)):
        a, b = _plan(PROD, dtype, bottleneck_attention=True), _plan(PROD, dtype)
        B, T, C = 1, 8 * 8 * 8, 256
        # + the block's output tensor and its statistics rows (one per 16 voxels), the norm's scale / shift and
        # mean / rstd, qkv and a
        extra = up(B * T * C * es) + up(B * (T // 16) * C * 8) + up(B * C * 8) + up(B * 32 * 8) + \
            up(B * T * 3 * C * es) + up(B * T * C * es)
        assert a.workspace_bytes(B, 128, 128, 128) - b.workspace_bytes(B, 128, 128, 128) == extra
