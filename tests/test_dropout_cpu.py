"""dropout > 0 without a GPU: the constructor contract (no new parameters, the refusals), the plan's sizes with
the field off and on, and the restated mask's kept fraction (plan creation and the oracle need no device)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import dropout_oracle as dro
from conftest import GOLDEN
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
    kw.setdefault("bottleneck_attention", False)
    return (cls or UNetModel)(image_size=64, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                              out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                              attention_resolutions=(), channel_mult=cfg["channel_mult"], dims=3,
                              resblock_updown=True, resample_2d=False, num_groups=_groups(cfg), **kw)


def test_model_builds_with_the_parameters_of_p0():
    m, m0 = _model(TINY, dropout=0.1), _model(TINY)
    assert m.dropout == 0.1 and m0.dropout == 0
    sd, sd0 = m.state_dict(), m0.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in sd0.items()]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(n, tuple(s)) for n, s in ou.param_shapes(**TINY)]
    # a checkpoint of the plain model loads
    P = ou.random_params(seed=5, **TINY)
    m.load_state_dict(P)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in P.items())
    assert m.dropout_seed is None and m.last_dropout_seed is None
    # FiLM and the other topology switches keep their own parameter lists
    f, f0 = _model(TINY, dropout=0.5, use_scale_shift_norm=True), _model(TINY, use_scale_shift_norm=True)
    assert [(k, tuple(v.shape)) for k, v in f.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in f0.state_dict().items()]
    with pytest.raises(RuntimeError, match="ROCm device"):   # no CPU fallback, in training mode either
        m.train()(torch.zeros(1, 32, 16, 16, 16), torch.zeros(1))


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_out_of_range_p_is_a_value_error(p):
    with pytest.raises(ValueError, match="dropout"):
        _model(TINY, dropout=p)
    with pytest.raises(ValueError, match="dropout"):
        _plan(TINY, dropout=p)


def test_wavunet_still_raises():
    from guided_diffusion.wunet import WavUNetModel
    with pytest.raises(NotImplementedError, match="dropout"):
        _model(dict(TINY, num_res_blocks=2), cls=WavUNetModel, use_freq=True, dropout=0.1)


def test_plan_refuses_dropout_with_use_freq():
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
    cfg.use_freq, cfg.dropout = 1, 0.0
    assert create()[0] == 0
    cfg.use_freq, cfg.dropout = 0, 0.25
    assert create()[0] == 0
    cfg.use_freq, cfg.dropout = 1, 0.25
    rc, msg = create()
    assert rc == _lib.E_UNSUPPORTED and b"dropout" in msg and b"use_freq" in msg
    assert _lib.lib().cwdm_unet_set_dropout_seed(None, 1) == _lib.E_INVALID


def _sizes(plan, B, n):
    return {"B": B, "edge": n, "workspace_bytes": plan.workspace_bytes(B, n, n, n),
            "train_workspace_bytes": plan.train_workspace_bytes(B, n, n, n),
            "grad_workspace_bytes": plan.grad_workspace_bytes(B, n, n, n)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_dropout_zero_is_the_plan_without_the_field(dtype):
    """dropout = 0.0 passed explicitly: every size equals the one tests/golden/route_sizes.json recorded from a
    library whose config had no such field, and the default plan's."""
    with open(os.path.join(GOLDEN, "route_sizes.json")) as f:
        golden = json.load(f)
    for name, cfg in (("tiny", TINY), ("production", PROD)):
        rec = [p for p in golden["plans"] if p["name"] == name and p["dtype"] == dtype]
        assert len(rec) == 1
        rec = rec[0]["sizes"] if "sizes" in rec[0] else rec[0]
        off, dflt = _plan(cfg, dtype, dropout=0.0), _plan(cfg, dtype)
        assert off.packed_bytes == rec["packed_bytes"] == dflt.packed_bytes
        assert off.packed_bwd_bytes == max(rec["packed_bwd_bytes"], 1) == dflt.packed_bwd_bytes
        assert len(rec["grids"]) >= 4
        for g in rec["grids"]:
            assert _sizes(off, g["B"], g["edge"]) == g == _sizes(dflt, g["B"], g["edge"])
        assert off.param_specs == dflt.param_specs and off.num_segments == dflt.num_segments
        assert off.flops(1, 32, 32, 32) == dflt.flops(1, 32, 32, 32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dropout_plan_adds_only_the_u_tensors(dtype):
    es = 4 if dtype == "fp32" else 2
    for cfg in (TINY, PROD):
        off, on = _plan(cfg, dtype), _plan(cfg, dtype, dropout=0.3)
        assert on.param_specs == off.param_specs and on.grad_numel == off.grad_numel
        assert on.packed_bytes == off.packed_bytes and on.packed_bwd_bytes == off.packed_bwd_bytes
        assert on.num_segments == off.num_segments
        B, n = 2, 32
        assert on.flops(B, n, n, n) == off.flops(B, n, n, n)
        # one u tensor per ResBlock, of the block's output shape
        u_bytes = 0
        level = 0
        for b in ou.topology(**cfg):
            if b["kind"] != "res":
                continue
            if b["updown"] == "down":
                level += 1
            elif b["updown"] == "up":
                level -= 1
            u_bytes += B * (n >> level) ** 3 * b["cout"] * es
        assert u_bytes > 0
        assert on.workspace_bytes(B, n, n, n) >= off.workspace_bytes(B, n, n, n) + u_bytes
        grow = on.train_workspace_bytes(B, n, n, n) - off.train_workspace_bytes(B, n, n, n)
        if dtype == "fp32":
            assert grow >= u_bytes
        else:
            # a 16-bit training workspace kept the chunk-major SiLU(GN(h1)) of the DMA-staged conv2s for their
            # weight gradients: the dropout plan's conv2 reads u instead (no prologue, nothing kept), so u takes
            # the place of those copies, each exactly its size
            assert 0 <= grow <= u_bytes + 256 * 64
        assert on.train_workspace_bytes(B, n, n, n) >= on.workspace_bytes(B, n, n, n)
        # the u tensors take no gradient buffer (their gradient passes through the dgrad's scratch)
        assert on.grad_workspace_bytes(B, n, n, n) == off.grad_workspace_bytes(B, n, n, n)


def test_model_keeps_one_plan_per_mode():
    m = _model(TINY, dropout=0.3, compute_dtype="bf16")
    off, on = m._plan("bf16"), m._plan("bf16", drop=True)
    assert off is m.plan and on is not off
    assert off.dropout == 0.0 and on.dropout == 0.3
    assert m._plan("bf16", drop=True) is on
    assert m._drops() and not m.eval()._drops() and m.train()._drops()
    assert not _model(TINY).train()._drops()


def test_seed_draw_follows_the_cpu_generator():
    m = _model(TINY, dropout=0.3)
    torch.manual_seed(11)
    a = m._draw_dropout_seed()
    b = m._draw_dropout_seed()
    torch.manual_seed(11)
    assert m._draw_dropout_seed() == a and m.last_dropout_seed == a and a != b and 0 <= a < 2 ** 62
    m.dropout_seed = 2 ** 40 + 7
    assert m._draw_dropout_seed() == 2 ** 40 + 7 == m.last_dropout_seed


def test_script_util_builds_the_dropout_model():
    from guided_diffusion import script_util
    m = script_util.create_model(image_size=128, num_channels=32, num_res_blocks=1, channel_mult="1,2",
                                 attention_resolutions="", dims=3, num_groups=8, in_channels=32, out_channels=8,
                                 bottleneck_attention=False, resblock_updown=True, resample_2d=False, dropout=0.2)
    assert m.dropout == 0.2
    assert [k for k in m.state_dict()] == [n for n, _ in ou.param_shapes(**TINY)]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_oracle_kept_fraction(p):
    """2^20 draws: the kept fraction lies within 4 standard deviations of 1 - p."""
    N = 2 ** 20
    m = dro.keep_mask(seed=0x1234567890ABCDEF, site=3, B=2, V=2 ** 13, C=64, p=p)
    assert m.size == N
    assert abs(m.mean() - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / N)


def test_oracle_mask_is_what_the_header_states():
    """One element by hand, and the mask's independence of B and of the other sites."""
    from oracle import philox
    seed, site, p = (5 << 32) | 9, 2, 0.5
    m = dro.keep_mask(seed, site, 3, 40, 16, p)
    b, v, c = 2, 37, 13
    blk = philox.philox4x32_10(np.array([v, 0, site, (b << 16) | (c >> 2)], np.uint32), np.array([9, 5], np.uint32))
    assert bool(m[b, v, c]) == bool((int(blk[c & 3]) >> 8) >= 2 ** 23)
    assert np.array_equal(dro.keep_mask(seed, site, 2, 40, 16, p), m[:2])
    assert not np.array_equal(dro.keep_mask(seed, site + 1, 3, 40, 16, p), m)
    assert not np.array_equal(dro.keep_mask(seed + 1, site, 3, 40, 16, p), m)
    assert dro.keep_mask(seed, site, 3, 40, 16, 0.0).all()
    assert dro.threshold(0.1) == 1677721 and dro.threshold(0.5) == 2 ** 23
