"""Class conditioning (num_classes, label_emb, y) without a GPU: the state_dict
contract, the plan's refusals and segment ranges, the factory, and forward's
``y`` assertion (raised before any device work)."""
import ctypes
import math

import pytest
import torch

import class_cond_oracle as cco
from oracle import cases, unet as ou

PROD_CFG = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
CONFIGS = [(cases.C1_CFG, cases.C1_GROUPS, 4), (PROD_CFG, 32, 2)]
IDS = ["c1", "production"]


def _model(cfg, groups, num_classes, **kw):
    from guided_diffusion.unet import UNetModel
    return UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                     out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                     channel_mult=cfg["channel_mult"], dims=3, resblock_updown=True, bottleneck_attention=False,
                     resample_2d=False, num_groups=groups, num_classes=num_classes, **kw)


@pytest.mark.parametrize("cfg,groups,n", CONFIGS, ids=IDS)
def test_state_dict_names_shapes_order(cfg, groups, n):
    """label_emb.weight (n, 4 model_channels) sits right after time_embed.2.bias and before
    input_blocks.0.0.weight, the reference's registration order; everything else is the plain model's."""
    m = _model(cfg, groups, n)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    mc = cfg["model_channels"]
    E = 4 * mc
    head = [("time_embed.0.weight", (E, mc)), ("time_embed.0.bias", (E,)),
            ("time_embed.2.weight", (E, E)), ("time_embed.2.bias", (E,)),
            ("label_emb.weight", (n, E)),
            ("input_blocks.0.0.weight", (mc, cfg["in_channels"], 3, 3, 3)), ("input_blocks.0.0.bias", (mc,))]
    assert got[:len(head)] == head
    assert got == [(k, tuple(s)) for k, s in cco.param_shapes(n, **cfg)]
    plain = [(k, tuple(s)) for k, s in ou.param_shapes(**cfg)]
    assert [e for e in got if e[0] != "label_emb.weight"] == plain
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in got]
    # the flat parameter buffer follows the same order: the table's view starts where time_embed ends
    off = sum(math.prod(s) for _, s in head[:4])
    assert m.label_emb.weight.data_ptr() == m.flat_params.data_ptr() + 4 * off
    assert m.label_emb.weight.dtype == torch.float32


@pytest.mark.parametrize("cfg,groups,n", CONFIGS, ids=IDS)
def test_parameter_count_grows_by_the_table(cfg, groups, n):
    a, b = _model(cfg, groups, None), _model(cfg, groups, n)
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert count(b) - count(a) == n * 4 * cfg["model_channels"]
    assert b.plan.grad_numel == count(b)
    if cfg is PROD_CFG:
        assert count(a) == 81_511_048


@pytest.mark.parametrize("cfg,groups,n", CONFIGS, ids=IDS)
def test_models_without_classes_keep_their_names_and_sizes(cfg, groups, n):
    m = _model(cfg, groups, None)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in ou.param_shapes(**cfg)]
    assert m.num_classes is None and m.plan.num_classes == 0
    # the table is packed too: the class-conditional plan's packed weights grow, the plain plan's do not move
    from cwdm_hip.unet_runtime import UNetPlan
    args = (cfg["in_channels"], cfg["model_channels"], cfg["out_channels"], cfg["num_res_blocks"],
            cfg["channel_mult"], groups, "bf16")
    p0, p00, pn = UNetPlan(*args), UNetPlan(*args, num_classes=0), UNetPlan(*args, num_classes=n)
    assert p0.param_specs == p00.param_specs and p0.packed_bytes == p00.packed_bytes
    assert p0.workspace_bytes(1, 16, 16, 16) == pn.workspace_bytes(1, 16, 16, 16)
    assert p0.grad_workspace_bytes(1, 16, 16, 16) == pn.grad_workspace_bytes(1, 16, 16, 16)
    assert pn.packed_bytes >= p0.packed_bytes + n * 4 * cfg["model_channels"] * 4
    assert pn.num_segments == p0.num_segments


def test_label_emb_default_init_is_standard_normal():
    torch.manual_seed(0)
    m = _model(PROD_CFG, 32, 64)
    w = m.label_emb.weight.detach()
    assert w.shape == (64, 256)
    assert abs(float(w.mean())) < 0.05 and abs(float(w.std()) - 1.0) < 0.05
    assert float(w.abs().max()) > 2.5     # N(0, 1), not Linear's bounded uniform


def test_plan_refusals():
    from cwdm_hip._lib import CwdmError
    from cwdm_hip.unet_runtime import UNetPlan
    with pytest.raises(CwdmError, match="num_classes with use_freq"):
        UNetPlan(32, 32, 8, 2, (1, 2), 8, "fp32", use_freq=True, num_classes=2)
    with pytest.raises(ValueError, match="num_classes must not be negative"):
        UNetPlan(32, 32, 8, 1, (1, 2), 8, "fp32", num_classes=-1)
    UNetPlan(32, 32, 8, 2, (1, 2), 8, "fp32", use_freq=True, num_classes=0)


def test_config_struct_puts_num_classes_behind_dropout():
    from cwdm_hip import _lib
    names = [f[0] for f in _lib.UNetConfig._fields_]
    assert names[-2:] == ["dropout", "num_classes"]
    assert _lib.UNetConfig().num_classes == 0          # a zeroed struct: no class conditioning


def test_labels_on_a_plan_without_classes_are_refused():
    from cwdm_hip import _lib
    from cwdm_hip.unet_runtime import UNetPlan
    plan = UNetPlan(32, 32, 8, 1, (1, 2), 8, "fp32")
    dummy = ctypes.c_void_p(64)      # never dereferenced: the refusal comes first
    assert _lib.lib().cwdm_unet_set_labels(plan._h, dummy) == _lib.E_INVALID
    assert b"no classes" in _lib.lib().cwdm_last_error()
    assert _lib.lib().cwdm_unet_set_labels(None, dummy) == _lib.E_INVALID
    assert _lib.DEV_E_LABEL == 2 and _lib.DEV_E_AA_TIMEOUT == 1


def test_wavunet_still_refuses_classes():
    from guided_diffusion.wunet import WavUNetModel
    with pytest.raises(NotImplementedError, match="class conditioning"):
        WavUNetModel(image_size=32, in_channels=32, model_channels=32, out_channels=8, num_res_blocks=2,
                     attention_resolutions=(), channel_mult=(1, 2), dims=3, resblock_updown=True,
                     bottleneck_attention=False, num_groups=8, num_classes=2)


def test_unet_model_refuses_a_non_positive_class_count():
    with pytest.raises(ValueError, match="num_classes"):
        _model(cases.C1_CFG, cases.C1_GROUPS, 0)


def test_factory_builds_class_cond():
    from guided_diffusion import script_util
    m = script_util.create_model(image_size=32, num_channels=32, num_res_blocks=1, channel_mult="1,2",
                                 attention_resolutions="", dims=3, num_groups=8, in_channels=32, out_channels=8,
                                 bottleneck_attention=False, resblock_updown=True, resample_2d=False,
                                 class_cond=True)
    assert m.num_classes == script_util.NUM_CLASSES == 2
    assert tuple(m.state_dict()["label_emb.weight"].shape) == (2, 128)


@pytest.mark.parametrize("cfg,groups,n", CONFIGS, ids=IDS)
def test_segment_ranges_cover_the_flat_buffer_once(cfg, groups, n):
    """label_emb.weight lies inside the last segment (conv_in + time_embed), whose range stays contiguous."""
    m = _model(cfg, groups, n)
    plan = m.plan
    cover = torch.zeros(plan.grad_numel, dtype=torch.int32)
    for s in range(plan.num_segments):
        off, cnt = plan.segment_range(s)
        cover[off:off + cnt] += 1
    assert bool((cover == 1).all())
    offs, o = {}, 0
    for name, shape in plan.param_specs:
        offs[name] = (o, math.prod(shape))
        o += math.prod(shape)
    off, cnt = plan.segment_range(plan.num_segments - 1)
    lo, ln = offs["label_emb.weight"]
    assert off == 0 and off <= lo and lo + ln <= off + cnt
    assert off + cnt == sum(offs["input_blocks.0.0.bias"])     # time_embed, the table, conv_in: nothing else


def test_forward_asserts_y_iff_class_conditional():
    """The reference's assertion, before any device work (the tensors are host tensors: no kernel could run)."""
    x, t = torch.zeros(2, 32, 16, 16, 16), torch.zeros(2)
    cc = _model(cases.C1_CFG, cases.C1_GROUPS, 4)
    with pytest.raises(AssertionError, match="must specify y if and only if the model is class-conditional"):
        cc(x, t)
    plain = _model(cases.C1_CFG, cases.C1_GROUPS, None)
    with pytest.raises(AssertionError, match="must specify y if and only if the model is class-conditional"):
        plain(x, t, y=torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="ROCm device"):     # and no CPU fallback once the contract holds
        cc(x, t, y=torch.tensor([0, 1]))


def test_state_dict_round_trip_cpu():
    P = cco.random_params(4, seed=3, **cases.C1_CFG)
    m = _model(cases.C1_CFG, cases.C1_GROUPS, 4)
    m.load_state_dict(P)
    sd = m.state_dict()
    assert list(sd) == list(P)
    for k in P:
        assert torch.equal(sd[k], P[k]), k
    plain = _model(cases.C1_CFG, cases.C1_GROUPS, None)
    with pytest.raises(RuntimeError, match="label_emb.weight"):
        plain.load_state_dict(P)
