"""End-to-end parity on the GPU: native UNetModel forward, the sampling loop
and training_losses against the oracle (fp32 within 1e-3 rel)."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import cases, diffusion as od, haar, unet as ou

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _product_model(cfg, groups, params, dtype):
    from guided_diffusion.unet import UNetModel
    m = UNetModel(image_size=2 * 16, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resblock_updown=True, bottleneck_attention=False,
                  resample_2d=False, num_groups=groups, compute_dtype=dtype)
    m.load_state_dict(params)
    return m.to(DEV)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 6e-2), ("fp16", 1e-2)])
def test_tiny_unet_forward_and_trace(dtype, tol):
    cfg, G = cases.C1_CFG, cases.C1_GROUPS
    P = ou.random_params(seed=1, **cfg)
    model = _product_model(cfg, G, P, dtype)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 16, 16, 16, generator=g)
    t = torch.tensor([3, 917])
    trace = []
    ref = ou.unet_forward(P, x, t, num_groups=G, trace=trace, **cfg)
    with torch.no_grad():  # inference path: activations land in the plan's own workspace
        out = model(x.to(DEV), t.to(DEV))
    assert out.shape == ref.shape
    assert rel_err(out, ref) < tol
    # block-by-block (NDHWC workspace views)
    ws = model.plan.workspace(2, 16, 16, 16, DEV)
    got = model.plan.trace_tensors(ws, 2, 16, 16, 16)
    assert len(got) == len(trace)
    for i, (gt, rf) in enumerate(zip(got, trace)):
        if gt is None:
            continue
        assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i


@pytest.mark.parametrize("grid", [(16, 16, 16), (32, 16, 48)])
def test_production_unet_forward_fp32(grid):
    P = ou.random_params(seed=11)
    model = _product_model(dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2,
                                channel_mult=(1, 2, 2, 4, 4)), 32, P, "fp32")
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 32, *grid, generator=g)
    t = torch.tensor([500])
    ref = ou.unet_forward(P, x, t)
    out = model(x.to(DEV), t.to(DEV))
    assert rel_err(out, ref) < 1e-3


@pytest.mark.parametrize("grid", [(16, 16, 32), (32, 32, 64)])
def test_production_unet_forward_dma_kernel(grid):
    """Every conv the shape allows on the DMA-staged kernel (path 2), including
    the fused GroupNorm + 1x1-skip pass of the skip ResBlocks, vs the oracle
    (fp32, 1e-3); then the bf16 model on the same path within 6e-2 of it."""
    from cwdm_hip._lib import lib
    P = ou.random_params(seed=13)
    cfg = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 32, *grid, generator=g)
    t = torch.tensor([700])
    prev = lib().cwdm_conv3d_set_path(2)
    try:
        m32 = _product_model(cfg, 32, P, "fp32")
        with torch.no_grad():
            out = m32(x.to(DEV), t.to(DEV))
            # the oracle at every grid, including 32x32x64 (R0 and R1 on the DMA kernel, the
            # 16^3-class levels on the small-grid kernel)
            assert rel_err(out, ou.unet_forward(P, x, t)) < 1e-3
            for half, tol in (("bf16", 6e-2), ("fp16", 1e-2)):
                m16 = _product_model(cfg, 32, P, half)
                assert rel_err(m16(x.to(DEV), t.to(DEV)), out) < tol, half
    finally:
        lib().cwdm_conv3d_set_path(prev)


@pytest.mark.parametrize("grid", [(16, 16, 32), (32, 32, 64)])
def test_production_unet_accurate_fast_mode_vs_oracle(grid):
    """compute_dtype "fp32x" (fp32 storage, every 3x3x3 conv's MFMAs on bf16 hi/lo
    splits: conv3d_v5s_kernel on the wide grids, the K-expanded small-grid kernel
    below them, the K-expanded head): the 81.5 M production U-Net within the north
    star's 1e-3 of the oracle, and within 4e-5 of the exact-fp32 plan (the three
    products drop lo.lo, ~2^-16 of each product: 2.04e-5 measured at 32x32x64)."""
    P = ou.random_params(seed=14)
    cfg = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 32, *grid, generator=g)
    t = torch.tensor([300])
    with torch.no_grad():
        mx = _product_model(cfg, 32, P, "fp32x")
        out = mx(x.to(DEV), t.to(DEV))
        ref = ou.unet_forward(P, x, t)
        assert rel_err(out, ref) < 1e-3
        m32 = _product_model(cfg, 32, P, "fp32")
        assert rel_err(out, m32(x.to(DEV), t.to(DEV))) < 4e-5


@pytest.mark.parametrize("half,tol", [("bf16", 6e-2), ("fp16", 1e-2)])
def test_production_unet_half_close_to_fp32(half, tol):
    P = ou.random_params(seed=12)
    cfg = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
    m32 = _product_model(cfg, 32, P, "fp32")
    m16 = _product_model(cfg, 32, P, half)
    x = torch.randn(1, 32, 32, 32, 32, device=DEV)
    t = torch.tensor([250], device=DEV)
    a, b = m32(x, t), m16(x, t)
    assert rel_err(b, a) < tol


def _c1_product(dtype):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         diffusion_steps=2, sample_schedule="sampled")
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    diffusion.mode = "i2i"
    return model, diffusion


def test_c1_sampling_loop_matches_golden_fp32():
    vols, cond, x_T, noises, params = cases.c1_inputs()
    model, diffusion = _c1_product("fp32")
    model.load_state_dict(params)
    model.to(DEV)
    it = iter([n.to(DEV) for n in noises])
    sample = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), clip_denoised=True,
                                     progress=False, noise_fn=lambda x: next(it))
    gold = np.load(os.path.join(GOLDEN, "c1_sampling.npz"), allow_pickle=False)
    assert rel_err(sample, torch.from_numpy(gold["sample"])) < 1e-3
    from DWT_IDWT.DWT_IDWT_layer import IDWT_3D
    B, _, D, H, W = sample.shape
    img = IDWT_3D("haar")(*[sample[:, i].view(B, 1, D, H, W) * (3.0 if i == 0 else 1.0) for i in range(8)])
    img = img.clamp(0, 1)
    img[vols["t1c"].to(DEV) == 0] = 0
    assert rel_err(img, torch.from_numpy(gold["image"])) < 1e-3


def test_generic_model_path_equals_native_loop():
    """A plain callable model (reference seam) and the native resident loop agree."""
    vols, cond, x_T, noises, params = cases.c1_inputs(32)
    model, diffusion = _c1_product("fp32")
    model.load_state_dict(params)
    model.to(DEV)

    def run(m):
        it = iter([n.to(DEV) for n in noises])
        return diffusion.p_sample_loop(m, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), progress=False,
                                       noise_fn=lambda x: next(it), device=DEV)

    native = run(model)
    generic = run(lambda x, t: model(x, t))
    assert rel_err(generic, native) < 1e-6


def test_respaced_ddim50_tables_and_loop_runs():
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         timestep_respacing="ddim50")
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys})
    model.load_state_dict(ou.random_params(seed=1, **cases.C1_CFG))
    model.to(DEV)
    assert diffusion.num_timesteps == 50 and diffusion.timestep_map[-1] == 980
    cond = torch.rand(1, 24, 16, 16, 16, device=DEV)
    out = diffusion.p_sample_loop(model, (1, 8, 16, 16, 16), cond=cond, progress=False)
    assert torch.isfinite(out).all()


def _c1_respaced(respacing, dtype="fp32", steps=1000, schedule="direct"):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         diffusion_steps=steps, sample_schedule=schedule,
                                         timestep_respacing=respacing)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    return model, diffusion


def _c1_loop_inputs(n=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    vols = cases.data.brats_batch(2 * n, seed=seed, batch=1)
    cond = torch.cat([haar.dwt_cat(vols[k]) for k in ("t1c", "t2w", "t2f")], dim=1)
    x_T = torch.randn(1, 8, n, n, n, generator=g)
    return cond, x_T, g


@pytest.mark.parametrize("respacing", ["ddim10", "25,15"])
def test_respaced_ancestral_loop_vs_oracle(respacing):
    """SpacedDiffusion's p_sample_loop (native resident loop, fp32) over
    respaced tables vs oracle.p_sample_loop on Tables(use_timesteps=...),
    same injected noise: 1e-3 (respace.py:65-132, gaussian_diffusion.py:668-719)."""
    P = ou.random_params(seed=1, **cases.C1_CFG)
    model, diffusion = _c1_respaced(respacing)
    model.load_state_dict(P)
    model.to(DEV)
    cond, x_T, g = _c1_loop_inputs()
    T = diffusion.num_timesteps
    noises = [torch.randn(x_T.shape, generator=g) for _ in range(T)]
    it = iter([z.to(DEV) for z in noises])
    out = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), progress=False,
                                  noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"),
                    use_timesteps=od.space_timesteps(1000, respacing))
    assert tab.timestep_map == diffusion.timestep_map
    ref = od.p_sample_loop(tab, ou.OracleUNet(P, num_groups=8, **cases.C1_CFG), x_T, cond, noises)
    assert rel_err(out, ref) < 1e-3


@pytest.mark.parametrize("eta", [0.0, 0.3])
def test_ddim_loop_vs_oracle(eta):
    """i2i DDIM (config 4's sampler; the reference raises for i2i, so the
    oracle restates ddim_sample by spec): the native HIP-graph-captured DDIM
    loop over ddim10 tables vs oracle.ddim_sample_loop, fp32, 1e-3; the eager
    loop is bit-identical to the graph replay."""
    P = ou.random_params(seed=1, **cases.C1_CFG)
    model, diffusion = _c1_respaced("ddim10")
    model.load_state_dict(P)
    model.to(DEV)
    cond, x_T, _ = _c1_loop_inputs(seed=7)
    x_dev = x_T.to(DEV)
    diffusion.use_hip_graph = True
    out = diffusion.ddim_sample_loop(model, x_T.shape, noise=x_dev, cond=cond.to(DEV), eta=eta)
    diffusion.use_hip_graph = False
    eager = diffusion.ddim_sample_loop(model, x_T.shape, noise=x_dev, cond=cond.to(DEV), eta=eta)
    diffusion.use_hip_graph = True
    assert torch.equal(out, eager)
    assert torch.equal(x_dev.cpu(), x_T)    # the caller's x_T is never written
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"), use_timesteps=od.space_timesteps(1000, "ddim10"))
    ref = od.ddim_sample_loop(tab, ou.OracleUNet(P, num_groups=8, **cases.C1_CFG), x_T, cond, eta=eta)
    assert rel_err(out, ref) < 1e-3
    # the progressive generator yields every step, and the generic-model seam agrees
    steps = list(diffusion.ddim_sample_loop_progressive(model, x_T.shape, noise=x_dev, cond=cond.to(DEV), eta=eta))
    assert len(steps) == 10 and torch.equal(steps[-1]["sample"], out)
    generic = diffusion.ddim_sample_loop(lambda x, t: model(x, t), x_T.shape, noise=x_dev, cond=cond.to(DEV),
                                         eta=eta, device=DEV)
    assert rel_err(generic, out) < 1e-6


def test_graph_loop_leaves_caller_noise_unchanged():
    """p_sample_loop with HIP-graph replay must not write into the x_T tensor
    it was given (the first step reads it; the graphs ping-pong their own)."""
    P = ou.random_params(seed=1, **cases.C1_CFG)
    model, diffusion = _c1_respaced("ddim10")
    model.load_state_dict(P)
    model.to(DEV)
    cond, x_T, _ = _c1_loop_inputs()
    x_dev = x_T.to(DEV)
    diffusion.use_hip_graph = True
    out = diffusion.p_sample_loop(model, x_T.shape, noise=x_dev, cond=cond.to(DEV), progress=False)
    assert torch.equal(x_dev.cpu(), x_T)
    assert out.data_ptr() != x_dev.data_ptr() and torch.isfinite(out).all()


@pytest.mark.parametrize("respacing,dtype,noise_src", [("", "fp32", "philox"), ("ddim10", "bf16", "philox"),
                                                        ("ddim10", "fp16", "torch")])
def test_hip_graph_loop_equals_eager_loop(respacing, dtype, noise_src):
    """The graph-captured sampling step (one capture, replayed per timestep,
    noise drawn in the sampler kernel by Philox with the device timestep in
    its counter, or from torch's graph-safe generator) reproduces the eager
    loop with the same seed, for the full and a respaced schedule (a 50-step
    direct schedule: beta_T = 0.4, every table column finite)."""
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         diffusion_steps=50, sample_schedule="direct",
                                         timestep_respacing=respacing)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    model.load_state_dict(ou.random_params(seed=1, **cases.C1_CFG))
    model.to(DEV)
    g = torch.Generator().manual_seed(5)
    cond = torch.rand(1, 24, 16, 16, 16, generator=g).to(DEV)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g).to(DEV)

    diffusion.native_noise = noise_src

    def run(graph):
        diffusion.use_hip_graph = graph
        torch.manual_seed(11)
        outs = [o["sample"] for o in diffusion.p_sample_loop_progressive(model, x_T.shape, noise=x_T, cond=cond,
                                                                        progress=False)]
        return outs

    eager, graph = run(False), run(True)
    diffusion.use_hip_graph = False
    assert len(eager) == len(graph) == diffusion.num_timesteps
    for a, b in zip(eager, graph):
        assert torch.equal(a, b), rel_err(b, a)


def test_training_losses_forward_vs_oracle():
    from guided_diffusion import script_util
    vols = {k: v.to(DEV) for k, v in cases.data.brats_batch(32, seed=4, batch=2).items()}
    P = ou.random_params(seed=1, **cases.C1_CFG)
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys})
    model.load_state_dict(P)
    model.to(DEV)
    t = torch.tensor([5, 700], device=DEV)
    noise = torch.randn(2, 1, 32, 32, 32, device=DEV)
    with torch.no_grad():
        terms, out, out_idwt = diffusion.training_losses(model, vols, t, mode="i2i", contr="t2w", noise=noise)
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    om = ou.OracleUNet(P, num_groups=8, **cases.C1_CFG)
    rterms, rout, ridwt = od.training_losses(tab, om, {k: v.cpu() for k, v in vols.items()}, t.cpu(), noise.cpu(),
                                             contr="t2w")
    assert rel_err(out, rout) < 1e-3
    assert rel_err(out_idwt, ridwt) < 1e-3
    assert rel_err(terms["mse_wav"], rterms["mse_wav"]) < 1e-3


S2_CFGS = [(dict(in_channels=32, model_channels=32, out_channels=8, num_res_blocks=1, channel_mult=(1, 2)), 8,
            (16, 16, 16)),
           (dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4)),
            32, (16, 32, 32))]


@pytest.mark.parametrize("k", [0, 1], ids=["tiny", "runsh"])
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 6e-2), ("fp16", 1e-2)])
def test_unet_resblock_updown_false_forward_vs_oracle(k, dtype, tol):
    """resblock_updown=False: Downsample(use_conv=True) = stride-2 Conv3d (run as
    a stride-1 conv over the space-to-depth input) and Upsample(use_conv=True) =
    nearest x2 + Conv3d (unet.py:40-100), whole U-Net vs the oracle."""
    from guided_diffusion.unet import UNetModel
    cfg, G, grid = S2_CFGS[k]
    P = ou.random_params(seed=17, resblock_updown=False, **cfg)
    m = UNetModel(image_size=2 * grid[0], in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resblock_updown=False, bottleneck_attention=False,
                  resample_2d=False, num_groups=G, compute_dtype=dtype)
    m.load_state_dict(P)
    m.to(DEV)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(1, 32, *grid, generator=g)
    t = torch.tensor([321])
    trace = []
    ref = ou.unet_forward(P, x, t, num_groups=G, trace=trace, resblock_updown=False, **cfg)
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV))
    assert rel_err(out, ref) < tol
    ws = m.plan.workspace(1, *grid, DEV)
    got = m.plan.trace_tensors(ws, 1, *grid)
    assert len(got) == len(trace)
    for i, (gt, rf) in enumerate(zip(got, trace)):
        if gt is not None:
            assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_fats_sampling_loop_vs_oracle(sampler):
    """FATS per-band schedules through the native, HIP-graph-captured loop
    (respaced ddim10): vs the oracle loop on per-band tables, fp32, 1e-3."""
    from guided_diffusion import script_util
    shift = [-1.2, 0.4, 0.5, 0.9, 0.3, 0.8, 1.0, 1.6]
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         timestep_respacing="ddim10")
    keys = script_util.model_and_diffusion_defaults().keys()
    model, _ = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype="fp32")
    diffusion = script_util.create_gaussian_diffusion(steps=1000, predict_xstart=True, mode="i2i",
                                                      timestep_respacing="ddim10", band_log_snr_shift=shift)
    P = ou.random_params(seed=1, **cases.C1_CFG)
    model.load_state_dict(P)
    model.to(DEV)
    cond, x_T, g = _c1_loop_inputs(seed=11)
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"), use_timesteps=od.space_timesteps(1000, "ddim10"),
                    band_shift=shift)
    om = ou.OracleUNet(P, num_groups=8, **cases.C1_CFG)
    if sampler == "ddim":
        out = diffusion.ddim_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV))
        ref = od.ddim_sample_loop(tab, om, x_T, cond)
    else:
        noises = [torch.randn(x_T.shape, generator=g) for _ in range(10)]
        it = iter([z.to(DEV) for z in noises])
        out = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), progress=False,
                                      noise_fn=lambda x: next(it))
        ref = od.p_sample_loop(tab, om, x_T, cond, noises)
    assert rel_err(out, ref) < 1e-3


WU_CFGS = {
    "tiny": (dict(in_channels=32, model_channels=32, out_channels=8, num_res_blocks=2, channel_mult=(1, 2)), 8,
             (16, 16, 16)),
    "three": (dict(in_channels=32, model_channels=32, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2)), 8,
              (32, 16, 24)),
    # script_util's use_freq model at the production topology (mc 64, (1, 2, 2, 4, 4), 90.1M parameters);
    # 32^3 puts the deepest level at 1^3
    "prod": (dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2,
                  channel_mult=(1, 2, 2, 4, 4)), 32, (32, 32, 32)),
}


def _wavunet(k, dtype, seed=21):
    from guided_diffusion import script_util
    from oracle import wunet as ow
    cfg, G, grid = WU_CFGS[k]
    m = script_util.create_model(image_size=128, num_channels=cfg["model_channels"],
                                 num_res_blocks=cfg["num_res_blocks"],
                                 channel_mult=",".join(str(v) for v in cfg["channel_mult"]), attention_resolutions="",
                                 dims=3, num_groups=G, in_channels=cfg["in_channels"],
                                 out_channels=cfg["out_channels"], bottleneck_attention=False, resample_2d=False,
                                 resblock_updown=True, use_freq=True, compute_dtype=dtype)
    P = ow.random_params(seed=seed, **cfg)
    full = dict(P)
    for alias, owner in ow.aliases(**cfg).items():
        for n, v in P.items():
            if n.startswith(owner + "."):
                full[alias + n[len(owner):]] = v
    m.load_state_dict(full)
    return m.to(DEV), P, cfg, G, grid


@pytest.mark.parametrize("k,dtype,tol", [("tiny", "fp32", 1e-3), ("three", "fp32", 1e-3), ("prod", "fp32", 1e-3),
                                         ("tiny", "bf16", 6e-2), ("tiny", "fp16", 1e-2)])
def test_wavunet_forward_vs_oracle(k, dtype, tol):
    """WavUNetModel (use_freq=True, wunet.py:754-795) forward on the native plan:
    DWT/IDWT ResBlocks, wavelet input pyramid, the reused decoder ResBlock
    (two state_dict names, run twice) -- output and every block's activation
    vs the oracle restatement."""
    from oracle import wunet as ow
    m, P, cfg, G, grid = _wavunet(k, dtype)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 32, *grid, generator=g)
    t = torch.tensor([37, 801])
    trace = []
    ref = ow.wunet_forward(P, x, t, num_groups=G, trace=trace, **cfg)
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV))
    assert rel_err(out, ref) < tol
    got = m.plan.trace_tensors(m.plan.workspace(2, *grid, DEV), 2, *grid)
    assert len(got) == len(trace)
    for i, (gt, rf) in enumerate(zip(got, trace)):
        if gt is not None:
            assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i


@pytest.mark.parametrize("k,dtype,tol", [("tiny", "fp32", 1e-3), ("three", "fp32", 1e-3), ("prod", "fp32", 1e-3),
                                         ("tiny", "bf16", 8e-2), ("tiny", "fp16", 2e-2)])
def test_wavunet_backward_vs_oracle_autograd(k, dtype, tol):
    """f4 training: WavUNetModel under autograd (model(x, t) with gradients, the
    reference's API) runs the plan's backward -- DWT ResBlocks (adjoint: IDWT of
    the LLL and skip-band gradients), IDWT ResBlocks (adjoint: DWT, the skip
    bands' gradient from both users), the wavelet-pyramid convs, the reused
    decoder ResBlocks (both uses summed into the owner's parameters) -- and
    every parameter gradient matches the oracle's autograd (rel L2)."""
    from oracle import wunet as ow
    m, P, cfg, G, grid = _wavunet(k, dtype)
    g = torch.Generator().manual_seed(23)
    B = 1 if k == "prod" else 2
    x = torch.randn(B, 32, *grid, generator=g)
    t = torch.tensor([37, 801][:B])
    R = torch.randn(B, 8, *grid, generator=g)
    out = m(x.to(DEV), t.to(DEV))
    (out * R.to(DEV)).sum().backward()
    Pr = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    ref = ow.wunet_forward(Pr, x, t, num_groups=G, **cfg)
    (ref * R).sum().backward()
    assert rel_err(out.detach(), ref.detach()) < tol
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert set(grads) == set(P)          # owners only: the reused blocks' second names alias them
    worst = {n: float((grads[n].double().cpu() - Pr[n].grad.double()).norm() /
                      Pr[n].grad.double().norm().clamp_min(1e-30)) for n in P}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(k, dtype, "worst gradients", top)
    assert top[0][1] < tol, top
    # the reused blocks' parameters got both contributions: without the second use they would differ
    for alias, owner in ow.aliases(**cfg).items():
        assert worst[owner + ".in_layers.2.weight"] < tol


def test_wavunet_trainloop_step(tmp_path, monkeypatch):
    """TrainLoop accepts the use_freq model (script_util.create_model(use_freq=True)):
    run_step with the native backward and the fused AdamW changes the weights
    and keeps them finite."""
    from guided_diffusion import dist_util, script_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    m, _, cfg, G, grid = _wavunet("tiny", "fp32")
    diffusion = script_util.create_gaussian_diffusion(steps=1000, predict_xstart=True, mode="i2i")
    batch = {k: v.to(DEV) for k, v in data_batch(2 * grid[0]).items()}
    loop = train_util.TrainLoop(model=m, diffusion=diffusion, data=[batch], batch_size=1, in_channels=32,
                                image_size=2 * grid[0], microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=10,
                                contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0, mode="i2i",
                                diffusion_steps=1000)
    p0 = m.flat_params.detach().clone()
    for _ in range(2):
        loss, _, _ = loop.run_step(batch, {})
    assert torch.isfinite(loss)
    assert not torch.equal(p0, m.flat_params) and torch.isfinite(m.flat_params).all()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def data_batch(n):
    from oracle import data
    return data.brats_batch(n, seed=5, batch=1)


def test_fast_ddpm_sampled10_production_loop_vs_oracle():
    """The production inference path (infer_pod.yml: brats_*_BEST_sampled_10.pt,
    diffusion_steps=10, sample_schedule='sampled'; gaussian_diffusion.py:45-58):
    the native HIP-graph loop over the 10-step Fast-DDPM schedule vs the
    oracle loop on the same tables and noise, fp32, 1e-3."""
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         diffusion_steps=10, sample_schedule="sampled")
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype="fp32")
    diffusion.mode = "i2i"
    P = ou.random_params(seed=1, **cases.C1_CFG)
    model.load_state_dict(P)
    model.to(DEV)
    assert diffusion.use_hip_graph
    cond, x_T, g = _c1_loop_inputs(seed=14)
    noises = [torch.randn(x_T.shape, generator=g) for _ in range(10)]
    it = iter([z.to(DEV) for z in noises])
    out = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), progress=False,
                                  noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 10, "sampled"))
    ref = od.p_sample_loop(tab, ou.OracleUNet(P, num_groups=8, **cases.C1_CFG), x_T, cond, noises)
    assert rel_err(out, ref) < 1e-3


def _lone_conv_with_stats(src, packed, bias):
    """A lone 64 -> 64 3x3x3 bf16 cwdm_conv3d_forward with statistics on src (1, D, H, W, 64);
    returns (out, statistics rows)."""
    import ctypes
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    _, D, H, W, C = src.shape
    out = torch.empty(1, D, H, W, 64, device=DEV, dtype=torch.bfloat16)
    st = torch.zeros(1, L.cwdm_conv3d_parts(_lib.CWDM_BF16, D, H, W, 64), 64, 2, device=DEV)
    d = _lib.ConvDesc()
    d.dtype, d.B, d.D, d.H, d.W, d.cout = _lib.CWDM_BF16, 1, D, H, W, 64
    d.a0, d.a_c0, d.a_w = src.data_ptr(), C, packed.data_ptr()
    d.bias, d.res_mode = bias.data_ptr(), -1
    d.out, d.out_dtype, d.stats = out.data_ptr(), _lib.CWDM_BF16, st.data_ptr()
    nws = L.cwdm_conv3d_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    d.workspace, d.ws_bytes = ws.data_ptr(), nws
    check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
    torch.cuda.synchronize()
    return out, st


def test_plan_leaves_lone_convs_and_the_stats_wg_hook_alone():
    """A plan forward + backward hands its convs their context explicitly, so nothing of it stays
    behind on the calling thread: a lone conv on the warp-specialised kernel (W = its minimum width,
    one tile per CU) gives the same output and statistics before and after, and a
    cwdm_debug_stats_wg(1) set before the plan runs is still set afterwards, with -1 reporting the
    lone conv's own rows."""
    import ctypes
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    k = math.isqrt(ncu - 1) + 1                      # k * k >= ncu tiles of 32 x 4 x 4 (CWDM_V5_MIN_TPC = 1)
    g = torch.Generator().manual_seed(61)
    src = torch.randn(1, 4 * k, 4 * k, 24, 64, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(64, 64, 3, 3, 3, generator=g) / math.sqrt(27 * 64)).to(DEV)
    bias = (0.1 * torch.randn(64, generator=g)).to(DEV)
    packed = torch.empty(L.cwdm_conv3d_packed_bytes(64, 64, 3, _lib.CWDM_BF16), dtype=torch.uint8, device=DEV)
    check(L.cwdm_conv3d_pack(ctypes.c_void_p(w.data_ptr()), 64, 64, 3, _lib.CWDM_BF16,
                             ctypes.c_void_p(packed.data_ptr()), None))
    cfg, G = cases.C1_CFG, cases.C1_GROUPS
    model = _product_model(cfg, G, ou.random_params(seed=1, **cfg), "bf16")
    x = torch.randn(1, 32, 16, 16, 16, generator=g).to(DEV)
    t = torch.tensor([300], device=DEV)

    def plan_step():
        model.zero_grad(set_to_none=True)
        model(x, t).float().square().sum().backward()
        torch.cuda.synchronize()

    for wg in (0, 1):
        prev = L.cwdm_debug_stats_wg(wg)
        try:
            out0, st0 = _lone_conv_with_stats(src, packed, bias)
            rows0 = L.cwdm_debug_stats_wg(-1)
            assert rows0 == (min(ncu, k * k) if wg else 0)   # one row per workgroup, one workgroup per CU
            assert bool(st0[0, rows0:].any()) == (not wg)    # (per workgroup: the rows past the grid untouched)
            plan_step()
            assert L.cwdm_debug_stats_wg(wg) == wg           # still set (and the rows count starts over)
            out1, st1 = _lone_conv_with_stats(src, packed, bias)
            assert L.cwdm_debug_stats_wg(-1) == rows0
            assert torch.equal(out1, out0) and torch.equal(st1, st0)
        finally:
            L.cwdm_debug_stats_wg(prev)
