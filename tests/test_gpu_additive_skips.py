"""additive_skips=True on the GPU: the cwdm_skip_avg kernels through the C ABI,
then the U-Net forward / trace, backward, sampling and training against the
CPU fp32 restatement of the additive forward (tests/additive_oracle.py) and
autograd on it."""
import numpy as np
import pytest
import torch

import additive_oracle as ao
from oracle import cases, diffusion as od

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _same(a, b, what=""):
    a, b = a.cpu(), b.cpu()
    if not torch.equal(a, b):
        d = (a.double() - b.double()).abs()
        raise AssertionError(f"{what}: not bit-exact, max |diff| {float(d.max()):.3e} at {int(d.argmax())}")


# --------------------------------------------------------------------------- the kernels (C ABI)
def _dt(dtype):
    from cwdm_hip import _lib
    return {torch.bfloat16: _lib.CWDM_BF16, torch.float16: _lib.CWDM_F16}.get(dtype, _lib.CWDM_F32)


def _skip_avg(a, b, stats=True):
    """a, b: (B, V, C) device tensors -> out, stats [B][parts][C][2] (or None), parts."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    L = _lib.lib()
    B, V, C = a.shape
    parts = int(L.cwdm_skip_avg_parts(V))
    out = torch.empty_like(a)
    st = torch.full((B, parts, C, 2), float("nan"), dtype=torch.float32, device=DEV) if stats else None
    check(L.cwdm_skip_avg(a.data_ptr(), b.data_ptr(), out.data_ptr(), st.data_ptr() if stats else None, _dt(a.dtype),
                          B, V, C, _stream()), "skip_avg")
    torch.cuda.synchronize()
    return out, st, parts


def _skip_avg_bwd(dy, da, acc_a, db, acc_b):
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    B, V, C = dy.shape
    check(_lib.lib().cwdm_skip_avg_bwd(dy.data_ptr(), da.data_ptr(), acc_a, db.data_ptr(), acc_b, _dt(dy.dtype),
                                       B, V, C, _stream()), "skip_avg_bwd")
    torch.cuda.synchronize()


# (C, grid); the last grid is past the size where a part grows, with a voxel tail
KERNEL_CASES = [(32, (3, 5, 4)), (96, (3, 5, 4)), (32, (8, 8, 6)), (96, (8, 8, 6)), (32, (33, 31, 33))]


def _kernel_inputs(C, grid, dtype, n, seed):
    V = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, V, C, generator=g).to(dtype) for _ in range(n)]


@pytest.mark.parametrize("C,grid", KERNEL_CASES, ids=[f"C{c}-{'x'.join(map(str, g))}" for c, g in KERNEL_CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_skip_avg_bit_exact_with_statistics(C, grid, dtype):
    """out = 0.5 (a + b) in fp32, rounded once: bit-exact; the summed partials vs
    float64 sums of the unrounded value; a second call gives the same bits."""
    a, b = _kernel_inputs(C, grid, dtype, 2, 41)
    out, st, parts = _skip_avg(a.to(DEV), b.to(DEV))
    if grid == KERNEL_CASES[-1][1]:
        assert parts > 1
    v = (a.float() + b.float()) * 0.5
    _same(out, v.to(dtype), "average")
    assert st.shape == (2, parts, C, 2) and torch.isfinite(st).all()   # every row written
    r64 = v.double()
    s = st.double().sum(1).cpu()
    assert torch.allclose(s[..., 0], r64.sum(1), rtol=1e-5, atol=1e-4)
    assert torch.allclose(s[..., 1], (r64 * r64).sum(1), rtol=1e-5, atol=1e-4)
    out2, st2, _ = _skip_avg(a.to(DEV), b.to(DEV))
    _same(st2, st, "statistics of a second call")
    _same(out2, out, "output of a second call")
    out3, none, _ = _skip_avg(a.to(DEV), b.to(DEV), stats=False)   # the statistics are optional
    assert none is None
    _same(out3, out, "output without statistics")


@pytest.mark.parametrize("C,grid", KERNEL_CASES, ids=[f"C{c}-{'x'.join(map(str, g))}" for c, g in KERNEL_CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_skip_avg_bwd_store_and_accumulate(C, grid, dtype):
    """The adjoint: both flags 0 -> da = db = 0.5 dy exactly; a flag set -> that
    destination is old + 0.5 dy computed in the buffer's dtype, the other stored."""
    dy, old_a, old_b = _kernel_inputs(C, grid, dtype, 3, 43)
    half = 0.5 * dy
    for acc_a, acc_b in ((0, 0), (1, 0), (0, 1), (1, 1)):
        da, db = old_a.clone().to(DEV), old_b.clone().to(DEV)
        _skip_avg_bwd(dy.to(DEV), da, acc_a, db, acc_b)
        _same(da, old_a + half if acc_a else half, f"da acc {acc_a}{acc_b}")
        _same(db, old_b + half if acc_b else half, f"db acc {acc_a}{acc_b}")


def test_skip_avg_refuses_bad_channels():
    from cwdm_hip import _lib
    a = torch.zeros(1, 8, 12, device=DEV)
    rc = _lib.lib().cwdm_skip_avg(a.data_ptr(), a.data_ptr(), a.data_ptr(), None, _lib.CWDM_F32, 1, 8, 12, None)
    assert rc == _lib.E_UNSUPPORTED


# --------------------------------------------------------------------------- the tiny U-Net
def _product_model(cfg, groups, params, dtype):
    from guided_diffusion.unet import UNetModel
    m = UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resblock_updown=True, bottleneck_attention=False,
                  resample_2d=False, num_groups=groups, additive_skips=True, compute_dtype=dtype)
    m.load_state_dict(params)
    return m.to(DEV)


def _unet_grads(cfg, G, P, x, t, R, dtype, hook=None):
    model = _product_model(cfg, G, P, dtype)
    model._grad_hook = hook
    out = model(x.to(DEV), t.to(DEV))
    (out * R.to(DEV)).sum().backward()
    return out.detach().cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters()}, model


_TINY = {}


def _tiny_case():
    """x (2, 32, 16, 16, 16), t [3, 917]: the restatement's output, trace and autograd gradients, once."""
    if not _TINY:
        cfg, G = cases.C1_CFG, cases.C1_GROUPS
        P = ao.random_params(seed=1, **cfg)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 32, 16, 16, 16, generator=g)
        t = torch.tensor([3, 917])
        R = torch.randn(2, 8, 16, 16, 16, generator=g)
        trace = []
        with torch.no_grad():
            ref = ao.unet_forward(P, x, t, num_groups=G, trace=trace, **cfg)
        ref_out, ref_grads = ao.grads(cfg, G, P, x, t, R)
        _TINY.update(P=P, x=x, t=t, R=R, ref=ref, trace=trace, ref_out=ref_out, ref_grads=ref_grads)
    return _TINY


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 6e-2), ("fp16", 1e-2)])
def test_tiny_unet_forward_and_trace(dtype, tol):
    c = _tiny_case()
    model = _product_model(cases.C1_CFG, cases.C1_GROUPS, c["P"], dtype)
    with torch.no_grad():
        out = model(c["x"].to(DEV), c["t"].to(DEV))
    assert out.shape == c["ref"].shape
    print(dtype, "out rel", rel_err(out, c["ref"]))
    assert rel_err(out, c["ref"]) < tol
    ws = model.plan.workspace(2, 16, 16, 16, DEV)
    got = model.plan.trace_tensors(ws, 2, 16, 16, 16)
    assert len(got) == len(c["trace"])      # one entry per topology block, in the concatenating model's order
    for i, (gt, rf) in enumerate(zip(got, c["trace"])):
        if gt is None:
            continue
        assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 8e-2), ("fp16", 1.5e-2)])
def test_tiny_unet_backward_vs_autograd(dtype, tol):
    c = _tiny_case()
    out, grads, model = _unet_grads(cases.C1_CFG, cases.C1_GROUPS, c["P"], c["x"], c["t"], c["R"], dtype)
    assert rel_err(out, c["ref_out"]) < tol
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print(dtype, "worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:5])
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    n = sum(p.numel() for p in model.parameters())
    assert model.flat_grad().numel() == n == sum(v.numel() for v in c["P"].values())


def test_tiny_unet_backward_segments_and_hook():
    """Segment-wise backward with a per-segment hook: every segment once, the flat
    buffer covered exactly once, the same gradients (the skip average owns no
    parameters: it runs inside its decoder block's segment)."""
    c = _tiny_case()
    cfg, G = cases.C1_CFG, cases.C1_GROUPS
    _, g_all, _ = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32")
    seen = []

    def hook(seg, flat, off, n):
        if seg is not None:
            seen.append((seg, off, n))
    _, g_seg, model = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32", hook=hook)
    n = sum(p.numel() for p in model.parameters())
    assert [s[0] for s in seen] == list(range(model.plan.num_segments))
    cover = torch.zeros(n, dtype=torch.int32)
    for _, off, cnt in seen:
        cover[off:off + cnt] += 1
    assert bool((cover == 1).all())
    for name in g_all:
        assert rel_err(g_seg[name], g_all[name]) < 1e-5, name


# --------------------------------------------------------------------------- production channels
PROD_CFG = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
PROD_GRID = (32, 32, 64)   # the smallest grid at which R0 and R1 run the DMA-staged kernel
_PROD = {}


def _prod_case():
    if not _PROD:
        P = ao.random_params(seed=51, **PROD_CFG)
        g = torch.Generator().manual_seed(52)
        x = torch.randn(1, 32, *PROD_GRID, generator=g)
        t = torch.tensor([500])
        R = torch.randn(1, 8, *PROD_GRID, generator=g)
        ref_out, ref = ao.grads(PROD_CFG, 32, P, x, t, R)
        _PROD.update(P=P, x=x, t=t, R=R, ref_out=ref_out, ref=ref)
    return _PROD


def _prod_run(dtype, path):
    from cwdm_hip._lib import lib
    c = _prod_case()
    prev = lib().cwdm_conv3d_set_path(path)
    try:
        out, grads, _ = _unet_grads(PROD_CFG, 32, c["P"], c["x"], c["t"], c["R"], dtype)
    finally:
        lib().cwdm_conv3d_set_path(prev)
    worst = {k: _rel_l2(grads[k], c["ref"][k]) for k in c["ref"]}
    assert set(grads) == set(c["ref"])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    eo = rel_err(out, c["ref_out"])
    print(dtype, "path", path, "out rel", eo, "worst grads", top)
    return eo, top


@pytest.mark.parametrize("path", [2, 0])
def test_production_unet_fp32_vs_autograd(path):
    """run.sh channels at the smallest grid where R0 and R1 run the DMA-staged kernel, conv path 2
    (forced wherever the shape allows) and 0 (the auto policy): output and every parameter gradient
    within 1e-3 of one cached CPU reference (measured 1.8e-6 / 1.0e-5)."""
    eo, top = _prod_run("fp32", path)
    assert eo < 1e-3
    assert top[0][1] < 1e-3, top


@pytest.mark.parametrize("dtype,tol_out,tol_grad", [("bf16", 5e-2, 8e-2), ("fp16", 1e-2, 1.5e-2)])
def test_production_unet_half_close_to_fp32_reference(dtype, tol_out, tol_grad):
    """The 16-bit plans against the same fp32 CPU reference, bounds of the concatenating model's
    test (measured: bf16 output 9.1e-3, worst gradient 5.1e-2 at output_blocks.1.0.out_layers.0.weight;
    fp16 1.2e-3 / 5.8e-3 at output_blocks.1.0.in_layers.0.weight)."""
    eo, top = _prod_run(dtype, 2)
    assert eo < tol_out
    assert top[0][1] < tol_grad, top


def test_production_unet_accurate_fast_mode_forward():
    c = _prod_case()
    model = _product_model(PROD_CFG, 32, c["P"], "fp32x")
    with torch.no_grad():
        out = model(c["x"].to(DEV), c["t"].to(DEV))
    print("fp32x out rel", rel_err(out, c["ref_out"]))
    assert rel_err(out, c["ref_out"]) < 1e-3


# --------------------------------------------------------------------------- sampling
def _c1_additive(dtype="fp32", **model_args):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         **model_args)
    keys = script_util.model_and_diffusion_defaults().keys()
    kw = {k: args[k] for k in keys}
    kw["additive_skips"] = True
    model, diffusion = script_util.create_model_and_diffusion(**kw, compute_dtype=dtype)
    diffusion.mode = "i2i"
    return model, diffusion


def test_sampling_loop_vs_restatement_fp32():
    _, cond, x_T, noises, _ = cases.c1_inputs(32)
    P = ao.random_params(seed=1, **cases.C1_CFG)
    model, diffusion = _c1_additive(diffusion_steps=2, sample_schedule="sampled")
    model.load_state_dict(P)
    model.to(DEV)
    it = iter([n.to(DEV) for n in noises])
    sample = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), clip_denoised=True,
                                     progress=False, noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 2, "sampled"))
    ref = od.p_sample_loop(tab, ao.AdditiveOracleUNet(P, num_groups=cases.C1_GROUPS, **cases.C1_CFG), x_T, cond,
                           noises)
    assert rel_err(sample, ref) < 1e-3


@pytest.mark.parametrize("respacing,dtype", [("", "fp32"), ("ddim10", "bf16")])
def test_hip_graph_loop_equals_eager_loop(respacing, dtype):
    model, diffusion = _c1_additive(dtype, diffusion_steps=50, sample_schedule="direct",
                                    timestep_respacing=respacing)
    model.load_state_dict(ao.random_params(seed=1, **cases.C1_CFG))
    model.to(DEV)
    g = torch.Generator().manual_seed(5)
    cond = torch.rand(1, 24, 16, 16, 16, generator=g).to(DEV)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g).to(DEV)
    diffusion.native_noise = "philox"

    def run(graph):
        diffusion.use_hip_graph = graph
        torch.manual_seed(11)
        return [o["sample"] for o in diffusion.p_sample_loop_progressive(model, x_T.shape, noise=x_T, cond=cond,
                                                                        progress=False)]

    eager, graph = run(False), run(True)
    diffusion.use_hip_graph = False
    assert len(eager) == len(graph) == diffusion.num_timesteps
    for a, b in zip(eager, graph):
        assert torch.equal(a, b), rel_err(b, a)
    assert torch.isfinite(eager[-1]).all()


# --------------------------------------------------------------------------- training
def test_training_step_loss_and_gradients_vs_restatement():
    vols = {k: v.to(DEV) for k, v in cases.data.brats_batch(32, seed=4, batch=2).items()}
    P = ao.random_params(seed=31, **cases.C1_CFG)
    model, diffusion = _c1_additive()
    model.load_state_dict(P)
    model.to(DEV)
    t = torch.tensor([5, 700], device=DEV)
    noise = torch.randn(2, 1, 32, 32, 32, device=DEV)
    terms, _, _ = diffusion.training_losses(model, vols, t, mode="i2i", contr="t2w", noise=noise)
    loss = terms["mse_wav"].mean()
    loss.backward()
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}

    def om(x, tt, **kw):
        return ao.unet_forward(Pr, x, tt, num_groups=cases.C1_GROUPS, **cases.C1_CFG)
    rterms, _, _ = od.training_losses(tab, om, {k: v.cpu() for k, v in vols.items()}, t.cpu(), noise.cpu(),
                                      contr="t2w")
    rloss = rterms["mse_wav"].mean()
    rloss.backward()
    assert abs(float(loss) - float(rloss)) / float(rloss) < 1e-4
    for n, p in model.named_parameters():
        assert _rel_l2(p.grad, Pr[n].grad) < 1e-3, n


def test_trainloop_two_steps_bitwise_reproducible(tmp_path, monkeypatch):
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = ao.random_params(seed=41, **cases.C1_CFG)
    batch = cases.data.brats_batch(32, seed=5, batch=1)
    bdev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def run():
        model, diffusion = _c1_additive()
        model.load_state_dict(P)
        model.to(DEV)
        loop = train_util.TrainLoop(model=model, diffusion=diffusion, data=[batch], batch_size=1, in_channels=32,
                                    image_size=64, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=100,
                                    contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0,
                                    lr_anneal_steps=0, mode="i2i", diffusion_steps=1000)
        torch.manual_seed(0)
        np.random.seed(0)
        for _ in range(2):
            loop.run_step(bdev, {}, info={})
        torch.cuda.synchronize()
        return model.flat_params.detach().clone(), model.flat_grad().detach().clone()

    try:
        p_a, g_a = run()
        p_b, g_b = run()
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert torch.isfinite(p_a).all() and float(g_a.abs().max()) > 0
    p0 = torch.cat([v.reshape(-1) for v in P.values()])
    assert not torch.equal(p_a.cpu(), p0)
    assert torch.equal(g_a, g_b)
    assert torch.equal(p_a, p_b)
