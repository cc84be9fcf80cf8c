"""use_scale_shift_norm=True on the GPU: the FiLM finalize (cwdm_gn_finalize_film)
against float64, the fused finalize + pre-pass against the unfused pair, the FiLM
GroupNorm/SiLU backward (cwdm_gn_silu_bwd_film) against autograd, then the U-Net
forward / trace, backward, the segment-wise backward, the captured sampling loop
and training against the CPU fp32 restatement (tests/scale_shift_oracle.py) and
autograd on it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scale_shift_oracle as sso
from oracle import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _nd(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _nc(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _dt(name):
    from cwdm_hip import _lib
    return {"fp32": (_lib.CWDM_F32, torch.float32), "bf16": (_lib.CWDM_BF16, torch.bfloat16),
            "fp16": (_lib.CWDM_F16, torch.float16)}[name]


def _film_buffer(B, C, g, pad=24, off=8, fill=7.0):
    """Rows [s | t] (std 0.3) inside a wider buffer: batch stride 2 C + pad, first row at element off.
    -> (s, t) on the CPU, the device buffer, the pointer of row 0, the stride."""
    s = 0.3 * torch.randn(B, C, generator=g)
    t = 0.3 * torch.randn(B, C, generator=g)
    stride = 2 * C + pad
    buf = torch.full((B * stride + off,), fill)
    rows = buf[off:off + B * stride].view(B, stride)
    rows[:, :C] = s
    rows[:, C:2 * C] = t
    buf = buf.to(DEV)
    return s, t, buf, buf.data_ptr() + 4 * off, stride


# --------------------------------------------------------------------------- 1. the FiLM finalize
@pytest.mark.parametrize("parts", [4, 1024])
@pytest.mark.parametrize("C,G", [(64, 32), (32, 8)])
def test_gn_finalize_film_vs_float64(C, G, parts):
    """cwdm_gn_finalize_film on fabricated partials, B = 2 with different rows per batch entry, the
    rows at a stride above 2 C and a row offset: x sc' + sh' against GroupNorm(x) (1 + s) + t in
    float64 within 1e-5 (cwdm_gn_finalize's bound), mean / rstd as there, a second call bitwise
    equal, and with s = t = 0 the bits of cwdm_gn_finalize."""
    from cwdm_hip._lib import check, lib
    L = lib()
    B, n = 2, 16
    V = n ** 3
    g = torch.Generator().manual_seed(70 + C + parts)
    x = torch.randn(B, C, n, n, n, generator=g) * 2.5 + 0.5
    xv = x.reshape(B, C, parts, -1)
    st = torch.stack([xv.sum(-1), (xv ** 2).sum(-1)], -1).permute(0, 2, 1, 3).contiguous().to(DEV)   # B, P, C, 2
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    s, t, fbuf, fptr, fstride = _film_buffer(B, C, g)

    def film(ptr, stride):
        out, mr = torch.empty(B, C, 2, device=DEV), torch.empty(B, G, 2, device=DEV)
        check(L.cwdm_gn_finalize_film(st.data_ptr(), parts, C, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), G, B, V,
                                      1e-5, out.data_ptr(), mr.data_ptr(), ptr, stride, None))
        return out.cpu(), mr.cpu()
    o, mr = film(fptr, fstride)
    o2, mr2 = film(fptr, fstride)
    assert torch.equal(o, o2) and torch.equal(mr, mr2)
    xd = x.double()
    ref = F.group_norm(xd, G, gamma.cpu().double(), beta.cpu().double(), eps=1e-5) * \
        (1 + s.double())[:, :, None, None, None] + t.double()[:, :, None, None, None]
    y = xd * o[..., 0].double()[:, :, None, None, None] + o[..., 1].double()[:, :, None, None, None]
    err = rel_err(y, ref)
    print("finalize_film", C, G, parts, "rel", err)
    assert err < 1e-5
    xg = xd.view(B, G, -1)
    assert torch.allclose(mr[..., 0].double(), xg.mean(-1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(mr[..., 1].double(), 1 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5), rtol=1e-5)
    # the rows of the two batch entries differ, and so do their tables beyond the statistics
    assert not torch.equal(s[0], s[1])
    # s = t = 0: the plain finalize, bit for bit
    zero = torch.zeros(B, 2 * C, device=DEV)
    oz, mrz = film(zero.data_ptr(), 2 * C)
    op, mrp = torch.empty(B, C, 2, device=DEV), torch.empty(B, G, 2, device=DEV)
    check(L.cwdm_gn_finalize(st.data_ptr(), parts, C, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), G, B, V, 1e-5,
                             op.data_ptr(), mrp.data_ptr(), None))
    assert torch.equal(oz, op.cpu()) and torch.equal(mrz, mrp.cpu())
    assert torch.equal(mr, mrp.cpu())


# --------------------------------------------------------------------------- 2. fused against unfused
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cpg", [2, 8])
def test_gn_fin_apply_film_matches_finalize_film_plus_apply(cpg, dtype_name):
    """cwdm_debug_gn_fin_apply_film == cwdm_gn_finalize_film + cwdm_gn_apply, with the bounds of the
    plain pair's test: (scale, shift) and (mean, rstd) within 1e-6, activations within one 16-bit ulp."""
    from cwdm_hip._lib import check, lib
    dt, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(140 + cpg)
    B, C, parts, V = 2, 64, 8, 512
    G = C // cpg
    x = (torch.randn(B, V, C, generator=g) * 1.5 + 0.3).to(tdt).float()
    xv = x.view(B, parts, V // parts, C)
    st = torch.stack([xv.sum(2), (xv ** 2).sum(2)], -1).contiguous().to(DEV)     # [B][P][C][2]
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    s, _, fbuf, fptr, fstride = _film_buffer(B, C, g)
    xd = x.to(DEV, tdt)
    L = lib()
    ss_a, mr_a = torch.empty(B, C, 2, device=DEV), torch.empty(B, G, 2, device=DEV)
    act_a = torch.empty(B, V, C, device=DEV, dtype=tdt)
    check(L.cwdm_gn_finalize_film(st.data_ptr(), parts, C, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), G, B, V,
                                  1e-5, ss_a.data_ptr(), mr_a.data_ptr(), fptr, fstride, None))
    check(L.cwdm_gn_apply(xd.data_ptr(), C, None, 0, ss_a.data_ptr(), B, V, dt, act_a.data_ptr(), None))
    ss_b, mr_b = torch.empty_like(ss_a), torch.empty_like(mr_a)
    act_b = torch.empty(B, C // 16, V, 16, device=DEV, dtype=tdt)
    check(L.cwdm_debug_gn_fin_apply_film(st.data_ptr(), parts, C, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), G, B,
                                         V, 1e-5, xd.data_ptr(), None, dt, ss_b.data_ptr(), mr_b.data_ptr(),
                                         act_b.data_ptr(), fptr, fstride, None))
    # and the plain fused pass, to see that the rows were applied at all
    ss_p, mr_p = torch.empty_like(ss_a), torch.empty_like(mr_a)
    act_p = torch.empty_like(act_b)
    check(L.cwdm_debug_gn_fin_apply(st.data_ptr(), parts, C, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), G, B, V,
                                    1e-5, xd.data_ptr(), None, dt, ss_p.data_ptr(), mr_p.data_ptr(), act_p.data_ptr(),
                                    None))
    torch.cuda.synchronize()
    print("fin_apply_film", cpg, dtype_name, "ss", rel_err(ss_b, ss_a), "mr", rel_err(mr_b, mr_a))
    assert rel_err(ss_b, ss_a) < 1e-6
    assert rel_err(mr_b, mr_a) < 1e-6
    assert rel_err(ss_p, ss_a) > 0.05 and rel_err(mr_p, mr_a) < 1e-6
    a = act_a.float().view(B, V, C // 16, 16).permute(0, 2, 1, 3).cpu()
    b = act_b.float().cpu()
    ulp = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}[dtype_name]
    assert torch.all((a - b).abs() <= ulp * a.abs() + 1e-6), float((a - b).abs().max())


# --------------------------------------------------------------------------- 3. the FiLM backward
@pytest.mark.parametrize("B,grid,G,dtype_name", [
    (2, (4, 8, 6), 8, "fp32"), (2, (4, 8, 6), 8, "bf16"), (2, (4, 8, 6), 8, "fp16"),
    (2, (4, 8, 6), 32, "fp32"), (2, (4, 8, 6), 32, "bf16"), (2, (4, 8, 6), 32, "fp16"),
    (1, (32, 32, 32), 32, "bf16")])     # 1024 reduce blocks
def test_gn_silu_bwd_film_vs_autograd(B, grid, G, dtype_name):
    """cwdm_gn_silu_bwd_film against autograd on SiLU(GN(x) (1 + s) + t): dx, dgamma, dbeta, ds, dt
    within cwdm_gn_silu_bwd's bounds (1e-4 fp32, 3e-2 16-bit); s drawn with std 0.3."""
    from cwdm_hip._lib import check, lib
    dtype, tdt = _dt(dtype_name)
    C = 64
    g = torch.Generator().manual_seed(19 + G)
    x = (1.5 * torch.randn(B, C, *grid, generator=g) + 0.3).to(tdt).float()
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    du = torch.randn(B, C, *grid, generator=g).to(tdt).float()
    s, t, fbuf, fptr, fstride = _film_buffer(B, C, g)
    xr, gr, br = (v.clone().requires_grad_(True) for v in (x, gamma, beta))
    sr, tr = s.clone().requires_grad_(True), t.clone().requires_grad_(True)
    y = F.silu(F.group_norm(xr, G, gr, br, eps=1e-5) * (1 + sr)[:, :, None, None, None] + tr[:, :, None, None, None])
    (y * du).sum().backward()
    # the forward's tables as cwdm_gn_finalize_film produces them
    xg = x.view(B, G, -1).double()
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5)
    mr = torch.stack([mean, rstd], -1).float().contiguous()
    cpg = C // G
    sc = gamma[None] * rstd.float().repeat_interleave(cpg, 1)
    sh = beta[None] - mean.float().repeat_interleave(cpg, 1) * sc
    ss = torch.stack([sc * (1 + s), sh * (1 + s) + t], -1).contiguous()
    xd = _nd(x).to(DEV, tdt)
    dud = _nd(du).to(DEV, tdt)
    dx = torch.empty(B, *grid, C, device=DEV, dtype=tdt)
    dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dstride, doff = 2 * C + 40, 16
    dbuf = torch.full((B * dstride + doff,), 7.0, device=DEV)
    L = lib()
    nws = L.cwdm_gn_silu_bwd_workspace_bytes(C, B, *grid)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    ssd, mrd, gd, bd = ss.to(DEV), mr.to(DEV), gamma.to(DEV), beta.to(DEV)
    check(L.cwdm_gn_silu_bwd_film(xd.data_ptr(), C, None, 0, dud.data_ptr(), 0, ssd.data_ptr(), mrd.data_ptr(),
                                  gd.data_ptr(), G, B, *grid, dtype, dx.data_ptr(), 0, None, 0, dgam.data_ptr(),
                                  dbet.data_ptr(), ws.data_ptr(), nws, bd.data_ptr(), fptr, fstride,
                                  dbuf.data_ptr() + 4 * doff, dstride, None))
    torch.cuda.synchronize()
    rows = dbuf[doff:].view(B, dstride).cpu()
    errs = dict(dx=rel_err(_nc(dx.float().cpu()), xr.grad), dgamma=rel_err(dgam, gr.grad),
                dbeta=rel_err(dbet, br.grad), ds=rel_err(rows[:, :C], sr.grad), dt=rel_err(rows[:, C:2 * C], tr.grad))
    print("gn_silu_bwd_film", B, grid, G, dtype_name, errs)
    tol = 1e-4 if dtype_name == "fp32" else 3e-2
    assert max(errs.values()) < tol, errs
    # nothing written outside the two halves of each row
    assert bool((rows[:, 2 * C:] == 7.0).all()) and bool((dbuf[:doff] == 7.0).all())
    # the draw puts 1 + s far from 1 on both sides
    assert float((1 + s).min()) < 0.7 and float((1 + s).max()) > 1.3


# --------------------------------------------------------------------------- 4. the tiny U-Net
VARIANTS = {
    "plain": dict(),
    "additive": dict(additive_skips=True),
    "attention": dict(bottleneck_attention=True, num_heads=4),
    "no-updown": dict(resblock_updown=False),
}


def _product_model(cfg, groups, params, dtype, **opts):
    from guided_diffusion.unet import UNetModel
    opts = dict(opts)
    opts.setdefault("resblock_updown", True)
    opts.setdefault("bottleneck_attention", False)
    m = UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resample_2d=False, num_groups=groups,
                  use_scale_shift_norm=True, compute_dtype=dtype, **opts)
    m.load_state_dict(params)
    return m.to(DEV)


def _unet_grads(cfg, G, P, x, t, R, dtype, hook=None, **opts):
    model = _product_model(cfg, G, P, dtype, **opts)
    model._grad_hook = hook
    out = model(x.to(DEV), t.to(DEV))
    (out * R.to(DEV)).sum().backward()
    return out.detach().cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters()}, model


_TINY = {}


def _tiny_case(variant):
    """x (2, 32, 16, 16, 16), t [3, 917]: the restatement's output, trace and autograd gradients, once."""
    if variant not in _TINY:
        cfg, G, opts = cases.C1_CFG, cases.C1_GROUPS, VARIANTS[variant]
        shape_opts = {k: v for k, v in opts.items() if k in ("additive_skips", "bottleneck_attention",
                                                             "resblock_updown")}
        P = sso.random_params(seed=1, **shape_opts, **cfg)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 32, 16, 16, 16, generator=g)
        t = torch.tensor([3, 917])
        R = torch.randn(2, 8, 16, 16, 16, generator=g)
        trace, scales = [], []
        with torch.no_grad():
            ref = sso.unet_forward(P, x, t, num_groups=G, trace=trace, scales=scales, **cfg, **opts)
        ref_out, ref_grads = sso.grads(cfg, G, P, x, t, R, **opts)
        # not vacuous: the rows move the norm visibly, and out_layers.3 is not the reference's zero init
        assert max(float(s.abs().max()) for s in scales) >= 0.05
        assert all(float(v.abs().max()) > 0 for k, v in P.items() if ".out_layers.3." in k)
        _TINY[variant] = dict(P=P, x=x, t=t, R=R, ref=ref, trace=trace, ref_out=ref_out, ref_grads=ref_grads)
    return _TINY[variant]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 6e-2), ("fp16", 1e-2)])
def test_tiny_unet_forward_and_trace(variant, dtype, tol):
    c = _tiny_case(variant)
    model = _product_model(cases.C1_CFG, cases.C1_GROUPS, c["P"], dtype, **VARIANTS[variant])
    with torch.no_grad():
        out = model(c["x"].to(DEV), c["t"].to(DEV))
    assert out.shape == c["ref"].shape
    ws = model.plan.workspace(2, 16, 16, 16, DEV)
    got = model.plan.trace_tensors(ws, 2, 16, 16, 16)
    assert len(got) == len(c["trace"])
    errs = [rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) for gt, rf in zip(got, c["trace"]) if gt is not None]
    print("tiny forward", variant, dtype, "out rel", rel_err(out, c["ref"]), "worst trace", max(errs))
    assert rel_err(out, c["ref"]) < tol
    assert max(errs) < tol, errs


@pytest.mark.parametrize("variant,dtype,tol", [("plain", "fp32", 1e-3), ("additive", "fp32", 1e-3),
                                               ("attention", "fp32", 1e-3), ("no-updown", "fp32", 1e-3),
                                               ("plain", "bf16", 8e-2), ("plain", "fp16", 1.5e-2)])
def test_tiny_unet_backward_vs_autograd(variant, dtype, tol):
    c = _tiny_case(variant)
    out, grads, model = _unet_grads(cases.C1_CFG, cases.C1_GROUPS, c["P"], c["x"], c["t"], c["R"], dtype,
                                    **VARIANTS[variant])
    assert rel_err(out, c["ref_out"]) < tol
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print("tiny backward", variant, dtype, "worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:5])
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    n = sum(p.numel() for p in model.parameters())
    assert model.flat_grad().numel() == n == sum(v.numel() for v in c["P"].values())


# --------------------------------------------------------------------------- 5. production channels
PROD_CFG = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))


def test_production_channels_forward_fp32():
    """The 81.5 M configuration with the flag on, B = 1 at 16^3: 8 channels per group, 256 channels,
    the 1x1-skip blocks."""
    P = sso.random_params(seed=51, **PROD_CFG)
    g = torch.Generator().manual_seed(52)
    x = torch.randn(1, 32, 16, 16, 16, generator=g)
    t = torch.tensor([500])
    with torch.no_grad():
        ref = sso.unet_forward(P, x, t, num_groups=32, **PROD_CFG)
    model = _product_model(PROD_CFG, 32, P, "fp32")
    with torch.no_grad():
        out = model(x.to(DEV), t.to(DEV))
    print("production forward fp32 rel", rel_err(out, ref))
    assert rel_err(out, ref) < 1e-3


# --------------------------------------------------------------------------- 6. segments and the hook
def test_tiny_unet_backward_segments_and_hook():
    """Segment-wise backward with a per-segment hook: every segment once, the flat buffer covered
    exactly once, the one-shot backward's gradients, and two backwards on the same inputs bitwise equal."""
    c = _tiny_case("plain")
    cfg, G = cases.C1_CFG, cases.C1_GROUPS
    _, g_all, m_all = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32")
    flat_a = m_all.flat_grad().detach().clone()
    _, g_again, m_again = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32")
    assert torch.equal(flat_a, m_again.flat_grad())
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


# --------------------------------------------------------------------------- 7. sampling graph, training
def _c1_film(dtype="fp32", **model_args):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         use_scale_shift_norm=True, **model_args)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    diffusion.mode = "i2i"
    return model, diffusion


@pytest.mark.parametrize("respacing,dtype", [("", "fp32"), ("ddim10", "bf16")])
def test_hip_graph_loop_equals_eager_loop(respacing, dtype):
    model, diffusion = _c1_film(dtype, diffusion_steps=50, sample_schedule="direct", timestep_respacing=respacing)
    assert model.use_scale_shift_norm
    model.load_state_dict(sso.random_params(seed=1, **cases.C1_CFG))
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


def test_trainloop_two_steps_bitwise_reproducible(tmp_path, monkeypatch):
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = sso.random_params(seed=41, **cases.C1_CFG)
    batch = cases.data.brats_batch(32, seed=5, batch=1)
    bdev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def run():
        model, diffusion = _c1_film("bf16")
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
        return {n: p.detach().cpu().clone() for n, p in model.named_parameters()}, model.flat_grad().detach().clone()

    try:
        p_a, g_a = run()
        p_b, g_b = run()
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert torch.equal(g_a, g_b) and float(g_a.abs().max()) > 0
    for n in p_a:
        assert torch.isfinite(p_a[n]).all(), n
        assert torch.equal(p_a[n], p_b[n]), n
    moved = [n for n in p_a if ".emb_layers.1." in n and not torch.equal(p_a[n], P[n])]
    assert sorted(moved) == sorted(n for n in P if ".emb_layers.1." in n), moved
