"""The reference's model family on the GPU: 8 wavelet channels for the image plus 8 per condition volume
(run.sh:65), i.e. in_channels 8, 16, 24, 40 beside the 32 of the BraTS configuration -- the N-condition training
front end, the U-Net forward and backward with conv_in on a zero-padded staged input (16-bit plans: 8 -> 16,
24 -> 32, 40 -> 48), sampling and training through the public API, against the CPU oracle
(tests/cond_count_oracle.py restates the loss for N conditions).  The tiny model is oracle.cases.C1_CFG with
in_channels replaced."""
import numpy as np
import pytest
import torch

import cond_count_oracle as cco
from oracle import cases, diffusion as od, unet as ou

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = cases.C1_GROUPS
FWD_TOL = {"fp32": 1e-3, "bf16": 6e-2, "fp16": 1e-2}      # as tests/test_gpu_unet.py
BWD_TOL = {"fp32": 1e-3, "bf16": 8e-2, "fp16": 1.5e-2}    # as tests/test_gpu_train.py
FATS_SHIFT = [-1.2, 0.4, 0.5, 0.9, 0.3, 0.8, 1.0, 1.6]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cfg(cin):
    return dict(cases.C1_CFG, in_channels=cin)


def _model(cin, params, dtype):
    from guided_diffusion.unet import UNetModel
    cfg = _cfg(cin)
    m = UNetModel(image_size=32, in_channels=cin, model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resblock_updown=True, bottleneck_attention=False,
                  resample_2d=False, num_groups=G, compute_dtype=dtype)
    m.load_state_dict(params)
    return m.to(DEV)


def _model_and_diffusion(cin, params, dtype="fp32", **over):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         in_channels=cin, mode="default" if cin == 8 else "i2i", **over)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    model.load_state_dict(params)
    return model.to(DEV), diffusion


_CACHE = {}


def _once(key, fn):
    """A CPU reference computed once and shared by the cases that need it (never written to)."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# --------------------------------------------------------------------------- 1. the N-condition front end
SHAPES = [(1, 1, 8, 8, 8), (2, 1, 16, 12, 20)]


def _front_inputs(shape, n, seed=6):
    g = torch.Generator().manual_seed(seed)
    vols = [torch.rand(shape, generator=g) for _ in range(1 + n)]
    eps = torch.randn(shape, generator=g)
    t = torch.tensor([0, 999][:shape[0]])
    return vols, eps, t


def _diffusion(**kw):
    from guided_diffusion import script_util
    return script_util.create_gaussian_diffusion(steps=1000, predict_xstart=True, mode="i2i", **kw)


@pytest.mark.parametrize("per_band", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_prepare_batch_n_with_three_conditions_is_prepare_batch(shape, per_band):
    from cwdm_hip import ops
    d = _diffusion(band_log_snr_shift=FATS_SHIFT) if per_band else _diffusion()
    vols, eps, t = _front_inputs(shape, 3)
    dv = [v.to(DEV) for v in vols]
    coef = d.q_coef_table(DEV)
    a_in, a_0 = ops.prepare_batch(*dv, eps.to(DEV), coef, t.to(DEV), 1000, per_band=per_band)
    b_in, b_0 = ops.prepare_batch_n(dv[0], dv[1:], eps.to(DEV), coef, t.to(DEV), 1000, per_band=per_band)
    assert b_in.shape == a_in.shape and torch.equal(b_in, a_in)
    assert torch.equal(b_0, a_0)


@pytest.mark.parametrize("n", [0, 1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_prepare_batch_n_bitexact_vs_restatement(shape, n):
    from cwdm_hip import ops
    d = _diffusion()
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    vols, eps, t = _front_inputs(shape, n, seed=7 + n)
    x_in, x0 = ops.prepare_batch_n(vols[0].to(DEV), [v.to(DEV) for v in vols[1:]], eps.to(DEV), d.q_coef_table(DEV),
                                   t.to(DEV), 1000)
    r_in, r_0 = cco.front_end(tab, vols[0], vols[1:], t, eps)
    B, _, D, H, W = shape
    assert x_in.shape == (B, 8 + 8 * n, D // 2, H // 2, W // 2)
    assert torch.equal(x0.cpu(), r_0)
    assert torch.equal(x_in.cpu(), r_in)


def test_prepare_batch_n_refuses_eight_conditions():
    from cwdm_hip import ops
    from cwdm_hip._lib import CwdmError
    d = _diffusion()
    vols, eps, t = _front_inputs(SHAPES[0], 8)
    with pytest.raises(CwdmError, match="0..7 condition volumes"):
        ops.prepare_batch_n(vols[0].to(DEV), [v.to(DEV) for v in vols[1:]], eps.to(DEV), d.q_coef_table(DEV),
                            t.to(DEV), 1000)


# --------------------------------------------------------------------------- 2. forward
def _fwd_case(cin, n):
    def make():
        cfg = _cfg(cin)
        P = ou.random_params(seed=1, **cfg)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, cin, n, n, n, generator=g)
        t = torch.tensor([3, 917])
        trace = []
        ref = ou.unet_forward(P, x, t, num_groups=G, trace=trace, **cfg)
        return P, x, t, ref, trace
    return _once(("fwd", cin, n), make)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n", [16, 14])    # 14^3: tail tiles, 7^3 below
@pytest.mark.parametrize("cin", [8, 24, 40])
def test_forward_and_trace_on_a_nan_filled_workspace(cin, n, dtype):
    """The output and every traced block output against the oracle.  The workspace comes from the caller filled
    with 0xFF bytes -- every bf16, fp16 and fp32 lane a NaN -- so a padded input lane the plan did not write
    would poison conv_in (0 x NaN = NaN): finite, in-tolerance results prove the staging writes its zeros."""
    tol = FWD_TOL[dtype]
    P, x, t, ref, trace = _fwd_case(cin, n)
    model = _model(cin, P, dtype)
    plan = model.plan
    B = x.shape[0]
    with torch.no_grad():
        xin, tf = model._prep_inputs(x.to(DEV), t.to(DEV))
        assert xin.shape == (B, n, n, n, cin)        # the interface stays dense
        ws = torch.full((plan.workspace_bytes(B, n, n, n),), 0xFF, dtype=torch.uint8, device=DEV)
        out_nd = torch.empty((B, n, n, n, 8), dtype=torch.float32, device=DEV)
        plan.forward(model.packed_weights(), xin, tf, out_nd, B, n, n, n, ws=ws)
        out = out_nd.permute(0, 4, 1, 2, 3)
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) < tol
    got = plan.trace_tensors(ws, B, n, n, n)
    assert len(got) == len(trace)
    for i, (gt, rf) in enumerate(zip(got, trace)):
        if gt is None:
            continue
        assert torch.isfinite(gt).all(), i
        assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i
    # the nn.Module call (the plan's own workspace) gives the same bits
    with torch.no_grad():
        assert torch.equal(model(x.to(DEV), t.to(DEV)), out)


# --------------------------------------------------------------------------- 3. padding equivalence
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_padded_plan_equals_the_32_channel_plan_with_zero_columns(dtype):
    """in_channels=24 on x against in_channels=32 with eight zero weight columns on [x | 0]: the staged input and
    the packed weights of the first are exactly the second's, so the outputs are bitwise equal."""
    P24, x, t, _, _ = _fwd_case(24, 16)
    P32 = ou.random_params(seed=1, **_cfg(32))
    for k in P24:
        if k != "input_blocks.0.0.weight":
            P32[k] = P24[k].clone()
    w = torch.zeros_like(P32["input_blocks.0.0.weight"])
    w[:, :24] = P24["input_blocks.0.0.weight"]
    P32["input_blocks.0.0.weight"] = w
    x32 = torch.cat([x, torch.zeros(2, 8, 16, 16, 16)], dim=1)
    with torch.no_grad():
        a = _model(24, P24, dtype)(x.to(DEV), t.to(DEV))
        b = _model(32, P32, dtype)(x32.to(DEV), t.to(DEV))
    assert torch.isfinite(a).all() and torch.equal(a, b)


# --------------------------------------------------------------------------- 4. backward
def _bwd_case(cin):
    def make():
        cfg = _cfg(cin)
        P = ou.random_params(seed=21, **cfg)
        g = torch.Generator().manual_seed(22)
        x = torch.randn(2, cin, 16, 16, 16, generator=g)
        t = torch.tensor([5, 700])
        R = torch.randn(2, 8, 16, 16, 16, generator=g)
        Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        out = ou.unet_forward(Pr, x, t, num_groups=G, **cfg)
        (out * R).sum().backward()
        return P, x, t, R, out.detach(), {k: v.grad for k, v in Pr.items()}
    return _once(("bwd", cin), make)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("cin", [8, 24])
def test_backward_vs_oracle_autograd(cin, dtype):
    tol = BWD_TOL[dtype]
    P, x, t, R, ref_out, ref = _bwd_case(cin)
    model = _model(cin, P, dtype)
    model.keep_activations = True
    out = model(x.to(DEV), t.to(DEV))
    (out * R.to(DEV)).sum().backward()
    assert rel_err(out.detach(), ref_out) < tol
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
    assert set(grads) == set(ref)
    assert grads["input_blocks.0.0.weight"].shape == (32, cin, 3, 3, 3)
    worst = {}
    for k in ref:
        a, b = grads[k].double(), ref[k].double()
        assert torch.isfinite(a).all(), k
        worst[k] = float((a - b).norm() / b.norm().clamp_min(1e-30))
    print(f"backward in={cin} {dtype}: conv_in weight {worst['input_blocks.0.0.weight']:.3e}, "
          f"worst {max(worst.values()):.3e}")
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    n = sum(p.numel() for p in model.parameters())
    assert model.flat_grad().numel() == n == sum(v.numel() for v in P.values())


@pytest.mark.parametrize("cin,dtype", [(8, "bf16"), (24, "fp16"), (8, "fp32")])
def test_backward_segments_cover_the_flat_buffer_once(cin, dtype):
    """The segment-wise backward with a per-segment hook (the DDP bucket seam): the same gradients as the
    one-call backward, the ranges tiling the flat buffer exactly once -- no padded column in it."""
    P, x, t, R, _, _ = _bwd_case(cin)
    whole = _model(cin, P, dtype)
    (whole(x.to(DEV), t.to(DEV)) * R.to(DEV)).sum().backward()
    model = _model(cin, P, dtype)
    seen = []

    def hook(seg, flat, off, n):
        if seg is not None:
            seen.append((seg, off, n))
    model._grad_hook = hook
    (model(x.to(DEV), t.to(DEV)) * R.to(DEV)).sum().backward()
    n = sum(p.numel() for p in model.parameters())
    assert [s[0] for s in seen] == list(range(model.plan.num_segments))
    cover = torch.zeros(n, dtype=torch.int32)
    for _, off, cnt in seen:
        cover[off:off + cnt] += 1
    assert bool((cover == 1).all())
    for (name, p), (_, q) in zip(model.named_parameters(), whole.named_parameters()):
        assert rel_err(p.grad, q.grad) < 1e-5, name     # (as tests/test_gpu_train.py: the same launches)


# --------------------------------------------------------------------------- 5. sampling
def test_unconditional_sampling_vs_oracle_fp32():
    """mode='default', in_channels=8: 4 ancestral steps from t = 3 with injected noise, against the oracle's
    loop with a zero-channel condition."""
    cfg = _cfg(8)
    P = ou.random_params(seed=1, **cfg)
    model, diffusion = _model_and_diffusion(8, P)
    assert diffusion.mode == "default"
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g)
    noises = [torch.randn(x_T.shape, generator=g) for _ in range(4)]
    it = iter([z.to(DEV) for z in noises])
    out = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), progress=False, time=4,
                                  noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    ref = od.p_sample_loop(tab, ou.OracleUNet(P, num_groups=G, **cfg), x_T, torch.zeros(1, 0, 16, 16, 16), noises,
                           time=4)
    assert rel_err(out, ref) < 1e-3


def test_one_condition_sampling_vs_oracle_fp32():
    cfg = _cfg(16)
    P = ou.random_params(seed=1, **cfg)
    model, diffusion = _model_and_diffusion(16, P)
    g = torch.Generator().manual_seed(6)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g)
    cond = torch.rand(1, 8, 16, 16, 16, generator=g)
    noises = [torch.randn(x_T.shape, generator=g) for _ in range(4)]
    it = iter([z.to(DEV) for z in noises])
    out = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), progress=False, time=4,
                                  noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    ref = od.p_sample_loop(tab, ou.OracleUNet(P, num_groups=G, **cfg), x_T, cond, noises, time=4)
    assert rel_err(out, ref) < 1e-3
    with pytest.raises(AssertionError, match="model expects 16 input channels, got 8 \\+ 16"):
        diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=torch.cat([cond, cond], 1).to(DEV),
                                progress=False, time=4)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_unconditional_hip_graph_loop_equals_eager_loop(dtype):
    """The graph-captured step (the staging copy is one more captured launch) replays to the eager loop's bits:
    5 steps, Philox noise in the sampler kernel."""
    P = ou.random_params(seed=1, **_cfg(8))
    model, diffusion = _model_and_diffusion(8, P, dtype, diffusion_steps=50)
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g).to(DEV)
    diffusion.native_noise = "philox"

    def run(graph):
        diffusion.use_hip_graph = graph
        torch.manual_seed(11)
        return [o["sample"] for o in diffusion.p_sample_loop_progressive(model, x_T.shape, noise=x_T, time=5,
                                                                        progress=False)]

    eager, graph = run(False), run(True)
    diffusion.use_hip_graph = False
    assert len(eager) == len(graph) == 5
    for a, b in zip(eager, graph):
        assert torch.isfinite(a).all() and torch.equal(a, b), rel_err(b, a)


# --------------------------------------------------------------------------- 6. training
@pytest.mark.parametrize("n", [0, 1, 2])
def test_training_losses_vs_restatement_fp32(n):
    """mode='default' (n = 0) and the generic {"target", "cond"} dict with 1 and 2 conditions."""
    cin = 8 + 8 * n
    cfg = _cfg(cin)
    P = ou.random_params(seed=1, **cfg)
    model, diffusion = _model_and_diffusion(cin, P)
    g = torch.Generator().manual_seed(4 + n)
    vols = [torch.rand(2, 1, 32, 32, 32, generator=g) for _ in range(1 + n)]
    noise = torch.randn(2, 1, 32, 32, 32, generator=g)
    t = torch.tensor([5, 700])
    dv = [v.to(DEV) for v in vols]
    with torch.no_grad():
        if n == 0:
            terms, out, out_idwt = diffusion.training_losses(model, dv[0], t.to(DEV), mode="default",
                                                             noise=noise.to(DEV))
        else:
            terms, out, out_idwt = diffusion.training_losses(model, {"target": dv[0], "cond": dv[1:]}, t.to(DEV),
                                                             mode="i2i", contr="ignored", noise=noise.to(DEV))
    tab = od.Tables(od.beta_schedule("linear", 1000, "direct"))
    rterms, rout, ridwt = cco.training_losses(tab, ou.OracleUNet(P, num_groups=G, **cfg), vols[0], vols[1:], t, noise)
    assert terms["mse_wav"].shape == (8,)
    assert rel_err(out, rout) < 1e-3
    assert rel_err(out_idwt, ridwt) < 1e-3
    assert rel_err(terms["mse_wav"], rterms["mse_wav"]) < 1e-3


def test_training_losses_wrong_condition_count():
    P = ou.random_params(seed=1, **_cfg(16))
    model, diffusion = _model_and_diffusion(16, P)
    v = torch.rand(1, 1, 16, 16, 16, device=DEV)
    t = torch.tensor([5], device=DEV)
    with pytest.raises(AssertionError, match="model expects 16 input channels, got 8 \\+ 0"):
        diffusion.training_losses(model, v, t, mode="default")
    with pytest.raises(AssertionError, match="model expects 16 input channels, got 8 \\+ 16"):
        diffusion.training_losses(model, {"target": v, "cond": [v, v]}, t, mode="i2i")
    d2 = _diffusion(wavelet_levels=2)
    with pytest.raises(NotImplementedError, match="three conditions"):
        d2.training_losses(model, {"target": v, "cond": [v]}, t, mode="i2i")


def test_trainloop_default_mode_two_steps_repeatable(tmp_path, monkeypatch):
    """TrainLoop.run_loop with mode='default' on tensor batches (in_channels=8, bf16, 32^3 images): two steps,
    twice under the same seeds, bitwise equal parameters that moved."""
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = ou.random_params(seed=41, **_cfg(8))
    batch = torch.rand(1, 1, 32, 32, 32, generator=torch.Generator().manual_seed(5))

    def run():
        model, diffusion = _model_and_diffusion(8, P, "bf16")
        loop = train_util.TrainLoop(model=model, diffusion=diffusion, data=[batch], batch_size=1, in_channels=8,
                                    image_size=32, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=100,
                                    contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0,
                                    lr_anneal_steps=3, mode="default", diffusion_steps=1000)
        torch.manual_seed(0)
        np.random.seed(0)
        loop.run_loop()
        torch.cuda.synchronize()
        assert loop.step == 3    # two steps ran
        return {n: q.detach().cpu().clone() for n, q in model.named_parameters()}

    try:
        p_a, p_b = run(), run()
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    for n in p_a:
        assert torch.isfinite(p_a[n]).all(), n
        assert torch.equal(p_a[n], p_b[n]), n
    assert any(not torch.equal(p_a[n], P[n]) for n in p_a)


def test_trainloop_generic_condition_dict_runs(tmp_path, monkeypatch):
    """The batch-size lookup and the device move of run_loop take {"target", "cond": [...]} batches."""
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = ou.random_params(seed=42, **_cfg(24))
    g = torch.Generator().manual_seed(6)
    batch = {"target": torch.rand(1, 1, 32, 32, 32, generator=g),
             "cond": [torch.rand(1, 1, 32, 32, 32, generator=g) for _ in range(2)]}
    model, diffusion = _model_and_diffusion(24, P, "bf16")
    loop = train_util.TrainLoop(model=model, diffusion=diffusion, data=[batch], batch_size=1, in_channels=24,
                                image_size=32, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=100,
                                contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0,
                                lr_anneal_steps=2, mode="i2i", diffusion_steps=1000)
    try:
        loop.run_loop()
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert loop.step == 2
    assert torch.isfinite(model.flat_params).all()
    assert float(loop.last_info["norm/grad_max"]) > 0
    assert any(not torch.equal(p.detach().cpu(), P[n]) for n, p in model.named_parameters())
