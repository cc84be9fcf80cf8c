"""Class conditioning on the GPU: UNetModel(num_classes=4) on the tiny U-Net
(oracle.cases.C1_CFG, subband edge 16) against the CPU fp32 restatement
(tests/class_cond_oracle.py) and autograd on it -- forward, backward (the
table's gradient: a deterministic reduction over the batch), the other model
switches, the native sampling loops, the out-of-range rule and TrainLoop.

Batches: t = [3, 917] with y = [2, 0], and B = 3 with t = [3, 917, 500],
y = [1, 3, 1]: class 1 twice (the gradient kernel sums two rows), classes 0
and 2 absent (their rows must be written as exact zeros).

Caps: those of tests/test_gpu_attention.py for the same model, 1e-3 / 6e-2 /
1e-2 relative for the forward and 1e-3 / 8e-2 / 1.5e-2 rel-L2 per parameter
for the gradients (fp32 / bf16 / fp16)."""
import numpy as np
import pytest
import torch

import class_cond_oracle as cco
from oracle import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG, G, NC, EDGE = cases.C1_CFG, cases.C1_GROUPS, 4, 16
FWD_TOL = {"fp32": 1e-3, "bf16": 6e-2, "fp16": 1e-2}
BWD_TOL = {"fp32": 1e-3, "bf16": 8e-2, "fp16": 1.5e-2}
BATCHES = {"b2": ([3, 917], [2, 0]), "b3": ([3, 917, 500], [1, 3, 1])}
LABEL = cco.LABEL


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _model(params, dtype="fp32", num_classes=NC, **opts):
    from guided_diffusion.unet import UNetModel
    opts.setdefault("bottleneck_attention", False)
    m = UNetModel(image_size=32, in_channels=CFG["in_channels"], model_channels=CFG["model_channels"],
                  out_channels=CFG["out_channels"], num_res_blocks=CFG["num_res_blocks"], attention_resolutions=(),
                  channel_mult=CFG["channel_mult"], dims=3, resblock_updown=True, resample_2d=False, num_groups=G,
                  num_classes=num_classes, compute_dtype=dtype, **opts)
    m.load_state_dict(params)
    return m.to(DEV)


_CASES = {}


def _case(batch, **opts):
    """Inputs, weights and the restatement's output and autograd gradients, computed once and never written."""
    key = (batch, tuple(sorted(opts.items())))
    if key not in _CASES:
        ts, ys = BATCHES[batch]
        B = len(ts)
        P = cco.random_params(NC, seed=1, **CFG, **opts)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(B, 32, EDGE, EDGE, EDGE, generator=g)
        R = torch.randn(B, 8, EDGE, EDGE, EDGE, generator=g)
        t, y = torch.tensor(ts), torch.tensor(ys)
        ref_out, ref_grads = cco.grads(CFG, G, P, x, t, y, R, **opts)
        _CASES[key] = dict(P=P, x=x, t=t, y=y, R=R, ref_out=ref_out, ref_grads=ref_grads, opts=opts)
    return _CASES[key]


def _forward(model, c, y=None):
    with torch.no_grad():
        return model(c["x"].to(DEV), c["t"].to(DEV), (c["y"] if y is None else y).to(DEV)).cpu()


def _grads(c, dtype, hook=None):
    model = _model(c["P"], dtype, **c["opts"])
    model._grad_hook = hook
    out = model(c["x"].to(DEV), c["t"].to(DEV), c["y"].to(DEV))
    (out * c["R"].to(DEV)).sum().backward()
    return out.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}, model


# --------------------------------------------------------------------------- forward
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_forward_vs_restatement(dtype, batch):
    c = _case(batch)
    out = _forward(_model(c["P"], dtype), c)
    assert out.shape == c["ref_out"].shape
    print(dtype, batch, "forward rel", rel_err(out, c["ref_out"]))
    assert torch.isfinite(out).all()
    assert rel_err(out, c["ref_out"]) < FWD_TOL[dtype]


def test_labels_matter():
    """y = [2, 0] and y = [0, 2] give different outputs (by more than the fp32 cap), each the restatement's."""
    c = _case("b2")
    model = _model(c["P"], "fp32")
    y2 = torch.tensor([0, 2])
    a, b = _forward(model, c), _forward(model, c, y2)
    with torch.no_grad():
        ref_b = cco.unet_forward(c["P"], c["x"], c["t"], y2, num_groups=G, **CFG)
    print("labels swapped: rel", rel_err(b, a), "vs restatement", rel_err(a, c["ref_out"]), rel_err(b, ref_b))
    assert rel_err(a, c["ref_out"]) < 1e-3 and rel_err(b, ref_b) < 1e-3
    assert rel_err(b, a) > 1e-3
    # a host y and a device y, int32 or int64: the same bits
    assert torch.equal(_forward(model, c, c["y"].to(torch.int32)), a)
    with torch.no_grad():
        assert torch.equal(model(c["x"].to(DEV), c["t"].to(DEV), c["y"]).cpu(), a)


def test_zero_row_is_the_plain_model_bit_for_bit():
    """Row 2 of the table = +0.0 and y = [2, 2]: adding +0.0 is exact, so the fp32 forward equals the forward of
    a num_classes=None model with the same remaining weights, bit for bit -- nothing else moved."""
    c = _case("b2")
    P = {k: v.clone() for k, v in c["P"].items()}
    P[LABEL][2] = 0.0
    y = torch.tensor([2, 2])
    a = _forward(_model(P, "fp32"), c, y)
    plain = _model({k: v for k, v in P.items() if k != LABEL}, "fp32", num_classes=None)
    with torch.no_grad():
        b = plain(c["x"].to(DEV), c["t"].to(DEV)).cpu()
    assert torch.equal(a, b)
    assert not torch.equal(_forward(_model(P, "fp32"), c, torch.tensor([2, 1])), b)


# --------------------------------------------------------------------------- backward
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_backward_vs_autograd(dtype, batch):
    c = _case(batch)
    tol = BWD_TOL[dtype]
    out, grads, model = _grads(c, dtype)
    assert rel_err(out, c["ref_out"]) < FWD_TOL[dtype]
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print(dtype, batch, "worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    print(dtype, batch, "label_emb.weight grad rel-L2", worst[LABEL])
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert float(ref[LABEL].abs().max()) > 0
    used = sorted(set(c["y"].tolist()))
    for cls in range(NC):
        row = grads[LABEL][cls]
        if cls in used:
            assert float(row.abs().max()) > 0, cls
        else:   # written, as exact zeros (the flat buffer is not relied on to be zero there)
            assert torch.equal(row, torch.zeros_like(row)), cls
    assert model.flat_grad().numel() == sum(v.numel() for v in c["P"].values())
    # a second run: the same bits, every parameter
    _, again, _ = _grads(c, dtype)
    for k in grads:
        assert torch.equal(grads[k], again[k]), k


def test_backward_segments_and_hook():
    """Segment-wise backward with a hook: every segment once, each flat element covered once, the gradients of
    the one-call backward (the labels are set again before each segment)."""
    c = _case("b3")
    _, g_all, _ = _grads(c, "fp32")
    seen = []

    def hook(seg, flat, off, n):
        if seg is not None:
            seen.append((seg, off, n))
    _, g_seg, model = _grads(c, "fp32", hook=hook)
    n = sum(p.numel() for p in model.parameters())
    assert [s[0] for s in seen] == list(range(model.plan.num_segments))
    cover = torch.zeros(n, dtype=torch.int32)
    for _, off, cnt in seen:
        cover[off:off + cnt] += 1
    assert bool((cover == 1).all())
    for name in g_all:
        assert torch.equal(g_seg[name], g_all[name]), name


# --------------------------------------------------------------------------- with the other switches
@pytest.mark.parametrize("switch", ["use_scale_shift_norm", "bottleneck_attention", "additive_skips"])
def test_with_other_switches_fp32(switch):
    c = _case("b3", **{switch: True})
    out, grads, _ = _grads(c, "fp32")
    print(switch, "forward rel", rel_err(out, c["ref_out"]))
    assert rel_err(out, c["ref_out"]) < FWD_TOL["fp32"]
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print(switch, "worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:4], "label", worst[LABEL])
    bad = {k: v for k, v in worst.items() if v > BWD_TOL["fp32"]}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    for cls in (0, 2):
        assert not grads[LABEL][cls].any()


def test_with_dropout_same_seed_same_labels_same_bits():
    c = _case("b2")
    model = _model(c["P"], "bf16", dropout=0.1)
    model.eval()
    plain = _forward(model, c)
    model.train()
    model.dropout_seed = 7
    a, b = _forward(model, c), _forward(model, c)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(a, plain)                                   # it dropped
    assert not torch.equal(_forward(model, c, torch.tensor([0, 2])), a)   # and the twin plan reads the labels
    # training: forward + backward twice, the same gradient bits
    def step():
        for p in model.parameters():
            p.grad = None
        out = model(c["x"].to(DEV), c["t"].to(DEV), c["y"].to(DEV))
        (out * c["R"].to(DEV)).sum().backward()
        return model.flat_grad().detach().cpu().clone()
    g1, g2 = step(), step()
    assert torch.equal(g1, g2) and float(g1.abs().max()) > 0


# --------------------------------------------------------------------------- sampling
def _diffusion(steps=50, respacing="", schedule="direct"):
    from guided_diffusion import script_util
    return script_util.create_gaussian_diffusion(steps=steps, predict_xstart=True, timestep_respacing=respacing,
                                                 mode="i2i", sample_schedule=schedule)


def _sampling_inputs(B=2):
    g = torch.Generator().manual_seed(5)
    cond = torch.rand(B, 24, EDGE, EDGE, EDGE, generator=g).to(DEV)
    x_T = torch.randn(B, 8, EDGE, EDGE, EDGE, generator=g).to(DEV)
    return cond, x_T


@pytest.mark.parametrize("respacing,dtype", [("", "fp32"), ("ddim10", "bf16")])
def test_hip_graph_loop_equals_eager_loop(respacing, dtype):
    c = _case("b2")
    model = _model(c["P"], dtype)
    diffusion = _diffusion(respacing=respacing)
    cond, x_T = _sampling_inputs()
    diffusion.native_noise = "philox"
    y = c["y"].to(DEV)
    called = []
    native = diffusion._native_loop
    diffusion._native_loop = lambda *a, **k: (called.append(k.get("y")), native(*a, **k))[1]

    def run(graph, labels):
        diffusion.use_hip_graph = graph
        torch.manual_seed(11)
        return [o["sample"] for o in diffusion.p_sample_loop_progressive(model, x_T.shape, noise=x_T, cond=cond, time=3,
                                                                        progress=False, model_kwargs={"y": labels})]

    eager, graph = run(False, y), run(True, y)
    other = run(True, torch.tensor([0, 2], device=DEV))
    diffusion.use_hip_graph = False
    assert len(called) == 3 and all(v is not None for v in called)     # the native loop, with the labels
    assert len(eager) == len(graph) == 3
    for a, b in zip(eager, graph):
        assert torch.equal(a, b), rel_err(b, a)
    assert torch.isfinite(eager[-1]).all()
    assert not torch.equal(other[-1], graph[-1])                       # the captured step reads the labels


def test_native_loop_vs_generic_loop_fp32():
    c = _case("b2")
    model = _model(c["P"], "fp32")
    diffusion = _diffusion(steps=6, schedule="sampled")
    diffusion.native_noise = "torch"
    cond, x_T = _sampling_inputs()
    g = torch.Generator().manual_seed(9)
    noises = [torch.randn(x_T.shape, generator=g).to(DEV) for _ in range(3)]
    kw = {"y": c["y"].to(DEV)}
    it = iter(noises)
    native = diffusion.p_sample_loop(model, x_T.shape, noise=x_T, cond=cond, time=3, progress=False,
                                     noise_fn=lambda x: next(it), model_kwargs=kw)
    it2 = iter(noises)
    steps = list(diffusion._generic_loop(model, x_T, [2, 1, 0], x_T.shape[0], DEV, True, None, None, kw, cond,
                                         lambda x: next(it2), 0, 0.0))
    generic = steps[-1]["sample"]
    print("native vs generic loop rel", rel_err(native, generic))
    assert torch.isfinite(native).all()
    assert rel_err(native, generic) < 1e-3
    # and the labels reach it: other labels, another sample
    it3 = iter(noises)
    other = diffusion.p_sample_loop(model, x_T.shape, noise=x_T, cond=cond, time=3, progress=False,
                                    noise_fn=lambda x: next(it3), model_kwargs={"y": torch.tensor([0, 2])})
    assert rel_err(other, native) > 1e-3


def test_unknown_model_kwargs_key_takes_the_generic_loop():
    c = _case("b2")
    model = _model(c["P"], "fp32")
    diffusion = _diffusion()
    cond, x_T = _sampling_inputs()
    took = []
    diffusion._native_loop = lambda *a, **k: (took.append("native"), iter(()))[1]
    diffusion._generic_loop = lambda *a, **k: (took.append("generic"), iter(()))[1]
    run = lambda kw: list(diffusion.p_sample_loop_progressive(model, x_T.shape, noise=x_T, cond=cond, time=3,
                                                              progress=False, model_kwargs=kw))
    run({"y": c["y"].to(DEV), "scale": 2.0})
    run({"labels": c["y"].to(DEV)})
    run({"y": c["y"].to(DEV)})
    assert took == ["generic", "generic", "native"]
    plain = _model({k: v for k, v in c["P"].items() if k != LABEL}, "fp32", num_classes=None)
    took.clear()
    list(diffusion.p_sample_loop_progressive(plain, x_T.shape, noise=x_T, cond=cond, time=3, progress=False,
                                             model_kwargs={"y": c["y"].to(DEV)}))
    list(diffusion.p_sample_loop_progressive(plain, x_T.shape, noise=x_T, cond=cond, time=3, progress=False))
    assert took == ["generic", "native"]


# --------------------------------------------------------------------------- out-of-range labels
def test_host_label_out_of_range_raises_before_launch():
    c = _case("b2")
    model = _model(c["P"], "fp32")
    for bad in ([4, 0], [0, -1]):
        with pytest.raises(IndexError, match="Labels out of bounds"):
            model(c["x"].to(DEV), c["t"].to(DEV), torch.tensor(bad))
    with pytest.raises(AssertionError, match="y must have shape"):
        model(c["x"].to(DEV), c["t"].to(DEV), torch.tensor([1, 0, 1]))
    from cwdm_hip import _lib
    assert _lib.lib().cwdm_device_status(0) == 0


def test_device_label_out_of_range_sets_the_device_error_word():
    """A device y is not read back.  The kernel compares the label with num_classes before it forms any address
    (no fault by construction): it adds nothing for that sample -- the output is the restatement's with an
    all-zero row for it -- and raises CWDM_DEV_E_LABEL, which reads once and is clear afterwards."""
    from cwdm_hip import _lib
    c = _case("b2")
    model = _model(c["P"], "fp32")
    L = _lib.lib()
    assert L.cwdm_device_status(1) >= 0 and L.cwdm_device_status(0) == 0
    out = _forward(model, c, torch.tensor([4, 0], device=DEV))
    st = L.cwdm_device_status(1)
    assert st >= 0 and st & _lib.DEV_E_LABEL
    assert L.cwdm_device_status(0) == 0
    assert torch.isfinite(out).all()
    P5 = dict(c["P"])
    P5[LABEL] = torch.cat([c["P"][LABEL], torch.zeros(1, c["P"][LABEL].shape[1])])
    with torch.no_grad():
        ref = cco.unet_forward(P5, c["x"], c["t"], torch.tensor([4, 0]), num_groups=G, **CFG)
    assert rel_err(out, ref) < 1e-3
    # a good forward afterwards leaves the word clear
    assert rel_err(_forward(model, c), c["ref_out"]) < 1e-3
    assert L.cwdm_device_status(0) == 0


def test_plan_without_labels_is_refused():
    from cwdm_hip.unet_runtime import UNetPlan
    c = _case("b2")
    model = _model(c["P"], "fp32")
    plan = UNetPlan(32, 32, 8, 1, (1, 2), G, "fp32", num_classes=NC)      # a fresh plan: no labels yet
    xin = torch.zeros(2, EDGE, EDGE, EDGE, 32, device=DEV)
    out = torch.empty(2, EDGE, EDGE, EDGE, 8, device=DEV)
    with pytest.raises(ValueError, match="needs its labels"):
        plan.forward(model.packed_weights(), xin, c["t"].float().to(DEV), out, 2, EDGE, EDGE, EDGE)
    with pytest.raises(ValueError, match="int64"):
        plan.set_labels(torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="no classes"):
        _model({k: v for k, v in c["P"].items() if k != LABEL}, "fp32", num_classes=None).plan.set_labels(
            torch.zeros(2, dtype=torch.int64, device=DEV))


# --------------------------------------------------------------------------- TrainLoop, checkpoint
def test_trainloop_two_steps_repeatable_and_checkpoint_round_trip(tmp_path, monkeypatch):
    """TrainLoop.run_loop on {"target", "cond", "y"} batches (bf16, 32^3 images): the "y" key becomes the step's
    model_kwargs; two steps, twice under the same seeds, bitwise equal parameters; the table moved.  Then a
    saved and reloaded state_dict gives the same forward bits."""
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = cco.random_params(NC, seed=41, **CFG)
    g = torch.Generator().manual_seed(5)
    vols = [torch.rand(2, 1, 32, 32, 32, generator=g) for _ in range(4)]
    batch = {"target": vols[0], "cond": vols[1:], "y": torch.tensor([3, 1])}

    def run():
        model = _model(P, "bf16")
        diffusion = _diffusion(steps=1000)
        loop = train_util.TrainLoop(model=model, diffusion=diffusion, data=[batch], batch_size=2, in_channels=32,
                                    image_size=32, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=100,
                                    contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0,
                                    lr_anneal_steps=3, mode="i2i", diffusion_steps=1000)
        torch.manual_seed(0)
        np.random.seed(0)
        loop.run_loop()
        torch.cuda.synchronize()
        assert loop.step == 3
        return {n: q.detach().cpu().clone() for n, q in model.named_parameters()}, model

    try:
        (p_a, model), (p_b, _) = run(), run()
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert set(batch) == {"target", "cond", "y"}      # the loader's dict is left as it was
    for n in p_a:
        assert torch.isfinite(p_a[n]).all(), n
        assert torch.equal(p_a[n], p_b[n]), n
    moved = ~(p_a[LABEL] == P[LABEL]).all(dim=1)
    assert moved.tolist() == [False, True, False, True]     # the rows of the classes in the batch, no others
    c = _case("b2")
    a = _forward(model, c)
    path = tmp_path / "model.pt"
    torch.save(model.state_dict(), path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd)[4] == LABEL
    assert torch.equal(_forward(_model(sd, "bf16"), c), a)
