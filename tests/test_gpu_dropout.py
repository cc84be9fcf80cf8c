"""dropout > 0 on the GPU: the two kernels (cwdm_gn_silu_dropout, cwdm_dropout_bwd) against the restated
Philox mask (tests/dropout_oracle.py), then the tiny U-Net in training mode -- forward and every parameter
gradient against the CPU fp32 restatement with the same masks -- and the rules around it: eval() is the
dropout=0 model bit for bit, train() drops without grad too, forwards and backwards interleave, the sampling
loop never drops, TrainLoop is repeatable under torch.manual_seed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_oracle as dro
import scale_shift_oracle as sso
from oracle import cases
from oracle import unet as ou

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x5DEECE66D1234567 & (2 ** 62 - 1)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _dt(name):
    from cwdm_hip import _lib
    return {"fp32": (_lib.CWDM_F32, torch.float32), "bf16": (_lib.CWDM_BF16, torch.bfloat16),
            "fp16": (_lib.CWDM_F16, torch.float16)}[name]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# --------------------------------------------------------------------------- 1. the kernels
PAD, FILL = 64, 7.0


def _guarded(n, tdt):
    """A device buffer of n elements between two guards of PAD elements (16-byte aligned either way)."""
    buf = torch.full((n + 2 * PAD,), FILL, dtype=tdt, device=DEV)
    return buf, buf[PAD:PAD + n]


def _guards_intact(buf):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[-PAD:] == FILL).all())


_MASKS = {}


def _mask(seed, site, B, V, C, p):
    key = (seed, site, B, V, C, p)
    if key not in _MASKS:
        _MASKS[key] = torch.from_numpy(dro.keep_mask(seed, site, B, V, C, p))
    return _MASKS[key]


def _fwd(L, x, ss, dt, tdt, B, V, C, p, seed, site):
    from cwdm_hip._lib import check
    buf, out = _guarded(B * V * C, tdt)
    check(L.cwdm_gn_silu_dropout(x.data_ptr(), ss.data_ptr(), out.data_ptr(), dt, B, V, C, p, seed, site, None))
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    return out.view(B, V, C).cpu()


# (2, 27, 32): a tail of the 4-voxel slots; (1, 70000, 8): voxel indices past 16 bits; (2, 512, 256): 64 channel
# groups of 4 (the counter's low half-word) and several workgroups per batch entry
SHAPES = [(2, 27, 32), (3, 1000, 64), (1, 70000, 8), (2, 512, 256)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,V,C", SHAPES)
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
def test_dropout_kernels_vs_oracle(dtype_name, B, V, C, p):
    from cwdm_hip._lib import check, lib
    L = lib()
    dt, tdt = _dt(dtype_name)
    site = 5
    g = torch.Generator().manual_seed(1000 * C + V)
    # |x scale + shift| in [0.3, 3.5] before x is rounded to the storage dtype, so in [0.25, 4] after: no kept
    # output is zero, in any dtype
    y = (0.3 + 3.2 * torch.rand(B, V, C, generator=g)) * (torch.randint(0, 2, (B, V, C), generator=g) * 2 - 1)
    sc = (0.5 + 1.5 * torch.rand(B, C, generator=g)) * (torch.randint(0, 2, (B, C), generator=g) * 2 - 1)
    sh = 0.2 * torch.randn(B, C, generator=g)
    x = ((y - sh[:, None]) / sc[:, None]).to(tdt)
    yq = x.float() * sc[:, None] + sh[:, None]
    assert 0.25 <= float(yq.abs().min()) and float(yq.abs().max()) <= 4.0
    ss = torch.stack([sc, sh], -1).contiguous().to(DEV)
    xd = x.to(DEV)
    inv = torch.tensor(float(dro.inv_keep(p)), dtype=torch.float32)
    mask = _mask(SEED, site, B, V, C, p)

    # ---- forward: the zero pattern is the mask, every element; kept values against SiLU * inv in fp32
    out = _fwd(L, xd, ss, dt, tdt, B, V, C, p, SEED, site)
    assert torch.equal(out != 0, mask)
    ref = torch.where(mask, F.silu(yq) * inv, torch.zeros(()))
    a, b = out.float(), ref
    if dtype_name == "fp32":
        err = rel_err(a, b)
        print("gn_silu_dropout", dtype_name, (B, V, C), p, "rel", err, "kept", float(mask.float().mean()))
        assert err < 1e-5
    else:
        ulp = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}[dtype_name]
        worst = float(((a - b).abs() / b.abs().clamp_min(1e-6)).max())
        print("gn_silu_dropout", dtype_name, (B, V, C), p, "worst rel", worst, "kept", float(mask.float().mean()))
        assert torch.all((a - b).abs() <= ulp * b.abs() + 1e-6), float((a - b).abs().max())
    # a second call: the same bits; another seed, another site: another mask
    assert torch.equal(_bits(_fwd(L, xd, ss, dt, tdt, B, V, C, p, SEED, site)), _bits(out))
    o_seed = _fwd(L, xd, ss, dt, tdt, B, V, C, p, SEED + 1, site)
    o_site = _fwd(L, xd, ss, dt, tdt, B, V, C, p, SEED, site + 1)
    assert torch.equal(o_seed != 0, _mask(SEED + 1, site, B, V, C, p)) and not torch.equal(o_seed != 0, mask)
    assert torch.equal(o_site != 0, _mask(SEED, site + 1, B, V, C, p)) and not torch.equal(o_site != 0, mask)

    # ---- backward, in place: an fp32 multiply and one round-to-nearest-even conversion, bit for bit
    du = torch.randn(B, V, C, generator=g).to(tdt)
    want = torch.where(mask, (du.float() * inv).to(tdt), torch.zeros((), dtype=tdt))
    buf, dud = _guarded(B * V * C, tdt)
    for rep in range(2):
        dud.copy_(du.reshape(-1))
        check(L.cwdm_dropout_bwd(dud.data_ptr(), dt, B, V, C, p, SEED, site, None))
        torch.cuda.synchronize()
        assert _guards_intact(buf)
        assert torch.equal(_bits(dud.view(B, V, C).cpu()), _bits(want)), rep


def test_dropout_kernels_refusals():
    from cwdm_hip import _lib
    from cwdm_hip._lib import lib
    L = lib()
    x = torch.zeros(2 * 16 * 16, device=DEV)
    ss = torch.zeros(2 * 16 * 2, device=DEV)
    args = (_lib.CWDM_F32, 2, 16)
    assert L.cwdm_gn_silu_dropout(x.data_ptr(), ss.data_ptr(), x.data_ptr(), *args, 12, 0.1, 1, 0, None) == \
        _lib.E_UNSUPPORTED
    assert L.cwdm_dropout_bwd(x.data_ptr(), *args, 12, 0.1, 1, 0, None) == _lib.E_UNSUPPORTED
    assert L.cwdm_dropout_bwd(x.data_ptr(), _lib.CWDM_F32, 65536, 1, 8, 0.1, 1, 0, None) == _lib.E_UNSUPPORTED
    for p in (-0.1, 1.0):
        assert L.cwdm_dropout_bwd(x.data_ptr(), *args, 16, p, 1, 0, None) == _lib.E_INVALID
    assert L.cwdm_dropout_bwd(x.data_ptr() + 4, *args, 16, 0.1, 1, 0, None) == _lib.E_INVALID   # not 16-byte aligned
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# --------------------------------------------------------------------------- 2. the tiny U-Net
VARIANTS = {
    "plain": dict(),
    "film": dict(use_scale_shift_norm=True),
    "no-updown": dict(resblock_updown=False),
}
CFG, G = cases.C1_CFG, cases.C1_GROUPS


def _product_model(params, dtype, p, **opts):
    from guided_diffusion.unet import UNetModel
    opts = dict(opts)
    opts.setdefault("resblock_updown", True)
    m = UNetModel(image_size=32, in_channels=CFG["in_channels"], model_channels=CFG["model_channels"],
                  out_channels=CFG["out_channels"], num_res_blocks=CFG["num_res_blocks"], attention_resolutions=(),
                  channel_mult=CFG["channel_mult"], dims=3, resample_2d=False, num_groups=G,
                  bottleneck_attention=False, compute_dtype=dtype, dropout=p, **opts)
    m.load_state_dict(params)
    return m.to(DEV)


def _params(variant):
    if variant == "film":
        return sso.random_params(seed=1, **CFG)
    return ou.random_params(seed=1, **{**CFG, **{k: v for k, v in VARIANTS[variant].items() if k == "resblock_updown"}})


_TINY = {}


def _tiny_case(variant, p, n=16):
    """x (2, 32, n^3), t [3, 917]: the restatement's training forward and autograd gradients with the masks of
    SEED, once per (variant, p, grid)."""
    key = (variant, p, n)
    if key not in _TINY:
        P = _params(variant)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 32, n, n, n, generator=g)
        t = torch.tensor([3, 917])
        R = torch.randn(2, 8, n, n, n, generator=g)
        opts = {k: v for k, v in VARIANTS[variant].items() if k == "resblock_updown"}
        kept = []
        ref_out, ref_grads = dro.grads({**CFG, **opts}, G, P, x, t, R, p, SEED, film=variant == "film", kept=kept)
        # not vacuous: every site drops about p of its elements, and out_layers.3 is not the reference's zero init
        assert len(kept) == sum(1 for b in ou.topology(**{**CFG, **opts}) if b["kind"] == "res")
        assert all(abs(k - (1 - p)) < 0.02 for k in kept), kept
        assert all(float(v.abs().max()) > 0 for k, v in P.items() if ".out_layers.3." in k)
        _TINY[key] = dict(P=P, x=x, t=t, R=R, ref_out=ref_out, ref_grads=ref_grads)
    return _TINY[key]


def _train_grads(model, c, seed=SEED, hook=None):
    model.train()
    model.dropout_seed = seed
    model._grad_hook = hook
    for q in model.parameters():
        q.grad = None
    out = model(c["x"].to(DEV), c["t"].to(DEV))
    (out * c["R"].to(DEV)).sum().backward()
    assert model.last_dropout_seed == seed
    return out.detach().cpu(), {n: q.grad.detach().cpu().clone() for n, q in model.named_parameters()}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype,ftol,btol", [("fp32", 1e-3, 1e-3), ("bf16", 6e-2, 8e-2), ("fp16", 1e-2, 1.5e-2)])
def test_tiny_unet_train_forward_backward(dtype, ftol, btol, variant, p):
    c = _tiny_case(variant, p)
    model = _product_model(c["P"], dtype, p, **VARIANTS[variant])
    out, grads = _train_grads(model, c)
    ferr = rel_err(out, c["ref_out"])
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print("tiny dropout", variant, dtype, p, "forward rel", ferr, "worst grads",
          sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert ferr < ftol
    bad = {k: v for k, v in worst.items() if v > btol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_tiny_unet_train_14_cubed_fp32():
    """A grid that is no multiple of the conv tiles (14^3, 7^3 below)."""
    c = _tiny_case("plain", 0.1, n=14)
    model = _product_model(c["P"], "fp32", 0.1)
    out, grads = _train_grads(model, c)
    worst = {k: _rel_l2(grads[k], c["ref_grads"][k]) for k in grads}
    print("tiny dropout 14^3 forward rel", rel_err(out, c["ref_out"]), "worst grad", max(worst.values()))
    assert rel_err(out, c["ref_out"]) < 1e-3
    assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_is_the_dropout0_model_bitwise_and_train_drops_without_grad(dtype):
    c = _tiny_case("plain", 0.5)
    model, plain = _product_model(c["P"], dtype, 0.5), _product_model(c["P"], dtype, 0)
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    with torch.no_grad():
        ev = model.eval()(x, t)
        ev0 = plain.eval()(x, t)
        tr0 = plain.train()(x, t)     # dropout = 0: training mode changes nothing
        model.train()
        model.dropout_seed = SEED
        tr = model(x, t)
        assert model.last_dropout_seed == SEED
        model.dropout_seed = None
        torch.manual_seed(3)
        drawn = model(x, t)
        torch.manual_seed(3)
        assert int(torch.randint(0, 2 ** 62, (1,)).item()) == model.last_dropout_seed
    assert torch.equal(ev, ev0) and torch.equal(tr0, ev0)
    # eval() with grad: still the plain model's bits
    assert torch.equal(model.eval()(x, t).detach(), ev0)
    tol = 1e-3 if dtype == "fp32" else 6e-2
    print("train no_grad", dtype, "rel", rel_err(tr, c["ref_out"]), "vs eval", rel_err(tr, ev))
    assert rel_err(tr, c["ref_out"]) < tol
    assert rel_err(tr, ev) > 0.05 and rel_err(drawn, tr) > 0.05


def test_packed_layouts_of_the_two_plans_are_identical():
    """UNetModel shares one packed-weight cache between its plans: both plans write the same bytes."""
    c = _tiny_case("plain", 0.5)
    for dtype in ("fp32", "bf16"):
        model = _product_model(c["P"], dtype, 0.5)
        off, on = model._plan(dtype), model._plan(dtype, drop=True)
        params = model.param_list()
        assert off.packed_bytes == on.packed_bytes and off.packed_bwd_bytes == on.packed_bwd_bytes
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device=DEV)   # noqa: E731
        assert torch.equal(off.pack(params, packed=z(off.packed_bytes)), on.pack(params, packed=z(on.packed_bytes)))
        assert torch.equal(off.pack_bwd(params, packed_bwd=z(off.packed_bwd_bytes)),
                           on.pack_bwd(params, packed_bwd=z(on.packed_bwd_bytes)))


def test_forwards_and_backwards_interleave():
    """forward A, forward B, backward B, backward A == A and B run alone, bitwise (each autograd node hands its
    own seed to the plan before its backward)."""
    c = _tiny_case("plain", 0.5)
    model = _product_model(c["P"], "fp32", 0.5).train()
    x, t, R = c["x"].to(DEV), c["t"].to(DEV), c["R"].to(DEV)
    params = list(model.parameters())

    def fwd(seed):
        model.dropout_seed = seed
        return model(x, t)

    def bwd(out):
        return [g.clone() for g in torch.autograd.grad((out * R).sum(), params)]
    alone = {s: bwd(fwd(s)) for s in (111, 222)}
    assert not torch.equal(alone[111][0], alone[222][0])
    oa, ob = fwd(111), fwd(222)
    gb = bwd(ob)
    ga = bwd(oa)
    for got, want in ((ga, alone[111]), (gb, alone[222])):
        assert all(torch.equal(u, v) for u, v in zip(got, want))


def test_segmentwise_backward_with_a_hook_equals_the_whole():
    c = _tiny_case("plain", 0.1)
    model = _product_model(c["P"], "fp32", 0.1)
    _, whole = _train_grads(model, c)
    seen = []

    def hook(seg, flat, off, n):
        if seg is not None:
            seen.append(seg)
    _, seg = _train_grads(model, c, hook=hook)
    model._grad_hook = None
    assert seen == list(range(model.plan.num_segments))
    for k in whole:
        assert torch.equal(seg[k], whole[k]), k


# --------------------------------------------------------------------------- 3. sampling and training
def _c1(dropout, dtype="fp32", **model_args):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         dropout=dropout, **model_args)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype=dtype)
    diffusion.mode = "i2i"
    return model, diffusion


def test_p_sample_loop_of_an_eval_model_equals_dropout0():
    g = torch.Generator().manual_seed(5)
    cond = torch.rand(1, 24, 16, 16, 16, generator=g).to(DEV)
    x_T = torch.randn(1, 8, 16, 16, 16, generator=g).to(DEV)
    P = ou.random_params(seed=1, **CFG)
    outs = []
    for p in (0.3, 0.0):
        model, diffusion = _c1(p, "bf16", diffusion_steps=50, sample_schedule="direct")
        assert model.dropout == p
        model.load_state_dict(P)
        model.to(DEV).eval()
        diffusion.native_noise = "philox"
        torch.manual_seed(11)
        outs.append(diffusion.p_sample_loop(model, x_T.shape, noise=x_T, cond=cond, progress=False))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_trainloop_two_steps_repeatable_under_manual_seed(tmp_path, monkeypatch):
    from guided_diffusion import dist_util, train_util
    monkeypatch.setenv("CWDM_LOGDIR", str(tmp_path))
    dist_util.setup_dist()
    P = ou.random_params(seed=41, **CFG)
    batch = cases.data.brats_batch(32, seed=5, batch=1)
    bdev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def run(p, seed=0):
        model, diffusion = _c1(p, "bf16")
        model.load_state_dict(P)
        model.to(DEV)
        loop = train_util.TrainLoop(model=model, diffusion=diffusion, data=[batch], batch_size=1, in_channels=32,
                                    image_size=64, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=100,
                                    contr="t1n", save_interval=100, resume_checkpoint="", resume_step=0,
                                    lr_anneal_steps=0, mode="i2i", diffusion_steps=1000)
        torch.manual_seed(seed)
        np.random.seed(0)
        losses, seeds = [], []
        for _ in range(2):
            loss = loop.run_step(bdev, {}, info={})[0]
            losses.append(float(loss))
            seeds.append(model.last_dropout_seed)
        torch.cuda.synchronize()
        return {n: q.detach().cpu().clone() for n, q in model.named_parameters()}, losses, seeds

    try:
        p_a, l_a, s_a = run(0.1)
        p_b, l_b, s_b = run(0.1)
        p_0, l_0, s_0 = run(0.0)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    print("trainloop dropout losses", l_a, "without", l_0, "seeds", s_a)
    assert l_a == l_b and s_a == s_b and all(np.isfinite(l_a))
    assert s_a[0] is not None and s_a[0] != s_a[1] and s_0 == [None, None]
    for n in p_a:
        assert torch.isfinite(p_a[n]).all(), n
        assert torch.equal(p_a[n], p_b[n]), n
    assert any(not torch.equal(p_a[n], p_0[n]) for n in p_a)
