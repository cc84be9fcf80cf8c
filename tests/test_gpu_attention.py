"""bottleneck_attention=True on the GPU: the attention kernels through the C ABI
(cwdm_attention_forward / _backward against float64 on the rounded inputs), the
block (cwdm_attn_linear -> attention -> cwdm_attn_linear) against the restated
block, then the U-Net forward / trace, backward, sampling, training and
checkpointing against the CPU fp32 restatement (tests/attention_oracle.py) and
autograd on it."""
import ctypes
import math

import numpy as np
import pytest
import torch

import attention_oracle as ato
from oracle import cases, diffusion as od

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# one rounding of the dtype, relative: 2^-9 (bf16: 8 significand bits), 2^-12 (fp16: 11)
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}


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


def _dt(dtype):
    from cwdm_hip import _lib
    return {torch.bfloat16: _lib.CWDM_BF16, torch.float16: _lib.CWDM_F16}.get(dtype, _lib.CWDM_F32)


# --------------------------------------------------------------------------- the core (C ABI)
GUARD = 64   # elements past each output buffer that must stay untouched


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _desc(qkv, B, T, heads, ch):
    """qkv: (B, T, 3 heads ch) device tensor, rows [Q | K | V] -- the plan's layout (row stride 3C)."""
    from cwdm_hip import _lib
    C = heads * ch
    es = qkv.element_size()
    d = _lib.AttentionDesc()
    d.dtype, d.B, d.T, d.heads, d.ch = _dt(qkv.dtype), B, T, heads, ch
    d.q, d.k, d.v = qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es
    d.q_rs = d.k_rs = d.v_rs = 3 * C
    d.q_bs = d.k_bs = d.v_bs = T * 3 * C
    return d


def _forward(q, k, v, want_L=True):
    """q, k, v: (B, heads, T, ch) CPU tensors already in the dtype -> o (B, heads, T, ch), L (B, heads, T),
    and the raw guarded buffers."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    B, heads, T, ch = q.shape
    C = heads * ch
    qkv = torch.cat([p.transpose(1, 2).reshape(B, T, C) for p in (q, k, v)], dim=2).contiguous().to(DEV)
    obuf, o = _guarded(B * T * C, q.dtype, 7.0)
    Lbuf, L = _guarded(B * heads * T, torch.float32, 7.0)
    d = _desc(qkv, B, T, heads, ch)
    d.o, d.o_rs, d.o_bs = o.data_ptr(), C, T * C
    d.L = L.data_ptr() if want_L else None
    check(_lib.lib().cwdm_attention_forward(ctypes.byref(d), _stream()), "attention_forward")
    torch.cuda.synchronize()
    return (o.view(B, T, heads, ch).transpose(1, 2), L.view(B, heads, T), obuf, Lbuf, qkv)


def _backward(qkv, o_flat, L_flat, d_o, B, T, heads, ch):
    """d_o (B, T, C) device -> dq, dk, dv (B, heads, T, ch) and the raw buffer."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    C = heads * ch
    es = qkv.element_size()
    d = _desc(qkv, B, T, heads, ch)
    d.o, d.o_rs, d.o_bs, d.L = o_flat.data_ptr(), C, T * C, L_flat.data_ptr()
    Dm = torch.empty(B * heads * T, dtype=torch.float32, device=DEV)
    gbuf, g = _guarded(B * T * 3 * C, qkv.dtype, 7.0)
    d.D = Dm.data_ptr()
    d.d_o, d.do_rs, d.do_bs = d_o.data_ptr(), C, T * C
    d.dq, d.dk, d.dv = g.data_ptr(), g.data_ptr() + C * es, g.data_ptr() + 2 * C * es
    d.dq_rs = d.dk_rs = d.dv_rs = 3 * C
    d.dq_bs = d.dk_bs = d.dv_bs = T * 3 * C
    check(_lib.lib().cwdm_attention_backward(ctypes.byref(d), _stream()), "attention_backward")
    torch.cuda.synchronize()
    parts = [p.reshape(B, T, heads, ch).transpose(1, 2) for p in g.view(B, T, 3 * C).split(C, dim=2)]
    return parts, gbuf


# (B, heads, T, ch), q/k scale
CORE_CASES = {
    "1-one-tile": ((1, 1, 16, 64), 1.0),
    "2-below-a-tile": ((2, 1, 27, 32), 1.0),
    "3-7cubed-ch16": ((1, 4, 343, 16), 1.0),
    "4-production": ((1, 1, 512, 256), 1.0),
    "5-heads-x-batch": ((2, 4, 512, 64), 1.0),
    "6-many-blocks-tail": ((1, 2, 1100, 128), 1.0),
    "7-rescale-stress": ((1, 1, 512, 256), 6.0),
}
_CORE = {}


def _core_case(name, dtype):
    """Inputs drawn in fp32 and rounded to the dtype; the float64 reference on the ROUNDED inputs, once."""
    key = (name, dtype)
    if key not in _CORE:
        (B, heads, T, ch), qk = CORE_CASES[name]
        g = torch.Generator().manual_seed(100 + list(CORE_CASES).index(name))
        q, k, v = (torch.randn(B, heads, T, ch, generator=g) for _ in range(3))
        q, k = q * qk, k * qk
        if qk != 1.0:
            # plant each row's largest score: even rows in the LAST key block (the running max moves at the
            # end of the walk), odd rows in the FIRST (everything after it is rescaled against an old max)
            tgt = torch.tensor([(T - 1 - (t % 16)) if t % 2 == 0 else (t % 16) for t in range(T)])
            q = q + k[:, :, tgt, :]
        q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
        ref, lse = ato.attention_ref(q, k, v)
        s = q.double() @ k.double().transpose(-1, -2) / math.sqrt(ch)
        if qk != 1.0:
            am = s.argmax(-1)[0, 0]
            assert bool((am[0::2] >= T - 16).all()) and bool((am[1::2] < 16).all())
        _CORE[key] = dict(q=q, k=k, v=v, ref=ref, lse=lse, smax=float(s.abs().max()))
    return _CORE[key]


@pytest.mark.parametrize("name", list(CORE_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_attention_forward_vs_float64(name, dtype):
    """max |o - ref| <= 1.5 * 2 ulp_half * max|v| for the 16-bit dtypes (one rounding per softmax weight,
    a convex combination keeps it, one more for the output; 1.5x for exp2, the reciprocal and fp32
    accumulation), 1e-3 of max|ref| in fp32.  L within 1e-5 absolute of the float64 log-sum-exp while
    max |scaled score| < 16 (every case but 7); above that the bound grows with the score scale,
    1e-5 * max|score| / 16: L is stored in fp32, whose half-ulp at 700 is 3e-5, so 1e-5 absolute cannot
    hold there, and the scaled bound keeps the same number of fp32 ulps (about 10 of a value in [8, 16)).
    A second call gives the same bits; the guards past o and L stay untouched."""
    c = _core_case(name, dtype)
    o, L, obuf, Lbuf, _ = _forward(c["q"], c["k"], c["v"])
    assert torch.isfinite(o.float()).all() and torch.isfinite(L).all()
    err = float((o.double().cpu() - c["ref"]).abs().max())
    vmax = float(c["v"].double().abs().max())
    bound = 1e-3 * float(c["ref"].abs().max()) if dtype == torch.float32 else 1.5 * 2 * HALF_ULP[dtype] * vmax
    lerr = float((L.double().cpu() - c["lse"]).abs().max())
    lbound = 1e-5 * max(1.0, c["smax"] / 16.0)
    print(f"{name} {dtype}: max|o-ref| {err:.3e} (bound {bound:.3e}), L err {lerr:.3e} (bound {lbound:.3e})")
    assert err <= bound
    assert lerr <= lbound
    assert bool((obuf[-GUARD:] == 7.0).all()) and bool((Lbuf[-GUARD:] == 7.0).all())
    o2, L2, _, _, _ = _forward(c["q"], c["k"], c["v"])
    _same(o2, o, "o of a second call")
    _same(L2, L, "L of a second call")
    o3, _, _, Lb3, _ = _forward(c["q"], c["k"], c["v"], want_L=False)   # L is optional
    _same(o3, o, "o without L")
    assert bool((Lb3 == 7.0).all())


@pytest.mark.parametrize("name", list(CORE_CASES))
@pytest.mark.parametrize("dtype,cap", [(torch.float32, 1e-3), (torch.bfloat16, 8e-2), (torch.float16, 1.5e-2)],
                         ids=["fp32", "bf16", "fp16"])
def test_attention_backward_vs_float64_autograd(name, dtype, cap):
    """dq, dk, dv by rel-L2 per tensor against float64 autograd on the rounded inputs (caps: the project's
    16-bit gradient bounds for the tiny U-Net; locks, not targets); two calls give the same bits.
    Case 7 (|score| up to ~700, a softmax one-hot to ~1e-200): dv = P^T dO is well conditioned and holds
    the same cap.  Its true dq / dk vanish, so a relative error of them would measure only the
    cancellation in dS = P (dP - D); they are bounded absolutely instead.  With P one-hot at key s,
    dP - D = dO_t . (v_s - o_t) where o_t is v_s rounded once (elementwise error within 2 ulp_half |v| at worst,
    ulp_half |v| taken here: half the worst case, still 1.7x the rms of a rounding error), and dP, D
    are fp32 sums of ch terms (each within ch 2^-24 of sum |dO v|), so by Cauchy-Schwarz
    |dS| <= (2 ulp_half + 2 ch 2^-24) max_t |dO_t|_2 max_s |v_s|_2 (x 1.01 for the recomputed P and the
    operand rounding of dS); dq_t = scale dS k_s has entries <= scale |dS| max|k|, and a dk row collects one
    such term of max|q| per query whose largest score sits at that key (counted from the reference).
    ulp_half = 2^-24 in fp32.  An absolute lock scaled to max|dO| max|k| (for dq about 1 / 30 of the size an
    entry has when the softmax is not one-hot); not a target."""
    c = _core_case(name, dtype)
    B, heads, T, ch = c["q"].shape
    C = heads * ch
    g = torch.Generator().manual_seed(7)
    d_o = torch.randn(B, T, C, generator=g).to(dtype)
    o, L, obuf, Lbuf, qkv = _forward(c["q"], c["k"], c["v"])
    (dq, dk, dv), gbuf = _backward(qkv, obuf, Lbuf, d_o.to(DEV), B, T, heads, ch)
    q64, k64, v64 = (c[n].double().requires_grad_(True) for n in "qkv")
    s = q64 @ k64.transpose(-1, -2) / math.sqrt(ch)
    out = torch.softmax(s, -1) @ v64
    (out * d_o.double().view(B, T, heads, ch).transpose(1, 2)).sum().backward()
    errs = {n: _rel_l2(got, ref.grad) for n, got, ref in (("dq", dq, q64), ("dk", dk, k64), ("dv", dv, v64))}
    print(f"{name} {dtype}: rel-L2 {errs}")
    assert all(torch.isfinite(t.float()).all() for t in (dq, dk, dv))
    if CORE_CASES[name][1] == 1.0:
        assert max(errs.values()) < cap, errs
    else:
        assert errs["dv"] < cap, errs
        u = HALF_ULP.get(dtype, 2.0 ** -24)
        do_n = float(d_o.double().view(B, T, heads, ch).norm(dim=-1).max())
        v_n = float(c["v"].double().norm(dim=-1).max())
        ds_b = 1.01 * (2 * u + 2 * ch * 2.0 ** -24) * do_n * v_n
        per_key = int(torch.bincount(s.detach().argmax(-1).reshape(-1), minlength=T).max())   # (B = heads = 1)
        bounds = {"dq": ds_b * float(c["k"].double().abs().max()) / math.sqrt(ch),
                  "dk": ds_b * float(c["q"].double().abs().max()) / math.sqrt(ch) * per_key}
        worst = {n: float((got.double().cpu() - ref.grad).abs().max())
                 for n, got, ref in (("dq", dq, q64), ("dk", dk, k64))}
        print(f"{name} {dtype}: max |dq|, |dk| error {worst} (bounds {bounds}), "
              f"max |ref| {float(q64.grad.abs().max()):.3e} {float(k64.grad.abs().max()):.3e}")
        assert worst["dq"] <= bounds["dq"] and worst["dk"] <= bounds["dk"], (worst, bounds)
    assert bool((gbuf[-GUARD:] == 7.0).all())
    (dq2, dk2, dv2), _ = _backward(qkv, obuf, Lbuf, d_o.to(DEV), B, T, heads, ch)
    for a, b, n in ((dq2, dq, "dq"), (dk2, dk, "dk"), (dv2, dv, "dv")):
        _same(a, b, n + " of a second call")


def test_attention_refuses_unsupported_shapes():
    from cwdm_hip import _lib
    x = torch.zeros(1, 16, 3 * 512, device=DEV)
    for heads, ch in ((1, 24), (1, 8), (1, 272)):
        d = _desc(x, 1, 16, heads, ch)
        d.o, d.o_rs, d.o_bs = x.data_ptr(), heads * ch, 16 * heads * ch
        assert _lib.lib().cwdm_attention_forward(ctypes.byref(d), None) == _lib.E_UNSUPPORTED, (heads, ch)
        assert b"multiple of 16" in _lib.lib().cwdm_last_error()
    # B > 1: a batch stride that breaks the 16-byte alignment, or an output's that lets batches overlap
    x = torch.zeros(2, 16, 3 * 64, device=DEV)
    o = torch.zeros(2, 16, 64, device=DEV)
    for field, value in (("k_bs", 16 * 192 + 2), ("o_bs", 0), ("o_bs", 15 * 64 + 32)):
        d = _desc(x, 2, 16, 1, 64)
        d.o, d.o_rs, d.o_bs = o.data_ptr(), 64, 16 * 64
        setattr(d, field, value)
        assert _lib.lib().cwdm_attention_forward(ctypes.byref(d), None) == _lib.E_SHAPE, (field, value)
        assert b"batch stride" in _lib.lib().cwdm_last_error()
    assert not o.any()


# --------------------------------------------------------------------------- the block (C ABI)
def _linear(dtype, B, T, K, N, x, w, gn=None, bias=None, res=None, n_out=None, stats=None):
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    d = _lib.AttnLinearDesc()
    d.dtype, d.B, d.T, d.K, d.N = _dt(dtype), B, T, K, N
    d.in_, d.w = x.data_ptr(), w.data_ptr()
    for name, t in (("gn", gn), ("bias", bias), ("res", res), ("n_out", n_out), ("stats", stats)):
        setattr(d, name, t.data_ptr() if t is not None else None)
    obuf, out = _guarded(B * T * N, dtype, 7.0)
    d.out = out.data_ptr()
    check(_lib.lib().cwdm_attn_linear(ctypes.byref(d), _stream()), "attn_linear")
    torch.cuda.synchronize()
    return out.view(B, T, N), obuf


def _pack(w, rows, cols, heads, ch, legacy, transpose, dtype):
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    out = torch.empty(rows * cols, dtype=dtype, device=DEV)
    check(_lib.lib().cwdm_attn_pack(w.data_ptr(), rows, cols, heads, ch, legacy, transpose, _dt(dtype),
                                    out.data_ptr(), _stream()), "attn_pack")
    return out


@pytest.mark.parametrize("T", [512, 343])
@pytest.mark.parametrize("new_order", [False, True], ids=["legacy", "new"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 6e-2), (torch.float16, 1e-2)],
                         ids=["fp32", "bf16", "fp16"])
def test_block_vs_restatement(T, new_order, dtype, tol):
    """C = 64, 8 groups, 4 heads: GroupNorm + qkv, the core, proj_out + residual against the restated block
    in fp32 on the rounded input (the model-level forward bounds).  The statistics partials, summed, against
    the float64 sum and sum of squares of the UNROUNDED output, rtol 1e-5 / atol 1e-4 in every dtype: the
    unrounded output is x + W a + b in float64 from exactly what the projection kernel read (the stored a,
    the packed W, the fp32 bias, x), i.e. the kernel's value before rounding up to its fp32 accumulation."""
    from cwdm_hip import _lib
    B, C, G, heads = 2, 64, 8, 4
    ch = C // heads
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(B, T, C, generator=g) * 1.5 + 0.3).to(dtype)
    P = {"middle_block.1.norm.weight": 1 + 0.1 * torch.randn(C, generator=g),
         "middle_block.1.norm.bias": 0.1 * torch.randn(C, generator=g),
         "middle_block.1.qkv.weight": 0.15 * torch.randn(3 * C, C, 1, generator=g),
         "middle_block.1.qkv.bias": 0.05 * torch.randn(3 * C, generator=g),
         "middle_block.1.proj_out.weight": 0.15 * torch.randn(C, C, 1, generator=g),
         "middle_block.1.proj_out.bias": 0.05 * torch.randn(C, generator=g)}
    ref = ato.attention_block(P, x.float().transpose(1, 2), G, heads, new_order).transpose(1, 2)
    # the scale / shift cwdm_gn_finalize would hand the projection
    xg = x.double().view(B, T, G, C // G)
    mean = xg.mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-5)
    gam, bet = P["middle_block.1.norm.weight"].double(), P["middle_block.1.norm.bias"].double()
    sc = gam[None] * rstd.repeat_interleave(C // G, dim=1)
    sh = bet[None] - mean.repeat_interleave(C // G, dim=1) * sc
    ss = torch.stack([sc, sh], dim=-1).float().contiguous().to(DEV)
    wq = _pack(P["middle_block.1.qkv.weight"].to(DEV), 3 * C, C, heads, ch, 0 if new_order else 1, 0, dtype)
    bq = _pack(P["middle_block.1.qkv.bias"].to(DEV), 3 * C, 1, heads, ch, 0 if new_order else 1, 0, torch.float32)
    wp = _pack(P["middle_block.1.proj_out.weight"].to(DEV), C, C, heads, ch, 0, 0, dtype)
    xd = x.to(DEV)
    nbuf, n_out = _guarded(B * T * C, dtype, 7.0)
    qkv, qbuf = _linear(dtype, B, T, C, 3 * C, xd, wq, gn=ss, bias=bq, n_out=n_out)
    assert bool((qbuf[-GUARD:] == 7.0).all()) and bool((nbuf[-GUARD:] == 7.0).all())
    n_ref = torch.nn.functional.group_norm(x.float().transpose(1, 2), G, gam.float(), bet.float(), eps=1e-5)
    assert rel_err(n_out.view(B, T, C).float(), n_ref.transpose(1, 2)) < tol
    q, k, v = (p.reshape(B, T, heads, ch).transpose(1, 2).cpu() for p in qkv.split(C, dim=2))
    a, _, abuf, _, _ = _forward(q, k, v, want_L=False)
    parts = int(_lib.lib().cwdm_attn_parts(T))
    assert parts == (T + 15) // 16
    st = torch.full((B, parts, C, 2), float("nan"), dtype=torch.float32, device=DEV)
    y, ybuf = _linear(dtype, B, T, C, C, abuf[:B * T * C], wp, bias=P["middle_block.1.proj_out.bias"].to(DEV), res=xd,
                      stats=st)
    assert bool((ybuf[-GUARD:] == 7.0).all())
    e = rel_err(y.float(), ref)
    print(f"block T={T} new_order={new_order} {dtype}: rel {e:.3e}")
    assert e < tol
    assert torch.isfinite(st).all()   # every row written
    a64 = abuf[:B * T * C].view(B, T, C).double().cpu()
    w64 = wp.view(C, C).double().cpu()                      # packed [out][in], as the kernel multiplies it
    y64 = x.double() + a64 @ w64.t() + P["middle_block.1.proj_out.bias"].double()
    # (the stored output is that value rounded once: unit roundoff 2^-8 / 2^-11 / 2^-24 of its magnitude)
    assert float((y.double().cpu() - y64).abs().max()) <= (2 * HALF_ULP.get(dtype, 2.0 ** -25) + 1e-6) * float(y64.abs().max())
    s = st.double().sum(1).cpu()
    print(f"  statistics: sum err {float((s[..., 0] - y64.sum(1)).abs().max()):.3e}, "
          f"sum^2 err {float((s[..., 1] - (y64 * y64).sum(1)).abs().max()):.3e}")
    assert torch.allclose(s[..., 0], y64.sum(1), rtol=1e-5, atol=1e-4)
    assert torch.allclose(s[..., 1], (y64 * y64).sum(1), rtol=1e-5, atol=1e-4)
    st2 = torch.full_like(st, float("nan"))
    y2, _ = _linear(dtype, B, T, C, C, abuf[:B * T * C], wp, bias=P["middle_block.1.proj_out.bias"].to(DEV), res=xd,
                    stats=st2)
    _same(y2, y, "block output of a second call")
    _same(st2, st, "statistics of a second call")


# --------------------------------------------------------------------------- the tiny U-Net
VARIANTS = [(1, False), (1, True), (4, False), (4, True)]
VIDS = [f"h{h}-{'new' if o else 'legacy'}" for h, o in VARIANTS]


def _product_model(cfg, groups, params, dtype, heads=1, new_order=False):
    from guided_diffusion.unet import UNetModel
    m = UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"],
                  out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"], attention_resolutions=(),
                  channel_mult=cfg["channel_mult"], dims=3, resblock_updown=True, bottleneck_attention=True,
                  resample_2d=False, num_groups=groups, num_heads=heads, use_new_attention_order=new_order,
                  compute_dtype=dtype)
    m.load_state_dict(params)
    return m.to(DEV)


def _unet_grads(cfg, G, P, x, t, R, dtype, heads=1, new_order=False, hook=None):
    model = _product_model(cfg, G, P, dtype, heads, new_order)
    model._grad_hook = hook
    out = model(x.to(DEV), t.to(DEV))
    (out * R.to(DEV)).sum().backward()
    return out.detach().cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters()}, model


_TINY = {}


def _tiny_case(heads, new_order, edge=16):
    """x (2, 32, e, e, e), t [3, 917]: the restatement's output, trace and autograd gradients, once."""
    key = (heads, new_order, edge)
    if key not in _TINY:
        cfg, G = cases.C1_CFG, cases.C1_GROUPS
        P = ato.random_params(seed=1, **cfg)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 32, edge, edge, edge, generator=g)
        t = torch.tensor([3, 917])
        R = torch.randn(2, 8, edge, edge, edge, generator=g)
        trace = []
        with torch.no_grad():
            ref = ato.unet_forward(P, x, t, num_groups=G, trace=trace, num_heads=heads, new_order=new_order, **cfg)
        ref_out, ref_grads = ato.grads(cfg, G, P, x, t, R, num_heads=heads, new_order=new_order)
        _TINY[key] = dict(P=P, x=x, t=t, R=R, ref=ref, trace=trace, ref_out=ref_out, ref_grads=ref_grads)
    return _TINY[key]


@pytest.mark.parametrize("heads,new_order", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 6e-2), ("fp16", 1e-2)])
def test_tiny_unet_forward_and_trace(heads, new_order, dtype, tol):
    c = _tiny_case(heads, new_order)
    model = _product_model(cases.C1_CFG, cases.C1_GROUPS, c["P"], dtype, heads, new_order)
    with torch.no_grad():
        out = model(c["x"].to(DEV), c["t"].to(DEV))
    assert out.shape == c["ref"].shape
    print(dtype, heads, new_order, "out rel", rel_err(out, c["ref"]))
    assert rel_err(out, c["ref"]) < tol
    ws = model.plan.workspace(2, 16, 16, 16, DEV)
    got = model.plan.trace_tensors(ws, 2, 16, 16, 16)
    assert len(got) == len(c["trace"])
    from oracle import unet as ou
    assert len(got) == len(ou.topology(**cases.C1_CFG)) + 1      # one more entry than without attention
    for i, (gt, rf) in enumerate(zip(got, c["trace"])):
        if gt is None:
            continue
        assert rel_err(gt.float().permute(0, 4, 1, 2, 3), rf) < tol, i


@pytest.mark.parametrize("heads,new_order", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 8e-2), ("fp16", 1.5e-2)])
def test_tiny_unet_backward_vs_autograd(heads, new_order, dtype, tol):
    c = _tiny_case(heads, new_order)
    out, grads, model = _unet_grads(cases.C1_CFG, cases.C1_GROUPS, c["P"], c["x"], c["t"], c["R"], dtype, heads,
                                    new_order)
    assert rel_err(out, c["ref_out"]) < tol
    ref = c["ref_grads"]
    assert set(grads) == set(ref)
    worst = {k: _rel_l2(grads[k], ref[k]) for k in ref}
    print(dtype, heads, new_order, "worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:5])
    print(dtype, heads, new_order, "attention grads", {k: v for k, v in worst.items() if "middle_block.1." in k})
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    n = sum(p.numel() for p in model.parameters())
    assert model.flat_grad().numel() == n == sum(v.numel() for v in c["P"].values())


def test_tiny_unet_backward_segments_and_hook():
    """Segment-wise backward with a per-segment hook: every segment once (the attention block has its own),
    the flat buffer covered exactly once, the same gradients."""
    c = _tiny_case(4, False)
    cfg, G = cases.C1_CFG, cases.C1_GROUPS
    _, g_all, _ = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32", 4, False)
    seen = []

    def hook(seg, flat, off, n):
        if seg is not None:
            seen.append((seg, off, n))
    _, g_seg, model = _unet_grads(cfg, G, c["P"], c["x"], c["t"], c["R"], "fp32", 4, False, hook=hook)
    n = sum(p.numel() for p in model.parameters())
    assert [s[0] for s in seen] == list(range(model.plan.num_segments))
    cover = torch.zeros(n, dtype=torch.int32)
    for _, off, cnt in seen:
        cover[off:off + cnt] += 1
    assert bool((cover == 1).all())
    for name in g_all:
        assert rel_err(g_seg[name], g_all[name]) < 1e-5, name


def test_tiny_unet_tail_grid_fp32():
    """14^3 subbands: the bottleneck is 7^3 = 343 voxels, a tail in the last key and query tile inside the plan."""
    c = _tiny_case(4, False, edge=14)
    out, grads, _ = _unet_grads(cases.C1_CFG, cases.C1_GROUPS, c["P"], c["x"], c["t"], c["R"], "fp32", 4, False)
    assert rel_err(out, c["ref_out"]) < 1e-3
    worst = {k: _rel_l2(grads[k], c["ref_grads"][k]) for k in c["ref_grads"]}
    print("14^3 worst grads", sorted(worst.items(), key=lambda kv: -kv[1])[:5])
    assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


# --------------------------------------------------------------------------- production channels
PROD_CFG = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4))
PROD_GRID = (32, 32, 64)   # bottleneck 2 x 2 x 4: T = 16, C = 256, one head of 256 channels
_PROD = {}


def _prod_case():
    if not _PROD:
        P = ato.random_params(seed=51, **PROD_CFG)
        g = torch.Generator().manual_seed(52)
        x = torch.randn(1, 32, *PROD_GRID, generator=g)
        t = torch.tensor([500])
        R = torch.randn(1, 8, *PROD_GRID, generator=g)
        ref_out, ref = ato.grads(PROD_CFG, 32, P, x, t, R)
        _PROD.update(P=P, x=x, t=t, R=R, ref_out=ref_out, ref=ref)
    return _PROD


def _prod_run(dtype):
    c = _prod_case()
    out, grads, _ = _unet_grads(PROD_CFG, 32, c["P"], c["x"], c["t"], c["R"], dtype)
    assert set(grads) == set(c["ref"])
    worst = {k: _rel_l2(grads[k], c["ref"][k]) for k in c["ref"]}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    eo = rel_err(out, c["ref_out"])
    print(dtype, "out rel", eo, "worst grads", top, "attention",
          {k: v for k, v in worst.items() if "middle_block.1." in k})
    return eo, top


def test_production_unet_fp32_vs_autograd():
    eo, top = _prod_run("fp32")
    assert eo < 1e-3
    assert top[0][1] < 1e-3, top


def test_production_unet_bf16_close_to_fp32_reference():
    """The bounds of the concatenating and additive models' production tests: output 5e-2, gradients 8e-2."""
    eo, top = _prod_run("bf16")
    assert eo < 5e-2
    assert top[0][1] < 8e-2, top


# --------------------------------------------------------------------------- sampling, training, checkpoint
def _c1_attention(dtype="fp32", heads=4, **model_args):
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=32, channel_mult="1,2", num_res_blocks=1, num_groups=8,
                                         **model_args)
    keys = script_util.model_and_diffusion_defaults().keys()
    kw = {k: args[k] for k in keys}
    kw.update(bottleneck_attention=True, attention_resolutions="", num_heads=heads)
    model, diffusion = script_util.create_model_and_diffusion(**kw, compute_dtype=dtype)
    diffusion.mode = "i2i"
    return model, diffusion


def test_sampling_loop_vs_restatement_fp32():
    _, cond, x_T, _, _ = cases.c1_inputs(32)
    g = torch.Generator().manual_seed(9)
    noises = [torch.randn(x_T.shape, generator=g) for _ in range(6)]
    P = ato.random_params(seed=1, **cases.C1_CFG)
    model, diffusion = _c1_attention(diffusion_steps=6, sample_schedule="sampled")
    model.load_state_dict(P)
    model.to(DEV)
    it = iter([n.to(DEV) for n in noises])
    sample = diffusion.p_sample_loop(model, x_T.shape, noise=x_T.to(DEV), cond=cond.to(DEV), clip_denoised=True,
                                     progress=False, noise_fn=lambda x: next(it))
    tab = od.Tables(od.beta_schedule("linear", 6, "sampled"))
    ref = od.p_sample_loop(tab, ato.AttentionOracleUNet(P, num_groups=cases.C1_GROUPS, num_heads=4, **cases.C1_CFG),
                           x_T, cond, noises)
    assert rel_err(sample, ref) < 1e-3


@pytest.mark.parametrize("respacing,dtype", [("", "fp32"), ("ddim10", "bf16")])
def test_hip_graph_loop_equals_eager_loop(respacing, dtype):
    model, diffusion = _c1_attention(dtype, diffusion_steps=50, sample_schedule="direct",
                                     timestep_respacing=respacing)
    model.load_state_dict(ato.random_params(seed=1, **cases.C1_CFG))
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
    P = ato.random_params(seed=41, **cases.C1_CFG)
    batch = cases.data.brats_batch(32, seed=5, batch=1)
    bdev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def run():
        model, diffusion = _c1_attention("bf16")
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
    moved = [n for n in p_a if n.startswith("middle_block.1.") and not torch.equal(p_a[n], P[n])]
    assert sorted(moved) == sorted(n for n in P if n.startswith("middle_block.1.")), moved


def test_checkpoint_round_trip_same_forward_bits(tmp_path):
    c = _tiny_case(4, False)
    model = _product_model(cases.C1_CFG, cases.C1_GROUPS, c["P"], "bf16", 4, False)
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    with torch.no_grad():
        a = model(x, t)
    path = tmp_path / "model.pt"
    torch.save(model.state_dict(), path)
    fresh = _product_model(cases.C1_CFG, cases.C1_GROUPS, torch.load(path, map_location="cpu"), "bf16", 4, False)
    with torch.no_grad():
        b = fresh(x, t)
    assert torch.equal(a, b)
    assert rel_err(a, c["ref"]) < 6e-2
