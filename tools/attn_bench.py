#!/usr/bin/env python3
"""What the bottleneck attention block costs.  Not bench.py.

HIP-event timings, after warm-up, of
  * the 81.5 M-parameter model's forward (the sampling step's model call) and
    training step (forward + backward) at --edge^3 subbands, B = 1, in --dtype, with and
    without bottleneck_attention, alternating in one process;
  * each attention launch alone through the C ABI at (B, heads, T, ch) =
    (1, 1, 512, 256) and (1, 4, 512, 64): the GroupNorm + qkv projection, the
    core, proj_out + residual + statistics, and the backward call (row dots,
    the key-tile kernel and the query-tile kernel together).
Prints one JSON line per measurement.  Run it under `timeout`.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fast-cwdm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda"


def timed(fn, warmup, iters, batch=20):
    """Median and minimum milliseconds per fn() over iters event pairs of `batch` back-to-back calls
    (the launches queue behind each other, so the pair times the kernels, not the host)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    return statistics.median(ms), min(ms)


def kernels(B, heads, T, ch, dtype, warmup, iters):
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    from cwdm_hip.ops import _stream
    L = _lib.lib()
    C = heads * ch
    dt = {torch.bfloat16: _lib.CWDM_BF16, torch.float16: _lib.CWDM_F16, torch.float32: _lib.CWDM_F32}[dtype]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, C, generator=g).to(dtype).to(DEV)
    ss = torch.stack([torch.ones(B, C), torch.zeros(B, C)], -1).contiguous().to(DEV)
    wq = (0.06 * torch.randn(3 * C, C, generator=g)).to(dtype).to(DEV)
    wp = (0.06 * torch.randn(C, C, generator=g)).to(dtype).to(DEV)
    bq, bp = torch.zeros(3 * C, device=DEV), torch.zeros(C, device=DEV)
    qkv = torch.empty(B, T, 3 * C, dtype=dtype, device=DEV)
    a = torch.empty(B, T, C, dtype=dtype, device=DEV)
    y = torch.empty(B, T, C, dtype=dtype, device=DEV)
    n = torch.empty(B, T, C, dtype=dtype, device=DEV)
    st = torch.empty(B, int(L.cwdm_attn_parts(T)), C, 2, device=DEV)
    Lse = torch.empty(B, heads, T, device=DEV)
    Dm = torch.empty(B, heads, T, device=DEV)
    dqkv = torch.empty_like(qkv)
    da = torch.randn(B, T, C, generator=g).to(dtype).to(DEV)
    es = x.element_size()

    def lin(inp, gn, w, bias, res, out, n_out, stats, K, N):
        d = _lib.AttnLinearDesc()
        d.dtype, d.B, d.T, d.K, d.N = dt, B, T, K, N
        d.in_, d.w, d.out = inp.data_ptr(), w.data_ptr(), out.data_ptr()
        d.gn = gn.data_ptr() if gn is not None else None
        d.bias = bias.data_ptr() if bias is not None else None
        d.res = res.data_ptr() if res is not None else None
        d.n_out = n_out.data_ptr() if n_out is not None else None
        d.stats = stats.data_ptr() if stats is not None else None
        return d

    ad = _lib.AttentionDesc()
    ad.dtype, ad.B, ad.T, ad.heads, ad.ch = dt, B, T, heads, ch
    ad.q, ad.k, ad.v = qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es
    ad.q_rs = ad.k_rs = ad.v_rs = 3 * C
    ad.q_bs = ad.k_bs = ad.v_bs = T * 3 * C
    ad.o, ad.o_rs, ad.o_bs, ad.L, ad.D = a.data_ptr(), C, T * C, Lse.data_ptr(), Dm.data_ptr()
    ad.d_o, ad.do_rs, ad.do_bs = da.data_ptr(), C, T * C
    ad.dq, ad.dk, ad.dv = dqkv.data_ptr(), dqkv.data_ptr() + C * es, dqkv.data_ptr() + 2 * C * es
    ad.dq_rs = ad.dk_rs = ad.dv_rs = 3 * C
    ad.dq_bs = ad.dk_bs = ad.dv_bs = T * 3 * C
    d_qkv = lin(x, ss, wq, bq, None, qkv, None, None, C, 3 * C)
    d_qkv_keep = lin(x, ss, wq, bq, None, qkv, n, None, C, 3 * C)
    d_proj = lin(a, None, wp, bp, x, y, None, st, C, C)
    s = _stream()
    runs = [("attn_qkv", lambda: check(L.cwdm_attn_linear(ctypes.byref(d_qkv), s))),
            ("attn_qkv_keep_n", lambda: check(L.cwdm_attn_linear(ctypes.byref(d_qkv_keep), s))),
            ("attn_core", lambda: check(L.cwdm_attention_forward(ctypes.byref(ad), s))),
            ("attn_proj", lambda: check(L.cwdm_attn_linear(ctypes.byref(d_proj), s))),
            ("attn_core_backward", lambda: check(L.cwdm_attention_backward(ctypes.byref(ad), s)))]
    for name, fn in runs:
        med, lo = timed(fn, warmup, iters)
        print(json.dumps(dict(kind="kernel", name=name, shape=[B, heads, T, ch], dtype=str(dtype).split(".")[-1],
                              us_median=round(med * 1e3, 2), us_min=round(lo * 1e3, 2))), flush=True)


def models(edge, dtype, warmup, iters, train):
    from guided_diffusion.unet import UNetModel

    def make(attn):
        torch.manual_seed(1)
        m = UNetModel(image_size=2 * edge, in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2,
                      attention_resolutions=(), channel_mult=(1, 2, 2, 4, 4), dims=3, resblock_updown=True,
                      bottleneck_attention=attn, resample_2d=False, num_groups=32, compute_dtype=dtype)
        with torch.no_grad():   # zero-initialised layers would hide nothing from a timer, but keep the data live
            for p in m.parameters():
                if not p.any():
                    p.normal_(0, 0.01)
        return m.to(DEV)

    pair = {False: make(False), True: make(True)}
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 32, edge, edge, edge, generator=g).to(DEV)
    t = torch.tensor([500], device=DEV)
    out = torch.empty(1, edge, edge, edge, 8, device=DEV)
    res = {(k, mode): [] for k in pair for mode in ("forward", "train")}
    xin = {k: m._prep_inputs(x, t) for k, m in pair.items()}

    def fwd(k):
        with torch.no_grad():
            pair[k].forward_ndhwc(xin[k][0], xin[k][1], out)

    def trn(k):
        m = pair[k]
        for p in m.parameters():
            p.grad = None
        m(x, t).square().mean().backward()

    for mode, fn in (("forward", fwd),) + ((("train", trn),) if train else ()):
        for k in pair:
            for _ in range(warmup):
                fn(k)
        torch.cuda.synchronize()
        for _ in range(iters):          # alternating: the parent configuration, then the new one
            for k in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(k)
                b.record()
                b.synchronize()
                res[(k, mode)].append(a.elapsed_time(b))
        base, att = statistics.median(res[(False, mode)]), statistics.median(res[(True, mode)])
        print(json.dumps(dict(kind="model", mode=mode, edge=edge, dtype=dtype, ms_without=round(base, 4),
                              ms_with=round(att, 4), delta_us=round((att - base) * 1e3, 1),
                              min_without=round(min(res[(False, mode)]), 4), min_with=round(min(res[(True, mode)]), 4))),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"], help="kernels and models")
    ap.add_argument("--warmup", type=int, default=5, help="model runs: warm-up calls per model")
    ap.add_argument("--iters", type=int, default=30, help="model runs: timed pairs (without, with)")
    ap.add_argument("--kernel-warmup", type=int, default=20, help="kernel runs: warm-up launches")
    ap.add_argument("--kernel-iters", type=int, default=50, help="kernel runs: event pairs of 20 launches")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_bench needs a GPU"
    kdtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    for shape in ((1, 1, 512, 256), (1, 4, 512, 64)):
        kernels(*shape, kdtype, a.kernel_warmup, a.kernel_iters)
    if not a.no_model:
        models(a.edge, a.dtype, a.warmup, a.iters, not a.no_train)


if __name__ == "__main__":
    main()
