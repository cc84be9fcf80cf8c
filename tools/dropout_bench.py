"""The two dropout kernels beside cwdm_gn_apply on one tensor.

cwdm_gn_silu_dropout and cwdm_dropout_bwd read and write what cwdm_gn_apply does (one tensor in, one out), plus
two Philox4x32-10 blocks per 8 channels.  Each round times the three kernels one after the other (HIP events
around --reps back-to-back launches); prints one JSON line with the per-launch median, minimum and maximum over
the rounds and the bytes moved per second.

usage: python tools/dropout_bench.py [--grid 128] [--channels 64] [--dtype bf16] [--p 0.1] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "fast-cwdm_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from cwdm_hip._lib import check, lib
    from cwdm_hip.unet_runtime import TORCH_DT, parse_dtype
    L = lib()
    dt = parse_dtype(args.dtype)
    tdt = TORCH_DT[dt]
    B, V, C = 1, args.grid ** 3, args.channels
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, V, C, generator=g).to(dev, tdt)
    ss = torch.stack([1 + 0.2 * torch.randn(B, C, generator=g), 0.2 * torch.randn(B, C, generator=g)],
                     -1).contiguous().to(dev)
    out = torch.empty_like(x)
    du = torch.randn(B, V, C, generator=g).to(dev, tdt)
    seed = 0x0123456789ABCDEF

    kernels = {
        "gn_apply": lambda: check(L.cwdm_gn_apply(x.data_ptr(), C, None, 0, ss.data_ptr(), B, V, dt, out.data_ptr(),
                                                  None)),
        "gn_silu_dropout": lambda: check(L.cwdm_gn_silu_dropout(x.data_ptr(), ss.data_ptr(), out.data_ptr(), dt, B, V,
                                                                C, args.p, seed, 3, None)),
        "dropout_bwd": lambda: check(L.cwdm_dropout_bwd(du.data_ptr(), dt, B, V, C, args.p, seed, 3, None)),
    }
    for f in kernels.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in kernels}
    for _ in range(args.rounds):
        for name, f in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.reps)
    nbytes = 2 * x.numel() * x.element_size()
    res = {"tensor": [B, V, C], "dtype": args.dtype, "p": args.p, "reps": args.reps, "rounds": args.rounds,
           "bytes_per_launch": nbytes}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "tb_per_s": round(nbytes / med / 1e9, 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
