#!/usr/bin/env python3
"""What use_scale_shift_norm=True costs.  Not bench.py.

HIP-event timings, after warm-up, of the 81.5 M-parameter model's forward (the
sampling step's model call) and training step (forward + backward) at --edge^3
subbands, B = 1, in --dtype, with the flag off and on, alternating in one
process.  Prints one JSON line per mode.  Run it under `timeout`.
"""
import argparse
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


def models(edge, dtype, warmup, iters, train):
    from guided_diffusion.unet import UNetModel

    def make(film):
        torch.manual_seed(1)
        m = UNetModel(image_size=2 * edge, in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2,
                      attention_resolutions=(), channel_mult=(1, 2, 2, 4, 4), dims=3, resblock_updown=True,
                      bottleneck_attention=False, resample_2d=False, num_groups=32, use_scale_shift_norm=film,
                      compute_dtype=dtype)
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
        for _ in range(iters):          # alternating: the flag off, then on
            for k in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(k)
                b.record()
                b.synchronize()
                res[(k, mode)].append(a.elapsed_time(b))
        off, on = statistics.median(res[(False, mode)]), statistics.median(res[(True, mode)])
        print(json.dumps(dict(kind="model", mode=mode, edge=edge, dtype=dtype, ms_off=round(off, 4),
                              ms_on=round(on, 4), delta_us=round((on - off) * 1e3, 1),
                              min_off=round(min(res[(False, mode)]), 4), min_on=round(min(res[(True, mode)]), 4),
                              spread_off_us=round((max(res[(False, mode)]) - min(res[(False, mode)])) * 1e3, 1))),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--warmup", type=int, default=5, help="warm-up calls per model")
    ap.add_argument("--iters", type=int, default=30, help="timed pairs (off, on)")
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "film_bench needs a GPU"
    models(a.edge, a.dtype, a.warmup, a.iters, not a.no_train)


if __name__ == "__main__":
    main()
