#!/usr/bin/env python3
"""Record the workspace / packed sizes a libcwdm build answers, as tests/golden/route_sizes.json.

    tools/build_ab_lib.sh parent <commit>
    python3 tools/record_route_sizes.py --lib ablib/libcwdm_parent.so --commit <commit> \
        > tests/golden/route_sizes.json

Run it on a machine without a GPU and with no CWDM_* knob set (the size functions make no device
call but the CU-count and occupancy queries, which then answer 256 and 1).  The library is loaded
through ctypes alone, so any build with the entries used here will do, whatever else it exports.
tests/test_conv_route_cpu.py replays the file against the tree's library: the file names every
case it holds, the test adds none.
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-cwdm_amd"))

from cwdm_hip._lib import CWDM_BF16, CWDM_F16, CWDM_F32, ConvDesc, UNetConfig  # noqa: E402

i64 = ctypes.c_int64
DT = {"bf16": CWDM_BF16, "fp16": CWDM_F16, "fp32": CWDM_F32}
FLAG = ctypes.c_void_p(1)   # a presence flag: the size functions read no pointer

PRODUCTION = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=[1, 2, 2, 4, 4],
                  num_groups=32)
# (name, config, dtypes, cubic grid edges): what bench.py and tests/test_gpu_fullsize.py build, and
# the same plans on the smaller grids where the small-grid and K-expanded routes begin earlier
PLANS = [
    ("production", PRODUCTION, ["bf16", "fp16", "fp32", "fp32x"], [128, 64, 32]),
    ("production_updown_false", dict(PRODUCTION, resblock_updown=0), ["bf16", "fp32", "fp32x"], [128, 64]),
    ("production_additive_skips", dict(PRODUCTION, additive_skips=1), ["bf16", "fp16", "fp32"], [128, 64]),
    ("production_use_freq", dict(PRODUCTION, use_freq=1), ["bf16", "fp32"], [128, 64]),
    ("config5", dict(in_channels=256, model_channels=64, out_channels=64, num_res_blocks=2, channel_mult=[1, 2, 2],
                     num_groups=32), ["fp16", "bf16", "fp32"], [56]),
    ("tiny", dict(in_channels=32, model_channels=32, out_channels=8, num_res_blocks=1, channel_mult=[1, 2],
                  num_groups=8), ["bf16", "fp16", "fp32", "fp32x"], [32, 16]),
]
CONV_AXES = [
    ("dtype", ["bf16", "fp16", "fp32"]),
    ("edge", [8, 16, 24, 32, 64, 128]),
    ("channels", [[32, 64], [64, 64], [128, 128], [192, 64], [256, 256]]),   # (cin, cout)
    ("gn", [0, 1]),
    ("skip", [0, 1]),
    ("a_mode", [0, 1]),
    ("res_mode", [-1, 0]),
    ("B", [1, 2]),
]


def load(path):
    L = ctypes.CDLL(path)
    L.cwdm_unet_create.argtypes = [ctypes.POINTER(UNetConfig), ctypes.POINTER(ctypes.c_void_p)]
    L.cwdm_unet_destroy.argtypes = [ctypes.c_void_p]
    L.cwdm_unet_destroy.restype = None
    for name in ("cwdm_unet_workspace_bytes", "cwdm_unet_train_workspace_bytes", "cwdm_unet_grad_workspace_bytes"):
        f = getattr(L, name)
        f.restype, f.argtypes = i64, [ctypes.c_void_p, i64, i64, i64, i64]
    for name in ("cwdm_unet_packed_bytes", "cwdm_unet_packed_bwd_bytes"):
        f = getattr(L, name)
        f.restype, f.argtypes = i64, [ctypes.c_void_p]
    L.cwdm_conv3d_workspace_bytes.restype = i64
    L.cwdm_conv3d_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    L.cwdm_conv3d_packed_bytes.restype = i64
    L.cwdm_conv3d_packed_bytes.argtypes = [ctypes.c_int] * 4
    return L


def plan_sizes(L, cfg, dtype, edges):
    c = UNetConfig()
    c.resblock_updown = 1
    for k, v in cfg.items():
        if k == "channel_mult":
            c.num_levels = len(v)
            for i, m in enumerate(v):
                c.channel_mult[i] = m
        else:
            setattr(c, k, v)
    c.dtype = DT["fp32" if dtype == "fp32x" else dtype]
    c.mfma_split = 1 if dtype == "fp32x" else 0
    h = ctypes.c_void_p()
    rc = L.cwdm_unet_create(ctypes.byref(c), ctypes.byref(h))
    assert rc == 0, (cfg, dtype, rc)
    out = {"packed_bytes": L.cwdm_unet_packed_bytes(h), "packed_bwd_bytes": L.cwdm_unet_packed_bwd_bytes(h), "grids": []}
    for n, B in itertools.product(edges, (1, 2)):
        out["grids"].append({"B": B, "edge": n,
                             "workspace_bytes": L.cwdm_unet_workspace_bytes(h, B, n, n, n),
                             "train_workspace_bytes": L.cwdm_unet_train_workspace_bytes(h, B, n, n, n),
                             "grad_workspace_bytes": L.cwdm_unet_grad_workspace_bytes(h, B, n, n, n)})
    L.cwdm_unet_destroy(h)
    return out


def conv_desc(dtype, edge, channels, gn, skip, a_mode, res_mode, B):
    """The lone-conv desc of one point of CONV_AXES (pointers: presence flags)."""
    cin, cout = channels
    d = ConvDesc()
    d.dtype = DT[dtype]
    d.B, d.D, d.H, d.W = B, edge, edge, edge
    d.cout = cout
    d.a0, d.a_c0, d.a_w, d.a_mode = FLAG, cin, FLAG, a_mode
    if gn:
        d.a_gn = FLAG
    if skip:
        d.b0, d.b_c0, d.b_w = FLAG, cin, FLAG
    d.res_mode = res_mode
    if res_mode >= 0:
        d.res = FLAG
    d.out, d.out_dtype = FLAG, DT[dtype]
    return d


def conv_points(axes):
    return itertools.product(*[vals for _, vals in axes])


def record(L, commit):
    plans = []
    for name, cfg, dtypes, edges in PLANS:
        for dt in dtypes:
            plans.append(dict(name=name, config=cfg, dtype=dt, **plan_sizes(L, cfg, dt, edges)))
    conv = [L.cwdm_conv3d_workspace_bytes(ctypes.byref(conv_desc(*pt))) for pt in conv_points(CONV_AXES)]
    packed = [{"dtype": dt, "cout": co, "cin": ci, "ksize": k, "bytes": L.cwdm_conv3d_packed_bytes(co, ci, k, DT[dt])}
              for dt in DT for ci, co in dict(CONV_AXES)["channels"] for k in (3, 1)]
    return {"parent": commit, "plans": plans,
            "conv": {"axes": CONV_AXES, "order": "itertools.product over the axes, the last one fastest",
                     "workspace_bytes": conv},
            "packed": packed}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="the library to ask (tools/build_ab_lib.sh)")
    ap.add_argument("--commit", required=True, help="the commit that library was built from")
    a = ap.parse_args()
    knobs = sorted(k for k in os.environ if k.startswith("CWDM_"))
    assert not knobs, f"unset {knobs}: the recorded sizes are the defaults'"
    r = record(load(a.lib), a.commit)
    # one plan / one row of lone-conv sizes (the innermost three axes) per line: readable diffs
    ws = r["conv"].pop("workspace_bytes")
    rows = [json.dumps(ws[i:i + 8])[1:-1] for i in range(0, len(ws), 8)]
    sys.stdout.write('{"parent": %s,\n"plans": [\n%s\n],\n"conv": {%s,\n"workspace_bytes": [\n%s\n]},\n"packed": [\n%s\n]}\n' % (
        json.dumps(r["parent"]), ",\n".join(json.dumps(p) for p in r["plans"]), json.dumps(r["conv"])[1:-1],
        ",\n".join(rows), ",\n".join(json.dumps(p) for p in r["packed"])))


if __name__ == "__main__":
    main()
