"""The conv route (csrc/conv_route.cpp) without a GPU: the workspace and packed
sizes the library answers equal the recorded ones of the commit before the
routing moved into one function (tests/golden/route_sizes.json, written by
tools/record_route_sizes.py), and lone calls take the routes DESIGN.md states
(cwdm_debug_conv_route).  No CWDM_* knob may be set: the sizes and the rules
are the defaults'."""
import ctypes
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_route_sizes as rec  # noqa: E402  (the case builders the golden file was written with)

# ConvKernel / GnInput of include/cwdm.h (cwdm_debug_conv_route)
HEAD, POINTWISE, SMALL_GRID, V5_PHASE, V5, V5_GN, V5_AA, V5_SPLIT, V4, BRICK = range(10)
GN_NONE, GN_APPLY, GN_FIN_APPLY, GN_IN_KERNEL = range(4)


@pytest.fixture(scope="module")
def L():
    knobs = sorted(k for k in os.environ if k.startswith("CWDM_") and k not in ("CWDM_LIB", "CWDM_ALLOW_STALE_LIB"))
    assert not knobs, f"this module checks the default routing: unset {knobs}"
    from cwdm_hip import _lib
    _lib.lib()   # (the build-id check)
    return rec.load(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "route_sizes.json")) as f:
        return json.load(f)


def test_golden_file_holds_the_cases_it_must(golden):
    """Plan sizes for every plan bench.py and test_gpu_fullsize.py build (each at B = 1 and 2), the
    lone-conv cross product and the packed sizes of its channel pairs."""
    assert len(golden["parent"]) >= 7
    have = {(p["name"], p["dtype"]) for p in golden["plans"]}
    for need in [("production", "bf16"), ("production", "fp16"), ("production", "fp32"), ("production", "fp32x"),
                 ("production_updown_false", "bf16"), ("production_additive_skips", "bf16"),
                 ("production_use_freq", "fp32"), ("production_use_freq", "bf16"), ("config5", "fp16")]:
        assert need in have, need
    for p in golden["plans"]:
        assert {g["B"] for g in p["grids"]} == {1, 2}
        if p["name"].startswith("production"):
            assert 128 in {g["edge"] for g in p["grids"]}
    assert dict(golden["conv"]["axes"]) == {
        "dtype": ["bf16", "fp16", "fp32"], "edge": [8, 16, 24, 32, 64, 128],
        "channels": [[32, 64], [64, 64], [128, 128], [192, 64], [256, 256]],
        "gn": [0, 1], "skip": [0, 1], "a_mode": [0, 1], "res_mode": [-1, 0], "B": [1, 2]}
    assert len(golden["conv"]["workspace_bytes"]) == 3 * 6 * 5 * 2 ** 5
    assert len(golden["packed"]) == 3 * 5 * 2


def test_plan_sizes_equal_the_recorded_ones(L, golden):
    for p in golden["plans"]:
        edges = sorted({g["edge"] for g in p["grids"]}, reverse=True)
        got = rec.plan_sizes(L, p["config"], p["dtype"], edges)
        want = {k: p[k] for k in ("packed_bytes", "packed_bwd_bytes")}
        want["grids"] = sorted(p["grids"], key=lambda g: (-g["edge"], g["B"]))
        assert got == want, (p["name"], p["dtype"])


def test_lone_conv_sizes_equal_the_recorded_ones(L, golden):
    axes = [(n, v) for n, v in golden["conv"]["axes"]]
    want = golden["conv"]["workspace_bytes"]
    bad = []
    for pt, w in zip(rec.conv_points(axes), want):
        got = L.cwdm_conv3d_workspace_bytes(ctypes.byref(rec.conv_desc(*pt)))
        if got != w:
            bad.append((pt, got, w))
    assert not bad, bad[:10]


def test_packed_sizes_equal_the_recorded_ones(L, golden):
    for p in golden["packed"]:
        assert L.cwdm_conv3d_packed_bytes(p["cout"], p["cin"], p["ksize"], rec.DT[p["dtype"]]) == p["bytes"], p


def route(L, dtype="bf16", edge=32, cin=128, cout=128, gn=0, skip=0, a_mode=0, res_mode=-1, B=1, ws=1 << 40):
    d = rec.conv_desc(dtype, edge, [cin, cout], gn, skip, a_mode, res_mode, B)
    d.workspace, d.ws_bytes = rec.FLAG, ws
    out = (ctypes.c_int * 6)()
    f = L.cwdm_debug_conv_route
    f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(rec.ConvDesc), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    assert f(ctypes.byref(d), out, 6) == 0
    return dict(zip(("kernel", "gn", "skip", "ksplit", "aa_units", "ws_total"), out))


def test_routes_follow_the_documented_rules(L):
    """bf16, B = 1, enough workspace unless stated; each expectation is a rule of DESIGN.md or of the
    predicates' own comments, none is an output of the code under test."""
    # 128^3 64 -> 64 with GroupNorm: 4096 tiles >= 256 CUs -> the warp-specialised kernel; 4 input chunks
    # < CWDM_V5_AA_MINCH (8) -> no apply-ahead; CWDM_V5 = 3 -> the gn_apply pre-pass, not the in-LDS transform
    r = route(L, edge=128, cin=64, cout=64, gn=1)
    assert (r["kernel"], r["gn"], r["ksplit"], r["aa_units"]) == (V5, GN_APPLY, 1, 0), r
    # 32^3 128 -> 128: 128 tiles, fewer than 256 CUs (not v5), at least the split target 64 (no K split) -> v4
    r = route(L, edge=32, cin=128, cout=128)
    assert (r["kernel"], r["gn"], r["ksplit"]) == (V4, GN_NONE, 1), r
    # "16^3: 256 workgroups, no split"; at 8^3 the small-grid kernel splits K
    r = route(L, edge=16, cin=256, cout=256)
    assert (r["kernel"], r["ksplit"]) == (SMALL_GRID, 1), r
    r = route(L, edge=8, cin=256, cout=256)
    assert r["kernel"] == SMALL_GRID and r["ksplit"] > 1, r
    # the DMA path needs its workspace (the activated input): without one, the brick kernels
    assert route(L, edge=32, cin=128, cout=128, gn=1)["kernel"] == V4
    assert route(L, edge=32, cin=128, cout=128, gn=1, ws=0)["kernel"] == BRICK
    # the 1x1 skip product is added through the residual slot: a desc with both goes to the brick kernels
    for edge, cin, cout in ((32, 128, 128), (128, 64, 64), (16, 256, 256)):
        assert route(L, edge=edge, cin=cin, cout=cout, skip=1, res_mode=0)["kernel"] == BRICK
    # fp32 without split weights never reaches the warp-specialised kernels
    r = route(L, dtype="fp32", edge=32, cin=128, cout=128)
    assert r["kernel"] not in (V5_PHASE, V5, V5_GN, V5_AA, V5_SPLIT), r


def test_route_entry_refuses_bad_arguments(L):
    d = rec.conv_desc("bf16", 32, [64, 64], 0, 0, 0, -1, 1)
    out = (ctypes.c_int * 6)()
    f = L.cwdm_debug_conv_route
    f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(rec.ConvDesc), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    assert f(ctypes.byref(d), out, 5) != 0
    assert f(None, out, 6) != 0
    d.W = 0
    assert f(ctypes.byref(d), out, 6) != 0
