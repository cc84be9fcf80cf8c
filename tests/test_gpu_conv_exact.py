"""Integer-exact tests of the conv routes and of the GroupNorm statistics their
epilogues emit (libcwdm through the C ABI).

Operands are small integers (or integers times a power of two), so every
product, every partial sum in any order, every stored 16-bit output, every
statistics row and every dW element is exactly representable: the assertions
are torch.equal against a float64 reference, and one wrong voxel anywhere --
a dropped halo tap, an off-by-one mask on a partial tile, a K slice that skips
a chunk -- fails them.  Each test asserts the conditions that make this true
on its float64 reference before it touches the GPU (_assert_exact); they are
conditions on the inputs, not tolerances.

GroupNorm prologues stay exact in the 16-bit kernels with (scale, shift) =
(32, 0), x in {0..3} and weights in {-1, 0, 1} / 32: SiLU(0) = 0, and SiLU(32 k)
differs from 32 k by far less than half a 16-bit ulp (exp2(-46) vanishes against
1, rcp is good to 1 ulp in fp32), so the value staged in 16 bits is exactly
32 x.  This rests on the staging rounding to 16 bits; fp32 GroupNorm'd
instantiations are checked with the derived bounds of part D instead.

Part D (random real-valued data): which tensor each epilogue's statistics
describe, read from the epilogues (STATS_DESCRIBE), and the fp32-summation
bounds that follow."""
import ctypes
import functools
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K
import test_gpu_stride2 as S2
import test_gpu_train as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# ConvKernel / GnInput / SkipKernel of csrc/internal.hpp, as cwdm_debug_conv_route reports them
HEAD, POINTWISE, SMALL_GRID, V5_PHASE, V5, V5_GN, V5_AA, V5_SPLIT, V4, BRICK = range(10)
GN_NONE, GN_APPLY, GN_FIN_APPLY, GN_IN_KERNEL = range(4)
SKIP_NONE, SKIP_SG, SKIP_PW, SKIP_PW_SPLIT, SKIP_BRICK = range(5)

_nd, _nc = K._nd, K._nc


def _dt(name):
    return K._DTN[name]


def _case(cases, name):
    (c,) = {c for c in cases if c[0] == name}
    return c


# --------------------------------------------------------------------------- operands
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _tern(g, cout, cin, k, fan=None, terms=256.0):
    """Weights in {-1, 0, 1}, non-zero with probability min(1, terms / (k^3 fan)): about `terms` (256)
    products per output; fan: the channels one output sums over (cin; cout for a dgrad)."""
    p = min(1.0, terms / (k ** 3 * (fan or cin)))
    sign = torch.randint(0, 2, (cout, cin, k, k, k), generator=g).double() * 2 - 1
    keep = torch.rand(cout, cin, k, k, k, generator=g, dtype=torch.float64) < p
    return sign * keep


class _Ops:
    pass


def _terms(V, nseg, ex2, ex1):
    """Products per output: 256, or fewer on a large volume, so that condition 2 holds: sum y^2 per (b, c)
    is about V (nseg terms (E[x^2] + 9 E[x]^2) + 64) -- a channel whose +1 / -1 weights are 3 sigma out of
    balance carries a mean of 3 sqrt(terms) E[x] where the inputs are not centred (the GroupNorm recipe's
    x in {0..3}) -- and this is kept below 1.2e7 < 2^24.  The weight density is lowered, never an assertion."""
    return min(256.0, (1.2e7 / V - 64) / (nseg * (ex2 + 9 * ex1 * ex1)))


@functools.lru_cache(maxsize=1)
def _operands(case, use_gn, bias_const=None):
    """float64 operands and reference of a conv case (name, B, grid, c0, c1, cout, amode, gn, skip, rmode);
    shared by every dtype / grid cap of the case and never modified.  The cache holds one case: the case
    name is the slowest-varying parameter of every test here, so its dtypes and caps run back to back."""
    name, B, grid, c0, c1, cout, amode, _, skip, rmode = case
    g = torch.Generator().manual_seed(20261021)
    D, H, W = grid
    half, twice = (D // 2, H // 2, W // 2), (2 * D, 2 * H, 2 * W)
    cin = c0 + c1
    o = _Ops()
    sgrid = {0: grid, 1: half, 2: twice}[amode]
    terms = _terms(D * H * W, 2 if skip else 1, 3.5 if use_gn else (16.0 if amode == 2 else 2.0), 1.5 if use_gn else 0.0)
    if use_gn:
        o.x = _ints(g, 0, 3, B, cin, *sgrid)
        o.gn = torch.tensor([32.0, 0.0]).repeat(B, cin, 1)
        h, wscale = 32 * o.x, 1.0 / 32
    else:
        # (the pooled source averages 8 voxels: multiples of 8 keep it an integer)
        o.x = _ints(g, -2, 2, B, cin, *sgrid) * (8 if amode == 2 else 1)
        o.gn = None
        h, wscale = o.x, 1.0
    if amode == 2:
        h = F.avg_pool3d(h, 2)
    elif amode == 1:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    o.w = _tern(g, cout, cin, 3, terms=terms) * wscale
    o.bias = _ints(g, -4, 4, cout) if bias_const is None else torch.full((cout,), float(bias_const), dtype=torch.float64)
    o.y_conv = F.conv3d(h, o.w, o.bias, padding=1)
    o.y = o.y_conv
    o.wb = o.y_skip = None
    if skip:
        o.wb = _tern(g, cout, cin, 1, terms=terms)
        o.y_skip = F.conv3d(o.x, o.wb)   # (the 1x1 skip reads the raw input)
        o.y = o.y + o.y_skip
    o.res = None
    if rmode >= 0:
        o.res = _ints(g, -8, 8, B, cout, *{0: grid, 1: half, 2: twice}[rmode]) * (8 if rmode == 2 else 1)
        o.y = o.y + {0: o.res, 1: F.interpolate(o.res, scale_factor=2, mode="nearest"),
                     2: F.avg_pool3d(o.res, 2)}[rmode]
    return o


def _assert_exact(tdt, *tensors, stats_of=None):
    """The conditions of exactness, on float64 references: every listed tensor (the output and what a
    route stores on the way: the conv + bias a kernel stages in 16 bits before the residual add, the
    1x1 skip product written to the workspace) is representable in the storage dtype; and for the
    statistics sum |y| and sum y^2 per (b, c) over the whole volume stay below 2^24, so a row is an exact
    fp32 integer under any order and any grouping of its voxels."""
    for t in tensors:
        if t is not None:
            assert torch.equal(t.to(tdt).double(), t), "a reference value is not representable in the storage dtype"
            assert float(t.abs().max()) < 2 ** 24
    if stats_of is not None:
        assert float(stats_of.abs().sum(dim=(2, 3, 4)).max()) < 2 ** 24
        assert float((stats_of ** 2).sum(dim=(2, 3, 4)).max()) < 2 ** 24


# --------------------------------------------------------------------------- the call
@contextmanager
def _forced(path=None, v5_grid=None, aa=None, wg=None, head2=None):
    """Set the library's test knobs, restore them on the way out."""
    from cwdm_hip._lib import lib
    L = lib()
    knobs = [(L.cwdm_conv3d_set_path, path), (L.cwdm_debug_v5_grid, v5_grid), (L.cwdm_debug_v5_aa, aa),
             (L.cwdm_debug_stats_wg, wg), (L.cwdm_debug_head2, head2)]
    prev = []
    try:
        for f, v in knobs:
            if v is not None:
                prev.append((f, f(v)))
        yield L
    finally:
        for f, p in reversed(prev):
            f(int(p))


def _pack(w, k, dtype):
    from cwdm_hip._lib import check, lib
    L = lib()
    cout, cin = w.shape[:2]
    n = L.cwdm_conv3d_packed_bytes(cout, cin, k, dtype)
    assert n > 0
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    wd = w.float().contiguous().to(DEV)
    check(L.cwdm_conv3d_pack(ctypes.c_void_p(wd.data_ptr()), cout, cin, k, dtype, ctypes.c_void_p(buf.data_ptr()), None))
    return buf


def _desc(dtype_name, B, grid, cout, a0, pa, a1=None, amode=0, gn=None, bias=None, bias_bs=0, b0=None, b1=None,
          pb=None, res=None, rmode=-1, out_f32=False, stats=True, split=True, psplit=None):
    """A cwdm_conv3d_desc on device tensors (NDHWC), output and statistics buffers filled with NaN.
    Returns (desc, out, stats, keep-alive list).  Call it with the path knobs already set: the workspace
    is the one the forced route asks for."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    D, H, W = grid
    out = torch.full((B, D, H, W, cout), NAN, device=DEV, dtype=torch.float32 if out_f32 else tdt)
    parts = L.cwdm_conv3d_parts(dtype, D, H, W, cout)
    st = torch.full((B, parts, cout, 2), NAN, device=DEV) if stats else None
    d = _lib.ConvDesc()
    d.dtype, d.B, d.D, d.H, d.W, d.cout = dtype, B, D, H, W, cout
    if pa is not None:
        d.a0, d.a_c0 = a0.data_ptr(), a0.shape[-1]
        d.a1, d.a_c1 = (a1.data_ptr(), a1.shape[-1]) if a1 is not None else (None, 0)
        d.a_mode = amode
        d.a_gn = gn.data_ptr() if gn is not None else None
        d.a_w = pa.data_ptr()
    if pb is not None:
        d.b0, d.b_c0 = b0.data_ptr(), b0.shape[-1]
        d.b1, d.b_c1 = (b1.data_ptr(), b1.shape[-1]) if b1 is not None else (None, 0)
        d.b_w = pb.data_ptr()
    if bias is not None:
        d.bias, d.bias_bstride = bias.data_ptr(), bias_bs
    d.res, d.res_mode = (res.data_ptr() if res is not None else None), rmode
    d.out, d.out_dtype = out.data_ptr(), (_lib.CWDM_F32 if out_f32 else dtype)
    d.stats = st.data_ptr() if st is not None else None
    if psplit is not None:
        d.a_w_split = psplit.data_ptr()
    nws = L.cwdm_conv3d_workspace_bytes(ctypes.byref(d))
    assert nws >= 0
    ws = None
    if nws > 0 and split:
        # (stale workspace, as in the plan: NaN bytes, not zeros)
        ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
        d.workspace, d.ws_bytes = ws.data_ptr(), nws
    return d, out, st, [a0, a1, gn, pa, b0, b1, pb, bias, res, psplit, ws]


def _desc_of(ops, case, dtype_name, **kw):
    name, B, grid, c0, c1, cout, amode, _, skip, rmode = case
    dtype, tdt = _dt(dtype_name)
    xd = _nd(ops.x).to(DEV, tdt)
    a0 = xd[..., :c0].contiguous()
    a1 = xd[..., c0:].contiguous() if c1 else None
    psplit = None
    if kw.pop("wsplit", False):   # the accurate fast mode's split-bf16 weights (fp32 convs)
        from cwdm_hip._lib import check, lib
        L = lib()
        psplit = torch.empty(L.cwdm_conv3d_packed_split_bytes(cout, c0 + c1), dtype=torch.uint8, device=DEV)
        wd = ops.w.float().contiguous().to(DEV)
        check(L.cwdm_conv3d_pack_split(ctypes.c_void_p(wd.data_ptr()), cout, c0 + c1, ctypes.c_void_p(psplit.data_ptr()),
                                       None))
    return _desc(dtype_name, B, grid, cout, a0, _pack(ops.w, 3, dtype), a1=a1, amode=amode,
                 gn=ops.gn.float().to(DEV) if ops.gn is not None else None, bias=ops.bias.float().to(DEV),
                 b0=a0 if skip else None, b1=a1 if skip else None, pb=_pack(ops.wb, 1, dtype) if skip else None,
                 res=_nd(ops.res).to(DEV, tdt) if ops.res is not None else None, rmode=rmode, psplit=psplit, **kw)


def _route(d):
    from cwdm_hip._lib import check, lib
    out = (ctypes.c_int * 6)()
    check(lib().cwdm_debug_conv_route(ctypes.byref(d), out, 6))
    return dict(zip(("kernel", "gn", "skip", "ksplit", "aa_units", "ws_total"), out))


def _assert_route(d, kernel, gn=GN_NONE, skip=SKIP_NONE, ksplit=None, aa=False):
    """ksplit: None = exactly 1, "split" = more than one K slice."""
    r = _route(d)
    assert r["kernel"] == kernel, f"the case landed on kernel {r['kernel']}, it is meant for {kernel}: {r}"
    assert r["gn"] == gn and r["skip"] == skip, r
    assert (r["ksplit"] > 1) if ksplit == "split" else (r["ksplit"] == 1), r
    assert (r["aa_units"] > 0) == aa, r
    return r


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _run_exact(d, out, st, y, wg=False):
    """Two calls into the same buffers (bitwise equal); the stored output equals the float64 reference
    cast to the output dtype; every word of the statistics rows the call owns is finite (the buffer was
    NaN), with per-workgroup partials (wg) every other word is still NaN; the rows summed in float64
    equal sum y and sum y^2 per (b, c)."""
    from cwdm_hip._lib import check, lib
    L = lib()
    check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
    torch.cuda.synchronize()
    rows = int(L.cwdm_debug_stats_wg(-1)) if wg else 0
    o1 = out.clone()
    s1 = st.clone() if st is not None else None
    check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o1), _bits(out)), "second call differs"
    got = o1.cpu()
    want = _nd(y).to(out.dtype)
    assert not torch.isnan(got).any(), "output voxels never written"
    assert torch.equal(got, want), f"{int((got != want).sum())} stored values differ from the float64 reference"
    if st is None:
        return
    assert torch.equal(_bits(s1), _bits(st)), "second call's statistics differ"
    B, parts, cout, _ = s1.shape
    s = s1.cpu()
    if wg:
        assert B == 1 and 0 < rows <= parts, f"per-workgroup rows were not granted (rows {rows}, per-tile {parts})"
        flat = s.view(parts, cout, 2)
        assert torch.isnan(flat[rows:]).all(), "words outside the per-workgroup rows were written"
        owned = flat[:rows][None]
    else:
        owned = s
    assert torch.isfinite(owned).all(), f"{int((~torch.isfinite(owned)).sum())} statistics words never written"
    tot = owned.double().sum(1)
    assert torch.equal(tot[..., 0], y.sum(dim=(2, 3, 4))), "sum y"
    assert torch.equal(tot[..., 1], (y ** 2).sum(dim=(2, 3, 4))), "sum y^2"


def _exact_forward(case, dtype_name, kernel, *, gn=None, skip=None, ksplit=None, aa=False, use_gn=None,
                   split=True, wg=False, wsplit=False, bias_const=None):
    """One exact forward case under the knobs the caller forced; gn / skip: the route's expected
    GnInput / SkipKernel (default: none unless the case has one -- then the caller says which)."""
    name, B, grid, c0, c1, cout, amode, case_gn, case_skip, rmode = case
    use_gn = case_gn if use_gn is None else use_gn
    _, tdt = _dt(dtype_name)
    ops = _operands(case, use_gn, bias_const)
    _assert_exact(tdt, ops.y, ops.y_conv, ops.y_skip, stats_of=ops.y)
    d, out, st, keep = _desc_of(ops, case, dtype_name, split=split, wsplit=wsplit)
    _assert_route(d, kernel, gn=GN_NONE if gn is None else gn, skip=SKIP_NONE if skip is None else skip,
                  ksplit=ksplit, aa=aa)
    _run_exact(d, out, st, ops.y, wg=wg)
    return d, out, st, keep, ops


# --------------------------------------------------------------------------- A. forward, per route
BRICK_NAMES = ["plain", "gn_concat_skip", "same_res", "up_res"]


@pytest.mark.parametrize("split", [True, False], ids=["splitk", "nosplit"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", BRICK_NAMES + ["sg_skip_plus_res_legacy"])
def test_brick_kernels_exact(name, dtype_name, split):
    """conv3d_kernels.hpp (kernel path 1; a 1x1 skip AND a residual lands there on every path), with and
    without the workspace its K split needs.  GroupNorm and the 1x1 skip run inside the kernel."""
    case = _case(K.CASES + K.SG_CASES, name)
    with _forced(path=0 if name == "sg_skip_plus_res_legacy" else 1):
        _exact_forward(case, dtype_name, BRICK, split=split)


@pytest.mark.parametrize("split", [True, False], ids=["splitk", "nosplit"])
def test_brick_kernels_pooled_source_fp32_exact(split):
    """a_mode 2 / res_mode 2 (2x2x2 average of the source and of the residual: fp32 brick kernels only),
    without GroupNorm; sources in multiples of 8 so that the pooled values are integers."""
    with _forced(path=1):
        _exact_forward(_case(K.CASES, "down_pool_res"), "fp32", BRICK, use_gn=False, split=split)


# V4_CASES' v4_ksplit_gn_skip and v4_gn_concat_skip_res carry a residual beside the 1x1 skip: the DMA path
# refuses that pair (the skip product takes the residual slot), so on every path they are brick-kernel
# cases (test_skip_plus_residual_shapes_are_brick_cases).  What their names describe -- v4's K split / CT32
# tiles behind the GroupNorm pre-pass and the pointwise skip -- is the same shape without the residual:
V4_KSPLIT_GN_SKIP = ("v4_ksplit_gn_skip_nores", 1, (8, 4, 32), 96, 32, 128, 0, True, True, -1)
V4_CT32_GN_SKIP = ("v4_gn_concat_skip_nores", 2, (4, 8, 32), 32, 16, 64, 0, True, True, -1)
# 2 x (4 x 4 x 8) = 256 64-channel tiles, the fewest that take the 64-channel fast epilogue, with a partial x tile
V4_FAST = ("v4_fast_256_tiles_partial_x", 2, (32, 16, 120), 32, 0, 64, 0, False, False, -1)
V4_LOCAL = [V4_KSPLIT_GN_SKIP, V4_CT32_GN_SKIP, V4_FAST]

# name -> (GnInput, SkipKernel, K split); path 3.  v4_plain, v4_concat_nogn and v4_gn_concat_skip_nores have
# 8, 6 and 4 64-channel tiles and too few chunks to split: 32-channel tiles (CT32 epilogue);
# v4_fast_256_tiles_partial_x has 256: the 64-channel fast epilogue.  The others split K: slices + finish pass.
V4_EXACT = {
    "v4_plain": (GN_NONE, SKIP_NONE, None),
    "v4_concat_nogn": (GN_NONE, SKIP_NONE, None),
    "v4_gn_concat_skip_nores": (GN_APPLY, SKIP_PW, None),
    "v4_ksplit_gn_skip_nores": (GN_APPLY, SKIP_PW, "split"),
    "v4_ksplit_up": (GN_APPLY, SKIP_NONE, "split"),
    "v4_partial_x_gn_res": (GN_APPLY, SKIP_NONE, "split"),
    "v4_w26_up_res": (GN_APPLY, SKIP_NONE, "split"),
    "v4_fast_256_tiles_partial_x": (GN_NONE, SKIP_NONE, None),
}


def _v4_tiles(case):
    _, B, (D, H, W), _, _, cout = case[:6]
    return B * ((W + 31) // 32) * (H // 4) * (D // 4) * (cout // 64)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(V4_EXACT))
def test_v4_exact(name, dtype_name):
    """conv3d_v4.hpp forced on small shapes (path 3): the CT32 epilogue, the 64-channel fast epilogue,
    and K slices + conv3d_reduce_kernel's finish; GroupNorm by the cwdm_gn_apply pre-pass, the 1x1
    skip product through the residual slot.

    What is observed and what is not: cwdm_debug_conv_route reports the kernel and the K split, not which
    epilogue an unsplit launch takes.  CT32 against the 64-channel fast epilogue is inferred from a copy
    of route_launch's rule (conv_route.cpp: ct32 = 16-bit, one slice, plain output, fewer than 256
    64-channel tiles; _v4_tiles); if that threshold moved, these cases would run the other epilogue and
    still pass, exactly."""
    case = _case(K.V4_CASES + V4_LOCAL, name)
    gn, skip, ksplit = V4_EXACT[name]
    # which epilogue an unsplit 16-bit launch takes (conv_route.cpp route_launch: ct32 below 256 tiles)
    if name in ("v4_plain", "v4_concat_nogn", "v4_gn_concat_skip_nores"):
        assert _v4_tiles(case) < 256
    if name == "v4_fast_256_tiles_partial_x":
        assert _v4_tiles(case) == 256
    with _forced(path=3):
        _exact_forward(case, dtype_name, V4, gn=gn, skip=skip, ksplit=ksplit)


@pytest.mark.parametrize("path", [3, 2, 0])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["v4_ksplit_gn_skip", "v4_gn_concat_skip_res"])
def test_skip_plus_residual_shapes_are_brick_cases(name, dtype_name, path):
    """A 1x1 skip AND a residual: whatever path is forced, the brick kernels run it (GroupNorm and the
    skip inside the kernel), exactly."""
    with _forced(path=path):
        _exact_forward(_case(K.V4_CASES, name), dtype_name, BRICK)


V5_NAMES = ["v5_nogn_c192", "v5_w24_up_nogn", "v5_gn_res_2chunk", "v5_gn_concat_c128", "v5_partial_x_res",
            "v5_skip_c12"]


@pytest.mark.parametrize("cap", [1, 5, 0])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", V5_NAMES)
def test_v5_exact(name, dtype_name, cap):
    """conv3d_v5.hip (path 2) with the persistent grid capped at 1 / 5 workgroups or uncapped, per-tile
    statistics rows.  GroupNorm'd inputs go through the cwdm_gn_apply pre-pass (the default CWDM_V5 = 3;
    apply-ahead is switched off here and has its own test)."""
    case = _case(K.V5_CASES, name)
    with _forced(path=2, v5_grid=cap, aa=0):
        _exact_forward(case, dtype_name, V5, gn=GN_APPLY if case[7] else GN_NONE,
                       skip=SKIP_PW if case[8] else SKIP_NONE)


@pytest.mark.parametrize("cap", [1, 5])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["v5_gn_concat_c128", "v5_skip_c12"])
def test_v5_per_workgroup_rows_exact(name, dtype_name, cap):
    """cwdm_debug_stats_wg(1): batch 1, at most two channel tiles, no more workgroups than tiles -- each
    workgroup writes one row (both channel tiles, zeros where it ran none); the words behind those rows
    stay untouched."""
    case = _case(K.V5_CASES, name)
    assert case[1] == 1 and case[5] // 64 <= 2
    with _forced(path=2, v5_grid=cap, aa=0, wg=1):
        _exact_forward(case, dtype_name, V5, gn=GN_APPLY, skip=SKIP_PW if case[8] else SKIP_NONE, wg=True)


# aa_partial_x_res_8wg of AA_CASES shrunk from D = 24 to 20: 2 x 4 x 5 tiles on 8 workgroups = 5 sweep
# iterations; 4 input chunks -> lead 3: the ranges of iterations 3 and 4 are written ahead and waited on
AA_EXACT = ("aa_partial_x_res_8wg_d20", 1, (20, 16, 56), 64, 0, 64, 0, True, False, 0)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_v5_apply_ahead_exact(dtype_name):
    """Apply-ahead: the conv writes the SiLU(GroupNorm) copy of its input itself, range by range ahead
    of its sweep.  A partial x tile, a residual, per-tile statistics."""
    with _forced(path=2, v5_grid=8, aa=2) as L:
        n0 = L.cwdm_debug_v5_aa(-1)
        _exact_forward(AA_EXACT, dtype_name, V5_AA, gn=GN_IN_KERNEL, aa=True)
        assert L.cwdm_debug_v5_aa(-1) - n0 == 2, "the apply-ahead instance did not run"


@pytest.mark.parametrize("cap", [3, 0])
@pytest.mark.parametrize("name", ["x_partial_x_nogn", "x_w24_up_nogn"])
def test_split_bf16_accurate_mode_exact(name, cap):
    """conv3d_v5s_kernel (fp32 in / out on bf16 hi / lo splits): the lo halves of integer operands are
    zero, so hi.hi is the whole product and the result is exact too."""
    case = _case(K.SPLIT_CASES, name)
    with _forced(path=0, v5_grid=cap):
        _exact_forward(case, "fp32", V5_SPLIT, wsplit=True)


# name -> (GnInput, SkipKernel, K split)
SG_EXACT = {
    "sg8_up_nogn": (GN_NONE, SKIP_NONE, "any"),
    "sg12_concat_nogn": (GN_NONE, SKIP_NONE, "any"),
    "sg_odd_gn_res": (GN_APPLY, SKIP_NONE, "any"),
    "sg14_ksplit_skip": (GN_APPLY, SKIP_SG, "split"),
    "sg14_ksplit_res": (GN_APPLY, SKIP_NONE, "split"),
    "sg14_config5_concat_skip": (GN_APPLY, SKIP_SG, "any"),
    "sg20_up_res": (GN_APPLY, SKIP_NONE, "any"),
    "sg8_production": (GN_APPLY, SKIP_SG, "split"),
}


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(SG_EXACT))
def test_small_grid_exact(name, dtype_name):
    """conv3d_sg.hip on the default path: partial bricks on every axis (their zero-padded voxels are
    dropped from stores, residual and statistics), the K split of the 8^3 / 14-wide levels, the 1x1 skip
    through the same kernel; sg8_production with cin 512."""
    case = _case(K.SG_CASES, name)
    gn, skip, ksplit = SG_EXACT[name]
    _, tdt = _dt(dtype_name)
    ops = _operands(case, case[7])
    _assert_exact(tdt, ops.y, ops.y_conv, ops.y_skip, stats_of=ops.y)
    with _forced(path=0):
        d, out, st, keep = _desc_of(ops, case, dtype_name)
        r = _route(d)
        assert (r["kernel"], r["gn"], r["skip"]) == (SMALL_GRID, gn, skip), r
        if ksplit == "split":   # (elsewhere the library's work-item target decides)
            assert r["ksplit"] > 1, r
        _run_exact(d, out, st, ops.y)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", S2.FWD_SHAPES[1:], ids=S2._FWD_IDS[1:])
def test_stride2_route_exact(shape, dtype_name):
    """The stride-2 conv as it runs in the plan: cwdm_space_to_depth, then a stride-1 conv of the 8 cin
    deep tensor with cwdm_conv3d_pack_s2's expanded weights, statistics requested.  16-bit (3, 5, 7) with
    cout 64 is a small-grid conv (K split: 256 deep channels on few bricks), cout 96 a brick-kernel one."""
    from cwdm_hip._lib import lib
    cin, cout, grid, B = shape
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(20261022)
    x = _ints(g, -2, 2, B, cin, *[2 * s for s in grid])
    w = _tern(g, cout, cin, 3)
    bias = _ints(g, -4, 4, cout)
    y = F.conv3d(x, w, bias, stride=2, padding=1)
    _assert_exact(tdt, y, stats_of=y)
    deep = torch.full((B, *grid, 8 * cin), NAN, device=DEV, dtype=tdt)
    S2._space_to_depth(_nd(x).to(DEV, tdt), cin, B, grid, dtype, deep, 1, 0)
    packed = S2._pack_s2(w, cout, cin, dtype, 0)
    with _forced(path=0):
        d, out, st, keep = _desc(dtype_name, B, grid, cout, deep, packed, bias=bias.float().to(DEV))
        r = _route(d)
        want = SMALL_GRID if (dtype_name != "fp32" and cout % 64 == 0) else BRICK
        assert r["kernel"] == want, r
        if want == SMALL_GRID:
            assert r["ksplit"] > 1, r
        _run_exact(d, out, st, y)
    assert lib().cwdm_device_status(0) == 0


# HEAD_CASES[0], HEAD_CASES[3] and a cout of 3, each with the heads that take it: the first head
# (gen -1) needs W % 32, so W = 48 runs on the second one only (gen 0; 3: its grid capped at 3)
HEAD_EXACT = [(K.HEAD_CASES[0] + (8,), gen) for gen in (-1, 0, 3)] + [(K.HEAD_CASES[3] + (8,), gen) for gen in (0, 3)] + \
             [(K.HEAD_CASES[0] + (3,), gen) for gen in (-1, 0, 3)]
_GEN_ID = {-1: "head1", 0: "head2", 3: "head2_grid3"}


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,gen", HEAD_EXACT,
                         ids=[f"{'x'.join(map(str, s[0]))}_cout{s[3]}_{_GEN_ID[g]}" for s, g in HEAD_EXACT])
def test_output_heads_exact(shape, gen, dtype_name):
    """conv3d_head.hip: GroupNorm + SiLU staged in 16 bits, fp32 output, no statistics.

    The route says only that a head kernel runs, not which: gen selects the first head, the second, or
    the second on a grid of 3 through cwdm_debug_head2 as test_output_head_kernel_vs_torch does, and
    nothing reports back which instance was launched.  If that knob stopped working, every case would run
    the default head and still pass."""
    grid, B, cin, cout = shape
    case = (f"head_{cout}", B, grid, cin, 0, cout, 0, True, False, -1)
    ops = _operands(case, True)
    _assert_exact(torch.float32, ops.y)
    with _forced(path=0, head2=gen):
        d, out, st, keep = _desc_of(ops, case, dtype_name, out_f32=True, stats=False)
        _assert_route(d, HEAD, gn=GN_IN_KERNEL)
        _run_exact(d, out, None, ops.y)


# --------------------------------------------------------------------------- B. dgrad and pointwise
@functools.lru_cache(maxsize=1)
def _dgrad_operands(cfg):
    cin, cout, grid = cfg
    g = torch.Generator().manual_seed(20261023)
    w = _tern(g, cout, cin, 3, fan=cout)   # (a dgrad sums over cout)
    dy = _ints(g, -2, 2, 1, cout, *grid)
    return w, dy, torch.nn.grad.conv3d_input((1, cin, *grid), w, dy, padding=1)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("cfg", [(64, 64, (8, 8, 16)), (192, 64, (4, 8, 8)), (64, 8, (8, 8, 8)), (128, 256, (2, 2, 2))],
                         ids=lambda c: f"{c[0]}_{c[1]}_{'x'.join(map(str, c[2]))}")
def test_dgrad_packing_exact(cfg, dtype_name):
    """cwdm_conv3d_pack_dgrad (flipped, transposed weights; dy channels padded to the chunk) + forward
    against float64 conv3d_input; the padding channels of dy hold a non-zero integer times zero weights."""
    from cwdm_hip._lib import check, lib
    L = lib()
    cin, cout, grid = cfg
    dtype, tdt = _dt(dtype_name)
    ck = 8 if dtype_name == "fp32" else 16
    cpad = (cout + ck - 1) // ck * ck
    B = 1
    w, dy, ref = _dgrad_operands(cfg)
    _assert_exact(tdt, ref)
    pk = torch.empty(L.cwdm_conv3d_packed_bytes(cin, cpad, 3, dtype), dtype=torch.uint8, device=DEV)
    wd = w.float().to(DEV).contiguous()
    check(L.cwdm_conv3d_pack_dgrad(ctypes.c_void_p(wd.data_ptr()), cout, cin, 3, dtype, ctypes.c_void_p(pk.data_ptr()),
                                   None))
    a = torch.full((B, *grid, cpad), 3.0, device=DEV, dtype=tdt)
    a[..., :cout] = _nd(dy).to(DEV, tdt)
    with _forced(path=0):
        d, out, st, keep = _desc(dtype_name, B, grid, cin, a, pk, stats=False)
        _run_exact(d, out, None, ref)


B_ONLY_SHAPES = [(1, (4, 8, 16), 32, 40, 56), (2, (4, 4, 40), 64, 24, 48), (1, (4, 4, 64), 128, 128, 64),
                 (1, (3, 5, 7), 16, 8, 24), (2, (3, 4, 22), 64, 128, 64), (1, (2, 3, 40), 64, 64, 64),
                 (1, (2, 4, 12), 32, 20, 28)]


@functools.lru_cache(maxsize=1)
def _b_only_operands(shape):
    B, grid, cout, c0, c1 = shape
    g = torch.Generator().manual_seed(20261024)
    w = _tern(g, cout, c0 + c1, 1, fan=cout)
    dy = _ints(g, -2, 2, B, cout, *grid)
    base0, base1 = _ints(g, -8, 8, B, *grid, c0), _ints(g, -8, 8, B, *grid, c1)
    return w, dy, base0, base1, _nd(torch.nn.grad.conv3d_input((B, c0 + c1, *grid), w, dy))


@pytest.mark.parametrize("acc", [1, 0])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", B_ONLY_SHAPES, ids=lambda s: f"b{s[0]}_{'x'.join(map(str, s[1]))}_{s[2]}_{s[3]}_{s[4]}")
def test_b_only_dual_output_accumulate_exact(shape, dtype_name, acc):
    """The 1x1 skip dgrad (pw_kernel, 16-bit only): channel slices to two buffers, accumulating onto
    integer bases or storing.

    One epilogue only, the swapped-lane one (pw_kernel<T, false, 4>).  cwdm_debug_pw_lt chooses the
    row-major epilogue only for a launch that takes the fused GroupNorm-backward apply (pointwise.hip:
    lt = g_pw_lt && ga), which a lone cwdm_conv3d_forward never does and whose SiLU'(GroupNorm) arithmetic
    is not integer-exact; test_gpu_bwd_fusions.py and test_gpu_train.py cover it with float64 bounds and
    a bitwise on / off comparison.  The launch counter (cwdm_debug_pw_lt(-1)) must not move here."""
    from cwdm_hip._lib import check, lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    B, grid, cout, c0, c1 = shape
    cin = c0 + c1
    w, dy, base0, base1, prod = _b_only_operands(shape)
    ref = prod + acc * torch.cat([base0, base1], -1)   # (condition 1 applies to base + result)
    _assert_exact(tdt, ref, prod)
    pk = torch.empty(L.cwdm_conv3d_packed_bytes(cin, cout, 1, dtype), dtype=torch.uint8, device=DEV)
    wd = w.float().to(DEV).contiguous()
    check(L.cwdm_conv3d_pack_dgrad(ctypes.c_void_p(wd.data_ptr()), cout, cin, 1, dtype, ctypes.c_void_p(pk.data_ptr()),
                                   None))
    a = _nd(dy).to(DEV, tdt)
    with _forced(path=0):
        n_lt = L.cwdm_debug_pw_lt(-1)
        d, out, st, keep = _desc(dtype_name, B, grid, cin, None, None, b0=a, pb=pk, stats=False)
        assert _route(d)["kernel"] == POINTWISE
        outs = []
        for _ in range(2):   # (an accumulating call cannot run twice into the same buffers: fresh bases)
            o0, o1 = base0.to(DEV, tdt), base1.to(DEV, tdt)
            d.out, d.out1, d.out_c0, d.accumulate = o0.data_ptr(), o1.data_ptr(), c0, acc
            assert _route(d)["kernel"] == POINTWISE
            check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
            torch.cuda.synchronize()
            outs.append(torch.cat([o0, o1], -1).cpu())
        assert L.cwdm_debug_pw_lt(-1) == n_lt, "a lone 1x1 took the fused-apply (row-major) epilogue"
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(outs[0], ref.to(tdt))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_pointwise_two_sources_per_batch_bias_exact(dtype_name):
    """The forward skip product's shape: a pure 1x1 of two channels-last sources, per-batch integer bias
    (pw_kernel<T, false, 4>: see test_b_only_dual_output_accumulate_exact for the other epilogue)."""
    from cwdm_hip._lib import lib
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(20261025)
    B, grid, k0, k1, cout = 2, (4, 6, 36), 48, 16, 96
    x = _ints(g, -2, 2, B, k0 + k1, *grid)
    w = _tern(g, cout, k0 + k1, 1)
    bias = _ints(g, -4, 4, B, cout)
    ref = F.conv3d(x, w) + bias[:, :, None, None, None]
    _assert_exact(tdt, ref)
    xd = _nd(x).to(DEV, tdt)
    with _forced(path=0):
        n_lt = lib().cwdm_debug_pw_lt(-1)
        d, out, st, keep = _desc(dtype_name, B, grid, cout, None, None, b0=xd[..., :k0].contiguous(),
                                 b1=xd[..., k0:].contiguous(), pb=_pack(w, 1, dtype), bias=bias.float().to(DEV),
                                 bias_bs=cout, stats=False)
        assert _route(d)["kernel"] == POINTWISE
        _run_exact(d, out, None, ref)
        assert lib().cwdm_debug_pw_lt(-1) == n_lt


# --------------------------------------------------------------------------- C. wgrad
def _wgrad_kernel(case, dtype_name, cm):
    """The kernel cwdm_conv3d_wgrad dispatches to, from wgrad.hip's predicates in its order: hw_eligible
    (head_wgrad_kernel), wg1_eligible (wgrad1_kernel), u_cm (the DMA kernel: warp-specialised for cin <=
    cout, else 64-output tiles MC 2 above 32 outputs), else wgrad_kernel.

    A copy of wgrad.hip's wg1_eligible, hw_shape_ok / hw_eligible and the ws / mc rule and dispatch order
    in cwdm_conv3d_wgrad, at their defaults: the env knobs CWDM_HEAD_WG, CWDM_WG1_OFF and CWDM_WG_WS are
    taken as unset.  Nothing compares it with the library at run time, so it has to follow those
    predicates by hand when they change."""
    name, B, (D, H, W), c0, c1, cout, umode, use_gn, k, dy_cs = case
    half = dtype_name != "fp32"
    cin = c0 + c1
    if dtype_name == "fp32" and dy_cs == 16:
        dy_cs = 8
    if (k == 3 and 1 <= cout <= 8 and cin == 64 and half and umode == 0 and not cm and c1 == 0 and dy_cs >= 8 and
            dy_cs % 8 == 0 and W % 16 == 0 and H % 4 == 0 and D % 4 == 0):
        return "head_wgrad_kernel"
    if k == 1 and half and not use_gn and umode == 0 and not cm and c0 % 16 == 0 and cin % 32 == 0 and dy_cs % 8 == 0:
        return "wgrad1_kernel"
    if cm:
        assert half and k == 3 and c1 == 0
        return "dma_ws" if cin <= cout else ("dma_mc2" if cout > 32 else "dma_mc1")
    return "wgrad_kernel"


WG_EXACT = (
    [(n, False, "wgrad_kernel") for n in ("gn_64_64", "concat_odd", "up", "plain_in32", "tiny_grid")] +
    [(n, False, "head_wgrad_kernel") for n in ("head_hw_b2", "head_hw_cout3", "head_hw_nogn", "head_hw_straddle")] +
    [(n, False, "wgrad1_kernel") for n in ("skip1x1_r0", "skip1x1_cout40", "skip1x1_wide")] +
    [("cm_mc2_cin_gt_cout", True, "dma_mc2"), ("cm_ws_square", True, "dma_ws"), ("cm_ws_up_wide", True, "dma_ws"),
     ("cm_interior_ragged", True, "dma_ws"), ("cm_interior_cs_short", True, "dma_ws")])


def _wgrad_ref(h, dy, k):
    """dW[o, c, tap] = sum over batch and voxels of dy[o, v] h[c, v + tap - k // 2] (zero padding), float64,
    tap by tap."""
    B, cin = h.shape[:2]
    cout, (D, H, W) = dy.shape[1], dy.shape[2:]
    hp = F.pad(h, (k // 2,) * 6)
    dyf = dy.reshape(B, cout, -1)
    ref = torch.zeros(cout, cin, k, k, k, dtype=torch.float64)
    for kz in range(k):
        for ky in range(k):
            for kx in range(k):
                sl = hp[:, :, kz:kz + D, ky:ky + H, kx:kx + W].reshape(B, cin, -1)
                ref[:, :, kz, ky, kx] = torch.einsum("bov,bcv->oc", dyf, sl)
    return ref


@functools.lru_cache(maxsize=1)
def _wgrad_operands(case, use_gn):
    name, B, grid, c0, c1, cout, umode, _, k, dy_cs = case
    g = torch.Generator().manual_seed(20261026)
    D, H, W = grid
    sgrid = (D // 2, H // 2, W // 2) if umode == 1 else grid
    cin = c0 + c1
    if use_gn:   # (scale, shift) = (32, 0): the staged activation is 32 x
        x = _ints(g, 0, 3, B, cin, *sgrid)
        h_src = 32 * x
    else:
        x = _ints(g, -2, 2, B, cin, *sgrid)
        h_src = x
    h = F.interpolate(h_src, scale_factor=2, mode="nearest") if umode == 1 else h_src
    dy = _ints(g, -2, 2, B, cout, D, H, W)
    dw0 = _ints(g, -64, 64, cout, cin, k, k, k)
    return x, h_src, h, dy, dw0, _wgrad_ref(h, dy, k), _wgrad_ref(h.abs(), dy.abs(), k) + dw0.abs()


def _wgrad_exact(case, dtype_name, cm):
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    name, B, grid, c0, c1, cout, umode, use_gn, k, dy_cs = case
    dtype, tdt = _dt(dtype_name)
    if dtype_name == "fp32" and dy_cs == 16:
        dy_cs = 8
    use_gn = use_gn and not cm   # (u_cm hands the activated tensor over: no prologue)
    D, H, W = grid
    sgrid = (D // 2, H // 2, W // 2) if umode == 1 else grid
    cin = c0 + c1
    x, h_src, h, dy, dw0, ref, mag = _wgrad_operands(case, use_gn)
    # condition 3: per weight element, sum over batch and voxels of |h dy| plus |dw0| stays below 2^24
    # (all terms integers: the unit is 1), so dw0 + dW is exact in fp32 under any order and any slab split
    assert float(mag.max()) < 2 ** 24
    assert torch.equal(h.to(tdt).double(), h)
    xd = _nd(x).to(DEV, tdt)
    x0 = xd[..., :c0].contiguous()
    x1 = xd[..., c0:].contiguous() if c1 else None
    dyd = torch.full((B, D, H, W, dy_cs), 7.0, device=DEV, dtype=tdt)   # padding channels: ignored, not zero
    dyd[..., :cout] = _nd(dy).to(DEV, tdt)
    d = _lib.WgradDesc()
    d.dtype, d.B, d.D, d.H, d.W, d.ksize = dtype, B, D, H, W, k
    d.u0, d.u_c0 = x0.data_ptr(), c0
    d.u1, d.u_c1 = (x1.data_ptr(), c1) if c1 else (None, 0)
    d.u_mode = umode
    gnd = torch.tensor([32.0, 0.0]).repeat(B, cin, 1).to(DEV) if use_gn else None
    d.u_gn = gnd.data_ptr() if gnd is not None else None
    d.dy, d.dy_cs, d.cout = dyd.data_ptr(), dy_cs, cout
    if cm:
        sv = sgrid[0] * sgrid[1] * sgrid[2]
        act = _nd(h_src).reshape(B, sv, cin // 16, 16).permute(0, 2, 1, 3).contiguous().to(DEV, tdt)
        d.u0, d.u_c0, d.u1, d.u_c1, d.u_gn, d.u_cm = act.data_ptr(), cin, None, 0, None, 1
    wsw = torch.full((lib().cwdm_conv3d_wgrad_workspace_bytes(cout, cin, k),), 0xFF, dtype=torch.uint8, device=DEV)
    d.workspace, d.ws_bytes = wsw.data_ptr(), wsw.numel()
    dws = []
    for _ in range(2):
        dw = dw0.float().to(DEV)
        d.dw = dw.data_ptr()
        check(lib().cwdm_conv3d_wgrad(ctypes.byref(d), None))
        torch.cuda.synchronize()
        dws.append(dw.cpu())
    assert torch.equal(_bits(dws[0]), _bits(dws[1])), "a second call onto a fresh dw0 differs"
    got = dws[0].double() - dw0
    assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.numel()} dW elements differ"


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name,cm,kernel", WG_EXACT, ids=[w[0] for w in WG_EXACT])
def test_wgrad_exact(name, cm, kernel, dtype_name):
    """Every 16-bit kernel of wgrad.hip: dw - dw0 equals the float64 weight gradient, bit for bit."""
    case = _case(T.WG_CASES + T.CM_CASES, name)
    assert _wgrad_kernel(case, dtype_name, cm) == kernel
    _wgrad_exact(case, dtype_name, cm)


@pytest.mark.parametrize("name", ["plain_in32", "head_hw_nogn", "skip1x1_r0", "skip1x1_cout40", "skip1x1_wide"])
def test_wgrad_fp32_exact(name):
    """The fp32 instantiation of wgrad_kernel (every fp32 call takes it), cases without GroupNorm."""
    case = _case(T.WG_CASES, name)
    assert not case[7] and _wgrad_kernel(case, "fp32", False) == "wgrad_kernel"
    _wgrad_exact(case, "fp32", False)


# --------------------------------------------------------------------------- D. random data, both words
# Which tensor the emitted (sum, sum of squares) describe, read from each epilogue:
#   brick kernels (conv3d_kernels.hpp epilogue)        the fp32 value before the output rounding
#   v4 fast / CT32 epilogue (conv3d_v4.hpp)            the fp32 value before the output rounding
#   v4 K-split finish (conv3d_reduce_kernel)           the fp32 value before the output rounding (brick epilogue)
#   small-grid kernel (conv3d_sg.hip), K split or not  the fp32 value before the output rounding
#   v5, v5 apply-ahead, the phase instance             conv + bias as staged in 16 bits, plus the residual in
#                                                      fp32: the stored tensor without a residual / 1x1 skip,
#                                                      else the fp32 value before the (second) rounding
#   split-bf16 accurate mode (conv3d_v5s_kernel)       the stored fp32 output
# n_row: voxels one statistics row covers (32 x 4 x 4 tiles and bricks from W >= 24, 16 x 4 x 4 or 8 x 8 x 4
# bricks below: conv3d_kernels.hpp pick_brick).
# how: "f32" = the kernel writes fp32 on the same route (asserted), so the stored tensor is the summed one
#      "stored" = the statistics describe the stored tensor
#      "weak" = pre-rounding kernel that cannot write fp32 on its route: the float64 sums of the stored
#               16-bit output, with the storage rounding added to the bound
STATS_DESCRIBE = {
    "brick": ("pre-rounding fp32", "f32"),
    "v4_ksplit": ("pre-rounding fp32", "f32"),
    "v4_ct32": ("pre-rounding fp32", "weak"),     # fp32 output takes v4's general epilogue, not CT32 / fast
    "sg": ("pre-rounding fp32", "weak"),          # a lone fp32-output call is not a small-grid conv
    "v5": ("stored 16-bit", "stored"),
    "v5_res": ("16-bit conv + fp32 residual, pre-rounding", "weak"),   # v5 never writes fp32
    "split_bf16": ("stored fp32", "stored"),
    "brick_f32": ("stored fp32", "stored"),
    "v4_f32": ("stored fp32", "stored"),
}
U24 = 2.0 ** -24
STORE_EPS = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12, "fp32": 0.0}
_RATIOS = {}


def _random_desc(case, dtype_name, seed=7, **kw):
    """Device operands of _run_conv_case's recipe (randn inputs, weights / sqrt(27 cin), GroupNorm scale
    1 + 0.2 randn, shift 0.2 randn); no CPU reference: part D compares the statistics with the call's own output."""
    import math
    name, B, grid, c0, c1, cout, amode, use_gn, skip, rmode = case
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(seed)
    D, H, W = grid
    half, twice = (D // 2, H // 2, W // 2), (2 * D, 2 * H, 2 * W)
    cin = c0 + c1
    sgrid = {0: grid, 1: half, 2: twice}[amode]
    xd = torch.randn(B, *sgrid, cin, generator=g).to(DEV, tdt)
    a0 = xd[..., :c0].contiguous()
    a1 = xd[..., c0:].contiguous() if c1 else None
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    bias = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gn = None
    if use_gn:
        gn = torch.stack([1 + 0.2 * torch.randn(B, cin, generator=g), 0.2 * torch.randn(B, cin, generator=g)],
                         -1).contiguous().to(DEV)
    wb = torch.randn(cout, cin, 1, 1, 1, generator=g) / math.sqrt(cin) if skip else None
    res = None
    if rmode >= 0:
        res = torch.randn(B, *{0: grid, 1: half, 2: twice}[rmode], cout, generator=g).to(DEV, tdt)
    psplit = None
    if kw.pop("wsplit", False):
        from cwdm_hip._lib import check, lib
        L = lib()
        psplit = torch.empty(L.cwdm_conv3d_packed_split_bytes(cout, cin), dtype=torch.uint8, device=DEV)
        wd = w.contiguous().to(DEV)
        check(L.cwdm_conv3d_pack_split(ctypes.c_void_p(wd.data_ptr()), cout, cin, ctypes.c_void_p(psplit.data_ptr()), None))
    return _desc(dtype_name, B, grid, cout, a0, _pack(w, 3, dtype), a1=a1, amode=amode, gn=gn, bias=bias,
                 b0=a0 if skip else None, b1=a1 if skip else None, pb=_pack(wb, 1, dtype) if skip else None,
                 res=res, rmode=rmode, psplit=psplit, **kw)


def _stats_vs_output(route, case, dtype_name, kernel, n_row, *, ksplit=None, wsplit=False):
    """Both statistics words against float64 sums of the tensor they describe, within the fp32 summation
    bound  |d sum| <= n_row 2^-24 sum |y|,  |d sq| <= (n_row + 1) 2^-24 sum y^2  (a row adds n_row values,
    each square is rounded once; the rows themselves are added in float64 here).  These are derived, not
    measured.  ksplit: None = one slice, "split" = several, "any" = not asserted.

    The weak cases compare with the stored 16-bit tensor s = round(v) of the summed fp32 value v:
    |s - v| <= eps |s| with eps = 2^-9 (bf16) / 2^-12 (fp16) (half an ulp), so the storage term  eps sum |s|
    is added to the first bound and, from |s^2 - v^2| = |s - v| |s + v| <= (2 eps + eps^2) s^2, the term
    (2 eps + eps^2) sum s^2  to the second; nothing else is added (an fp16 subnormal's 2^-25 absolute
    error included: the bound stays the stated one).  This is the weak check: it sees a
    statistics error only above about eps of the sums."""
    from cwdm_hip._lib import check, lib
    L = lib()
    how = STATS_DESCRIBE[route][1]
    out_f32 = how == "f32" and dtype_name != "fp32"
    d, out, st, keep = _random_desc(case, dtype_name, out_f32=out_f32, wsplit=wsplit)
    r = _route(d)
    assert r["kernel"] == kernel, r
    if ksplit != "any":
        assert (r["ksplit"] > 1) == (ksplit == "split"), r
    if out_f32:   # the same route as the 16-bit-output call
        d16 = _random_desc(case, dtype_name, wsplit=wsplit)[0]
        r16 = _route(d16)
        assert (r16["kernel"], r16["gn"], r16["skip"], r16["ksplit"]) == (r["kernel"], r["gn"], r["skip"], r["ksplit"])
    check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
    torch.cuda.synchronize()
    s = st.cpu()
    assert torch.isfinite(s).all()
    tot = s.double().sum(1)
    y = out.cpu().double()
    sa, sq = y.abs().sum(dim=(1, 2, 3)), (y ** 2).sum(dim=(1, 2, 3))
    b_sum, b_sq = n_row * U24 * sa, (n_row + 1) * U24 * sq
    if how == "weak":
        eps = STORE_EPS[dtype_name]
        b_sum = b_sum + eps * sa
        b_sq = b_sq + (2 * eps + eps * eps) * sq
    e_sum, e_sq = (tot[..., 0] - y.sum(dim=(1, 2, 3))).abs(), (tot[..., 1] - sq).abs()
    r_sum, r_sq = float((e_sum / b_sum).max()), float((e_sq / b_sq).max())
    w = _RATIOS.setdefault(route, [0.0, 0.0])
    w[0], w[1] = max(w[0], r_sum), max(w[1], r_sq)
    print(f"stats error/bound {route} {case[0]} {dtype_name} ({how}): sum {r_sum:.3f} sq {r_sq:.3f}; "
          f"worst of the route so far: sum {w[0]:.3f} sq {w[1]:.3f}")
    assert r_sum <= 1.0 and r_sq <= 1.0, (case[0], r_sum, r_sq)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["gn_concat_skip", "same_res", "up_res"])
def test_stats_both_words_brick(name, dtype_name):
    case = _case(K.CASES, name)
    n_row = 512 if case[2][2] >= 24 else 256
    with _forced(path=1):
        _stats_vs_output("brick_f32" if dtype_name == "fp32" else "brick", case, dtype_name, BRICK, n_row)


def test_stats_both_words_brick_pooled_fp32():
    """The only a_mode 2 / res_mode 2 GroupNorm instance: fp32 brick kernels, 16 x 4 x 4 bricks."""
    with _forced(path=1):
        _stats_vs_output("brick_f32", _case(K.CASES, "down_pool_res"), "fp32", BRICK, 256)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_stats_both_words_brick_skip_plus_residual(dtype_name):
    """GroupNorm, 1x1 skip and residual in one brick launch (8 x 8 x 4 bricks), fp32 output on the same route."""
    with _forced(path=0):
        _stats_vs_output("brick", _case(K.SG_CASES, "sg_skip_plus_res_legacy"), dtype_name, BRICK, 256)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_stats_both_words_v5_apply_ahead(dtype_name):
    """The apply-ahead instance shares v5's drain; AA_EXACT has a residual: the weak case."""
    with _forced(path=2, v5_grid=8, aa=2) as L:
        n0 = L.cwdm_debug_v5_aa(-1)
        _stats_vs_output("v5_res", AA_EXACT, dtype_name, V5_AA, 512)
        assert L.cwdm_debug_v5_aa(-1) - n0 == 1


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["v4_ksplit_gn_skip_nores", "v4_ksplit_up", "v4_partial_x_gn_res", "v4_w26_up_res",
                                  "v4_gn_concat_skip_nores"])
def test_stats_both_words_v4(name, dtype_name):
    """The K-split finish writes fp32 on the same route; v4_gn_concat_skip_nores is unsplit on 4 tiles: in
    16 bits the CT32 epilogue, which cannot (the weak case); fp32 data splits K on its 8-channel chunks."""
    case = _case(K.V4_CASES + V4_LOCAL, name)
    ct32 = name == "v4_gn_concat_skip_nores"
    route = "v4_f32" if dtype_name == "fp32" else ("v4_ct32" if ct32 else "v4_ksplit")
    with _forced(path=3):
        if ct32 and dtype_name != "fp32":
            assert _v4_tiles(case) < 256
        ks = "any" if dtype_name == "fp32" else (None if ct32 else "split")
        _stats_vs_output(route, case, dtype_name, V4, 512, ksplit=ks)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["v5_gn_res_2chunk", "v5_gn_concat_c128", "v5_partial_x_res", "v5_skip_c12"])
def test_stats_both_words_v5(name, dtype_name):
    """Without a residual the statistics are those of the stored tensor; with one (or a 1x1 skip, added
    through the residual slot) they describe round16(conv + bias) + residual before its rounding: weak."""
    case = _case(K.V5_CASES, name)
    with _forced(path=2, v5_grid=5, aa=0):
        _stats_vs_output("v5_res" if (case[9] >= 0 or case[8]) else "v5", case, dtype_name, V5, 512)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["sg_odd_gn_res", "sg14_ksplit_skip", "sg14_ksplit_res", "sg14_config5_concat_skip",
                                  "sg20_up_res", "sg8_production"])
def test_stats_both_words_small_grid(name, dtype_name):
    """The weak case: the small-grid kernel sums fp32 values and a lone call cannot ask it for fp32 output."""
    case = _case(K.SG_CASES, name)
    with _forced(path=0):
        d = _random_desc(case, dtype_name)[0]
        ks = "split" if _route(d)["ksplit"] > 1 else None
        if "ksplit" in name or name == "sg8_production":
            assert ks == "split"
        _stats_vs_output("sg", case, dtype_name, SMALL_GRID, 256, ksplit=ks)


@pytest.mark.parametrize("name", ["x_gn_res", "x_gn_concat_c128"])
def test_stats_both_words_split_bf16(name):
    case = _case(K.SPLIT_CASES, name)
    with _forced(path=0, v5_grid=3):
        _stats_vs_output("split_bf16", case, "fp32", V5_SPLIT, 512, wsplit=True)


# --------------------------------------------------------------------------- E. producer -> finalize
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name,kernel", [("v5_partial_x_res", V5), ("sg_odd_gn_res", SMALL_GRID)])
def test_large_mean_rows_through_finalize(name, kernel, dtype_name):
    """bias = 64: the mean is several sigma, where E[y^2] - mean^2 cancels most.  The kernel's rows are
    exact integers, so cwdm_gn_finalize's mean / rstd differ from float64 group_norm statistics of the
    exact reference only by its double arithmetic and fp32 casts: rtol 1e-6."""
    from cwdm_hip._lib import check, lib
    L = lib()
    case = _case(K.V5_CASES + K.SG_CASES, name)
    _, B, grid, c0, c1, cout = case[:6]
    G, V = 32, grid[0] * grid[1] * grid[2]
    with _forced(path=2 if kernel == V5 else 0, v5_grid=5, aa=0):
        d, out, st, keep, ops = _exact_forward(case, dtype_name, kernel, use_gn=False, bias_const=64)
    yg = ops.y.reshape(B, G, -1)
    mean, var = yg.mean(-1), yg.var(-1, unbiased=False)
    assert float((mean.abs() / var.sqrt()).min()) > 3.0   # the cancellation the case is about
    gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    ss = torch.empty(B, cout, 2, device=DEV)
    mr = torch.empty(B, G, 2, device=DEV)
    check(L.cwdm_gn_finalize(ctypes.c_void_p(st.data_ptr()), st.shape[1], cout, None, 0, 0,
                             ctypes.c_void_p(gamma.data_ptr()), ctypes.c_void_p(beta.data_ptr()), G, B, V, 1e-5,
                             ctypes.c_void_p(ss.data_ptr()), ctypes.c_void_p(mr.data_ptr()), None))
    torch.cuda.synchronize()
    got = mr.cpu().double()
    assert torch.allclose(got[..., 0], mean, rtol=1e-6, atol=0)
    assert torch.allclose(got[..., 1], 1 / torch.sqrt(var + 1e-5), rtol=1e-6, atol=0)
