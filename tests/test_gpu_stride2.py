"""The stride-2 convolution path (resblock_updown=False: csrc/stride2.hip and
the stride-2 branch of the weight pack in csrc/conv3d.hip) kernel by kernel
through the C ABI, against plain PyTorch-CPU references of the same operation.

The references are this file's own space-to-depth / expanded-weight helpers;
test_s2_reference_helpers_cpu pins them (float64, no GPU) before any kernel
is compared with them.  Permutations, single adds and integer-valued
convolutions are compared bit for bit."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

# (one CPU test lives here, so the mark sits on each GPU test, not on the module)
gpu = pytest.mark.gpu
DEV = "cuda"
DTYPES = ["fp32", "bf16", "fp16"]


def _dt(name):
    from cwdm_hip import _lib
    return {"fp32": (_lib.CWDM_F32, torch.float32), "bf16": (_lib.CWDM_BF16, torch.bfloat16),
            "fp16": (_lib.CWDM_F16, torch.float16)}[name]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _nd(x):  # NCDHW -> NDHWC
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _nc(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


# --------------------------------------------------------------------------- CPU references
def s2d(x):
    """[B, C, 2d, 2h, 2w] -> [B, 8C, d, h, w], channel ph * C + c with ph = 4 pz + 2 py + px."""
    B, C, D2, H2, W2 = x.shape
    d, h, w = D2 // 2, H2 // 2, W2 // 2
    return x.reshape(B, C, d, 2, h, 2, w, 2).permute(0, 3, 5, 7, 1, 2, 4, 6).reshape(B, 8 * C, d, h, w)


def d2s(y):
    """Inverse of s2d."""
    B, C8, d, h, w = y.shape
    C = C8 // 8
    return y.reshape(B, 2, 2, 2, C, d, h, w).permute(0, 4, 5, 1, 6, 2, 7, 3).reshape(B, C, 2 * d, 2 * h, 2 * w)


def _orig_tap(t, p):
    """Original tap carried by expanded tap t at phase p along one axis, or None (a zero weight)."""
    if t == 1:
        return 1 + p
    if t == 0 and p == 1:
        return 0
    return None


def expand(w):
    """[cout, cin, 3, 3, 3] -> [cout, 8 cin, 3, 3, 3]: the stride-1 kernel over s2d(x) of the stride-2 conv."""
    cout, cin = w.shape[:2]
    we = torch.zeros(cout, 8 * cin, 3, 3, 3, dtype=w.dtype)
    for ph in range(8):
        pz, py, px = ph >> 2, (ph >> 1) & 1, ph & 1
        for tz in range(3):
            for ty in range(3):
                for tx in range(3):
                    k = (_orig_tap(tz, pz), _orig_tap(ty, py), _orig_tap(tx, px))
                    if None not in k:
                        we[:, ph * cin:(ph + 1) * cin, tz, ty, tx] = w[:, :, k[0], k[1], k[2]]
    return we


# original tap k -> the one (phase, expanded tap) that holds it, per axis (written out, not derived from expand)
_FOLD = {0: (1, 0), 1: (0, 1), 2: (1, 1)}


def fold(we):
    """[cout, 8 cin, 3, 3, 3] -> [cout, cin, 3, 3, 3]: gather each original weight from its slot."""
    cout, cin = we.shape[0], we.shape[1] // 8
    w = torch.empty(cout, cin, 3, 3, 3, dtype=we.dtype)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                (pz, tz), (py, ty), (px, tx) = _FOLD[kz], _FOLD[ky], _FOLD[kx]
                ph = 4 * pz + 2 * py + px
                w[:, :, kz, ky, kx] = we[:, ph * cin:(ph + 1) * cin, tz, ty, tx]
    return w


def test_s2_reference_helpers_cpu():
    g = torch.Generator().manual_seed(20)
    for B, cin, cout, grid in [(2, 3, 5, (1, 1, 1)), (1, 4, 2, (2, 3, 4)), (2, 2, 3, (3, 5, 2))]:
        x = torch.randint(-4, 5, (B, cin, *[2 * s for s in grid]), generator=g).double()
        w = torch.randint(-4, 5, (cout, cin, 3, 3, 3), generator=g).double()
        xs = s2d(x)
        assert xs.shape == (B, 8 * cin, *grid)
        # the layout, element by element: channel ph * C + c of coarse voxel o is x[2 o + p]
        for ph in range(8):
            pz, py, px = ph >> 2, (ph >> 1) & 1, ph & 1
            assert torch.equal(xs[:, ph * cin:(ph + 1) * cin], x[:, :, pz::2, py::2, px::2])
        assert torch.equal(d2s(xs), x)
        we = expand(w)
        assert torch.equal(F.conv3d(xs, we, padding=1), F.conv3d(x, w, stride=2, padding=1))
        assert torch.equal(fold(we), w)
        # the 27 slots fold reads are exactly the non-zero ones of expand(ones)
        ones = expand(torch.ones(1, 1, 3, 3, 3, dtype=torch.float64))
        assert int(ones.sum()) == 27
        junk = torch.randn(cout, 8 * cin, 3, 3, 3, generator=g).double()
        mask = ones.repeat_interleave(cin, 1).bool().expand_as(junk)
        assert torch.equal(fold(torch.where(mask, we, junk)), w)


# --------------------------------------------------------------------------- ABI helpers
def _space_to_depth(src, C, B, grid, dtype, out, to_depth, accumulate):
    from cwdm_hip._lib import check, lib
    check(lib().cwdm_space_to_depth(src.data_ptr(), C, B, *grid, dtype, out.data_ptr(), to_depth, accumulate, None))
    torch.cuda.synchronize()


def _pack_s2(w, cout, cin, dtype, transpose):
    """cwdm_conv3d_pack_s2 of OIDHW fp32 weights (CPU tensor); returns the packed device buffer."""
    from cwdm_hip._lib import check, lib
    L = lib()
    ck = 8 if dtype == 0 else 16
    if transpose:
        nbytes = L.cwdm_conv3d_packed_bytes(8 * cin, (cout + ck - 1) // ck * ck, 3, dtype)
    else:
        nbytes = L.cwdm_conv3d_packed_bytes(cout, 8 * cin, 3, dtype)
    assert nbytes > 0
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wd = w.float().contiguous().to(DEV)
    check(L.cwdm_conv3d_pack_s2(wd.data_ptr(), cout, cin, dtype, buf.data_ptr(), transpose, None))
    torch.cuda.synchronize()
    return buf


def _conv(dtype, tdt, a, packed, cout, bias=None, split=True):
    """cwdm_conv3d_forward of the channels-last device tensor a with packed 3x3x3 weights."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    B, D, H, W, cin = a.shape
    out = torch.empty(B, D, H, W, cout, device=DEV, dtype=tdt)
    d = _lib.ConvDesc()
    d.dtype, d.B, d.D, d.H, d.W, d.cout = dtype, B, D, H, W, cout
    d.a0, d.a_c0, d.a_w = a.data_ptr(), cin, packed.data_ptr()
    bd = bias.float().to(DEV) if bias is not None else None
    d.bias = bd.data_ptr() if bd is not None else None
    d.res_mode = -1
    d.out, d.out_dtype = out.data_ptr(), dtype
    nws = L.cwdm_conv3d_workspace_bytes(ctypes.byref(d))
    assert nws >= 0
    ws = None
    if nws > 0 and split:
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        d.workspace, d.ws_bytes = ws.data_ptr(), nws
    check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
    torch.cuda.synchronize()
    return out


def _ints(g, *shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# --------------------------------------------------------------------------- 1. space-to-depth
S2D_GRIDS = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (4, 4, 8)]
S2D_C = {"fp32": [4, 8, 48], "bf16": [8, 16, 48], "fp16": [8, 16, 48]}   # from one 16-byte row up


@gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("grid", S2D_GRIDS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_space_to_depth_layout_and_round_trip(dtype_name, grid, B):
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(21)
    for C in S2D_C[dtype_name]:
        x = torch.randn(B, C, *[2 * s for s in grid], generator=g).to(tdt)
        xd = _nd(x).to(DEV)
        deep = torch.full((B, *grid, 8 * C), float("nan"), device=DEV, dtype=tdt)
        _space_to_depth(xd, C, B, grid, dtype, deep, 1, 0)
        assert torch.equal(deep.cpu(), _nd(s2d(x))), (C, "to_depth")
        back = torch.full_like(xd, float("nan"))
        _space_to_depth(deep, C, B, grid, dtype, back, 0, 0)
        assert torch.equal(back.cpu(), _nd(x)), (C, "from_depth")


@gpu
def test_space_to_depth_refusals():
    from cwdm_hip import _lib
    from cwdm_hip._lib import lib
    L = lib()
    buf = torch.zeros(4096, device=DEV)
    out = torch.full((4096,), 7.0, device=DEV)
    for dtype, C in [(_lib.CWDM_F32, 2), (_lib.CWDM_F32, 6), (_lib.CWDM_BF16, 4), (_lib.CWDM_F16, 12)]:
        for to_depth in (0, 1):
            assert L.cwdm_space_to_depth(buf.data_ptr(), C, 1, 2, 2, 2, dtype, out.data_ptr(), to_depth, 0,
                                         None) == _lib.E_SHAPE
    assert L.cwdm_space_to_depth(None, 8, 1, 2, 2, 2, _lib.CWDM_F32, out.data_ptr(), 1, 0, None) == _lib.E_INVALID
    assert L.cwdm_space_to_depth(buf.data_ptr(), 8, 1, 2, 2, 2, _lib.CWDM_F32, None, 1, 0, None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched


# --------------------------------------------------------------------------- 2. accumulate
@gpu
@pytest.mark.parametrize("to_depth", [1, 0], ids=["to_depth", "from_depth"])
@pytest.mark.parametrize("grid,B", [((1, 1, 1), 1), ((3, 5, 7), 2), ((4, 4, 8), 1)],
                         ids=["1x1x1", "3x5x7_b2", "4x4x8"])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_space_to_depth_accumulate_bitexact(dtype_name, grid, B, to_depth):
    """dst += permuted src: one fp32 add and one rounding to nearest even per element
    (pack2 is a plain float -> bf16 / fp16 vector conversion)."""
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(22)
    for C in S2D_C[dtype_name]:
        fine = torch.randn(B, C, *[2 * s for s in grid], generator=g).to(tdt)
        deep = torch.randn(B, 8 * C, *grid, generator=g).to(tdt)
        if to_depth:
            src, dst0, perm = _nd(fine), _nd(deep), _nd(s2d(fine))
        else:
            src, dst0, perm = _nd(deep), _nd(fine), _nd(d2s(deep))
        dst = dst0.to(DEV).clone()
        _space_to_depth(src.to(DEV), C, B, grid, dtype, dst, to_depth, 1)
        want = (dst0.float() + perm.float()).to(tdt)
        assert torch.equal(dst.cpu(), want), C


# --------------------------------------------------------------------------- 3. forward
FWD_SHAPES = [
    # cin, cout, coarse grid, B
    (16, 32, (2, 2, 2), 1),
    (32, 64, (3, 5, 7), 2),
    (48, 96, (4, 8, 16), 1),
]
_FWD_IDS = [f"{s[0]}_{s[1]}_{'x'.join(map(str, s[2]))}_b{s[3]}" for s in FWD_SHAPES]


def _s2_forward(dtype, tdt, x, w, bias, split):
    """x NCDHW (CPU, already representable in tdt) -> stride-2 conv output NCDHW (CPU float)."""
    B, cin = x.shape[:2]
    grid = tuple(s // 2 for s in x.shape[2:])
    cout = w.shape[0]
    deep = torch.empty(B, *grid, 8 * cin, device=DEV, dtype=tdt)
    _space_to_depth(_nd(x).to(DEV, tdt), cin, B, grid, dtype, deep, 1, 0)
    packed = _pack_s2(w, cout, cin, dtype, 0)
    return _nc(_conv(dtype, tdt, deep, packed, cout, bias=bias, split=split).float().cpu())


@gpu
@pytest.mark.parametrize("split", [True, False], ids=["splitk", "nosplit"])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_FWD_IDS)
def test_s2_forward_integer_operands_exact(shape, split):
    """Integers in [-4, 4]: every product and partial sum is an integer below
    27 * 48 * 16 + 4 < 2^24, exact in fp32 in any summation order."""
    cin, cout, grid, B = shape
    dtype, tdt = _dt("fp32")
    g = torch.Generator().manual_seed(23)
    x = _ints(g, B, cin, *[2 * s for s in grid])
    w = _ints(g, cout, cin, 3, 3, 3)
    bias = _ints(g, cout)
    ref = F.conv3d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    assert float(ref.abs().max()) < 2 ** 24 and 27 * cin * 16 + 4 < 2 ** 24
    got = _s2_forward(dtype, tdt, x, w, bias, split)
    assert torch.equal(got.double(), ref)


@gpu
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_FWD_IDS)
def test_s2_forward_vs_float64(shape, dtype_name):
    cin, cout, grid, B = shape
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(B, cin, *[2 * s for s in grid], generator=g).to(tdt).float()
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(tdt).float()
    bias = torch.randn(cout, generator=g) * 0.1
    ref = F.conv3d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    got = _s2_forward(dtype, tdt, x, w, bias, True)
    tol = {"fp32": 2e-5, "bf16": 2e-2, "fp16": 3e-3}[dtype_name]   # output rounding: 2^-8 / 2^-11
    err = rel_err(got, ref)
    print(f"s2 forward {dtype_name} {shape}: rel err {err:.3e}")
    assert err < tol


# --------------------------------------------------------------------------- 4. dgrad
DG_SHAPES = [
    # cin, cout, coarse grid, B  (cout 8 and 24 are zero-padded to the 16-channel chunk for bf16 / fp16)
    (16, 8, (2, 2, 2), 1),
    (8, 24, (3, 5, 7), 2),
    (32, 64, (4, 4, 8), 1),
]
_DG_IDS = [f"{s[0]}_{s[1]}_{'x'.join(map(str, s[2]))}_b{s[3]}" for s in DG_SHAPES]


def _s2_dgrad(dtype, tdt, dy, w, cin, base, acc, pad_fill=0.0):
    """dy NCDHW (CPU) -> the gradient buffer after the chain pack(transpose) / conv / depth-to-space,
    NCDHW CPU float.  base (NDHWC, tdt) is what the buffer held before."""
    B, cout = dy.shape[:2]
    grid = tuple(dy.shape[2:])
    ck = 8 if tdt == torch.float32 else 16
    cpad = (cout + ck - 1) // ck * ck
    a = torch.full((B, *grid, cpad), pad_fill, device=DEV, dtype=tdt)
    a[..., :cout] = _nd(dy).to(DEV, tdt)
    packed = _pack_s2(w, cout, cin, dtype, 1)
    deep = _conv(dtype, tdt, a, packed, 8 * cin)
    dx = base.to(DEV).clone()
    _space_to_depth(deep, cin, B, grid, dtype, dx, 0, acc)
    return _nc(dx.float().cpu())


@gpu
@pytest.mark.parametrize("acc", [1, 0], ids=["acc", "store"])
@pytest.mark.parametrize("shape", DG_SHAPES, ids=_DG_IDS)
def test_s2_dgrad_integer_operands_exact(shape, acc):
    cin, cout, grid, B = shape
    dtype, tdt = _dt("fp32")
    g = torch.Generator().manual_seed(25)
    fine = [2 * s for s in grid]
    w = _ints(g, cout, cin, 3, 3, 3)
    dy = _ints(g, B, cout, *grid)
    base = _ints(g, B, *fine, cin) if acc else torch.full((B, *fine, cin), float("nan"))
    ref = torch.nn.grad.conv3d_input((B, cin, *fine), w.double(), dy.double(), stride=2, padding=1)
    if acc:
        ref = ref + _nc(base).double()
    assert 27 * cout * 16 + 4 < 2 ** 24
    got = _s2_dgrad(dtype, tdt, dy, w, cin, base, acc)
    assert torch.equal(got.double(), ref)


@gpu
@pytest.mark.parametrize("acc", [1, 0], ids=["acc", "store"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shape", DG_SHAPES, ids=_DG_IDS)
def test_s2_dgrad_vs_torch(shape, dtype_name, acc):
    cin, cout, grid, B = shape
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(26)
    fine = [2 * s for s in grid]
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(tdt).float()
    dy = torch.randn(B, cout, *grid, generator=g).to(tdt).float()
    ref = torch.nn.grad.conv3d_input((B, cin, *fine), w.double(), dy.double(), stride=2, padding=1)
    if acc:   # a base gradient of the size of the result
        base = (float(ref.abs().max()) * 0.5 * torch.randn(B, *fine, cin, generator=g)).to(tdt)
        ref = ref + _nc(base).double()
    else:
        base = torch.full((B, *fine, cin), float("nan")).to(tdt)
    got = _s2_dgrad(dtype, tdt, dy, w, cin, base, acc)
    tol = 2e-5 if dtype_name == "fp32" else 2e-2
    err = rel_err(got, ref)
    print(f"s2 dgrad {dtype_name} {shape} acc={acc}: rel err {err:.3e}")
    assert err < tol


@gpu
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", DG_SHAPES[:2], ids=_DG_IDS[:2])
def test_s2_dgrad_padded_channels_have_zero_weights(shape, dtype_name):
    """The transposed pack zeroes the weights of dy's padding channels [cout, 16k): whatever
    (finite) those channels hold, the result is bit for bit the zero-padded one."""
    cin, cout, grid, B = shape
    dtype, tdt = _dt(dtype_name)
    assert cout % 16
    g = torch.Generator().manual_seed(26)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(tdt).float()
    dy = torch.randn(B, cout, *grid, generator=g).to(tdt).float()
    base = torch.full((B, *[2 * s for s in grid], cin), float("nan")).to(tdt)
    zero = _s2_dgrad(dtype, tdt, dy, w, cin, base, 0)
    junk = _s2_dgrad(dtype, tdt, dy, w, cin, base, 0, pad_fill=1000.0)
    assert torch.equal(zero, junk)


# --------------------------------------------------------------------------- 5. wgrad + fold
WG_SHAPES = [
    # cin, cout, coarse grid, B
    (16, 32, (2, 2, 2), 1),
    (8, 24, (3, 5, 7), 2),
    (32, 64, (4, 4, 8), 1),
]
_WG_IDS = [f"{s[0]}_{s[1]}_{'x'.join(map(str, s[2]))}_b{s[3]}" for s in WG_SHAPES]


def _fold_dw(dwe, cout, cin, dw, acc):
    from cwdm_hip._lib import check, lib
    check(lib().cwdm_conv3d_s2_fold_dw(dwe.data_ptr(), cout, cin, dw.data_ptr(), acc, None))
    torch.cuda.synchronize()


def _s2_wgrad(dtype, tdt, x, dy, base, acc):
    """x, dy NCDHW (CPU) -> dw [cout, cin, 3, 3, 3] (CPU) after wgrad over the space-to-depth
    activation into a zeroed expanded gradient and the fold onto base."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    B, cin = x.shape[:2]
    cout = dy.shape[1]
    grid = tuple(dy.shape[2:])
    deep = torch.empty(B, *grid, 8 * cin, device=DEV, dtype=tdt)
    _space_to_depth(_nd(x).to(DEV, tdt), cin, B, grid, dtype, deep, 1, 0)
    dyd = _nd(dy).to(DEV, tdt)
    dwe = torch.zeros(cout, 8 * cin, 27, device=DEV)
    nws = L.cwdm_conv3d_wgrad_workspace_bytes(cout, 8 * cin, 3)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    d = _lib.WgradDesc()
    d.dtype, d.B, (d.D, d.H, d.W), d.ksize = dtype, B, grid, 3
    d.u0, d.u_c0, d.u_mode = deep.data_ptr(), 8 * cin, 0
    d.dy, d.dy_cs, d.cout = dyd.data_ptr(), cout, cout
    d.dw = dwe.data_ptr()
    d.workspace, d.ws_bytes = ws.data_ptr(), nws
    check(L.cwdm_conv3d_wgrad(ctypes.byref(d), None))
    dw = base.to(DEV).clone()
    _fold_dw(dwe, cout, cin, dw, acc)
    return dw.cpu()


@gpu
@pytest.mark.parametrize("acc", [1, 0], ids=["acc", "store"])
@pytest.mark.parametrize("shape", WG_SHAPES, ids=_WG_IDS)
def test_s2_wgrad_fold_integer_operands_exact(shape, acc):
    cin, cout, grid, B = shape
    dtype, tdt = _dt("fp32")
    g = torch.Generator().manual_seed(27)
    x = _ints(g, B, cin, *[2 * s for s in grid])
    dy = _ints(g, B, cout, *grid)
    base = _ints(g, cout, cin, 3, 3, 3, lo=-64, hi=64) if acc else torch.full((cout, cin, 3, 3, 3), float("nan"))
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dy.double(), stride=2, padding=1)
    if acc:
        ref = ref + base.double()
    assert B * math.prod(grid) * 16 + 64 < 2 ** 24
    got = _s2_wgrad(dtype, tdt, x, dy, base, acc)
    assert torch.equal(got.double(), ref)


@gpu
@pytest.mark.parametrize("acc", [1, 0], ids=["acc", "store"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", WG_SHAPES, ids=_WG_IDS)
def test_s2_wgrad_fold_vs_torch(shape, dtype_name, acc):
    cin, cout, grid, B = shape
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(28)
    x = torch.randn(B, cin, *[2 * s for s in grid], generator=g).to(tdt).float()
    dy = torch.randn(B, cout, *grid, generator=g).to(tdt).float()
    base = _ints(g, cout, cin, 3, 3, 3) if acc else torch.full((cout, cin, 3, 3, 3), float("nan"))
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dy.double(), stride=2, padding=1)
    got = _s2_wgrad(dtype, tdt, x, dy, base, acc)
    if acc:
        got = got - base
    err = rel_err(got, ref)
    print(f"s2 wgrad {dtype_name} {shape} acc={acc}: rel err {err:.3e}")
    assert err < 1e-2


@gpu
@pytest.mark.parametrize("acc", [1, 0], ids=["acc", "store"])
@pytest.mark.parametrize("cout,cin", [(1, 1), (5, 3), (32, 16), (24, 40)])
def test_s2_fold_alone_bitexact(cout, cin, acc):
    """Random floats in every slot of the expanded gradient, the 189 of 216 the
    fold must ignore included: dw is the CPU gather (plus base: one fp32 add)."""
    g = torch.Generator().manual_seed(29)
    dwe = torch.randn(cout, 8 * cin, 3, 3, 3, generator=g)
    base = torch.randn(cout, cin, 3, 3, 3, generator=g) if acc else torch.full((cout, cin, 3, 3, 3), float("nan"))
    dw = base.to(DEV).clone()
    _fold_dw(dwe.to(DEV), cout, cin, dw, acc)
    want = base + fold(dwe) if acc else fold(dwe)
    assert torch.equal(dw.cpu(), want)
