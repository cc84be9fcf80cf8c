"""The warp-specialised conv's chunk loop (conv3d_v5.hip, V5_STEP) issues the
next step's LDS operand reads and the weight loads two groups ahead inside the
MFMA gaps, behind counted waits.  The counts are right only if every step finds
exactly the groups in flight that its wait assumes -- across the chunk seam, the
tile seam (the next tile's first groups, possibly of another channel tile) and
the dummy reloads after the last tile.  test_gpu_kernels.py covers 2, 4, 6, 8 and
12 chunks per tile; these cases add the shortest tiles the launcher takes, an odd
chunk count (another phase of the three-slot weight ring), three channel tiles
walked by one workgroup, the gather instance at the W = 24 edge, and bit-exact
comparisons against the independent v4 kernel.

The launcher refuses Cin = 16 (v5_eligible: a tile's drain spans two chunks), so
the "shortest tile" cases run Cin = 32, two chunks, the smallest it accepts."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import DEV, _DTN, _conv_call, _nc, _nd, rel_err

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case_data(B, grid, cin, cout, amode, dtype_name):
    """Operands quantised to the compute dtype and the fp64 F.conv3d reference (computed once per case)."""
    tdt = _DTN[dtype_name][1]
    g = torch.Generator().manual_seed(23)
    D, H, W = grid
    sD, sH, sW = (D // 2, H // 2, W // 2) if amode == 1 else (D, H, W)
    x = torch.randn(B, cin, sD, sH, sW, generator=g).to(tdt).float()
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(tdt).float()
    bias = torch.randn(cout, generator=g) * 0.1
    h = F.interpolate(x, scale_factor=2, mode="nearest") if amode == 1 else x
    ref = F.conv3d(h.double(), w.double(), bias.double(), padding=1)
    return x, w, bias, ref


def _run(B, grid, cin, cout, amode, dtype_name, cap):
    from cwdm_hip._lib import lib
    L = lib()
    dtype, tdt = _DTN[dtype_name]
    x, w, bias, ref = _case_data(B, grid, cin, cout, amode, dtype_name)
    D, H, W = grid
    prev, prevg = L.cwdm_conv3d_set_path(2), L.cwdm_debug_v5_grid(cap)
    try:
        out, st = _conv_call(dtype, (B, D, H, W), _nd(x).to(DEV, tdt), None, amode, None, w.to(DEV), bias.to(DEV))
    finally:
        L.cwdm_conv3d_set_path(prev)
        L.cwdm_debug_v5_grid(prevg)
    got = _nc(out.float().cpu())
    # the tolerance of test_conv3d_v5_kernel_vs_torch: the output rounding (2^-8 / 2^-11)
    tol = {"bf16": 2e-2, "fp16": 3e-3}[dtype_name]
    err = rel_err(got, ref)
    print(f"rel_err {err:.3e} (tol {tol:g})")
    assert err < tol
    s = st.sum(1).cpu().double()
    assert torch.allclose(s[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-3, atol=1e-2 * ref.abs().max().item() * 8)


@pytest.mark.parametrize("cap", [1, 3, 0])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cin", [32, 48], ids=["2chunk", "3chunk"])
def test_v5_short_tiles_vs_torch(cin, dtype_name, cap):
    """Two chunks (the fewest the launcher takes: most of a tile's weight prefetch then belongs to
    the next chunk or tile) and three (odd: the weight ring enters every chunk in another slot phase
    than the 2- and 4-chunk cases); capped at 1 one workgroup walks all four tiles and the prefetch
    crosses every tile seam."""
    _run(2, (4, 8, 32), cin, 64, 0, dtype_name, cap)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_v5_three_channel_tiles_one_workgroup(dtype_name):
    """Cout = 192 at cap 1: the tile-seam prefetch (nxt) crosses channel tiles 0 -> 1 -> 2 -> 0."""
    _run(2, (4, 8, 32), 32, 192, 0, dtype_name, 1)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cin", [32, 48], ids=["2chunk", "3chunk"])
def test_v5_gather_instance_w24(cin, dtype_name):
    """The gather instance (MODE 1: a nearest-x2 upsampled source) on one partial x tile per line."""
    _run(2, (4, 8, 24), cin, 64, 1, dtype_name, 1)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cin", [32, 48], ids=["2chunk", "3chunk"])
def test_v5_short_tiles_bitexact_vs_v4(cin, dtype_name):
    """The scheme of test_conv3d_v5_bitexact_vs_v4 (paths 3 and 2, no residual, equal 16-bit words)
    at the smallest kind of grid where path 3 is plain v4: 256 tiles of 64 channels (2 x 2 x 8 x 2
    spatial x 4 channel tiles), below which v4 splits K or runs 32-channel tiles."""
    from cwdm_hip._lib import lib
    L = lib()
    dtype, tdt = _DTN[dtype_name]
    B, (D, H, W), cout = 2, (8, 32, 64), 256
    g = torch.Generator().manual_seed(29)
    a0 = torch.randn(B, D, H, W, cin, generator=g).to(DEV, tdt)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(DEV)
    bias = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    outs = {}
    for path in (3, 2):
        prev, prevg = L.cwdm_conv3d_set_path(path), L.cwdm_debug_v5_grid(7)
        try:
            outs[path] = _conv_call(dtype, (B, D, H, W), a0, None, 0, None, w, bias)
        finally:
            L.cwdm_conv3d_set_path(prev)
            L.cwdm_debug_v5_grid(prevg)
    (o4, s4), (o5, s5) = outs[3], outs[2]
    assert torch.equal(o4.view(torch.int16), o5.view(torch.int16))
    assert rel_err(s5.cpu(), s4.cpu()) < {"bf16": 2e-3, "fp16": 3e-4}[dtype_name]
