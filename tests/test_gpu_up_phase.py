"""Nearest-x2 upsampling convs as eight 2x2x2 phase convs in one launch of the
warp-specialised kernel (conv3d_v5.hip MODE 2, cwdm_conv3d_desc.a_w_phase,
DESIGN.md §3f): the phase path against the 27-tap gather path, against the
definition, its GroupNorm statistics, the weight pack, and through the U-Net
plan.  Output grids are (D, H, W); the lone convs run on kernel path 2 (the
DMA-staged kernels wherever the shape allows), as the v5 cases of
test_gpu_kernels.py do."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the bounds test_gpu_kernels.py applies to its v5_up_* cases (_run_conv_case): max-norm relative
# error of the output (16-bit output rounding: 2^-8 / 2^-11), and its statistics check
CONV_TOL = {"bf16": 2e-2, "fp16": 3e-3}
# unit roundoff of one 16-bit weight (8 / 11 significand bits)
W_EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
# test_gpu_unet.py test_tiny_unet_forward_and_trace (bf16 U-Net vs the oracle, max-norm) and
# test_gpu_train.py test_unet_backward_vs_oracle_autograd (bf16, rel-L2 per parameter)
UNET_BF16_TOL = 6e-2
GRAD_BF16_TOL = 8e-2


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _dt(name):
    from cwdm_hip import _lib
    return {"bf16": (_lib.CWDM_BF16, torch.bfloat16), "fp16": (_lib.CWDM_F16, torch.float16)}[name]


def _nd(x):  # NCDHW -> NDHWC
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _nc(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _fold(w):
    """fp32 fold of OIDHW weights: [8 phases][8 taps][cout][cin]; per axis phase p tap t sums the
    original taps {0} / {1, 2} (p = 0) or {0, 1} / {2} (p = 1), in fp32, kz then ky then kx ascending
    (the order of cwdm_conv3d_pack_phase)."""
    w = w.float()
    ks = lambda p, t: ([0] if t == 0 else [1, 2]) if p == 0 else ([0, 1] if t == 0 else [2])  # noqa: E731
    out = torch.zeros(8, 8, w.shape[0], w.shape[1])
    for ph in range(8):
        pz, py, px = ph >> 2, (ph >> 1) & 1, ph & 1
        for tap in range(8):
            tz, ty, tx = tap >> 2, (tap >> 1) & 1, tap & 1
            acc = torch.zeros(w.shape[0], w.shape[1])
            for kz in ks(pz, tz):
                for ky in ks(py, ty):
                    for kx in ks(px, tx):
                        acc = acc + w[:, :, kz, ky, kx]
            out[ph, tap] = acc
    return out


def _phase_conv64(src, wf, bias):
    """fp64 conv of the definition through the folded weights: src (B, cin, d, h, w) -> (B, cout, 2d, 2h, 2w);
    bias (B, cout)."""
    B, _, d, h, w = src.shape
    cout = wf.shape[2]
    xp = F.pad(src.double(), (1, 1, 1, 1, 1, 1))
    out = torch.zeros(B, cout, 2 * d, 2 * h, 2 * w, dtype=torch.float64)
    for ph in range(8):
        pz, py, px = ph >> 2, (ph >> 1) & 1, ph & 1
        k = wf[ph].double().permute(1, 2, 0).reshape(cout, -1, 2, 2, 2)   # [cout][cin][tz][ty][tx]
        y = F.conv3d(xp, k)   # y[j] = sum_t k[t] xp[j + t]; source offset p - 1 + t <-> j = i + p
        out[:, :, pz::2, py::2, px::2] = y[:, :, pz:pz + d, py:py + h, px:px + w]
    return out + bias.double()[:, :, None, None, None]


def _pack_phase(w, dtype):
    from cwdm_hip._lib import check, lib
    L = lib()
    cout, cin = w.shape[:2]
    n = L.cwdm_conv3d_packed_phase_bytes(cout, cin, dtype)
    assert n == 64 * cout * cin * 2
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)
    check(L.cwdm_conv3d_pack_phase(ctypes.c_void_p(w.data_ptr()), cout, cin, dtype, ctypes.c_void_p(buf.data_ptr()),
                                   None))
    return buf


def _up_conv(dtype_name, out_grid, src, w, bias, gn=None, phase=True, stats=False, cap=0, wg=False):
    """cwdm_conv3d_forward of an a_mode 1 conv on kernel path 2 with the phase weights attached; src NDHWC
    on the source grid (16-bit, device), w fp32 master weights (device), bias (cout,) or (B, cout) fp32.
    wg: ask for the per-workgroup statistics layout (cwdm_debug_stats_wg).
    Returns (out NDHWC, stats or None, phase launches), with wg also the rows written that way."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    B, D, H, W = out_grid
    cout, cin = w.shape[:2]
    pa = torch.empty(L.cwdm_conv3d_packed_bytes(cout, cin, 3, dtype), dtype=torch.uint8, device=DEV)
    check(L.cwdm_conv3d_pack(ctypes.c_void_p(w.data_ptr()), cout, cin, 3, dtype, ctypes.c_void_p(pa.data_ptr()), None))
    pp = _pack_phase(w, dtype)
    out = torch.empty(B, D, H, W, cout, device=DEV, dtype=tdt)
    parts = L.cwdm_conv3d_parts(dtype, D, H, W, cout)
    st = torch.zeros(B, parts, cout, 2, device=DEV) if stats else None
    d = _lib.ConvDesc()
    d.dtype, d.B, d.D, d.H, d.W, d.cout = dtype, B, D, H, W, cout
    d.a0, d.a_c0, d.a_mode = src.data_ptr(), cin, 1
    d.a_gn = gn.data_ptr() if gn is not None else None
    d.a_w, d.a_w_phase = pa.data_ptr(), pp.data_ptr()
    d.bias, d.bias_bstride = bias.data_ptr(), (cout if bias.dim() == 2 else 0)
    d.res_mode = -1
    d.out, d.out_dtype = out.data_ptr(), dtype
    d.stats = st.data_ptr() if stats else None
    prev, prevg, prevp = L.cwdm_conv3d_set_path(2), L.cwdm_debug_v5_grid(cap), L.cwdm_debug_up_phase(1 if phase else 0)
    try:
        nws = L.cwdm_conv3d_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
        d.workspace, d.ws_bytes = ws.data_ptr(), nws
        n0 = L.cwdm_debug_up_phase(-1)
        prevw = L.cwdm_debug_stats_wg(1 if wg else 0)
        try:
            check(L.cwdm_conv3d_forward(ctypes.byref(d), None))
            rows = L.cwdm_debug_stats_wg(-1)
        finally:
            L.cwdm_debug_stats_wg(prevw)
        torch.cuda.synchronize()
        ran = L.cwdm_debug_up_phase(-1) - n0
    finally:
        L.cwdm_conv3d_set_path(prev)
        L.cwdm_debug_v5_grid(prevg)
        L.cwdm_debug_up_phase(prevp)
    return (out, st, ran, rows) if wg else (out, st, ran)


# name, B, output grid, cin, cout, the phase path takes it
EXACT_CASES = [
    ("one_partial_tile", 2, (8, 8, 48), 32, 64, True),     # one partial x tile, 2 chunks, all six faces in one tile
    ("two_x_tiles", 1, (16, 16, 80), 128, 128, True),      # 2 x tiles (one partial), 2x2 y/z, 2 cout tiles, 8 chunks
    ("full_tiles_3chunk", 1, (8, 8, 128), 48, 64, True),
    ("source_too_narrow", 1, (8, 8, 32), 32, 64, False),   # source W = 16 < 24: the gather path
]


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_phase_equals_gather_bitwise_on_integers(case, dtype_name):
    """Integer inputs in [-3, 3], master weights in [-2, 2], integer bias: every folded weight and
    every partial sum is exact in the 16-bit type / fp32 (|sum| <= 3 * 2 * 27 * 128 < 2^24), so the
    phase path must reproduce the gather path bit for bit."""
    name, B, (D, H, W), cin, cout, takes = case
    _, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(31)
    src = torch.randint(-3, 4, (B, D // 2, H // 2, W // 2, cin), generator=g).to(DEV, tdt)
    w = torch.randint(-2, 3, (cout, cin, 3, 3, 3), generator=g).float().to(DEV)
    bias = torch.randint(-4, 5, (cout,), generator=g).float().to(DEV)
    ref, _, ran0 = _up_conv(dtype_name, (B, D, H, W), src, w, bias, phase=False)
    got, _, ran1 = _up_conv(dtype_name, (B, D, H, W), src, w, bias, phase=True)
    assert ran0 == 0
    assert ran1 == (1 if takes else 0), name
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (name, rel_err(got, ref))
    # several work items per workgroup: tile hand-off and weight ring across phases / channel tiles
    got5, _, ran5 = _up_conv(dtype_name, (B, D, H, W), src, w, bias, phase=True, cap=3)
    assert ran5 == (1 if takes else 0)
    assert torch.equal(got5.view(torch.int16), ref.view(torch.int16)), name


DEF_CASES = [
    # name, B, output grid, cin, cout, GroupNorm pre-pass route
    ("raw", 2, (8, 8, 48), 32, 64, False),
    ("gn", 2, (8, 8, 48), 32, 64, True),
    ("gn_two_x_tiles", 1, (16, 16, 80), 128, 128, True),
]


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", DEF_CASES, ids=[c[0] for c in DEF_CASES])
def test_phase_against_the_definition(case, dtype_name):
    """Random 16-bit activations, random fp32 master weights, per-batch bias: the phase path against
    CPU-fp32 F.conv3d(F.interpolate(x, 2, nearest), w, padding=1) within the bound of the v5_up_*
    cases; and against fp64 with the folded fp32 weights it must be no worse than the gather path by
    more than the rounding of one folded weight."""
    name, B, (D, H, W), cin, cout, use_gn = case
    _, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(37)
    x = torch.randn(B, cin, D // 2, H // 2, W // 2, generator=g).to(tdt).float()
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    bias = 0.1 * torch.randn(B, cout, generator=g)
    gn, h = None, x
    if use_gn:
        scale = 1 + 0.2 * torch.randn(B, cin, generator=g)
        shift = 0.2 * torch.randn(B, cin, generator=g)
        gn = torch.stack([scale, shift], -1).contiguous().to(DEV)
        h = F.silu(x * scale[:, :, None, None, None] + shift[:, :, None, None, None])
    h = h.to(tdt).float()   # the 16-bit-rounded activations both paths stage
    ref32 = F.conv3d(F.interpolate(h, scale_factor=2, mode="nearest"), w, padding=1) + bias[:, :, None, None, None]
    ref64 = _phase_conv64(h, _fold(w), bias)
    assert rel_err(ref64, ref32) < 1e-5   # the fold is the definition
    src = _nd(x).to(DEV, tdt)
    a = (dtype_name, (B, D, H, W), src, w.to(DEV), bias.to(DEV))
    gat, _, ran0 = _up_conv(*a, gn=gn, phase=False)
    got, _, ran1 = _up_conv(*a, gn=gn, phase=True)
    assert (ran0, ran1) == (0, 1), name
    e_def = rel_err(_nc(got.float().cpu()), ref32)
    e_phase, e_gather = rel_err(_nc(got.float().cpu()), ref64), rel_err(_nc(gat.float().cpu()), ref64)
    print(f"{name} {dtype_name}: vs definition {e_def:.3e}; vs fp64 fold: phase {e_phase:.3e} gather {e_gather:.3e}")
    assert e_def < CONV_TOL[dtype_name], name
    assert e_phase <= e_gather + W_EPS[dtype_name], name


@pytest.mark.parametrize("case", EXACT_CASES[:2], ids=[c[0] for c in EXACT_CASES[:2]])
def test_phase_statistics_per_tile(case):
    """The (sum, sum^2) rows of a lone call, reduced over the rows as cwdm_gn_finalize reduces them,
    against fp64 sums over the kernel's own output (the bound of _run_conv_case's statistics check,
    the squares scaled by the same factor of the largest square).  The per-tile layout holds one row
    per (source tile, phase) only where those are the caller's cwdm_conv3d_parts rows: the 80-wide
    grid (3 output x tiles, 2 x 2 phase rows) stays on the gather path when statistics are asked for."""
    name, B, (D, H, W), cin, cout, _ = case
    g = torch.Generator().manual_seed(41)
    src = torch.randn(B, D // 2, H // 2, W // 2, cin, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(DEV)
    bias = (0.1 * torch.randn(cout, generator=g)).to(DEV)
    out, st, ran = _up_conv("bf16", (B, D, H, W), src, w, bias, phase=True, stats=True)
    assert ran == (1 if (W + 31) // 32 == 2 * ((W // 2 + 31) // 32) else 0), name
    o = out.double().cpu()
    s = st.double().sum(1).cpu()
    mx = float(o.abs().max())
    assert torch.allclose(s[..., 0], o.sum(dim=(1, 2, 3)), rtol=1e-3, atol=1e-2 * mx * 8)
    assert torch.allclose(s[..., 1], (o * o).sum(dim=(1, 2, 3)), rtol=1e-3, atol=1e-2 * mx * mx * 8)


# several source tiles in x, y and z (2 x 2 x 2, the last x tile partial: source W = 56), two cout tiles, 8 chunks;
# ceil(112 / 32) = 4 = 2 ceil(56 / 32), so the per-tile rows are the caller's and the phase path keeps the call
STAT_GRID, STAT_CIN, STAT_COUT = (16, 16, 112), 128, 128


def _stat_inputs(B, seed):
    D, H, W = STAT_GRID
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, D // 2, H // 2, W // 2, STAT_CIN, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(STAT_COUT, STAT_CIN, 3, 3, 3, generator=g) / math.sqrt(27 * STAT_CIN)).to(DEV)
    bias = (0.1 * torch.randn(STAT_COUT, generator=g)).to(DEV)
    return src, w, bias


def _item_sums(o, sl, ph, tx, ty):
    """fp64 (sum, sum^2) per channel over the output voxels of work item (source tile sl, phase ph):
    o (D, H, W, C) the conv's own output; voxel (2 x + px, 2 y + py, 2 z + pz) of the tile's 32 x 4 x 4 brick."""
    sx, sy, sz = sl % tx, (sl // tx) % ty, sl // (tx * ty)
    pz, py, px = ph >> 2, (ph >> 1) & 1, ph & 1
    r = o[8 * sz + pz:8 * sz + 8:2, 8 * sy + py:8 * sy + 8:2, 64 * sx + px:64 * sx + 64:2]
    return torch.stack([r.sum(dim=(0, 1, 2)), (r * r).sum(dim=(0, 1, 2))], -1)


def _close_rows(got, want, mx):
    # the bound of _run_conv_case's statistics check, per row (the squares: the same factor of the largest square)
    return torch.allclose(got[..., 0], want[..., 0], rtol=1e-3, atol=1e-2 * mx * 8) and \
        torch.allclose(got[..., 1], want[..., 1], rtol=1e-3, atol=1e-2 * mx * mx * 8)


def test_phase_statistics_per_tile_rows():
    """Per-tile layout on the phase path, B = 2, several source tiles and two cout tiles: EVERY row
    against fp64 sums over the conv's own output -- row ((2 sz + pz) 2 ty + 2 sy + py) 2 tx + 2 sx + px of a
    batch entry holds work item (source tile (sx, sy, sz), phase (px, py, pz)), all cout channels."""
    B, (D, H, W) = 2, STAT_GRID
    src, w, bias = _stat_inputs(B, 47)
    out, st, ran = _up_conv("bf16", (B, D, H, W), src, w, bias, phase=True, stats=True)
    assert ran == 1
    tx, ty, tz = (W // 2 + 31) // 32, H // 8, D // 8
    assert st.shape[1] == 8 * tx * ty * tz
    o, s = out.double().cpu(), st.double().cpu()
    mx = float(o.abs().max())
    want = torch.zeros_like(s)
    for b in range(B):
        for r in range(st.shape[1]):
            bx, by, bz = r % (2 * tx), (r // (2 * tx)) % (2 * ty), r // (4 * tx * ty)
            sl = ((bz // 2) * ty + by // 2) * tx + bx // 2
            want[b, r] = _item_sums(o[b], sl, 4 * (bz % 2) + 2 * (by % 2) + bx % 2, tx, ty)
    assert _close_rows(s, want, mx)
    assert _close_rows(s.sum(1), torch.stack([o.sum(dim=(1, 2, 3)), (o * o).sum(dim=(1, 2, 3))], -1), mx)


@pytest.mark.parametrize("cap", [5, 64])
def test_phase_statistics_per_workgroup_rows(cap):
    """Per-workgroup layout (what the plan asks for around its convs) on a lone phase launch with the
    persistent grid capped at G workgroups: row g against fp64 sums over the conv's own output of the work
    items workgroup g ran (item t = g + it G through the per-XCD map; item -> source tile, phase, cout
    tile), the rows past G untouched, and the reduction over the rows against the whole output."""
    D, H, W = STAT_GRID
    src, w, bias = _stat_inputs(1, 53)
    out, st, ran, rows = _up_conv("bf16", (1, D, H, W), src, w, bias, phase=True, stats=True, cap=cap, wg=True)
    assert ran == 1 and rows == cap
    tx, ty, tz, nct = (W // 2 + 31) // 32, H // 8, D // 8, STAT_COUT // 64
    nblk = tx * ty * tz * nct * 8
    o, s = out[0].double().cpu(), st[0].double().cpu()
    mx = float(o.abs().max())
    want = torch.zeros_like(s)
    q8, r8 = nblk >> 3, nblk & 7
    for g in range(cap):
        for t in range(g, nblk, cap):
            xcd = t & 7
            item = (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (t >> 3)
            sl, inn = divmod(item, 8 * nct)
            ph, ct = divmod(inn, nct)
            want[g, 64 * ct:64 * ct + 64] += _item_sums(o, sl, ph, tx, ty)[64 * ct:64 * ct + 64]
    assert _close_rows(s[:cap], want[:cap], mx)
    assert not s[cap:].any()
    assert _close_rows(s.sum(0), torch.stack([o.sum(dim=(0, 1, 2)), (o * o).sum(dim=(0, 1, 2))], -1), mx)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cout,cin", [(64, 32), (128, 128)])
def test_pack_phase_bytes(cout, cin, dtype_name):
    """cwdm_conv3d_pack_phase against a fold of the same weights done here, byte for byte: layout
    [phase][cout tile][chunk][tap][64 rows][2 quads, swizzled by bit 3 of the row][8]."""
    from cwdm_hip._lib import lib
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(43)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g)
    got = _pack_phase(w.to(DEV), dtype).cpu()
    assert lib().cwdm_conv3d_packed_phase_bytes(cout, cin, dtype) * 27 == \
        lib().cwdm_conv3d_packed_bytes(cout, cin, 3, dtype) * 64
    wf = _fold(w).to(tdt)                                        # rounded once
    v = wf.view(8, 8, cout // 64, 64, cin // 16, 2, 8)           # [ph][tap][ct][n][chunk][q][e]
    v = v.permute(0, 2, 4, 1, 3, 5, 6).contiguous()              # [ph][ct][chunk][tap][n][q][e]
    sw = ((torch.arange(64) >> 3) & 1).bool()
    v[:, :, :, :, sw] = v[:, :, :, :, sw].flip(-2)               # slot qp holds quad qp ^ bit 3 of n
    assert torch.equal(got.view(torch.int16), v.reshape(-1).view(torch.int16))
    assert lib().cwdm_conv3d_packed_phase_bytes(cout, 24, dtype) == -1
    assert lib().cwdm_conv3d_packed_phase_bytes(96, cin, dtype) == -1


# ------------------------------------------------------------------------------- through the plan
PLAN_CFG = dict(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=1, channel_mult=(1, 2))
PLAN_GROUPS = 8
PLAN_GRID = (8, 8, 48)


def _seeded(model, seed):
    """Non-degenerate weights as bench.seeded_weights builds them."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 1 and (".in_layers.0." in name or ".out_layers.0." in name or name.startswith("out.0.")):
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))


def _plan_model():
    from guided_diffusion import script_util
    args = script_util.run_sh_model_args(num_channels=64, channel_mult="1,2", num_res_blocks=1,
                                         num_groups=PLAN_GROUPS)
    keys = script_util.model_and_diffusion_defaults().keys()
    model, diffusion = script_util.create_model_and_diffusion(**{k: args[k] for k in keys}, compute_dtype="bf16")
    _seeded(model, 3)
    return model.to(DEV), diffusion


class _Switches:
    """kernel path 2 (the small grid's convs on the DMA-staged kernels), a grid cap, the phase switch"""

    def __init__(self, phase, cap=0):
        self.phase, self.cap = phase, cap

    def __enter__(self):
        from cwdm_hip._lib import lib
        L = lib()
        self.prev = (L.cwdm_conv3d_set_path(2), L.cwdm_debug_v5_grid(self.cap),
                     L.cwdm_debug_up_phase(1 if self.phase else 0))
        return L

    def __exit__(self, *exc):
        from cwdm_hip._lib import lib
        L = lib()
        L.cwdm_conv3d_set_path(self.prev[0])
        L.cwdm_debug_v5_grid(self.prev[1])
        L.cwdm_debug_up_phase(self.prev[2])


def test_plan_forward_graph_and_training():
    """A small resblock_updown U-Net whose one up-ResBlock conv (4x4x24 -> 8x8x48, 128 -> 128) takes
    the phase path: forward with the switch on and off against the CPU oracle, exactly one phase launch
    per forward, per-workgroup statistics (grid capped below the output's tiles) as good as per-tile
    ones, a HIP-graph replay equal to the eager output, and training gradients within the bf16
    per-parameter bound of the switch-off gradients."""
    from oracle import unet as ou
    model, diffusion = _plan_model()
    P = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 32, *PLAN_GRID, generator=g)
    t = torch.tensor([300])
    ref = ou.unet_forward(P, x, t, num_groups=PLAN_GROUPS, **PLAN_CFG)
    xd, td = x.to(DEV), t.to(DEV)
    outs = {}
    for phase, cap in ((False, 0), (True, 0), (True, 5)):
        with _Switches(phase, cap) as L, torch.no_grad():
            n0 = L.cwdm_debug_up_phase(-1)
            outs[phase, cap] = model(xd, td).float().cpu()
            torch.cuda.synchronize()
            assert L.cwdm_debug_up_phase(-1) - n0 == (1 if phase else 0)
        e = rel_err(outs[phase, cap], ref)
        print(f"phase {phase} cap {cap}: vs oracle {e:.3e}")
        assert e < UNET_BF16_TOL
    # one captured forward, replayed: the eager output bitwise
    with _Switches(True) as L, torch.no_grad():
        eager = model(xd, td).clone()
        cs = torch.cuda.Stream()
        cs.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=cs):
            y = model(xd, td)
        torch.cuda.current_stream().wait_stream(cs)
        y.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
        del gr
    # training_losses + backward, switch on vs off
    vg = torch.Generator().manual_seed(7)
    vols = {k: torch.rand(1, 1, 16, 16, 96, generator=vg).to(DEV) for k in ("t1n", "t1c", "t2w", "t2f")}
    noise = torch.randn(1, 1, 16, 16, 96, generator=vg).to(DEV)
    tt = torch.tensor([400], device=DEV)
    grads = {}
    for phase in (False, True):
        with _Switches(phase) as L:
            n0 = L.cwdm_debug_up_phase(-1)
            model.zero_grad(set_to_none=True)
            terms, _, _ = diffusion.training_losses(model, vols, tt, mode="i2i", contr="t2w", noise=noise)
            terms["mse_wav"].sum().backward()
            torch.cuda.synchronize()
            ran = L.cwdm_debug_up_phase(-1) - n0
            assert (ran >= 1) if phase else (ran == 0)
            grads[phase] = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
    worst = {n: float((grads[True][n] - grads[False][n]).norm() / grads[False][n].norm().clamp_min(1e-30))
             for n in grads[False]}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print("gradients, phase vs gather (rel-L2):", top)
    assert top[0][1] < GRAD_BF16_TOL, top


def test_plan_batched_pack_equals_lone_pack():
    """The plan packs its phase weights inside its one batched pack launch: the bytes of a lone
    cwdm_conv3d_pack_phase of the up conv's weights appear in the plan's packed buffer, and no other
    3x3x3 conv of this model has a phase region."""
    from cwdm_hip import _lib
    model, _ = _plan_model()
    params = [p.detach().float().contiguous() for p in model.param_list()]
    packed = model.plan.pack(params).cpu().numpy().tobytes()
    found = []
    for (name, shape), p in zip(model.plan.param_specs, params):
        if len(shape) == 5 and shape[2] == 3 and shape[0] % 64 == 0 and shape[1] % 16 == 0 and shape[1] >= 32:
            lone = _pack_phase(p, _lib.CWDM_BF16).cpu().numpy().tobytes()
            if packed.find(lone) >= 0:
                found.append(name)
    assert len(found) == 1, found
