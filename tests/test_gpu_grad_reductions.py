"""The reductions and resampling adjoints of the backward (csrc/grad.hip)
through the C ABI: cwdm_resample_add, cwdm_channel_sum and
cwdm_adamw_device_step.

The first two run on integer-valued inputs sized so that every sum is exact
in fp32 and every stored value exact in bf16 / fp16; they are compared bit
for bit with an int64 / float64 CPU reference.  Each test checks those bounds
itself, so a change of shape cannot turn it into a rounding test."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
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


def _assert_exact_range(ref, tdt):
    """Every value of ref is an integer that fp32 holds exactly, and the storage type too."""
    assert torch.equal(ref, ref.round())
    assert float(ref.abs().max()) < 2 ** 24
    if tdt != torch.float32:
        assert float(ref.abs().max()) <= 256   # 8 significant bits (bf16); fp16 has 11


# --------------------------------------------------------------------------- resample_add
# (dst grid, modes): mode 0 same grid, mode 1 the source is the x2 grid (adjoint of nearest
# upsampling), mode 2 the source is the half grid (adjoint of AvgPool3d(2): even grids only)
RS_GRIDS = [((1, 1, 1), (0, 1)), ((2, 2, 2), (0, 1, 2)), ((3, 5, 7), (0, 1)), ((4, 6, 10), (0, 1, 2))]
RS_CASES = [(grid, mode) for grid, modes in RS_GRIDS for mode in modes]


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "acc"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("grid,mode", RS_CASES, ids=[f"{'x'.join(map(str, g))}_mode{m}" for g, m in RS_CASES])
def test_resample_add_integer_exact(grid, mode, dtype_name, acc):
    from cwdm_hip._lib import check, lib
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(30)
    B = 2
    for C in (8, 24, 64):
        sgrid = {0: grid, 1: tuple(2 * s for s in grid), 2: tuple(s // 2 for s in grid)}[mode]
        src = torch.randint(-8, 9, (B, C, *sgrid), generator=g).double()
        if mode == 2:
            src = src * 8          # the kernel scales by 1/8: multiples of 8 stay integers
        dst0 = torch.randint(-8, 9, (B, C, *grid), generator=g).double()
        xr = torch.zeros(B, C, *grid, dtype=torch.float64, requires_grad=True)
        y = xr if mode == 0 else (F.interpolate(xr, scale_factor=2, mode="nearest") if mode == 1
                                  else F.avg_pool3d(xr, 2))
        (y * src).sum().backward()
        ref = xr.grad + dst0 if acc else xr.grad
        _assert_exact_range(ref, tdt)
        _assert_exact_range(src, tdt)
        d = _nd(dst0).to(DEV, tdt) if acc else torch.full((B, *grid, C), float("nan"), device=DEV, dtype=tdt)
        s = _nd(src).to(DEV, tdt)
        check(lib().cwdm_resample_add(d.data_ptr(), s.data_ptr(), C, B, *grid, mode, acc, dtype, None))
        torch.cuda.synchronize()
        assert torch.equal(d.cpu().double(), _nd(ref)), C


def test_resample_add_refusals():
    from cwdm_hip import _lib
    from cwdm_hip._lib import lib
    L = lib()
    src = torch.zeros(8192, device=DEV)
    dst = torch.full((8192,), 7.0, device=DEV)
    for grid in [(3, 4, 4), (4, 5, 4), (4, 4, 7)]:
        assert L.cwdm_resample_add(dst.data_ptr(), src.data_ptr(), 8, 1, *grid, 2, 1, _lib.CWDM_F32,
                                   None) == _lib.E_SHAPE
    for C in (4, 12, 20):
        for mode in (0, 1, 2):
            assert L.cwdm_resample_add(dst.data_ptr(), src.data_ptr(), C, 1, 2, 2, 2, mode, 1, _lib.CWDM_F32,
                                       None) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())   # nothing was launched


# --------------------------------------------------------------------------- channel_sum
# C, cs, V, nb: nb = the per-batch partial rows the library reports (workspace bytes / (B C 4)),
# i.e. the nk of chs_reduce_kernel -- thread row r of 16 sums rows r, r + 16, ...: an
# 8-accumulator main loop while more than 112 rows lie ahead, then a tail of up to 7 rows
CS_CASES = [
    ("rows_lt_16", 256, 256, 576, 9),                 # fewer rows than the 16-row interleave
    ("tail_only", 256, 256, 4096, 64),                # 4 rows per thread, all in the tail
    ("main_and_tail", 64, 64, 35 * 31 * 33, 140),     # one main-loop trip, then a tail row for r < 12 only
    ("tail_7_rows", 256, 256, 112 * 64, 112),         # the longest tail: 7 rows, no main loop
    ("main_row0_only", 256, 256, 113 * 64, 113),      # thread row 0 takes the main loop, the others the tail
    ("main_and_tail7", 256, 256, 240 * 64, 240),      # a main-loop trip, then the 7-row tail
    ("cap_exact", 256, 256, 32768, 512),              # 512 blocks, 64 voxels each: 4 main-loop trips, no tail
    ("capped_vpb72", 256, 256, 36 * 32 * 32, 512),    # 576 wanted, capped: 72 voxels per block, 9 trips
    ("ncg25_idle", 200, 200, 1000, 13),               # 25 channel groups: 10 slots, 6 idle threads
    ("c12_cs16", 12, 16, 3000, 3),                    # C not a multiple of 8 inside a wider row
    ("ncg1", 8, 8, 5000, 3),                          # one channel group, 256 voxel slots
    ("ncg256", 2048, 2048, 37, 5),                    # 256 channel groups, one slot, small V
]


def _channel_sum_vpb(V, nb):
    return -(-V // nb)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", CS_CASES, ids=[c[0] for c in CS_CASES])
def test_channel_sum_integer_exact(case, dtype_name):
    from cwdm_hip._lib import check, lib
    L = lib()
    name, C, cs, V, nb = case
    dtype, tdt = _dt(dtype_name)
    B, bc_stride, guard = 2, C + 24, 8
    g = torch.Generator().manual_seed(31)
    nws = L.cwdm_channel_sum_workspace_bytes(B, V, C)
    assert nws > 0
    assert nws == B * nb * C * 4, (name, nws // (B * C * 4))
    if name == "capped_vpb72":
        assert _channel_sum_vpb(V, nb) == 72
    # (channels [C, cs) of a row hold values too: they belong to no sum)
    src = torch.randint(-8, 9, (B, V, cs), generator=g, dtype=torch.int8)
    sums = src[..., :C].to(torch.int64).sum(1)                                 # [B, C]
    bc0 = torch.randint(-8, 9, (B, bc_stride), generator=g).double()
    c0 = torch.randint(-8, 9, (C + guard,), generator=g).double()
    c20 = torch.randint(-8, 9, (C + guard,), generator=g).double()
    ref_bc = bc0.clone()
    ref_bc[:, :C] += sums.double()
    ref_c, ref_c2 = c0.clone(), c20.clone()
    ref_c[:C] += sums.sum(0).double()
    ref_c2[:C] += sums.sum(0).double()
    # every partial sum is bounded by 8 B V: exact in fp32 whatever the order
    assert 8 * B * V + 8 < 2 ** 24
    for r in (ref_bc, ref_c, ref_c2):
        _assert_exact_range(r, torch.float32)
    s = src.to(DEV).to(tdt)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):   # the second call finds the workspace dirty
        out_bc, out_c, out_c2 = bc0.float().to(DEV), c0.float().to(DEV), c20.float().to(DEV)
        check(L.cwdm_channel_sum(s.data_ptr(), dtype, B, V, C, cs, out_bc.data_ptr(), bc_stride, out_c.data_ptr(),
                                 out_c2.data_ptr(), ws.data_ptr(), nws, None))
        torch.cuda.synchronize()
        runs.append((out_bc.cpu(), out_c.cpu(), out_c2.cpu()))
    for out_bc, out_c, out_c2 in runs:
        assert torch.equal(out_bc.double(), ref_bc), name     # the gap [C, bc_stride) untouched
        assert torch.equal(out_c.double(), ref_c), name       # the guard past C untouched
        assert torch.equal(out_c2.double(), ref_c2), name
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("which", ["bc", "c", "c2"])
def test_channel_sum_single_output(which):
    """Each output alone (the others null), as the U-Net backward calls it."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    B, V, C = 2, 576, 24
    g = torch.Generator().manual_seed(32)
    src = torch.randint(-8, 9, (B, V, C), generator=g, dtype=torch.int8)
    sums = src.to(torch.int64).sum(1)
    nws = L.cwdm_channel_sum_workspace_bytes(B, V, C)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    s = src.to(DEV).to(torch.bfloat16)
    out0 = torch.randint(-8, 9, (B * C,), generator=g).double()
    out = out0.float().to(DEV)
    ref = out0.clone()
    if which == "bc":
        ref += sums.reshape(-1).double()
    else:
        ref[:C] += sums.sum(0).double()
    _assert_exact_range(ref, torch.float32)
    p = out.data_ptr()
    check(L.cwdm_channel_sum(s.data_ptr(), _lib.CWDM_BF16, B, V, C, C, p if which == "bc" else None, C,
                             p if which == "c" else None, p if which == "c2" else None, ws.data_ptr(), nws, None))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), ref)


# --------------------------------------------------------------------------- AdamW, device-side step
HYP = (1e-3, 0.9, 0.999, 1e-8, 0.01)   # lr, beta1, beta2, eps, weight_decay


def _device_step(p, grad, m, v, n, step, found_inf):
    from cwdm_hip._lib import check, lib
    check(lib().cwdm_adamw_device_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, *HYP,
                                       step.data_ptr(), found_inf.data_ptr() if found_inf is not None else None,
                                       None))
    torch.cuda.synchronize()


def test_adamw_device_step_count_and_found_inf():
    g = torch.Generator().manual_seed(33)
    n = 10007
    p0 = torch.randn(n, generator=g)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=HYP[0], betas=HYP[1:3], eps=HYP[3], weight_decay=HYP[4], foreach=False)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.float64, device=DEV)
    no_inf = torch.zeros(1, device=DEV)
    for _ in range(3):
        grad = torch.randn(n, generator=g)
        pr.grad = grad.clone()
        opt.step()
        _device_step(p, grad.to(DEV), m, v, n, step, no_inf)
    st = opt.state[pr]
    assert rel_err(p, pr.detach()) < 1e-6
    assert rel_err(m, st["exp_avg"]) < 1e-6
    assert rel_err(v, st["exp_avg_sq"]) < 1e-6
    assert step.item() == 3.0

    # found_inf set: the whole update and the count are skipped, bit for bit
    grad = torch.randn(n, generator=g).to(DEV)
    before = [t.clone() for t in (p, m, v, step)]
    _device_step(p, grad, m, v, n, step, torch.ones(1, device=DEV))
    for got, want in zip((p, m, v, step), before):
        assert torch.equal(got, want)
    # (any non-zero value counts, as GradScaler accumulates it)
    _device_step(p, grad, m, v, n, step, torch.full((1,), 2.0, device=DEV))
    for got, want in zip((p, m, v, step), before):
        assert torch.equal(got, want)

    # found_inf = NULL behaves as found_inf = 0: the same fourth step from the same state
    outs = []
    for fi in (no_inf, None):
        q = [t.clone() for t in before]
        _device_step(q[0], grad, q[1], q[2], n, q[3], fi)
        assert q[3].item() == 4.0
        assert not torch.equal(q[0], before[0])
        outs.append(q)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # ... and it is the fourth AdamW step
    pr.grad = grad.cpu().clone()
    opt.step()
    assert rel_err(outs[1][0], pr.detach()) < 1e-6
    assert rel_err(outs[1][1], st["exp_avg"]) < 1e-6
    assert rel_err(outs[1][2], st["exp_avg_sq"]) < 1e-6

    # n = 0 (an empty parameter group) still advances the count, and touches nothing else
    q = [t.clone() for t in before]
    _device_step(q[0], grad, q[1], q[2], 0, q[3], no_inf)
    assert q[3].item() == 4.0
    for got, want in zip(q[:3], before[:3]):
        assert torch.equal(got, want)
    _device_step(q[0], grad, q[1], q[2], 0, q[3], torch.ones(1, device=DEV))
    assert q[3].item() == 4.0
