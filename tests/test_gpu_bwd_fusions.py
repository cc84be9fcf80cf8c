"""The two backward fusions only a 16-bit U-Net plan reaches, at kernel level against float64:

* GbwdFuse -- a dgrad conv (conv3d_v4.hpp run_gb) whose epilogue writes the per-tile (sum dz, sum dz xhat)
  partials of the SiLU(GroupNorm) backward that consumes its output du;
* GapplyFuse -- the 1x1 skip dgrad (pointwise.hip pw_kernel<T, true, NM, LT>) whose epilogue adds that
  backward's apply pass;

and the plan-only arguments of gn_silu_bwd_impl (pre_part, coef_out, acc_affine, chs) with gb_part_reduce,
all through the cwdm_debug_* entry points that fill the call context as unet_plan.cpp does.

Every reference is float64 on the CPU, built from the rounded 16-bit operands the kernel reads; what lies
downstream of du uses the du the kernel STORED, so the conv's own rounding (test_gpu_train.py) stays out of
the fusion's bounds.  ss / mr are computed in float64 from the rounded x and cast to fp32 (what the kernels
read), and the references use those fp32 values.  Each test asserts the fusion was taken (used == 1).
Every test prints its worst error / bound ratio (pytest -s shows them)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SILU_D_MAX = 1.1   # max |SiLU'| = 1.0998...


def _dt(name):
    from cwdm_hip import _lib
    return {"fp32": (_lib.CWDM_F32, torch.float32), "bf16": (_lib.CWDM_BF16, torch.bfloat16),
            "fp16": (_lib.CWDM_F16, torch.float16)}[name]


def _nd(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _unit16(tdt):
    """unit roundoff of the 16-bit format: |round(v) - v| <= u |v|"""
    return 2.0 ** -8 if tdt is torch.bfloat16 else 2.0 ** -11


def _ulp16(v, tdt):
    """one ulp of the 16-bit format at |v| (float64 tensor); the smallest normal's below it"""
    p, emin = (8, -126) if tdt is torch.bfloat16 else (11, -14)
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** emin))   # |v| = m 2^e, m in [0.5, 1)
    return torch.exp2((e - 1 - (p - 1)).double())


def _report(what, ratio):
    print(f"[bwd_fusions] {what}: worst error/bound = {float(ratio):.3g}")


# --------------------------------------------------------------------------- float64 references
def _gn_stats(x, gamma, beta, G):
    """x [B, C, ...] (rounded values): the forward's (scale, shift) [B][C][2] and (mean, rstd) [B][G][2],
    float64 arithmetic cast to fp32 -- what the kernels read."""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, G, -1)
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5)
    cpg = C // G
    sc = gamma.double()[None] * rstd.repeat_interleave(cpg, 1)
    sh = beta.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    return torch.stack([sc, sh], -1).float().contiguous(), torch.stack([mean, rstd], -1).float().contiguous()


def _dz_terms(xl, dul, ss, mr):
    """channels-last float64 x, du [B, ..., C] -> dz = du SiLU'(x sc + sh), xhat, mu, rs (mu, rs [B, 1.., C])"""
    B, C = xl.shape[0], xl.shape[-1]
    cpg = C // mr.shape[1]
    shp = (B,) + (1,) * (xl.dim() - 2) + (C,)
    sc, sh = ss[..., 0].double().reshape(shp), ss[..., 1].double().reshape(shp)
    mu = mr[..., 0].double().repeat_interleave(cpg, 1).reshape(shp)
    rs = mr[..., 1].double().repeat_interleave(cpg, 1).reshape(shp)
    z = xl * sc + sh
    s = torch.sigmoid(z)
    return dul * (s * (1.0 + z * (1.0 - s))), (xl - mu) * rs, mu, rs


def _gn_bwd_ref(xl, dul, gamma, ss, mr):
    """Explicit float64 backward of SiLU(GroupNorm(x)) from the kernels' own operands: dx = k0 dz + k1 x + k2,
    the coefficients [B, C], dgamma, dbeta and the sums of |terms| their bounds are made of."""
    B, C = xl.shape[0], xl.shape[-1]
    G = mr.shape[1]
    cpg = C // G
    red = tuple(range(1, xl.dim() - 1))
    N = cpg * math.prod(xl.shape[1:-1])
    dz, xhat, mu, rs = _dz_terms(xl, dul, ss, mr)
    A, Bs = dz.sum(red), (dz * xhat).sum(red)                     # [B, C]
    g64 = gamma.double()[None]
    gs0 = (g64 * A).reshape(B, G, cpg).sum(-1).repeat_interleave(cpg, 1)
    gs1 = (g64 * Bs).reshape(B, G, cpg).sum(-1).repeat_interleave(cpg, 1)
    mu_c, rs_c = mu.reshape(B, C), rs.reshape(B, C)
    k0 = rs_c * g64
    k1 = -rs_c * rs_c * gs1 / N
    k2 = -rs_c * gs0 / N + rs_c * rs_c * gs1 * mu_c / N
    shp = mu.shape
    dx = k0.reshape(shp) * dz + k1.reshape(shp) * xl + k2.reshape(shp)
    mag = k0.abs().reshape(shp) * SILU_D_MAX * dul.abs() + (k1.reshape(shp) * xl).abs() + k2.abs().reshape(shp)
    return dict(dx=dx, mag=mag, dgamma=Bs.sum(0), dbeta=A.sum(0), dgamma_abs=(dz * xhat).abs().sum(red).sum(0),
                dbeta_abs=dz.abs().sum(red).sum(0))


def _gn_bwd_autograd(x, du, gamma, beta, G):
    """float64 autograd of SiLU(GroupNorm(x)) . du; x, du [B, C, ...] -> dx (channels-last), dgamma, dbeta"""
    xr = x.double().clone().requires_grad_(True)
    gr = gamma.double().clone().requires_grad_(True)
    br = beta.double().clone().requires_grad_(True)
    (F.silu(F.group_norm(xr, G, gr, br, eps=1e-5)) * du.double()).sum().backward()
    return xr.grad.movedim(1, -1).contiguous(), gr.grad, br.grad


def _dgrad_ref64(dyl, w):
    """3x3x3 input gradient in float64 as 27 shifted matmuls: dyl [B, D, H, W, co] channels-last, w [co, ci, 3, 3, 3]
    -> [B, D, H, W, ci]  (dx[q] = sum_t dy[q - t + 1] w[:, :, t])"""
    B, D, H, W, _ = dyl.shape
    p = F.pad(dyl, (0, 0, 1, 1, 1, 1, 1, 1))
    out = torch.zeros(B, D, H, W, w.shape[1], dtype=torch.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out += p[:, 2 - kz:2 - kz + D, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] @ w[:, :, kz, ky, kx]
    return out


def _tile_sums(t):
    """[B, D, H, W, C] -> [B, tiles, C]: sums over the 32 x 4 x 4 tiles, tile sl = x + tx (y + ty z)"""
    B, D, H, W, C = t.shape
    tx = (W + 31) // 32
    t = F.pad(t, (0, 0, 0, tx * 32 - W))
    return t.reshape(B, D // 4, 4, H // 4, 4, tx, 32, C).sum((2, 4, 6)).reshape(B, -1, C)


# --------------------------------------------------------------------------- A. the fused reduce partials
# name, B, dY channels, C, c0, groups, grid (D, H, W), conv path, mean of x
GB_CASES = {
    # 32-channel tiles (forced DMA path: 16 work items): a partial x tile (W = 24), 4 x 2 y / z tiles, batch 2
    "ct32_cpg2": (2, 32, 64, 64, 32, (8, 16, 24), 2, 0.0),
    "ct32_cpg16": (2, 32, 64, 64, 4, (8, 16, 24), 2, 0.0),
    # two sources, the seam at 32: on a 32-channel tile edge that is no 64 boundary
    "ct32_seam32": (1, 32, 128, 32, 32, (8, 8, 32), 2, 0.0),
    # 64-channel tiles (256 work items), two sources 64 | 192
    "ct64_two_src": (2, 32, 256, 64, 32, (16, 32, 32), 2, 0.0),
    # the auto policy on a shape the production plan produces (32^3 level, 64 -> 64)
    "auto_32cube": (1, 64, 64, 64, 32, (32, 32, 32), 0, 0.0),
    # |mu| >> sigma: the epilogue's fix-up rs (sum dz x - mu sum dz) subtracts two nearly equal fp32 numbers
    "ct32_mean_p4": (2, 32, 64, 64, 32, (8, 16, 24), 2, 4.0),
    "ct32_mean_m4": (2, 32, 64, 64, 32, (8, 16, 24), 2, -4.0),
}
SENTINEL = -77.25


def _gbwd_run(B, cy, C, c0, G, grid, path, mean, dtype_name, seed=21, part_short=0):
    """One dgrad through cwdm_debug_conv3d_gbwd.  Returns the operands (CPU, rounded), the stored du, the
    partials buffer (prefilled with SENTINEL, one guard row behind it) and used / nblk."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(seed)
    D, H, W = grid
    w = (torch.randn(cy, C, 3, 3, 3, generator=g) / math.sqrt(27 * cy)).to(tdt).float()
    dy = torch.randn(B, cy, *grid, generator=g).to(tdt).float()
    x = (mean + torch.randn(B, C, *grid, generator=g)).to(tdt).float()
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    ss, mr = _gn_stats(x, gamma, beta, G)
    pk = torch.empty(L.cwdm_conv3d_packed_bytes(C, cy, 3, dtype), dtype=torch.uint8, device=DEV)
    wd = w.to(DEV).contiguous()
    check(L.cwdm_conv3d_pack_dgrad(ctypes.c_void_p(wd.data_ptr()), cy, C, 3, dtype, ctypes.c_void_p(pk.data_ptr()), None))
    a = _nd(dy).to(DEV, tdt)
    xd = _nd(x).to(DEV, tdt)
    x0 = xd[..., :c0].contiguous()
    x1 = xd[..., c0:].contiguous() if c0 < C else None
    du = torch.empty(B, *grid, C, device=DEV, dtype=tdt)
    tiles = ((W + 31) // 32) * (H // 4) * (D // 4)
    rows = B * tiles - part_short
    part = torch.full((rows + 1, C, 2), SENTINEL, device=DEV)   # (+ a guard row)
    ssd, mrd = ss.to(DEV), mr.to(DEV)
    d = _lib.ConvDesc()
    d.dtype, d.B, (d.D, d.H, d.W), d.cout = dtype, B, grid, C
    d.a0, d.a_c0, d.a_w = a.data_ptr(), cy, pk.data_ptr()
    d.res_mode = -1
    d.out, d.out_dtype = du.data_ptr(), dtype
    used, nblk = ctypes.c_int(-1), ctypes.c_int(-1)
    prev = L.cwdm_conv3d_set_path(path)
    try:
        nws = L.cwdm_conv3d_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
        d.workspace, d.ws_bytes = ws.data_ptr(), nws
        check(L.cwdm_debug_conv3d_gbwd(ctypes.byref(d), x0.data_ptr(), x1.data_ptr() if x1 is not None else None, c0,
                                       ssd.data_ptr(), mrd.data_ptr(), G, part.data_ptr(), rows * C * 8,
                                       ctypes.byref(used), ctypes.byref(nblk), None))
        torch.cuda.synchronize()
    finally:
        L.cwdm_conv3d_set_path(prev)
    return dict(B=B, C=C, c0=c0, G=G, grid=grid, tiles=tiles, dtype=dtype, tdt=tdt, w=w, dyl=_nd(dy).double(),
                x=x, xl=_nd(x).double(), gamma=gamma, beta=beta, ss=ss, mr=mr, ssd=ssd, mrd=mrd, x0=x0, x1=x1,
                du=du, dul=du.cpu().double(), part=part, used=used.value, nblk=nblk.value, nterms=27 * cy)


@functools.lru_cache(maxsize=None)
def _gbwd_case(name, dtype_name):
    return _gbwd_run(*GB_CASES[name], dtype_name)


def _check_du(r, what):
    """du against the float64 dgrad of the rounded operands: one rounding to the 16-bit format (u |ref|) and the
    fp32 accumulation of the conv's 27 cy products (worst case n 2^-24 of sum |w| |dy|)."""
    ref = _dgrad_ref64(r["dyl"], r["w"].double())
    mag = _dgrad_ref64(r["dyl"].abs(), r["w"].double().abs())
    bound = 1.01 * _unit16(r["tdt"]) * ref.abs() + r["nterms"] * 2.0 ** -24 * mag + 1e-30
    ratio = ((r["dul"] - ref).abs() / bound).max()
    _report(f"{what} du vs float64 dgrad", ratio)
    assert ratio <= 1.0, what


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(GB_CASES))
def test_gbwd_partials_vs_float64(name, dtype_name):
    """Every (b, tile, channel) pair of partial words against float64 sums over that tile's voxels, formed from
    the stored du and the x, ss, mr the kernel read.  Bounds (derived: 1.1 bounds |SiLU'|; the rcpf / exp2f
    approximations and the fp32 accumulation over <= 512 terms sit two orders below 1e-4):
      sum dz:      1e-4 * 1.1 sum |du|
      sum dz xhat: 1e-4 * rs (1.1 sum |du x| + |mu| 1.1 sum |du|)
    Per tile, so a row written at the wrong index, a wrong source at the seam, a wrong group's (mu, rs) or an
    unmasked lane of the partial x tile each fail it."""
    r = _gbwd_case(name, dtype_name)
    B, C, tiles = r["B"], r["C"], r["tiles"]
    assert r["used"] == 1 and r["nblk"] == tiles, (r["used"], r["nblk"])
    _check_du(r, f"A {name} {dtype_name}")
    dz, xhat, mu, rs = _dz_terms(r["xl"], r["dul"], r["ss"], r["mr"])
    adu = _tile_sums(r["dul"].abs())
    adux = _tile_sums((r["dul"] * r["xl"]).abs())
    mu, rs = mu.reshape(B, 1, C), rs.reshape(B, 1, C)
    got = r["part"][:B * tiles].reshape(B, tiles, C, 2).cpu().double()
    ra = ((got[..., 0] - _tile_sums(dz)).abs() / (1e-4 * SILU_D_MAX * adu)).max()
    rb = ((got[..., 1] - _tile_sums(dz * xhat)).abs()
          / (1e-4 * rs * (SILU_D_MAX * adux + mu.abs() * SILU_D_MAX * adu))).max()
    _report(f"A {name} {dtype_name} sum dz", ra)
    _report(f"A {name} {dtype_name} sum dz xhat", rb)
    assert ra <= 1.0 and rb <= 1.0, (name, float(ra), float(rb))
    assert bool((r["part"][B * tiles:] == SENTINEL).all()), "wrote past [B][tiles][C][2]"


@pytest.mark.parametrize("why", ["c0_not_a_tile_multiple", "cpg_1", "part_one_row_short"])
def test_gbwd_refusals_leave_a_plain_dgrad(why):
    """An offer the route must refuse: used == 0, du still the dgrad, not one word of part written."""
    B, cy, C, c0, G, grid, path, mean = GB_CASES["ct32_cpg2"]
    short = 0
    if why == "c0_not_a_tile_multiple":
        c0 = 16          # 16 | 48: the seam inside a 32-channel tile
    elif why == "cpg_1":
        G = 64
    else:
        short = 1
    r = _gbwd_run(B, cy, C, c0, G, grid, path, mean, "bf16", part_short=short)
    assert r["used"] == 0
    _check_du(r, f"A refusal {why}")
    assert bool((r["part"] == SENTINEL).all())


# --------------------------------------------------------------------------- B. gb_part_reduce
@pytest.mark.parametrize("C", [64, 136])
@pytest.mark.parametrize("nblk", [1, 7, 513, 1000])
def test_gb_part_reduce_integer_exact(nblk, C):
    """Partial rows of small integers (every fp32 sum exact in any order): the slice sums equal the float64
    ones bit for bit, slices past the last row are zero, nothing is written beyond [B][slices][2 C]."""
    from cwdm_hip._lib import check, lib
    L = lib()
    B = 2
    S = L.cwdm_debug_gb_part_reduce(None, 0, 0, 0, 0, None, None)   # the plan's slice count
    assert S == 64
    g = torch.Generator().manual_seed(22 + nblk + C)
    rows = torch.randint(-8, 9, (B, nblk, 2 * C), generator=g).float()
    ind = rows.to(DEV)
    out = torch.full((B * S * 2 * C + 2 * C,), SENTINEL, device=DEV)
    check(L.cwdm_debug_gb_part_reduce(ind.data_ptr(), nblk, C, B, S, out.data_ptr(), None))
    per = -(-nblk // S)
    ref = torch.zeros(B, S, 2 * C, dtype=torch.float64)
    for s in range(S):
        if s * per < nblk:
            ref[:, s] = rows[:, s * per:min(nblk, (s + 1) * per)].double().sum(1)
    got = out[:B * S * 2 * C].reshape(B, S, 2 * C).cpu().double()
    assert torch.equal(got, ref)
    assert torch.equal(got.sum(1), rows.double().sum(1))
    assert bool((out[B * S * 2 * C:] == SENTINEL).all())


# --------------------------------------------------------------------------- C. partials -> finalize -> apply
def _gn_ex(L, r, x0, c0, x1, c1, dud, du_mode, dx0, acc0, dx1, acc1, dgam, dbet, ws, chs=None, chs_stride=0,
           acc_affine=0, pre_part=None, pre_nblk=0, coef_mode=0):
    coef = ctypes.c_void_p()
    rc = L.cwdm_debug_gn_silu_bwd_ex(
        x0.data_ptr(), c0, x1.data_ptr() if x1 is not None else None, c1, dud.data_ptr(), du_mode,
        r["ssd"].data_ptr(), r["mrd"].data_ptr(), r["gd"].data_ptr(), r["G"], r["B"], *r["grid"], r["dtype"],
        dx0.data_ptr(), acc0, dx1.data_ptr() if dx1 is not None else None, acc1, dgam.data_ptr(), dbet.data_ptr(),
        ws.data_ptr(), ws.numel(), chs.data_ptr() if chs is not None else None, chs_stride, acc_affine,
        pre_part.data_ptr() if pre_part is not None else None, pre_nblk, coef_mode, ctypes.byref(coef), None)
    return rc, coef.value


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["ct32_cpg2", "ct32_seam32"])
def test_gbwd_chain_finalize_apply_vs_float64_autograd(name, dtype_name):
    """The dgrad's partials as pre_part of the GroupNorm backward (no reduce pass of its own): dx0 / dx1, dgamma,
    dbeta against float64 autograd of SiLU(GroupNorm(x)) . du on the stored du.
      dgamma, dbeta (fp32): 1e-4 of the float64 sum of |terms|
      dx (16-bit): ulp16(|ref|) + 1e-5 (|k0| 1.1 |du| + |k1 x| + |k2|)
    and acc_affine = 1 adds to prefilled dgamma / dbeta (+ one fp32 rounding of the sum)."""
    from cwdm_hip._lib import check, lib
    L = lib()
    r = dict(_gbwd_case(name, dtype_name))
    assert r["used"] == 1
    B, C, c0, grid, tdt = r["B"], r["C"], r["c0"], r["grid"], r["tdt"]
    c1 = C - c0
    r["gd"] = r["gamma"].to(DEV)
    ws = torch.empty(L.cwdm_gn_silu_bwd_workspace_bytes(C, B, *grid), dtype=torch.uint8, device=DEV)
    dx0 = torch.empty(B, *grid, c0, device=DEV, dtype=tdt)
    dx1 = torch.empty(B, *grid, c1, device=DEV, dtype=tdt) if c1 else None
    dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rc, _ = _gn_ex(L, r, r["x0"], c0, r["x1"], c1, r["du"], 0, dx0, 0, dx1, 0, dgam, dbet, ws,
                   pre_part=r["part"], pre_nblk=r["nblk"])
    check(rc)
    du_nc = r["dul"].movedim(-1, 1)
    dx_ref, dg_ref, db_ref = _gn_bwd_autograd(r["x"], du_nc, r["gamma"], r["beta"], r["G"])
    e = _gn_bwd_ref(r["xl"], r["dul"], r["gamma"], r["ss"], r["mr"])
    # the explicit form (whose coefficients make the bound) is the autograd result, up to the fp32 cast of ss / mr
    assert float((e["dx"] - dx_ref).abs().max()) <= 1e-6 * float(dx_ref.abs().max())
    got = torch.cat([dx0.cpu().double()] + ([dx1.cpu().double()] if c1 else []), -1)
    rx = ((got - dx_ref).abs() / (_ulp16(dx_ref, tdt) + 1e-5 * e["mag"])).max()
    rg = ((dgam.cpu().double() - dg_ref).abs() / (1e-4 * e["dgamma_abs"])).max()
    rb = ((dbet.cpu().double() - db_ref).abs() / (1e-4 * e["dbeta_abs"])).max()
    for what, v in (("dx", rx), ("dgamma", rg), ("dbeta", rb)):
        _report(f"C {name} {dtype_name} {what}", v)
    assert rx <= 1.0 and rg <= 1.0 and rb <= 1.0, (float(rx), float(rg), float(rb))
    # the plan's route above 512 tiles, at this size: the slice sums of the partials as pre_part -- the same bounds
    S = L.cwdm_debug_gb_part_reduce(None, 0, 0, 0, 0, None, None)
    sl = torch.empty(B, S, C, 2, device=DEV)
    check(L.cwdm_debug_gb_part_reduce(r["part"].data_ptr(), r["nblk"], C, B, S, sl.data_ptr(), None))
    dx0s = torch.empty_like(dx0)
    dx1s = torch.empty_like(dx1) if c1 else None
    dgs, dbs = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rc, _ = _gn_ex(L, r, r["x0"], c0, r["x1"], c1, r["du"], 0, dx0s, 0, dx1s, 0, dgs, dbs, ws, pre_part=sl, pre_nblk=S)
    check(rc)
    gots = torch.cat([dx0s.cpu().double()] + ([dx1s.cpu().double()] if c1 else []), -1)
    assert bool(((gots - dx_ref).abs() <= _ulp16(dx_ref, tdt) + 1e-5 * e["mag"]).all())
    assert bool(((dgs.cpu().double() - dg_ref).abs() <= 1e-4 * e["dgamma_abs"]).all())
    assert bool(((dbs.cpu().double() - db_ref).abs() <= 1e-4 * e["dbeta_abs"]).all())
    # acc_affine = 1: added to what is there
    g = torch.Generator().manual_seed(23)
    pg, pb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dgam2, dbet2 = pg.to(DEV), pb.to(DEV)
    rc, _ = _gn_ex(L, r, r["x0"], c0, r["x1"], c1, r["du"], 0, dx0, 0, dx1, 0, dgam2, dbet2, ws, acc_affine=1,
                   pre_part=r["part"], pre_nblk=r["nblk"])
    check(rc)
    wg, wb = pg.double() + dg_ref, pb.double() + db_ref
    assert bool(((dgam2.cpu().double() - wg).abs() <= 1e-4 * e["dgamma_abs"] + 2.0 ** -23 * wg.abs()).all())
    assert bool(((dbet2.cpu().double() - wb).abs() <= 1e-4 * e["dbeta_abs"] + 2.0 ** -23 * wb.abs()).all())


def test_gn_silu_bwd_pre_part_refuses_resampled_du():
    """Fused partials belong to a du at the GroupNorm's own grid: du_mode != 0 with pre_part is CWDM_E_INVALID."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import lib
    L = lib()
    r = dict(_gbwd_case("ct32_cpg2", "bf16"))
    B, C, grid, tdt = r["B"], r["C"], r["grid"], r["tdt"]
    r["gd"] = r["gamma"].to(DEV)
    ws = torch.empty(L.cwdm_gn_silu_bwd_workspace_bytes(C, B, *grid), dtype=torch.uint8, device=DEV)
    dx0 = torch.zeros(B, *grid, C, device=DEV, dtype=tdt)
    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    du2 = torch.zeros(B, *(2 * s for s in grid), C, device=DEV, dtype=tdt)
    for mode, dud in ((1, du2), (2, r["du"])):
        rc, _ = _gn_ex(L, r, r["x0"], C, None, 0, dud, mode, dx0, 0, None, 0, dgam, dbet, ws, pre_part=r["part"],
                       pre_nblk=r["nblk"])
        assert rc == _lib.E_INVALID, mode


# --------------------------------------------------------------------------- D. the fused apply in the 1x1 skip dgrad
# name, N (n0 | n1), K (k0 | k1), B, grid, groups, accumulate
GA_CASES = {
    "n64_store": ((64, 0), (128, 0), 1, (4, 8, 8), 8, 0),                 # V = 256, 64-channel blocks, one output
    # V = 320: the 256-row blocks straddle batch entries, the last one has a row tail; outputs 128 | 64
    "n192_straddle_acc": ((128, 64), (64, 0), 3, (5, 8, 8), 32, 1),
    "n128_two_dy_acc": ((64, 64), (192, 64), 2, (4, 8, 10), 32, 1),       # 128-channel blocks, dY from two sources
    "n40_mask": ((40, 0), (16, 0), 1, (4, 8, 8), 8, 0),                   # the channel mask inside a 64-channel block
}


def _gapply_setup(Ns, Ks, B, grid, G, dtype_name, seed=24):
    from cwdm_hip._lib import check, lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    g = torch.Generator().manual_seed(seed)
    n0, n1 = Ns
    N, K = n0 + n1, Ks[0] + Ks[1]
    w = (torch.randn(K, N, 1, 1, 1, generator=g) / math.sqrt(K)).to(tdt).float()   # the skip conv: N -> K channels
    dyl = torch.randn(B, *grid, K, generator=g).to(tdt)
    x = (0.3 + 1.5 * torch.randn(B, N, *grid, generator=g)).to(tdt).float()
    dul = torch.randn(B, *grid, N, generator=g).to(tdt)
    gamma = 1 + 0.1 * torch.randn(N, generator=g)
    beta = 0.1 * torch.randn(N, generator=g)
    base = torch.randn(B, *grid, N, generator=g).to(tdt)
    ss, mr = _gn_stats(x, gamma, beta, G)
    pk = torch.empty(L.cwdm_conv3d_packed_bytes(N, K, 1, dtype), dtype=torch.uint8, device=DEV)
    wd = w.to(DEV).contiguous()
    check(L.cwdm_conv3d_pack_dgrad(ctypes.c_void_p(wd.data_ptr()), K, N, 1, dtype, ctypes.c_void_p(pk.data_ptr()), None))
    xd = _nd(x).to(DEV, tdt)
    dyd = dyl.to(DEV)
    r = dict(B=B, C=N, G=G, grid=grid, dtype=dtype, tdt=tdt, n0=n0, n1=n1, K0=Ks[0], K1=Ks[1], pk=pk,
             dy0=dyd[..., :Ks[0]].contiguous(), dy1=dyd[..., Ks[0]:].contiguous() if Ks[1] else None,
             x0=xd[..., :n0].contiguous(), x1=xd[..., n0:].contiguous() if n1 else None, dud=dul.to(DEV),
             ssd=ss.to(DEV), mrd=mr.to(DEV), gd=gamma.to(DEV), base=base,
             # float64 pieces of the reference
             conv=dyl.double() @ w.double().reshape(K, N), conv_abs=dyl.double().abs() @ w.double().abs().reshape(K, N),
             gn=_gn_bwd_ref(_nd(x).double(), dul.double(), gamma, ss, mr))
    ag, _, _ = _gn_bwd_autograd(x, dul.double().movedim(-1, 1), gamma, beta, G)
    assert float((r["gn"]["dx"] - ag).abs().max()) <= 1e-6 * float(ag.abs().max())   # (the fp32 cast of ss / mr)
    r["gn_dx"] = ag
    return r


def _gapply_call(L, r, coef, acc, lt, bias=None):
    """the skip dgrad through cwdm_debug_conv3d_gapply -> (dx [B, ..., N] on the CPU, used)"""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check
    n0, n1 = r["n0"], r["n1"]
    o0 = r["base"][..., :n0].contiguous().to(DEV)
    o1 = r["base"][..., n0:].contiguous().to(DEV) if n1 else None
    d = _lib.ConvDesc()
    d.dtype, d.B, (d.D, d.H, d.W), d.cout = r["dtype"], r["B"], r["grid"], n0 + n1
    d.b0, d.b_c0, d.b_w = r["dy0"].data_ptr(), r["K0"], r["pk"].data_ptr()
    if r["K1"]:
        d.b1, d.b_c1 = r["dy1"].data_ptr(), r["K1"]
    d.res_mode = -1
    d.out, d.out_dtype, d.accumulate = o0.data_ptr(), r["dtype"], acc
    if n1:
        d.out1, d.out_c0 = o1.data_ptr(), n0
    if bias is not None:
        d.bias, d.bias_bstride = bias.data_ptr(), n0 + n1
    used = ctypes.c_int(-1)
    prevlt = L.cwdm_debug_pw_lt(lt)
    try:
        check(L.cwdm_debug_conv3d_gapply(ctypes.byref(d), r["x0"].data_ptr(), r["x1"].data_ptr() if n1 else None,
                                         r["dud"].data_ptr(), r["ssd"].data_ptr(), coef, ctypes.byref(used), None))
        torch.cuda.synchronize()
    finally:
        L.cwdm_debug_pw_lt(prevlt)
    return torch.cat([o0.cpu()] + ([o1.cpu()] if n1 else []), -1), used.value


def _gapply_coef(L, r):
    """the coefficients as the plan gets them: reduce + finalize only; dx must stay untouched"""
    from cwdm_hip._lib import check
    B, N, grid, tdt = r["B"], r["C"], r["grid"], r["tdt"]
    ws = torch.empty(L.cwdm_gn_silu_bwd_workspace_bytes(N, B, *grid), dtype=torch.uint8, device=DEV)
    s0 = torch.full((B, *grid, r["n0"]), 3.0, device=DEV, dtype=tdt)
    s1 = torch.full((B, *grid, r["n1"]), 3.0, device=DEV, dtype=tdt) if r["n1"] else None
    dgam, dbet = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    rc, coef = _gn_ex(L, r, r["x0"], r["n0"], r["x1"], r["n1"], r["dud"], 0, s0, 0, s1, 0, dgam, dbet, ws, coef_mode=1)
    check(rc)
    torch.cuda.synchronize()
    assert coef and ws.data_ptr() <= coef < ws.data_ptr() + ws.numel()
    assert bool((s0 == 3.0).all()) and (s1 is None or bool((s1 == 3.0).all())), "coef_out mode wrote dx"
    return ws, coef   # (ws owns the coefficients)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(GA_CASES))
def test_gapply_skip_dgrad_vs_float64(name, dtype_name):
    """dx = W^T dY (+ base) + GroupNorm-backward(x, du), all float64, against the fused launch with both
    epilogues (cwdm_debug_pw_lt 1 / 0): each within
      ulp16(|ref|) + 1e-5 (sum |w| |dy| + |base| + |k0| 1.1 |du| + |k1 x| + |k2|),
    the two bitwise equal, and the row-major launch counter moving only for the row-major one."""
    from cwdm_hip._lib import lib
    L = lib()
    Ns, Ks, B, grid, G, acc = GA_CASES[name]
    r = _gapply_setup(Ns, Ks, B, grid, G, dtype_name)
    ws, coef = _gapply_coef(L, r)
    base = r["base"].double() if acc else torch.zeros_like(r["conv"])
    ref = r["conv"] + base + r["gn_dx"]
    bound = _ulp16(ref, r["tdt"]) + 1e-5 * (r["conv_abs"] + base.abs() + r["gn"]["mag"])
    n0 = L.cwdm_debug_pw_lt(-1)
    got1, used1 = _gapply_call(L, r, coef, acc, 1)
    n1 = L.cwdm_debug_pw_lt(-1)
    got0, used0 = _gapply_call(L, r, coef, acc, 0)
    assert used1 == 1 and used0 == 1
    assert n1 > n0 and L.cwdm_debug_pw_lt(-1) == n1
    for lt, got in ((1, got1), (0, got0)):
        ratio = ((got.double() - ref).abs() / bound).max()
        _report(f"D {name} {dtype_name} pw_lt={lt} dx", ratio)
        assert ratio <= 1.0, (name, lt, float(ratio))
    assert torch.equal(got1, got0)
    del ws


@pytest.mark.parametrize("why", ["fewer_than_256_voxels", "bias", "out_c0_not_in_8s"])
def test_gapply_refusals_leave_a_plain_skip_dgrad(why):
    """An offer the route must refuse: used == 0 and the output is the 1x1 conv alone (no apply term)."""
    from cwdm_hip._lib import lib
    L = lib()
    Ns, Ks, grid, bias = (64, 0), (128, 0), (4, 8, 8), None
    if why == "fewer_than_256_voxels":
        grid = (4, 7, 8)
    elif why == "out_c0_not_in_8s":
        Ns = (12, 52)
    r = _gapply_setup(Ns, Ks, 1, grid, 4, "bf16")
    ref = r["conv"]
    if why == "bias":
        b = torch.randn(1, 64, generator=torch.Generator().manual_seed(25))
        bias = b.to(DEV)
        ref = ref + b.double().reshape(1, 1, 1, 1, 64)
    # (coefficients are only offered; a refused call never reads them)
    coef = torch.zeros(1, 64, 4, device=DEV)
    got, used = _gapply_call(L, r, coef.data_ptr(), 0, 1, bias=bias)
    assert used == 0
    bound = _ulp16(ref, r["tdt"]) + 1e-5 * (r["conv_abs"] + 1.0)
    assert bool(((got.double() - ref).abs() <= bound).all())


# --------------------------------------------------------------------------- E. the fused channel sums
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_gn_silu_bwd_channel_sums_vs_float64(dtype_name):
    """chs[b * stride + c] += sum over voxels of the written dx0 (chs_reduce_kernel ADDS to what is there):
    prefilled with a sentinel, stride 80 > C = 64, the padding untouched.  Bound per channel against the float64
    sum of the stored dx0: eps(dtype) sum |dx0|, plus one fp32 rounding of (sentinel + sum) -- the add into the
    prefilled word, which the sum's own bound does not cover.  Two sources with chs: CWDM_E_UNSUPPORTED."""
    from cwdm_hip import _lib
    from cwdm_hip._lib import check, lib
    L = lib()
    dtype, tdt = _dt(dtype_name)
    B, C, G, grid, stride = 2, 64, 8, (4, 8, 6), 80
    g = torch.Generator().manual_seed(26)
    x = (0.3 + 1.5 * torch.randn(B, C, *grid, generator=g)).to(tdt).float()
    du = torch.randn(B, *grid, C, generator=g).to(tdt)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    ss, mr = _gn_stats(x, gamma, 0.1 * torch.randn(C, generator=g), G)
    r = dict(B=B, G=G, grid=grid, dtype=dtype, ssd=ss.to(DEV), mrd=mr.to(DEV), gd=gamma.to(DEV))
    xd, dud = _nd(x).to(DEV, tdt), du.to(DEV)
    ws = torch.empty(L.cwdm_gn_silu_bwd_workspace_bytes(C, B, *grid), dtype=torch.uint8, device=DEV)
    dx0 = torch.empty(B, *grid, C, device=DEV, dtype=tdt)
    dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    pre = torch.full((B, stride), 3.0)
    pre[:, C:] = SENTINEL
    chs = pre.to(DEV)
    rc, _ = _gn_ex(L, r, xd, C, None, 0, dud, 0, dx0, 0, None, 0, dgam, dbet, ws, chs=chs, chs_stride=stride)
    check(rc)
    st = dx0.cpu().double().reshape(B, -1, C)
    want = 3.0 + st.sum(1)
    eps = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -7}[dtype_name]
    got = chs.cpu().double()
    ratio = ((got[:, :C] - want).abs() / (eps * st.abs().sum(1) + 2.0 ** -24 * want.abs())).max()
    _report(f"E {dtype_name} channel sums", ratio)
    assert ratio <= 1.0
    assert bool((got[:, C:] == SENTINEL).all())
    x0, x1 = xd[..., :32].contiguous(), xd[..., 32:].contiguous()
    dx1 = torch.empty(B, *grid, 32, device=DEV, dtype=tdt)
    rc, _ = _gn_ex(L, r, x0, 32, x1, 32, dud, 0, dx0, 0, dx1, 0, dgam, dbet, ws, chs=chs, chs_stride=stride)
    assert rc == _lib.E_UNSUPPORTED
