// Host side of the DMA-staged conv3d (conv3d_v4.hpp) and its pre-passes:
//   * cwdm_gn_apply: SiLU(GroupNorm(x)) of one or two channels-last sources
//     written once into a workspace tensor (the conv then stages raw copies),
//   * the 1x1 skip segment (ResBlock skip_connection) runs first as a B-only
//     conv into a workspace tensor that the 3x3x3 conv adds as its residual.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "conv3d_v4.hpp"

namespace cwdm {

template __global__ void conv3d_v4_kernel<bf16_t, 0, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 0, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 0, true, false, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 0, true, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 1, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 1, true>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 0, false>(V4Params);
template __global__ void conv3d_v4_kernel<bf16_t, 1, false>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 0, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 0, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 0, true, false, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 0, true, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 1, true, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 1, true>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 0, false>(V4Params);
template __global__ void conv3d_v4_kernel<f16_t, 1, false>(V4Params);
template __global__ void conv3d_v4_kernel<float, 0, false>(V4Params);
template __global__ void conv3d_v4_kernel<float, 1, false>(V4Params);

namespace {

// out[v][c] = SiLU(x[v][c] * sc[b][c] + sh[b][c]); a thread handles one
// 8-channel group of VPT voxels a quarter of the volume apart (each load /
// store instruction still covers consecutive voxels across the lanes), so
// VPT loads are in flight together and the scale/shift reload only when the
// batch index changes.  32-bit item indices (host-checked: B * V * C / 8 < 2^31;
// the 64-bit version's three 64-bit divisions per voxel cost as much issue as
// the traffic it moves).
// cm: write the chunk-major layout [B][C / CK][V][CK] the DMA-staged conv reads
// as contiguous halo rows (CK = 16 bf16 / 8 fp32 channels = 32 bytes per voxel)
template <typename T, int VPT>
__global__ void __launch_bounds__(256) gn_apply_kernel(const T* __restrict__ x0, int c0, const T* __restrict__ x1,
                                                      int c1, const float* __restrict__ gn, FastDiv dvpb,
                                                      FastDiv dg8, unsigned nvox, unsigned nq, T* __restrict__ out,
                                                      int cm) {
  const int C = c0 + c1;
  const unsigned i0 = blockIdx.x * 256u + threadIdx.x;   // (voxel slot, group)
  const unsigned vq = fdiv(i0, dg8);                     // voxels vq, vq + nq, ...
  if (vq >= nq) return;
  const int c = (int)(i0 - vq * dg8.d) * 8;
  constexpr int CK = 32 / sizeof(T);
  const bool first = c < c0;
  const T* xs = first ? x0 + c : x1 + (c - c0);
  const unsigned xc = first ? c0 : c1;
  float xv[VPT][8];
  unsigned vs[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const unsigned v = vq + k * nq < nvox ? vq + k * nq : nvox - 1;
    vs[k] = v;
    const T* src = xs + (size_t)v * xc;
    if constexpr (sizeof(T) == 2) {
      unpack<T>(*reinterpret_cast<const u32x4*>(src), xv[k]);
    } else {
      unpack<float>(*reinterpret_cast<const u32x4*>(src), xv[k]);
      unpack<float>(*reinterpret_cast<const u32x4*>(src + 4), xv[k] + 4);
    }
  }
  unsigned bprev = 0xFFFFFFFFu;
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    if (vq + k * nq >= nvox) break;
    const unsigned v = vs[k];
    const unsigned b = fdiv(v, dvpb);
    if (b != bprev) {
      const float4* g4 = reinterpret_cast<const float4*>(gn + ((size_t)b * C + c) * 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 t = g4[e];  // (sc, sh) of channels c + 2e, c + 2e + 1
        silu_aff_coef(t.x, t.y, sc[2 * e], sh[2 * e]);
        silu_aff_coef(t.z, t.w, sc[2 * e + 1], sh[2 * e + 1]);
      }
      bprev = b;
    }
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = silu_aff(xv[k][e], sc[e], sh[e]);
    T* dst = cm ? out + ((size_t)(b * (unsigned)(C / CK) + (unsigned)(c / CK)) * dvpb.d + (v - b * dvpb.d)) * CK + (c % CK)
                : out + (size_t)v * C + c;
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<u32x4*>(dst) = pack<T>(y);
    } else {
      *reinterpret_cast<u32x4*>(dst) = pack<float>(y);
      *reinterpret_cast<u32x4*>(dst + 4) = pack<float>(y + 4);
    }
  }
}

// GroupNorm finalize + SiLU(GN(x)) pre-pass in one launch (small grids,
// GnFinFuse): workgroup (16-channel chunk j, voxel block, batch entry) first
// reduces the statistics partials of its 16 channels -- parts x 16 (sum, sum^2)
// pairs, 128 contiguous bytes per part -- in fp64 (thread (part slice r,
// channel cl) over parts r, r + 16, ..., then the 16 slices and the group's
// channels in order), derives (scale, shift) as gn_finalize does, and applies
// them to its voxels, writing the chunk-major layout (32 bytes of the chunk per
// voxel).  Workgroups of voxel block 0 also write ss / mr for later readers.
// 16-bit types; a chunk lies in one source (c0 % 16 == 0); cpg divides 16.
struct GnFinApplyArgs {
  const void* x0; int c0; const void* x1; int c1;
  const float* s0; long long p0; const float* s1; long long p1;
  const float* gamma; const float* beta; int groups; double n; float eps;
  float* ss; float* mr; void* out;
  int V, vblk;   // voxels per batch entry, voxels per workgroup
  static constexpr bool kFilm = false;
};
// ... of a FiLM ResBlock's out_layers.0: the rows [s | t] folded into the pair (film_fold), as
// gn_finalize_film_kernel does.  Its own instantiation: the plain kernel's arguments and code stay as they are.
struct GnFinApplyFilmArgs : GnFinApplyArgs {
  const float* film; long long film_bs;
  static constexpr bool kFilm = true;
};

template <typename T, typename Args = GnFinApplyArgs>
__global__ void __launch_bounds__(256) gn_fin_apply_kernel(Args a) {
  const int j = blockIdx.x, vb = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const int C = a.c0 + a.c1, cpg = C / a.groups, c16 = 16 * j;
  const bool first = c16 < a.c0;
  const int cs = first ? a.c0 : a.c1, cl0 = first ? c16 : c16 - a.c0;
  const long long P = first ? a.p0 : a.p1;
  const float2* part = reinterpret_cast<const float2*>(first ? a.s0 : a.s1) + (long long)b * P * cs + cl0;
  __shared__ double r1[256], r2[256];
  __shared__ float tab[32];
  {
    const int cl = t & 15, r = t >> 4;
    double s = 0.0, q = 0.0;
    for (long long k = r; k < P; k += 16) {
      const float2 u = part[k * cs + cl];
      s += (double)u.x;
      q += (double)u.y;
    }
    r1[t] = s;
    r2[t] = q;
  }
  __syncthreads();
  if (t < 16) {
    double s = 0.0, q = 0.0;
    for (int r = 0; r < 16; ++r) { s += r1[r * 16 + t]; q += r2[r * 16 + t]; }
    r1[t] = s;   // (slot t of slice 0 is read only by this thread)
    r2[t] = q;
  }
  __syncthreads();
  if (t < 16) {
    const int g0 = (t / cpg) * cpg;   // the group's first channel within the chunk
    double s = 0.0, q = 0.0;
    for (int k = 0; k < cpg; ++k) { s += r1[g0 + k]; q += r2[g0 + k]; }
    const double mean = s / a.n;
    double var = q / a.n - mean * mean;
    if (var < 0) var = 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    const float meanf = (float)mean;
    const int c = c16 + t;
    float sc = a.gamma[c] * rstd;
    float sh = a.beta[c] - meanf * sc;
    if constexpr (Args::kFilm) film_fold(sc, sh, a.film[b * a.film_bs + c], a.film[b * a.film_bs + C + c]);
    tab[2 * t] = sc;
    tab[2 * t + 1] = sh;
    if (vb == 0) {
      a.ss[((long long)b * C + c) * 2] = sc;
      a.ss[((long long)b * C + c) * 2 + 1] = sh;
      if (t % cpg == 0 && a.mr) {
        const int g = c / cpg;
        a.mr[((long long)b * a.groups + g) * 2] = meanf;
        a.mr[((long long)b * a.groups + g) * 2 + 1] = rstd;
      }
    }
  }
  __syncthreads();
  const int h = t & 1, vs = t >> 1;
  float sa[8], sb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) silu_aff_coef(tab[2 * (8 * h + e)], tab[2 * (8 * h + e) + 1], sa[e], sb[e]);
  const T* xs = reinterpret_cast<const T*>(first ? a.x0 : a.x1) + (long long)b * a.V * cs + cl0 + 8 * h;
  T* out = reinterpret_cast<T*>(a.out) + (((long long)b * (C / 16) + j) * a.V) * 16 + 8 * h;
  const int v0 = vb * a.vblk, v1 = min(a.V, v0 + a.vblk);
  for (int v = v0 + vs; v < v1; v += 128) {
    float f[8];
    unpack<T>(*reinterpret_cast<const u32x4*>(xs + (long long)v * cs), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = silu_aff(f[e], sa[e], sb[e]);
    *reinterpret_cast<u32x4*>(out + (long long)v * 16) = pack<T>(f);
  }
}

int64_t src_voxels(const cwdm_conv3d_desc* d) {
  const int64_t V = d->D * d->H * d->W;
  return d->a_mode == 1 ? V / 8 : V;
}

}  // namespace

std::atomic<unsigned long long*> g_stamps{nullptr};

int cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 256;
    return n > 0 ? n : 256;
  }();
  return ncu;
}

int gnfin_flush(const cwdm_conv3d_desc* d, GnFinFuse* f, hipStream_t s) {
  if (!f || f->used || !d->a_gn || f->ss != d->a_gn) return CWDM_OK;
  f->used = true;
  if (f->film)
    return cwdm_gn_finalize_film(f->s0, f->p0, f->c0, f->s1, f->p1, f->c1, f->gamma, f->beta, f->groups, f->B,
                                 f->voxels, f->eps, f->ss, f->mr, f->film, f->film_bs, s);
  return cwdm_gn_finalize(f->s0, f->p0, f->c0, f->s1, f->p1, f->c1, f->gamma, f->beta, f->groups, f->B, f->voxels,
                          f->eps, f->ss, f->mr, s);
}

// the fused finalize + pre-pass applies: 16-bit, every 16-channel chunk in one
// source and whole groups, few partials per chunk (the small grids: <= 256 parts)
bool gn_fin_fusable(const GnFinFuse& f, int dtype, int c0, int c1) {
  const int C = c0 + c1;
  if (!dtype_half(dtype) || C % 16 || c0 % 16 || f.c0 != c0 || f.c1 != c1 || f.groups <= 0 || C % f.groups) return false;
  const int cpg = C / f.groups;
  // the largest grid, in voxels, whose finalize the pre-pass takes (env CWDM_GNFIN_MAXV, A/B knob):
  // 32^3 -- with per-workgroup partials the 64^3 / 128^3 finalizes qualify too, but the fused pass
  // (~512 workgroups, each re-reducing its chunk's partials) streams the big grids far below the plain
  // pre-pass: r06 same box, 15.33 ms per step without the fusion there vs 15.52 (64^3) / 15.96 (128^3)
  static const long long maxv = env_ll("CWDM_GNFIN_MAXV", 32768);
  return cpg <= 16 && 16 % cpg == 0 && f.p0 <= 256 && (c1 == 0 || f.p1 <= 256) && f.voxels <= maxv;
}

namespace {
int gn_fin_apply(const GnFinFuse& f, const void* x0, int c0, const void* x1, int c1, int64_t B, int64_t V, int dtype,
                 void* out, hipStream_t s) {
  GnFinApplyFilmArgs a{};
  a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1;
  a.s0 = f.s0; a.p0 = f.p0; a.s1 = f.s1; a.p1 = f.p1;
  a.gamma = f.gamma; a.beta = f.beta; a.groups = f.groups;
  a.n = (double)((c0 + c1) / f.groups) * (double)f.voxels; a.eps = f.eps;
  a.ss = f.ss; a.mr = f.mr; a.out = out;
  CWDM_REQUIRE(V < (1LL << 31) && V * (c0 + c1) < (1LL << 31), CWDM_E_UNSUPPORTED, "gn_fin_apply: grid too large");
  a.V = (int)V;
  // ~512 workgroups in all
  const int nchunk = (c0 + c1) / 16;
  long long nvb = std::max<long long>(1, 512 / (nchunk * B));
  a.vblk = (int)std::max<long long>(128, ceil_div(V, nvb));
  nvb = ceil_div(V, (long long)a.vblk);
  CWDM_REQUIRE(B < 65536 && nvb < 65536, CWDM_E_UNSUPPORTED, "gn_fin_apply: grid too large");
  const dim3 grid((unsigned)nchunk, (unsigned)nvb, (unsigned)B);
  if (f.film) {
    a.film = f.film; a.film_bs = f.film_bs;
    if (dtype == CWDM_F16) hipLaunchKernelGGL((gn_fin_apply_kernel<f16_t, GnFinApplyFilmArgs>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gn_fin_apply_kernel<bf16_t, GnFinApplyFilmArgs>), grid, dim3(256), 0, s, a);
    CWDM_LAUNCHED();
    return CWDM_OK;
  }
  const GnFinApplyArgs& pa = a;
  if (dtype == CWDM_F16) hipLaunchKernelGGL(gn_fin_apply_kernel<f16_t>, grid, dim3(256), 0, s, pa);
  else hipLaunchKernelGGL(gn_fin_apply_kernel<bf16_t>, grid, dim3(256), 0, s, pa);
  CWDM_LAUNCHED();
  return CWDM_OK;
}
}  // namespace

int gn_apply(const void* x0, int c0, const void* x1, int c1, const float* gn, int64_t B, int64_t vpb, int dtype,
             void* out, hipStream_t s, int cm = 0) {
  constexpr int VPT = 4;
  const int G8 = (c0 + c1) / 8;
  CWDM_REQUIRE(B * vpb * G8 < (1LL << 31) - 256 * VPT, CWDM_E_UNSUPPORTED,
               "gn_apply: more than 2^31 channel groups in one launch");
  const int64_t nvox = B * vpb, nq = ceil_div(nvox, VPT);
  const dim3 grid((unsigned)ceil_div(nq * G8, 256));
  const FastDiv dvpb = make_fastdiv((unsigned)vpb), dg8 = make_fastdiv((unsigned)G8);
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((gn_apply_kernel<T, VPT>), grid, dim3(256), 0, s, reinterpret_cast<const T*>(x0), c0,
                       reinterpret_cast<const T*>(x1), c1, gn, dvpb, dg8, (unsigned)nvox, (unsigned)nq,
                       reinterpret_cast<T*>(out), cm);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}

V4Params fill_params(const cwdm_conv3d_desc* d, const void* a0, int c0, const void* a1, int c1, int a0_cm,
                     const void* res, int rmode, bool phase) {
  const int esz = dtype_size(d->dtype);
  const int ck = 32 / esz;
  const int64_t SV = src_voxels(d);
  V4Params p{};
  p.B = (int)d->B; p.D = (int)d->D; p.H = (int)d->H; p.W = (int)d->W;
  // the phase instance tiles the source grid (the output is 2D x 2H x 2W)
  if (phase) { p.D /= 2; p.H /= 2; p.W /= 2; }
  p.tx = (p.W + 31) / 32; p.ty = p.H / 4; p.tz = p.D / 4;
  p.cout = d->cout; p.nct = d->cout / 64;
  p.nch0 = c0 / ck; p.nch = (c0 + c1) / ck;
  p.a0 = a0; p.ac0 = c0; p.a1 = a1; p.ac1 = c1;
  p.a0_bstride = SV * c0 * esz; p.a1_bstride = SV * c1 * esz;
  p.a0_bytes = (unsigned)(SV * c0 * esz); p.a1_bytes = (unsigned)(SV * c1 * esz);
  p.amode = phase ? 0 : d->a_mode;
  p.a0_cm = a0_cm;
  p.a0_cvox = (int)SV;
  p.aw = reinterpret_cast<const unsigned char*>(phase ? d->a_w_phase : d->a_w);
  p.bias = d->bias; p.bias_bs = d->bias_bstride;
  p.res = res; p.rmode = rmode;
  p.out = d->out;
  p.out_f32 = (d->out_dtype == CWDM_F32 && d->dtype != CWDM_F32) ? 1 : 0;
  p.stats = d->stats;
  p.out1 = d->out1; p.out_c0 = d->out_c0;
  p.accumulate = d->accumulate;
  p.stamps = g_stamps.load(std::memory_order_relaxed);
  return p;
}

// launch of the route's kernel on prepared sources: a0 (c0 channels, chunk-major if a0_cm) and a1
// (c1 channels, channels-last), residual res / rmode; r: conv_route's, or conv_route_prepared(d, rmode, c);
// partial: fp32 scratch of r.ksplit output slices (unused without a K split)
int v4_launch(const cwdm_conv3d_desc* d, const void* a0, int c0, const void* a1, int c1, int a0_cm,
              const void* res, int rmode, void* partial, const ConvRoute& r, ConvCall& c, hipStream_t s) {
  switch (r.kernel) {
    case ConvKernel::SmallGrid:
      return sg_launch(fill_params(d, a0, c0, a1, c1, a0_cm, res, rmode), d, r.ksplit, partial, c, s);
    case ConvKernel::V5Phase:
      return v5_launch(d, a0, c0, a1, c1, a0_cm, nullptr, nullptr, -1, c, s, nullptr, true);
    case ConvKernel::V5:
    case ConvKernel::V5Split:
      return v5_launch(d, a0, c0, a1, c1, a0_cm, nullptr, res, rmode, c, s);
    case ConvKernel::V4:
      break;
    default:
      return fail(CWDM_E_INVALID, "conv3d: not a route of the DMA-staged launchers");
  }
  V4Params p = fill_params(d, a0, c0, a1, c1, a0_cm, res, rmode);
  const int S = r.ksplit;
  p.ksplit = S;
  p.kper = (p.nch + S - 1) / S;
  if (S > 1) {
    CWDM_REQUIRE(partial, CWDM_E_INVALID, "conv3d: K-split scratch missing");
    p.ks_stride = (long long)p.B * p.D * p.H * p.W * p.cout;
    p.bias = nullptr; p.res = nullptr; p.rmode = -1; p.stats = nullptr;
    p.out = partial; p.out_f32 = 1; p.out1 = nullptr; p.out_c0 = 0; p.accumulate = 0;
  }
  const bool ct32 = r.ct32, fast = r.fast;
  if (ct32) p.nct = d->cout / 32;
  const long long nblk = (long long)p.B * p.tx * p.ty * p.tz * p.nct * S;
  p.nblk = (int)nblk;
  // persistent: two workgroups per CU (80 KB LDS, <= 256 registers per lane each)
  const int ncu = cu_count();
  // workgroups per CU slot of the persistent grid (env CWDM_V4_GRID_MULT, A/B knob)
  static const long long gmul = env_ll("CWDM_V4_GRID_MULT", 4);
  const dim3 grid((unsigned)std::min<long long>(nblk, gmul * ncu));
  // half a tile: ~17k cycles per chunk and ~12k for the epilogue when shared (tools/conv_stamps.py)
  // CWDM_CONV_STAGGER=-1 restores the half-tile delay; measured (r01 v7 kernel,
  // bench.py A/B on one MI355X): no delay 57.15 vs half-tile 56.80 steps/s
  static const int stagger_env = env_int("CWDM_CONV_STAGGER", 0);
  p.stagger_cycles = nblk > 2LL * ncu ? (stagger_env >= 0 ? stagger_env : (p.nch * 17000 + 12000) / 2) : 0;
  prof_begin(c.prof, s);
  auto launch16 = [&](auto tag) {
    using T = decltype(tag);
    if (p.gx0) {   // fused GroupNorm-backward reduce (dgrad, same-grid source: amode 0)
      if (ct32) hipLaunchKernelGGL((conv3d_v4_kernel<T, 0, true, true, true>), grid, dim3(256), 0, s, p);
      else hipLaunchKernelGGL((conv3d_v4_kernel<T, 0, true, false, true>), grid, dim3(256), 0, s, p);
    } else if (ct32) {
      if (p.amode == 1) hipLaunchKernelGGL((conv3d_v4_kernel<T, 1, true, true>), grid, dim3(256), 0, s, p);
      else hipLaunchKernelGGL((conv3d_v4_kernel<T, 0, true, true>), grid, dim3(256), 0, s, p);
    } else if (fast) {
      if (p.amode == 1) hipLaunchKernelGGL((conv3d_v4_kernel<T, 1, true>), grid, dim3(256), 0, s, p);
      else hipLaunchKernelGGL((conv3d_v4_kernel<T, 0, true>), grid, dim3(256), 0, s, p);
    } else {
      if (p.amode == 1) hipLaunchKernelGGL((conv3d_v4_kernel<T, 1, false>), grid, dim3(256), 0, s, p);
      else hipLaunchKernelGGL((conv3d_v4_kernel<T, 0, false>), grid, dim3(256), 0, s, p);
    }
  };
  if (r.takes_gbwd) {   // the fused GroupNorm-backward reduce
    GbwdFuse& g = *c.gbwd;
    p.gx0 = g.x0; p.gx1 = g.x1; p.gc0 = g.c0;
    p.gss = g.ss; p.gmr = g.mr; p.ggroups = g.groups;
    p.gdiv = make_fastdiv((unsigned)(d->cout / g.groups));
    p.stats = g.part;
    g.used = true;
    g.nblk = p.tx * p.ty * p.tz;
  }
  if (d->dtype == CWDM_BF16) {
    launch16(bf16_t{});
  } else if (d->dtype == CWDM_F16) {
    launch16(f16_t{});
  } else {
    if (p.amode == 1) hipLaunchKernelGGL((conv3d_v4_kernel<float, 1, false>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv3d_v4_kernel<float, 0, false>), grid, dim3(256), 0, s, p);
  }
  prof_end(c.prof, s, 2.0 * p.B * p.D * p.H * p.W * (double)p.cout * 27.0 * (c0 + c1));
  CWDM_LAUNCHED();
  if (S > 1) {
    // finish: slice sum over the whole chip, then the per-tile epilogue
    const long long n4 = p.ks_stride / 4;
    float* part = reinterpret_cast<float*>(partial);
    hipLaunchKernelGGL(splitk_sum_kernel<0>, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, s, part, S, n4);
    CWDM_LAUNCHED();
    ConvParams q{};
    q.B = p.B; q.D = p.D; q.H = p.H; q.W = p.W;
    q.tx = p.tx; q.ty = p.ty; q.tz = p.tz;
    q.cout = p.cout; q.nct = p.nct;
    q.bias = d->bias; q.bias_bs = d->bias_bstride;
    q.res = res; q.rmode = rmode;
    q.out = d->out; q.out_f32 = (d->out_dtype == CWDM_F32 && d->dtype != CWDM_F32) ? 1 : (d->dtype == CWDM_F32);
    q.stats = d->stats;
    q.out1 = d->out1; q.out_c0 = d->out_c0;
    q.accumulate = d->accumulate;
    q.ksplit = 1;
    q.partial = part;
    const dim3 rg((unsigned)((long long)p.B * p.tx * p.ty * p.tz * (p.cout / 64)));
    dispatch_dtype(d->dtype, [&](auto tag) -> int {
      using T = decltype(tag);
      hipLaunchKernelGGL((conv3d_reduce_kernel<T, 32, 4, 4, 2>), rg, dim3(256), 0, s, q, 1);
      return CWDM_OK;
    });
    CWDM_LAUNCHED();
  }
  return CWDM_OK;
}

// a conv of the DMA path by its route: the GroupNorm'd input, the 1x1 skip product, the launch.  The
// workspace (>= r.ws_total: conv3d_forward) is carved in ConvRoute's region order
int conv3d_v4_forward(const cwdm_conv3d_desc* d, const ConvRoute& r, ConvCall& c, hipStream_t s) {
  unsigned char* ws = reinterpret_cast<unsigned char*>(d->workspace);
  const void* a0 = d->a0;
  const void* a1 = d->a1;
  int c0 = d->a_c0, c1 = d->a_c1;
  int a0_cm = 0;
  int rc;
  V5Aa aa{};
  if (d->a_gn && !r.gn_in_lds()) {
    // the activated input: in the workspace, or (training) where the plan keeps
    // it for the backward's DMA-staged wgrad
    void* act = ws;
    if (c.act_keep) {
      act = c.act_keep;
      c.act_kept = true;
    } else {
      ws += r.ws_act;
    }
    if (r.kernel == ConvKernel::V5Aa) {
      aa.units = r.aa_units; aa.lead = r.aa_lead;
      aa.x0 = a0; aa.c0 = c0; aa.x1 = a1; aa.c1 = c1; aa.gn = d->a_gn;
      // the sweep counters: the plan's zeroed sync block, else this launch's workspace tail (zeroed here)
      aa.cnt = plan_aa_counters(c.sync);
      if (!aa.cnt) {
        aa.cnt = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(d->workspace) + r.ws_total - r.ws_aa);
        CWDM_HIP(hipMemsetAsync(aa.cnt, 0, r.ws_aa, s));
      }
    } else if (r.gn == GnInput::FinApply) {
      c.gnfin->used = true;
      if ((rc = gn_fin_apply(*c.gnfin, a0, c0, a1, c1, d->B, src_voxels(d), d->dtype, act, s))) return rc;
    } else if ((rc = gn_apply(a0, c0, a1, c1, d->a_gn, d->B, src_voxels(d), d->dtype, act, s, 1))) {
      return rc;
    }
    a0 = act; c0 = c0 + c1; a1 = nullptr; c1 = 0;
    a0_cm = 1;
  }
  const void* res = d->res;
  int rmode = d->res_mode;
  if (d->b_w) {
    void* skip = ws;
    ws += r.ws_skip;
    const cwdm_conv3d_desc e = skip_desc(d, skip);
    switch (r.skip) {
      case SkipKernel::SmallGrid:   // ws: the K-split region, free until the conv
        rc = sg_skip_launch(&e, skip, ws, r.skip_ksplit, c, s);
        break;
      case SkipKernel::Pw: rc = pw_forward(&e, c, false, s); break;
      case SkipKernel::PwSplit: rc = pw_split_forward(&e, c.prof, s); break;
      default: rc = legacy_conv3d_forward(&e, c.prof, s);
    }
    if (rc) return rc;
    res = skip; rmode = 0;
  }
  if (r.gn_in_lds()) return v5_launch(d, a0, c0, a1, c1, 0, d->a_gn, res, rmode, c, s);
  if (r.kernel == ConvKernel::V5Aa) return v5_launch(d, a0, c0, nullptr, 0, 1, nullptr, res, rmode, c, s, &aa);
  return v4_launch(d, a0, c0, a1, c1, a0_cm, res, rmode, r.ksplit > 1 ? ws : nullptr, r, c, s);
}

// ---------------------------------------------------------------------------
// ResBlock with a 1x1 skip_connection (unet.py:264-271): x is read once for
// both users.  One pass writes act = SiLU(GN1(x)) (chunk-major, conv1's input)
// and skip = W_skip . x (channels-last, conv2's residual; its bias is folded
// into conv2's).  Per block of 128 voxels the workgroup copies the x rows into
// LDS with coalesced 16-byte loads (rows padded by 16 B: conflict-free column
// reads); then each wave takes 32 voxels: lane (v, hh) reads quad hh of every
// 16-channel chunk of voxel v, transforms it for act (stored 1 KB-contiguous per
// wave instruction) and feeds it raw as the MFMA B operand against W_skip (A
// operand, the conv packing of a 1x1 kernel, staged once per workgroup) -- the
// conv kernel's accumulator layout.
// ---------------------------------------------------------------------------
struct ApplySkipParams {
  const void* x0; int c0; const void* x1; int c1;
  const float* gn;     // [B][C][2] scale / shift
  long long vpb;       // voxels per batch (% 128 == 0)
  long long nvox;      // B * vpb
  int B;
  void* act;           // chunk-major [B][C / CK][vpb][CK]
  const unsigned char* ws;  // packed 1x1 weights, NT = 64 rows per channel tile
  int cout;            // 32 NF
  void* skip;          // [B][vpb][cout]
};

template <typename T, int NF, int QT>
__global__ void __launch_bounds__(256) gn_apply_skip_kernel(ApplySkipParams p) {
  constexpr int CK = ConvTr<T>::CK, EPQ = ConvTr<T>::EPQ, ES = sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int C = p.c0 + p.c1, nk = C / CK;
  const int wbytes = NF * 32 * C * ES;
  const int RS = C * ES + 16;                      // padded LDS row of one voxel
  for (int i = threadIdx.x * 16; i < wbytes; i += 256 * 16)
    *reinterpret_cast<u32x4*>(lds + i) = *reinterpret_cast<const u32x4*>(p.ws + i);
  float* gl = reinterpret_cast<float*>(lds + wbytes);
  for (int i = threadIdx.x; i < p.B * C * 2; i += 256) gl[i] = p.gn[i];
  unsigned char* xt = lds + wbytes + ((p.B * C * 8 + 15) & ~15);
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 31, hh = lane >> 5, wv = tid >> 6;
  const int q0 = p.c0 * ES / 16, q1 = p.c1 * ES / 16;   // 16-byte quads per row of each source
  const int nq0 = 128 * q0, nqt = (q0 + q1) / 2;        // quads of source 0 per block; per thread
  const long long nblocks = p.nvox / 128;
  // the next block's 128 x rows are loaded into registers while this block
  // computes (consecutive lanes read consecutive 16-byte quads), then copied
  // to LDS: HBM latency hides under the MFMA / store work
  u32x4 pf[QT];
  // quad i = tid + 256 j of a block: source 0 rows first (nq0 quads), then
  // source 1; its global offset within the block's rows is i (or i - nq0) x 16
  // bytes, its LDS offset (row vl, column) is fixed per thread: computed once,
  // so the block loop carries no integer division
  int loff[QT];
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    const int i = tid + 256 * j;
    int vl, col;
    if (i < nq0) { vl = i / q0; col = i - vl * q0; }
    else { const int i1 = i - nq0; vl = i1 / q1; col = q0 + (i1 - vl * q1); }
    loff[j] = vl * RS + col * 16;
  }
  const unsigned char* xb0 = reinterpret_cast<const unsigned char*>(p.x0);
  const unsigned char* xb1 = reinterpret_cast<const unsigned char*>(p.x1);
  auto fetch = [&](long long blk) {
    const unsigned char* s0 = xb0 + blk * 128 * q0 * 16;
    const unsigned char* s1 = xb1 + blk * 128 * q1 * 16 - (long long)nq0 * 16;
#pragma unroll
    for (int j = 0; j < QT; ++j) {
      if (j >= nqt) break;
      const int i = tid + 256 * j;
      pf[j] = *reinterpret_cast<const u32x4*>((i < nq0 ? s0 : s1) + (long long)i * 16);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < QT; ++j) {
      if (j >= nqt) break;
      *reinterpret_cast<u32x4*>(xt + loff[j]) = pf[j];
    }
  };
  if ((long long)blockIdx.x < nblocks) fetch(blockIdx.x);
  for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long long v0 = blk * 128;
    __syncthreads();  // previous block's column reads are done (and W / gn staged, first time)
    put();
    __syncthreads();
    if (blk + gridDim.x < nblocks) fetch(blk + gridDim.x);
    const int vl = wv * 32 + lr;
    const long long v = v0 + vl;
    const int b = (int)(v0 / p.vpb);
    const long long vb = v - (long long)b * p.vpb;
    f32x16 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;
    for (int k = 0; k < nk; ++k) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(xt + vl * RS + k * 32 + hh * 16);
      float xv[EPQ], y[EPQ];
      unpack<T>(q, xv);
      const float* gs = gl + ((long long)b * C + k * CK + hh * EPQ) * 2;
#pragma unroll
      for (int e = 0; e < EPQ; ++e) y[e] = silu(xv[e] * gs[2 * e] + gs[2 * e + 1]);
      T* dst = reinterpret_cast<T*>(p.act) + (((long long)b * nk + k) * p.vpb + vb) * CK + hh * EPQ;
      *reinterpret_cast<u32x4*>(dst) = pack<T>(y);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int n = (f & 1) * 32 + lr;
        const u32x4 a = *reinterpret_cast<const u32x4*>(
            lds + (((f >> 1) * nk + k) * 64 + n) * 32 + ((hh ^ ((n >> 3) & 1)) << 4));
        mfma_acc(acc[f], a, q, (T*)nullptr);
      }
    }
    // skip store: lane (v, hh) holds channels 32 f + 8 j + 4 hh + 0..3 of voxel v
#pragma unroll
    for (int f = 0; f < NF; ++f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        T* o = reinterpret_cast<T*>(p.skip) + v * p.cout + f * 32 + 8 * j + 4 * hh;
        if constexpr (sizeof(T) == 2) {
          uint2 w;
          w.x = pack2<T>(acc[f][4 * j], acc[f][4 * j + 1]);
          w.y = pack2<T>(acc[f][4 * j + 2], acc[f][4 * j + 3]);
          *reinterpret_cast<uint2*>(o) = w;
        } else {
          *reinterpret_cast<float4*>(o) = make_float4(acc[f][4 * j], acc[f][4 * j + 1], acc[f][4 * j + 2], acc[f][4 * j + 3]);
        }
      }
    }
  }
}

int64_t apply_skip_lds_bytes(int dtype, int C, int cout, int64_t B) {
  const int es = dtype_size(dtype);
  return (int64_t)cout * C * es + ((B * C * 8 + 15) & ~15) + 128LL * (C * es + 16);
}

bool apply_skip_ok(int dtype, int C, int cout, int64_t B, int64_t vpb) {
  const int ck = ck_of(dtype);
  const int qt = C * dtype_size(dtype) / 32;   // prefetch registers per thread (kernel's QT)
  return dtype_compute(dtype) && (cout == 64 || cout == 128) && vpb % 128 == 0 &&
         C % ck == 0 && qt <= 16 && apply_skip_lds_bytes(dtype, C, cout, B) <= 160 * 1024;
}

int gn_apply_skip(const void* x0, int c0, const void* x1, int c1, const float* gn, int64_t B, int64_t vpb, int dtype,
                  const void* wskip, int cout, void* act, void* skip, hipStream_t s) {
  CWDM_REQUIRE(apply_skip_ok(dtype, c0 + c1, cout, B, vpb), CWDM_E_UNSUPPORTED, "gn_apply_skip: unsupported shape");
  ApplySkipParams p{};
  p.x0 = x0; p.c0 = c0; p.x1 = x1; p.c1 = c1; p.gn = gn; p.vpb = vpb; p.nvox = B * vpb; p.B = (int)B;
  p.act = act; p.ws = reinterpret_cast<const unsigned char*>(wskip); p.cout = cout; p.skip = skip;
  const int64_t lds = apply_skip_lds_bytes(dtype, c0 + c1, cout, B);
  const int64_t nblocks = p.nvox / 128;
  static const int64_t cap = env_ll("CWDM_SKIP_GRID", 512);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(nblocks, cap)));
  auto go = [&](auto kern) -> int {
    CWDM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), (unsigned)lds, s, p);
    return CWDM_OK;
  };
  int rc;
  rc = dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    return cout == 64 ? go(gn_apply_skip_kernel<T, 2, 16>) : go(gn_apply_skip_kernel<T, 4, 16>);
  });
  if (rc) return rc;
  CWDM_LAUNCHED();
  return CWDM_OK;
}

}  // namespace cwdm

using namespace cwdm;

extern "C" int cwdm_gn_apply(const void* x0, int c0, const void* x1, int c1, const float* gn, int64_t B,
                             int64_t voxels, int dtype, void* out, cwdm_stream_t stream) {
  CWDM_REQUIRE(x0 && gn && out && (c1 == 0 || x1), CWDM_E_INVALID, "cwdm_gn_apply: null pointer");
  CWDM_REQUIRE(c0 > 0 && c0 % 8 == 0 && c1 % 8 == 0 && B > 0 && voxels > 0, CWDM_E_SHAPE,
               "cwdm_gn_apply: channels must be multiples of 8");
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, "cwdm_gn_apply: bad dtype");
  return gn_apply(x0, c0, x1, c1, gn, B, voxels, dtype, out, (hipStream_t)stream);
}

// diagnostics: the DMA-staged conv kernel writes 24 u64 per workgroup (s_memtime
// at start / after the prologue / after each of the first 16 chunks / at the end,
// and HW_ID, XCC_ID) into buf (device memory, >= 24 * workgroups); null disables
extern "C" int cwdm_debug_conv_stamps(void* buf) {
  g_stamps.store(reinterpret_cast<unsigned long long*>(buf));
  return CWDM_OK;
}

// diagnostics / tests: the fused GroupNorm finalize + pre-pass (gn_fin_apply_kernel)
// on its own, so it can be compared with cwdm_gn_finalize + cwdm_gn_apply in one
// process (the plan picks it per conv; CWDM_GNFIN is read once)
extern "C" int cwdm_debug_gn_fin_apply(const float* stats0, int64_t parts0, int c0, const float* stats1,
                                       int64_t parts1, int c1, const float* gamma, const float* beta, int groups,
                                       int64_t B, int64_t voxels, float eps, const void* x0, const void* x1,
                                       int dtype, float* scale_shift, float* mean_rstd, void* out_cm,
                                       cwdm_stream_t stream) {
  CWDM_REQUIRE(stats0 && x0 && gamma && beta && scale_shift && mean_rstd && out_cm && (c1 == 0 || (stats1 && x1)),
               CWDM_E_INVALID, "cwdm_debug_gn_fin_apply: null pointer");
  CWDM_REQUIRE(B > 0 && voxels > 0 && parts0 > 0 && (c1 == 0 || parts1 > 0), CWDM_E_SHAPE,
               "cwdm_debug_gn_fin_apply: empty shape");
  GnFinFuse f{};
  f.s0 = stats0; f.p0 = parts0; f.c0 = c0;
  f.s1 = stats1; f.p1 = parts1; f.c1 = c1;
  f.gamma = gamma; f.beta = beta; f.groups = groups; f.voxels = voxels; f.eps = eps;
  f.ss = scale_shift; f.mr = mean_rstd; f.B = B;
  CWDM_REQUIRE(gn_fin_fusable(f, dtype, c0, c1), CWDM_E_UNSUPPORTED,
               "cwdm_debug_gn_fin_apply: not a fusable shape (16-bit, 16-channel chunks, <= 16 channels per "
               "group dividing 16, <= 256 partials)");
  return gn_fin_apply(f, x0, c0, x1, c1, B, voxels, dtype, out_cm, (hipStream_t)stream);
}

// ... of a FiLM block's norm (GnFinFuse::film): compared with cwdm_gn_finalize_film + cwdm_gn_apply
extern "C" int cwdm_debug_gn_fin_apply_film(const float* stats0, int64_t parts0, int c0, const float* stats1,
                                            int64_t parts1, int c1, const float* gamma, const float* beta,
                                            int groups, int64_t B, int64_t voxels, float eps, const void* x0,
                                            const void* x1, int dtype, float* scale_shift, float* mean_rstd,
                                            void* out_cm, const float* film, int64_t film_bstride,
                                            cwdm_stream_t stream) {
  CWDM_REQUIRE(stats0 && x0 && gamma && beta && scale_shift && mean_rstd && out_cm && film &&
                   (c1 == 0 || (stats1 && x1)),
               CWDM_E_INVALID, "cwdm_debug_gn_fin_apply_film: null pointer");
  CWDM_REQUIRE(B > 0 && voxels > 0 && parts0 > 0 && (c1 == 0 || parts1 > 0), CWDM_E_SHAPE,
               "cwdm_debug_gn_fin_apply_film: empty shape");
  CWDM_REQUIRE(film_bstride >= 2 * (int64_t)(c0 + c1), CWDM_E_SHAPE,
               "cwdm_debug_gn_fin_apply_film: film rows need a batch stride of at least 2 C");
  GnFinFuse f{};
  f.s0 = stats0; f.p0 = parts0; f.c0 = c0;
  f.s1 = stats1; f.p1 = parts1; f.c1 = c1;
  f.gamma = gamma; f.beta = beta; f.groups = groups; f.voxels = voxels; f.eps = eps;
  f.ss = scale_shift; f.mr = mean_rstd; f.B = B;
  f.film = film; f.film_bs = film_bstride;
  CWDM_REQUIRE(gn_fin_fusable(f, dtype, c0, c1), CWDM_E_UNSUPPORTED,
               "cwdm_debug_gn_fin_apply_film: not a fusable shape (16-bit, 16-channel chunks, <= 16 channels per "
               "group dividing 16, <= 256 partials)");
  return gn_fin_apply(f, x0, c0, x1, c1, B, voxels, dtype, out_cm, (hipStream_t)stream);
}
