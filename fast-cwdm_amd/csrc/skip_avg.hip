// The additive skip of UNetModel(additive_skips=True) (guided_diffusion/unet.py:793-794):
// out = (a + b) / 2 over two channels-last (B, V, C) tensors, with the per-part
// (sum, sum^2) statistics of the GroupNorm that consumes the average (same
// [B][parts][C][2] contract as the conv epilogue and cwdm_haar_nd), and its
// adjoint for the backward.  An HBM-bound pass: two reads, one write, 16-byte
// accesses along C.  One thread = one voxel x 8 channels; a workgroup owns one
// contiguous voxel range of one batch index and writes that part's row, summed
// in a fixed order (no atomics: bitwise repeatable).
#include "internal.hpp"

namespace cwdm {
namespace {

// voxels per workgroup (= per statistics part): small grids keep enough workgroups in flight,
// large ones a short partials table
inline int64_t part_voxels(int64_t V) { return V <= 32768 ? 64 : 256; }

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* f) {
  if constexpr (sizeof(T) == 2) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = lo2f<T>(u[i]);
      f[2 * i + 1] = hi2f<T>(u[i]);
    }
  } else {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float* f) {
  if constexpr (sizeof(T) == 2) {
    uint4 q;
    q.x = pack2<T>(f[0], f[1]);
    q.y = pack2<T>(f[2], f[3]);
    q.z = pack2<T>(f[4], f[5]);
    q.w = pack2<T>(f[6], f[7]);
    *reinterpret_cast<uint4*>(p) = q;
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) skip_avg_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                       T* __restrict__ out, float* __restrict__ stats, int64_t V,
                                                       int C, int per, int parts) {
  __shared__ float red[256 * 16];
  const int G = C / 8;
  const int tid = threadIdx.x, g = tid % G, vl = tid / G, VB = 256 / G;
  const int64_t bi = blockIdx.x / parts, part = blockIdx.x % parts;
  const int64_t v0 = part * per;
  const int nv = (int)min((int64_t)per, V - v0);   // the last part's voxel tail
  float ssum[8], ssq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { ssum[e] = 0.f; ssq[e] = 0.f; }
  for (int vv = vl; vl < VB && vv < nv; vv += VB) {  // threads past G x VB idle (C / 8 not a power of two)
    const int64_t o = ((bi * V + v0 + vv) * G + g) * 8;
    float x[8], y[8];
    load8(a + o, x);
    load8(b + o, y);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[e] = 0.5f * (x[e] + y[e]);
      ssum[e] += x[e];
      ssq[e] += x[e] * x[e];
    }
    store8(out + o, x);
  }
  if (!stats) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[tid * 16 + e] = ssum[e]; red[tid * 16 + 8 + e] = ssq[e]; }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int gg = c / 8, e = c % 8;
    float sm = 0.f, sq = 0.f;
    for (int k = 0; k < VB; ++k) { sm += red[(k * G + gg) * 16 + e]; sq += red[(k * G + gg) * 16 + 8 + e]; }
    const int64_t pidx = (bi * parts + part) * C + c;
    stats[pidx * 2 + 0] = sm;
    stats[pidx * 2 + 1] = sq;
  }
}

// da (+)= dy / 2, db (+)= dy / 2; one thread = 8 channels of one voxel.  The half is rounded to
// the buffer's dtype before it is added (an fp16 subnormal half is not exact): dst = old + 0.5 * dy
// as the dtype's own arithmetic gives it
template <typename T>
__global__ void __launch_bounds__(256) skip_avg_bwd_kernel(int64_t n, const T* __restrict__ dy, T* __restrict__ da,
                                                           int acc_a, T* __restrict__ db, int acc_b) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float g[8];
  load8(dy + i * 8, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = Elem<T>::to_f(Elem<T>::from_f(0.5f * g[e]));
  T* const dst[2] = {da, db};
  const int acc[2] = {acc_a, acc_b};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = g[e];
    if (acc[k]) {
      float old[8];
      load8(dst[k] + i * 8, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += old[e];
    }
    store8(dst[k] + i * 8, o);
  }
}

}  // namespace
}  // namespace cwdm

using namespace cwdm;

extern "C" int64_t cwdm_skip_avg_parts(int64_t V) { return V > 0 ? ceil_div(V, part_voxels(V)) : 0; }

extern "C" int cwdm_skip_avg(const void* a, const void* b, void* out, float* stats, int dtype, int64_t B, int64_t V,
                             int C, cwdm_stream_t stream) {
  CWDM_REQUIRE(a && b && out, CWDM_E_INVALID, "cwdm_skip_avg: null pointer");
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, "cwdm_skip_avg: bad dtype");
  CWDM_REQUIRE(B > 0 && V > 0, CWDM_E_SHAPE, "cwdm_skip_avg: empty grid");
  CWDM_REQUIRE(C > 0 && C % 8 == 0 && C <= 2048, CWDM_E_UNSUPPORTED,
               "cwdm_skip_avg: channels must be a multiple of 8, at most 2048");
  const int64_t parts = cwdm_skip_avg_parts(V);
  CWDM_REQUIRE(B * parts < (1LL << 31), CWDM_E_SHAPE, "cwdm_skip_avg: grid too large");
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL(skip_avg_kernel<T>, dim3((unsigned)(B * parts)), dim3(256), 0, s,
                       reinterpret_cast<const T*>(a), reinterpret_cast<const T*>(b), reinterpret_cast<T*>(out), stats,
                       V, C, (int)part_voxels(V), (int)parts);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}

extern "C" int cwdm_skip_avg_bwd(const void* dy, void* da, int acc_a, void* db, int acc_b, int dtype, int64_t B,
                                 int64_t V, int C, cwdm_stream_t stream) {
  CWDM_REQUIRE(dy && da && db, CWDM_E_INVALID, "cwdm_skip_avg_bwd: null pointer");
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, "cwdm_skip_avg_bwd: bad dtype");
  CWDM_REQUIRE(B > 0 && V > 0, CWDM_E_SHAPE, "cwdm_skip_avg_bwd: empty grid");
  CWDM_REQUIRE(C > 0 && C % 8 == 0 && C <= 2048, CWDM_E_UNSUPPORTED,
               "cwdm_skip_avg_bwd: channels must be a multiple of 8, at most 2048");
  const int64_t n = B * V * (C / 8);
  CWDM_REQUIRE(ceil_div(n, 256) < (1LL << 31), CWDM_E_SHAPE, "cwdm_skip_avg_bwd: grid too large");
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL(skip_avg_bwd_kernel<T>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, n,
                       reinterpret_cast<const T*>(dy), reinterpret_cast<T*>(da), acc_a, reinterpret_cast<T*>(db),
                       acc_b);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}
