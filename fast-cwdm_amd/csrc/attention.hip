// The bottleneck attention block of UNetModel(bottleneck_attention=True)
// (AttentionBlock + QKVAttention(Legacy), guided_diffusion/unet.py:314-444):
//   n = GroupNorm(x) (no activation); qkv = W_qkv n + b; a = softmax(q k^T / sqrt(ch)) v;
//   y = x + W_proj a + b_proj
// over the T = d h w voxels of the coarsest grid, channels-last (B, T, C).
//
// Every product runs on one 16x16 MFMA tile primitive (mma below): the 16-bit
// dtypes on v_mfma_f32_16x16x16 (bf16 / f16), fp32 plans on four exact
// v_mfma_f32_16x16x4_f32 -- same operand contract, so each kernel is written
// once.  Element j of a lane's fragment is k = 4 (lane >> 4) + j of row / column
// lane & 15; a result tile has its column on the lane and rows 4 (lane >> 4) + i
// in its 4 registers.  The kernels orient each product so that the next one
// sums over the result's ROW index: the accumulators are then the next
// product's B operand as they stand (scores are computed transposed,
// S^T = K Q^T, and O^T = V^T P^T), and a lane owns ONE query's running
// max / sum.
//
// Kernels (launch order of the forward): attn_linear (the GroupNorm apply fused
// into the qkv projection), attn_fwd (streaming softmax(QK^T)V, K/V blocks
// through LDS), attn_linear again (proj_out + residual + GroupNorm partials).
// Backward: attn_rowdot (D = rowsum(dO o O)), attn_bwd_kv (one workgroup per key
// tile: dK, dV), attn_bwd_q (one per query tile: dQ), gn_lin_bwd (GroupNorm
// without SiLU).  No atomics anywhere: every sum has one owner and a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "internal.hpp"

namespace cwdm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// ---- the tile primitive ------------------------------------------------------
template <typename T> struct Frag;
template <> struct Frag<bf16_t> { s16x4 v; };
template <> struct Frag<f16_t> { h16x4 v; };
template <> struct Frag<float> { f32x4 v; };

__device__ __forceinline__ f32x4 mma(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<f16_t>& a, const Frag<f16_t>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
  // step j covers the logical k = 4 g + j of every lane group g: the same 16 products, exact fp32
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  return c;
}

template <typename T> __device__ __forceinline__ Frag<T> frag_zero() {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.v[j] = 0;
  return f;
}
// 4 contiguous elements (p aligned to 4 elements)
template <typename T> __device__ __forceinline__ Frag<T> frag_load(const T* p) {
  Frag<T> f;
  f.v = *reinterpret_cast<const decltype(f.v)*>(p);
  return f;
}
template <typename T> __device__ __forceinline__ void frag_store(T* p, const Frag<T>& f) {
  *reinterpret_cast<decltype(Frag<T>::v)*>(p) = f.v;
}
// 4 elements `stride` apart
__device__ __forceinline__ Frag<bf16_t> frag_load_strided(const bf16_t* p, int stride) {
  Frag<bf16_t> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.v[j] = (short)p[j * stride];
  return f;
}
__device__ __forceinline__ Frag<f16_t> frag_load_strided(const f16_t* p, int stride) {
  Frag<f16_t> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.v[j] = p[j * stride];
  return f;
}
__device__ __forceinline__ Frag<float> frag_load_strided(const float* p, int stride) {
  Frag<float> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.v[j] = p[j * stride];
  return f;
}
template <typename T> __device__ __forceinline__ float frag_get(const Frag<T>& f, int j);
template <> __device__ __forceinline__ float frag_get<bf16_t>(const Frag<bf16_t>& f, int j) {
  return bf2f((bf16_t)f.v[j]);
}
template <> __device__ __forceinline__ float frag_get<f16_t>(const Frag<f16_t>& f, int j) { return (float)f.v[j]; }
template <> __device__ __forceinline__ float frag_get<float>(const Frag<float>& f, int j) { return f.v[j]; }
// 4 fp32 values rounded once to T
template <typename T> __device__ __forceinline__ Frag<T> frag_make(float a, float b, float c, float d);
template <> __device__ __forceinline__ Frag<bf16_t> frag_make<bf16_t>(float a, float b, float c, float d) {
  Frag<bf16_t> f;
  f.v[0] = (short)f2bf(a); f.v[1] = (short)f2bf(b); f.v[2] = (short)f2bf(c); f.v[3] = (short)f2bf(d);
  return f;
}
template <> __device__ __forceinline__ Frag<f16_t> frag_make<f16_t>(float a, float b, float c, float d) {
  Frag<f16_t> f;
  f.v[0] = (f16_t)a; f.v[1] = (f16_t)b; f.v[2] = (f16_t)c; f.v[3] = (f16_t)d;
  return f;
}
template <> __device__ __forceinline__ Frag<float> frag_make<float>(float a, float b, float c, float d) {
  Frag<float> f;
  f.v[0] = a; f.v[1] = b; f.v[2] = c; f.v[3] = d;
  return f;
}

// Scores (and dP) accumulate over the channel tiles in four independent accumulators (tile c into
// c & 3), added pairwise at the end: the dependent MFMA chain is a quarter as long, and so is the
// running sum each fp32 rounding scales with (a score near 700 over 256 channels is otherwise off by
// several 1e-4).  Forward and backward use the same order, so the recomputed P matches L.
__device__ __forceinline__ f32x4 sum4(const f32x4 (&a)[4]) { return (a[0] + a[1]) + (a[2] + a[3]); }

// ---- attn_linear: out[t][n] = sum_c in'[t][c] W[n][c] (+ bias[n]) (+ res[t][n]) ------------
// in' = in, or in * scale + shift per (b, c) (the GroupNorm apply, rounded to T as the stored
// activation would be).  One wave per (16 rows, 64 output channels): W rows are the A operand
// and the rows of `in` the B operand, both read as 4 contiguous elements straight from memory
// (the operands of this block are L2-resident: <= 1 MB), and a lane ends up with 4 contiguous
// output channels of one row.  n_out (optional): in' as it was multiplied, (B, T, K).
// stats (optional): per 16-row tile the (sum, sum^2) of the fp32 result before rounding,
// [B][ceil(T / 16)][N][2], reduced over the tile's rows by lane shuffles in a fixed order.
struct LinP {
  const void* in; const float* gn; const void* w; const float* bias; const void* res;
  void* out; void* n_out; float* stats;
  int T, K, N;
};

template <typename T>
__global__ void __launch_bounds__(64) attn_linear_kernel(LinP p) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int t0 = blockIdx.x * 16, n0 = blockIdx.y * 64, b = blockIdx.z;
  const int t = t0 + r;
  const bool tv = t < p.T;
  const T* in = reinterpret_cast<const T*>(p.in) + ((long long)b * p.T + (tv ? t : 0)) * p.K;
  const T* w = reinterpret_cast<const T*>(p.w);
  const float* gn = p.gn ? p.gn + (long long)b * p.K * 2 : nullptr;
  T* nout = p.n_out && blockIdx.y == 0 ? reinterpret_cast<T*>(p.n_out) + ((long long)b * p.T + t) * p.K : nullptr;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.K; k0 += 16) {
    const int kc = k0 + 4 * g;
    Frag<T> x = tv ? frag_load<T>(in + kc) : frag_zero<T>();
    if (gn) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = frag_get<T>(x, j) * gn[(kc + j) * 2] + gn[(kc + j) * 2 + 1];
      x = tv ? frag_make<T>(v[0], v[1], v[2], v[3]) : frag_zero<T>();
      if (nout && tv) frag_store<T>(nout + kc, x);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + 16 * nt + r;
      if (n0 + 16 * nt < p.N) {   // (N is a multiple of 16: whole tiles)
        const Frag<T> a = frag_load<T>(w + (long long)n * p.K + kc);
        acc[nt] = mma(a, x, acc[nt]);
      }
    }
  }
  const long long row = (long long)b * p.T + t;
  const int parts = (p.T + 15) / 16;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = n0 + 16 * nt + 4 * g;   // this lane's 4 output channels of row t
    if (n0 + 16 * nt >= p.N) continue;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = acc[nt][i] + (p.bias ? p.bias[n + i] : 0.f);
    if (p.res && tv) {
      const Frag<T> rr = frag_load<T>(reinterpret_cast<const T*>(p.res) + row * p.N + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += frag_get<T>(rr, i);
    }
    if (tv) frag_store<T>(reinterpret_cast<T*>(p.out) + row * p.N + n, frag_make<T>(v[0], v[1], v[2], v[3]));
    if (p.stats) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s1 = tv ? v[i] : 0.f, s2 = tv ? v[i] * v[i] : 0.f;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          s1 += __shfl_xor(s1, m);
          s2 += __shfl_xor(s2, m);
        }
        if (r == 0) {
          float* o = p.stats + (((long long)b * parts + blockIdx.x) * p.N + n + i) * 2;
          o[0] = s1;
          o[1] = s2;
        }
      }
    }
  }
}

// ---- attn_fwd: streaming softmax(q k^T / sqrt(ch)) v ------------------------------------------
// A workgroup of NW waves owns 16 NW queries of one (batch, head); a wave its 16.  Key / value
// blocks of KB keys go through LDS (K row-major, V transposed, zero rows past T); per 16 keys
// the wave computes S^T = K Q^T (fp32), scales it by ch^-1/2 log2(e), masks keys >= T to -inf,
// updates its lane's running max m and sum l, and adds O^T += V^T P^T with P rounded to T only
// as that MFMA's operand.  NC: compiled channel tiles (ch <= 16 NC), nc = ch / 16 the live ones.
struct AttnP {
  const void* q; const void* k; const void* v; void* o;
  long long q_rs, k_rs, v_rs, o_rs, q_bs, k_bs, v_bs, o_bs;
  float* L; float* D;
  const void* d_o; void* dq; void* dk; void* dv;
  long long do_rs, dq_rs, dk_rs, dv_rs, do_bs, dq_bs, dk_bs, dv_bs;
  int T, heads, ch;
  float scale;
};

constexpr int kFwdWaves = 2;
template <typename T> struct FwdCfg {
  static constexpr int KB = sizeof(T) == 2 ? 32 : 16;   // keys per LDS block
  static constexpr int EPV = 16 / sizeof(T);            // elements per 16-byte load
  static constexpr int PK = EPV;                        // K row pad: rows stay 16-byte aligned
  static constexpr int PV = 4;                          // V^T row pad: fragments stay aligned
};
template <typename T> size_t fwd_lds_bytes(int ch) {
  return ((size_t)FwdCfg<T>::KB * (ch + FwdCfg<T>::PK) + (size_t)ch * (FwdCfg<T>::KB + FwdCfg<T>::PV)) * sizeof(T);
}

template <typename T, int NC>
__global__ void __launch_bounds__(64 * kFwdWaves) attn_fwd_kernel(AttnP p) {
  using C = FwdCfg<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ch = p.ch, nc = ch >> 4;
  const int krow = ch + C::PK, vrow = C::KB + C::PV;
  T* Ks = reinterpret_cast<T*>(smem);
  T* Vt = Ks + C::KB * krow;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int qi = (blockIdx.x * kFwdWaves + wave) * 16 + r;
  const bool qv = qi < p.T;
  const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (long long)(qv ? qi : 0) * p.q_rs + h * ch;
  const T* kp = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * ch;
  const T* vp = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * ch;
  Frag<T> qf[NC];
  f32x4 oacc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = (c < nc && qv) ? frag_load<T>(qp + 16 * c + 4 * g) : frag_zero<T>();
    oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float m = -INFINITY, l = 0.f;
  const float sl2 = p.scale * kLog2e;
  const int cpr = ch / C::EPV;   // 16-byte chunks per row
  for (int kb0 = 0; kb0 < p.T; kb0 += C::KB) {
    __syncthreads();   // the previous block's readers are done
    for (int idx = tid; idx < C::KB * cpr; idx += 64 * kFwdWaves) {
      const int row = idx / cpr, cc = idx - row * cpr;
      const int key = kb0 + row;
      uint4 kx = uint4{0, 0, 0, 0}, vx = uint4{0, 0, 0, 0};
      if (key < p.T) {
        kx = *reinterpret_cast<const uint4*>(kp + (long long)key * p.k_rs + cc * C::EPV);
        vx = *reinterpret_cast<const uint4*>(vp + (long long)key * p.v_rs + cc * C::EPV);
      }
      *reinterpret_cast<uint4*>(Ks + row * krow + cc * C::EPV) = kx;
      const T* ve = reinterpret_cast<const T*>(&vx);
#pragma unroll
      for (int e = 0; e < C::EPV; ++e) Vt[(cc * C::EPV + e) * vrow + row] = ve[e];
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < C::KB / 16; ++sub) {
      const int key0 = kb0 + 16 * sub;
      if (key0 >= p.T) break;
      f32x4 sa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) sa[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) sa[c & 3] = mma(frag_load<T>(Ks + (16 * sub + r) * krow + 16 * c + 4 * g), qf[c], sa[c & 3]);
      f32x4 s = sum4(sa);
      // s[i] = score of (key key0 + 4 g + i, this lane's query)
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = key0 + 4 * g + i < p.T ? s[i] * sl2 : -INFINITY;
        mx = fmaxf(mx, s[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);   // finite: key0 < T is a live key of every lane's column
      const float alpha = exp2f(m - mn);
      float pr[4], ps = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        pr[i] = exp2f(s[i] - mn);
        ps += pr[i];
      }
      ps += __shfl_xor(ps, 16);
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = mn;
      const Frag<T> pf = frag_make<T>(pr[0], pr[1], pr[2], pr[3]);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) {
#pragma unroll
          for (int i = 0; i < 4; ++i) oacc[c][i] *= alpha;
          oacc[c] = mma(frag_load<T>(Vt + (16 * c + r) * vrow + 16 * sub + 4 * g), pf, oacc[c]);
        }
    }
  }
  if (!qv) return;
  const float inv = 1.f / l;
  T* op = reinterpret_cast<T*>(p.o) + b * p.o_bs + (long long)qi * p.o_rs + h * ch;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc)
      frag_store<T>(op + 16 * c + 4 * g,
                    frag_make<T>(oacc[c][0] * inv, oacc[c][1] * inv, oacc[c][2] * inv, oacc[c][3] * inv));
  if (p.L && g == 0) p.L[((long long)b * p.heads + h) * p.T + qi] = (m + log2f(l)) * kLn2;
}

// ---- backward --------------------------------------------------------------------------------
// D[b][h][t] = sum_c dO[t][c] O[t][c]
template <typename T>
__global__ void __launch_bounds__(256) attn_rowdot_kernel(AttnP p, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % p.T);
  const long long bh = i / p.T;
  const int h = (int)(bh % p.heads);
  const long long b = bh / p.heads;
  const T* o = reinterpret_cast<const T*>(p.o) + b * p.o_bs + (long long)t * p.o_rs + h * p.ch;
  const T* d = reinterpret_cast<const T*>(p.d_o) + b * p.do_bs + (long long)t * p.do_rs + h * p.ch;
  float s = 0.f;
  for (int c = 0; c < p.ch; c += 4) {
    const Frag<T> a = frag_load<T>(o + c), e = frag_load<T>(d + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += frag_get<T>(a, j) * frag_get<T>(e, j);
  }
  p.D[i] = s;
}

// a 16-row tile [16][ch] of a (rows, row stride) matrix into LDS (rows >= T zero), one wave
template <typename T>
__device__ __forceinline__ void stage_tile(T* dst, int drow, const T* src, long long rs, int row0, int T_, int ch,
                                           int lane) {
  constexpr int EPV = 16 / sizeof(T);
  const int cpr = ch / EPV;
  for (int idx = lane; idx < 16 * cpr; idx += 64) {
    const int row = idx / cpr, cc = idx - row * cpr;
    uint4 x = uint4{0, 0, 0, 0};
    if (row0 + row < T_) x = *reinterpret_cast<const uint4*>(src + (long long)(row0 + row) * rs + cc * EPV);
    *reinterpret_cast<uint4*>(dst + row * drow + cc * EPV) = x;
  }
}

// One wave per 16-key tile of a (batch, head): walks the query tiles, recomputes
// P = exp(s - L) from q, k and L, and accumulates dV^T += dO^T P, dK^T += Q^T dS with
// dS = P o (dO V^T - D).  The query tile's Q and dO rows sit in LDS: read row-wise for the
// scores, column-wise (4 rows of one channel) as the A operand of the two accumulations.
template <typename T, int NC>
__global__ void __launch_bounds__(64) attn_bwd_kv_kernel(AttnP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int EPV = 16 / sizeof(T);
  const int ch = p.ch, nc = ch >> 4, srow = ch + EPV;
  T* Qs = reinterpret_cast<T*>(smem);
  T* Os = Qs + 16 * srow;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int key = blockIdx.x * 16 + r;
  const bool kv = key < p.T;
  const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + h * ch;
  const T* dop = reinterpret_cast<const T*>(p.d_o) + b * p.do_bs + h * ch;
  const T* kp = reinterpret_cast<const T*>(p.k) + b * p.k_bs + (long long)(kv ? key : 0) * p.k_rs + h * ch;
  const T* vp = reinterpret_cast<const T*>(p.v) + b * p.v_bs + (long long)(kv ? key : 0) * p.v_rs + h * ch;
  const float* Lp = p.L + ((long long)b * p.heads + h) * p.T;
  const float* Dp = p.D + ((long long)b * p.heads + h) * p.T;
  Frag<T> kf[NC], vf[NC];
  f32x4 dva[NC], dka[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    kf[c] = (c < nc && kv) ? frag_load<T>(kp + 16 * c + 4 * g) : frag_zero<T>();
    vf[c] = (c < nc && kv) ? frag_load<T>(vp + 16 * c + 4 * g) : frag_zero<T>();
    dva[c] = dka[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = p.scale * kLog2e;
  for (int q0 = 0; q0 < p.T; q0 += 16) {
    __syncthreads();
    stage_tile<T>(Qs, srow, qp, p.q_rs, q0, p.T, ch, lane);
    stage_tile<T>(Os, srow, dop, p.do_rs, q0, p.T, ch, lane);
    __syncthreads();
    f32x4 sa[4], da[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = da[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        sa[c & 3] = mma(frag_load<T>(Qs + r * srow + 16 * c + 4 * g), kf[c], sa[c & 3]);    // [query 4 g + i][key r]
        da[c & 3] = mma(frag_load<T>(Os + r * srow + 16 * c + 4 * g), vf[c], da[c & 3]);
      }
    const f32x4 s = sum4(sa), dp = sum4(da);
    float pr[4], ds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qi = q0 + 4 * g + i;
      const bool ok = kv && qi < p.T;
      const float Lq = ok ? Lp[qi] : 0.f, Dq = ok ? Dp[qi] : 0.f;
      pr[i] = ok ? exp2f(s[i] * sl2 - Lq * kLog2e) : 0.f;
      ds[i] = pr[i] * (dp[i] - Dq);
    }
    const Frag<T> pf = frag_make<T>(pr[0], pr[1], pr[2], pr[3]);
    const Frag<T> df = frag_make<T>(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        dva[c] = mma(frag_load_strided(Os + (4 * g) * srow + 16 * c + r, srow), pf, dva[c]);   // [ch 4 g + i][key r]
        dka[c] = mma(frag_load_strided(Qs + (4 * g) * srow + 16 * c + r, srow), df, dka[c]);
      }
  }
  if (!kv) return;
  T* dvp = reinterpret_cast<T*>(p.dv) + b * p.dv_bs + (long long)key * p.dv_rs + h * ch;
  T* dkp = reinterpret_cast<T*>(p.dk) + b * p.dk_bs + (long long)key * p.dk_rs + h * ch;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc) {
      frag_store<T>(dvp + 16 * c + 4 * g, frag_make<T>(dva[c][0], dva[c][1], dva[c][2], dva[c][3]));
      frag_store<T>(dkp + 16 * c + 4 * g, frag_make<T>(dka[c][0] * p.scale, dka[c][1] * p.scale, dka[c][2] * p.scale,
                                                        dka[c][3] * p.scale));
    }
}

// One wave per 16-query tile: walks the key tiles (K and V rows through LDS), recomputes
// P^T and dS^T = P^T o (V dO^T - D), and accumulates dQ^T += K^T dS^T.
template <typename T, int NC>
__global__ void __launch_bounds__(64) attn_bwd_q_kernel(AttnP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int EPV = 16 / sizeof(T);
  const int ch = p.ch, nc = ch >> 4, srow = ch + EPV;
  T* Ks = reinterpret_cast<T*>(smem);
  T* Vs = Ks + 16 * srow;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int qi = blockIdx.x * 16 + r;
  const bool qv = qi < p.T;
  const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (long long)(qv ? qi : 0) * p.q_rs + h * ch;
  const T* dop = reinterpret_cast<const T*>(p.d_o) + b * p.do_bs + (long long)(qv ? qi : 0) * p.do_rs + h * ch;
  const T* kp = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * ch;
  const T* vp = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * ch;
  const long long bh = ((long long)b * p.heads + h) * p.T;
  const float Lq = qv ? p.L[bh + qi] * kLog2e : 0.f, Dq = qv ? p.D[bh + qi] : 0.f;
  Frag<T> qf[NC], dof[NC];
  f32x4 dqa[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = (c < nc && qv) ? frag_load<T>(qp + 16 * c + 4 * g) : frag_zero<T>();
    dof[c] = (c < nc && qv) ? frag_load<T>(dop + 16 * c + 4 * g) : frag_zero<T>();
    dqa[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = p.scale * kLog2e;
  for (int k0 = 0; k0 < p.T; k0 += 16) {
    __syncthreads();
    stage_tile<T>(Ks, srow, kp, p.k_rs, k0, p.T, ch, lane);
    stage_tile<T>(Vs, srow, vp, p.v_rs, k0, p.T, ch, lane);
    __syncthreads();
    f32x4 sa[4], da[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sa[i] = da[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        sa[c & 3] = mma(frag_load<T>(Ks + r * srow + 16 * c + 4 * g), qf[c], sa[c & 3]);     // [key 4 g + i][query r]
        da[c & 3] = mma(frag_load<T>(Vs + r * srow + 16 * c + 4 * g), dof[c], da[c & 3]);
      }
    const f32x4 s = sum4(sa), dp = sum4(da);
    float ds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = qv && k0 + 4 * g + i < p.T;
      const float pr = ok ? exp2f(s[i] * sl2 - Lq) : 0.f;
      ds[i] = pr * (dp[i] - Dq);
    }
    const Frag<T> df = frag_make<T>(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) dqa[c] = mma(frag_load_strided(Ks + (4 * g) * srow + 16 * c + r, srow), df, dqa[c]);
  }
  if (!qv) return;
  T* dqp = reinterpret_cast<T*>(p.dq) + b * p.dq_bs + (long long)qi * p.dq_rs + h * ch;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc)
      frag_store<T>(dqp + 16 * c + 4 * g, frag_make<T>(dqa[c][0] * p.scale, dqa[c][1] * p.scale, dqa[c][2] * p.scale,
                                                        dqa[c][3] * p.scale));
}

// ---- GroupNorm without activation, backward ---------------------------------------------------
// n = (x - mean) rstd gamma + beta.  One workgroup per (batch, group): thread (ts, cl) sums
// dn and dn xhat of channel cl over the rows ts, ts + nts, ...; the per-thread sums are added
// per channel in ts order, the group's two means in channel order; then
// dx = rstd (gamma dn - mean(gamma dn) - xhat mean(gamma dn xhat)) (+ add) (+ dx).
// part [B][C][2]: the per-(batch, channel) sums (dn, dn xhat) for gn_affine_sum_kernel.
template <typename T>
__global__ void __launch_bounds__(256) gn_lin_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dn,
                                                         const float* __restrict__ mr, const float* __restrict__ gamma,
                                                         const T* __restrict__ add, T* __restrict__ dx, int acc,
                                                         float* __restrict__ part, int Tn, int C, int groups) {
  __shared__ float red[256][2];
  __shared__ float chs[256][2];
  const int grp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int cg = C / groups, nts = 256 / cg;
  const bool live = tid < nts * cg;
  const int cl = tid % cg, ts = tid / cg;
  const int c = grp * cg + cl;
  const float mean = mr[((long long)b * groups + grp) * 2], rstd = mr[((long long)b * groups + grp) * 2 + 1];
  const long long base = (long long)b * Tn * C + c;
  float s1 = 0.f, s2 = 0.f;
  if (live)
    for (int t = ts; t < Tn; t += nts) {
      const float d = Elem<T>::to_f(dn[base + (long long)t * C]);
      const float xh = (Elem<T>::to_f(x[base + (long long)t * C]) - mean) * rstd;
      s1 += d;
      s2 += d * xh;
    }
  red[tid][0] = s1;
  red[tid][1] = s2;
  __syncthreads();
  if (tid < cg) {
    float a1 = 0.f, a2 = 0.f;
    for (int k = 0; k < nts; ++k) {
      a1 += red[k * cg + tid][0];
      a2 += red[k * cg + tid][1];
    }
    part[((long long)b * C + c) * 2] = a1;
    part[((long long)b * C + c) * 2 + 1] = a2;
    chs[tid][0] = gamma[c] * a1;
    chs[tid][1] = gamma[c] * a2;
  }
  __syncthreads();
  float g1 = 0.f, g2 = 0.f;
  for (int k = 0; k < cg; ++k) {
    g1 += chs[k][0];
    g2 += chs[k][1];
  }
  const float invn = 1.f / ((float)cg * (float)Tn);
  g1 *= invn;
  g2 *= invn;
  if (!live) return;
  const float gm = gamma[c];
  for (int t = ts; t < Tn; t += nts) {
    const long long i = base + (long long)t * C;
    const float xh = (Elem<T>::to_f(x[i]) - mean) * rstd;
    float v = rstd * (gm * Elem<T>::to_f(dn[i]) - g1 - xh * g2);
    if (add) v += Elem<T>::to_f(add[i]);
    if (acc) v += Elem<T>::to_f(dx[i]);
    dx[i] = Elem<T>::from_f(v);
  }
}

// dgamma[c] += sum_b part[b][c][1], dbeta[c] += sum_b part[b][c][0] (batch order)
__global__ void gn_affine_sum_kernel(const float* __restrict__ part, int B, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, g = 0.f;
  for (int b = 0; b < B; ++b) {
    a += part[((long long)b * C + c) * 2];
    g += part[((long long)b * C + c) * 2 + 1];
  }
  dbeta[c] += a;
  dgamma[c] += g;
}

// ---- weight layouts ---------------------------------------------------------------------------
// The kernels see the projection rows as [Q of all heads | K of all | V of all].  Legacy order
// (use_new_attention_order=False) keeps head i's rows as [q_i | k_i | v_i]: packed row
// s C + i ch + j <- source row i 3 ch + s ch + j.
__device__ __host__ inline int legacy_row(int rp, int heads, int ch) {
  const int C = heads * ch;
  const int s = rp / C, i = (rp - s * C) / ch, j = rp % ch;
  return i * 3 * ch + s * ch + j;
}
// dst (T): [rows][cols], or transposed [cols][rows]; rows read through the legacy permutation if asked
template <typename T>
__global__ void attn_pack_kernel(const float* __restrict__ src, T* __restrict__ dst, int rows, int cols, int heads,
                                 int ch, int legacy, int transpose) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  const int rp = (int)(i / cols), c = (int)(i % cols);
  const int rs = legacy ? legacy_row(rp, heads, ch) : rp;
  const float v = src[(long long)rs * cols + c];
  dst[transpose ? (long long)c * rows + rp : i] = Elem<T>::from_f(v);
}
// the adjoint for the gradients: dst[source row][c] += src[packed row][c]
__global__ void attn_unperm_add_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols,
                                       int heads, int ch) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  const int rp = (int)(i / cols), c = (int)(i % cols);
  dst[(long long)legacy_row(rp, heads, ch) * cols + c] += src[i];
}

int check_desc(const cwdm_attention_desc* d, const char* who) {
  const std::string w(who);
  CWDM_REQUIRE(d, CWDM_E_INVALID, w + ": null desc");
  CWDM_REQUIRE(dtype_compute(d->dtype), CWDM_E_INVALID, w + ": bad dtype");
  CWDM_REQUIRE(d->B >= 1 && d->T >= 1 && d->heads >= 1, CWDM_E_SHAPE, w + ": B, T and heads must be >= 1");
  CWDM_REQUIRE(d->ch >= 16 && d->ch <= 256 && d->ch % 16 == 0, CWDM_E_UNSUPPORTED,
               w + ": head channels must be a multiple of 16 in [16, 256], got " + std::to_string(d->ch));
  CWDM_REQUIRE(d->T < (1LL << 24) && d->B < 65536 && d->heads < 65536, CWDM_E_UNSUPPORTED, w + ": shape too large");
  CWDM_REQUIRE(d->q && d->k && d->v && d->o, CWDM_E_INVALID, w + ": null q / k / v / o");
  const int epv = 16 / dtype_size(d->dtype);
  const int64_t need = (int64_t)d->heads * d->ch;
  for (const int64_t rs : {d->q_rs, d->k_rs, d->v_rs, d->o_rs})
    CWDM_REQUIRE(rs >= need && rs % epv == 0, CWDM_E_SHAPE,
                 w + ": a row stride must cover heads * ch and keep rows 16-byte aligned");
  for (const void* ptr : {d->q, d->k, d->v, (const void*)d->o})
    CWDM_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 16 == 0, CWDM_E_INVALID, w + ": pointers must be 16-byte aligned");
  if (d->B > 1) {
    // every batch starts 16-byte aligned; an input may repeat (stride 0), an output's batches may not overlap
    for (const int64_t bs : {d->q_bs, d->k_bs, d->v_bs})
      CWDM_REQUIRE(bs >= 0 && bs % epv == 0, CWDM_E_SHAPE,
                   w + ": a batch stride must be non-negative and keep batches 16-byte aligned");
    CWDM_REQUIRE(d->o_bs % epv == 0 && d->o_bs >= (d->T - 1) * d->o_rs + need, CWDM_E_SHAPE,
                 w + ": the output batch stride must cover a batch's rows and keep batches 16-byte aligned");
  }
  return CWDM_OK;
}

AttnP make_params(const cwdm_attention_desc* d) {
  AttnP p{};
  p.q = d->q; p.k = d->k; p.v = d->v; p.o = d->o;
  p.q_rs = d->q_rs; p.k_rs = d->k_rs; p.v_rs = d->v_rs; p.o_rs = d->o_rs;
  p.q_bs = d->q_bs; p.k_bs = d->k_bs; p.v_bs = d->v_bs; p.o_bs = d->o_bs;
  p.L = d->L; p.D = d->D;
  p.d_o = d->d_o; p.dq = d->dq; p.dk = d->dk; p.dv = d->dv;
  p.do_rs = d->do_rs; p.dq_rs = d->dq_rs; p.dk_rs = d->dk_rs; p.dv_rs = d->dv_rs;
  p.do_bs = d->do_bs; p.dq_bs = d->dq_bs; p.dk_bs = d->dk_bs; p.dv_bs = d->dv_bs;
  p.T = (int)d->T; p.heads = d->heads; p.ch = d->ch;
  p.scale = 1.f / std::sqrt((float)d->ch);
  return p;
}

template <typename T, int NC>
int launch_fwd(const AttnP& p, int B, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(p.T, 16 * kFwdWaves), (unsigned)p.heads, (unsigned)B);
  hipLaunchKernelGGL((attn_fwd_kernel<T, NC>), grid, dim3(64 * kFwdWaves), fwd_lds_bytes<T>(p.ch), s, p);
  CWDM_LAUNCHED();
  return CWDM_OK;
}
template <typename T, int NC>
int launch_bwd(const AttnP& p, int B, hipStream_t s) {
  const long long total = (long long)B * p.heads * p.T;
  hipLaunchKernelGGL((attn_rowdot_kernel<T>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, p, total);
  CWDM_LAUNCHED();
  const dim3 grid((unsigned)ceil_div(p.T, 16), (unsigned)p.heads, (unsigned)B);
  const size_t lds = (size_t)2 * 16 * (p.ch + 16 / sizeof(T)) * sizeof(T);
  hipLaunchKernelGGL((attn_bwd_kv_kernel<T, NC>), grid, dim3(64), lds, s, p);
  CWDM_LAUNCHED();
  hipLaunchKernelGGL((attn_bwd_q_kernel<T, NC>), grid, dim3(64), lds, s, p);
  CWDM_LAUNCHED();
  return CWDM_OK;
}

}  // namespace

int64_t attn_parts(int64_t T) { return ceil_div(T, 16); }

int attn_linear(int dtype, int64_t B, int64_t T, int K, int N, const void* in, const float* gn, const void* w,
                const float* bias, const void* res, void* out, void* n_out, float* stats, hipStream_t s) {
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, "cwdm_attn_linear: bad dtype");
  CWDM_REQUIRE(in && w && out, CWDM_E_INVALID, "cwdm_attn_linear: null pointer");
  CWDM_REQUIRE(B >= 1 && B < 65536 && T >= 1 && T < (1LL << 24), CWDM_E_SHAPE, "cwdm_attn_linear: bad B / T");
  CWDM_REQUIRE(K >= 16 && K % 16 == 0 && N >= 16 && N % 16 == 0, CWDM_E_UNSUPPORTED,
               "cwdm_attn_linear: K and N must be multiples of 16");
  CWDM_REQUIRE(!n_out || gn, CWDM_E_INVALID, "cwdm_attn_linear: n_out needs the GroupNorm scale / shift");
  LinP p{in, gn, w, bias, res, out, n_out, stats, (int)T, K, N};
  const dim3 grid((unsigned)ceil_div(T, 16), (unsigned)ceil_div(N, 64), (unsigned)B);
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using E = decltype(tag);
    hipLaunchKernelGGL((attn_linear_kernel<E>), grid, dim3(64), 0, s, p);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}

int attn_pack(const float* w, int rows, int cols, int heads, int ch, int legacy, int transpose, int dtype, void* out,
              hipStream_t s) {
  CWDM_REQUIRE(w && out && rows > 0 && cols > 0, CWDM_E_INVALID, "cwdm_attn_pack: bad argument");
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, "cwdm_attn_pack: bad dtype");
  CWDM_REQUIRE(!legacy || (heads > 0 && ch > 0 && rows == 3 * heads * ch), CWDM_E_SHAPE,
               "cwdm_attn_pack: the legacy order permutes 3 * heads * ch rows");
  const long long n = (long long)rows * cols;
  const dim3 grid((unsigned)ceil_div(n, 256));
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using E = decltype(tag);
    hipLaunchKernelGGL((attn_pack_kernel<E>), grid, dim3(256), 0, s, w, reinterpret_cast<E*>(out), rows, cols, heads,
                       ch, legacy, transpose);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}

int attn_unperm_add(const float* src, float* dst, int rows, int cols, int heads, int ch, hipStream_t s) {
  const long long n = (long long)rows * cols;
  hipLaunchKernelGGL(attn_unperm_add_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, src, dst, rows, cols,
                     heads, ch);
  CWDM_LAUNCHED();
  return CWDM_OK;
}

int gn_lin_bwd(int dtype, int64_t B, int64_t T, int C, int groups, const void* x, const void* dn, const float* mr,
               const float* gamma, const void* add, void* dx, int acc, float* part, float* dgamma, float* dbeta,
               hipStream_t s) {
  CWDM_REQUIRE(groups > 0 && C % groups == 0 && C / groups <= 256, CWDM_E_UNSUPPORTED,
               "gn_lin_bwd: at most 256 channels per group");
  const dim3 grid((unsigned)groups, (unsigned)B);
  const int rc = dispatch_dtype(dtype, [&](auto tag) -> int {
    using E = decltype(tag);
    hipLaunchKernelGGL((gn_lin_bwd_kernel<E>), grid, dim3(256), 0, s, reinterpret_cast<const E*>(x),
                       reinterpret_cast<const E*>(dn), mr, gamma, reinterpret_cast<const E*>(add),
                       reinterpret_cast<E*>(dx), acc, part, (int)T, C, groups);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(gn_affine_sum_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, s, part, (int)B, C, dgamma,
                     dbeta);
  CWDM_LAUNCHED();
  return CWDM_OK;
}

}  // namespace cwdm

using namespace cwdm;

extern "C" int cwdm_attention_forward(const cwdm_attention_desc* d, cwdm_stream_t stream) {
  if (int rc = check_desc(d, "cwdm_attention_forward")) return rc;
  const AttnP p = make_params(d);
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(d->dtype, [&](auto tag) -> int {
    using E = decltype(tag);
    return d->ch <= 64    ? launch_fwd<E, 4>(p, (int)d->B, s)
           : d->ch <= 128 ? launch_fwd<E, 8>(p, (int)d->B, s)
                          : launch_fwd<E, 16>(p, (int)d->B, s);
  });
}

extern "C" int cwdm_attention_backward(const cwdm_attention_desc* d, cwdm_stream_t stream) {
  if (int rc = check_desc(d, "cwdm_attention_backward")) return rc;
  CWDM_REQUIRE(d->L && d->D && d->d_o && d->dq && d->dk && d->dv, CWDM_E_INVALID,
               "cwdm_attention_backward: null L / D / d_o / dq / dk / dv");
  const int epv = 16 / dtype_size(d->dtype);
  const int64_t need = (int64_t)d->heads * d->ch;
  for (const int64_t rs : {d->do_rs, d->dq_rs, d->dk_rs, d->dv_rs})
    CWDM_REQUIRE(rs >= need && rs % epv == 0, CWDM_E_SHAPE,
                 "cwdm_attention_backward: a row stride must cover heads * ch and keep rows 16-byte aligned");
  for (const void* ptr : {d->d_o, (const void*)d->dq, (const void*)d->dk, (const void*)d->dv})
    CWDM_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 16 == 0, CWDM_E_INVALID,
                 "cwdm_attention_backward: pointers must be 16-byte aligned");
  if (d->B > 1) {
    CWDM_REQUIRE(d->do_bs >= 0 && d->do_bs % epv == 0, CWDM_E_SHAPE,
                 "cwdm_attention_backward: the d_o batch stride must be non-negative and keep batches 16-byte aligned");
    const int64_t obs[3] = {d->dq_bs, d->dk_bs, d->dv_bs}, ors[3] = {d->dq_rs, d->dk_rs, d->dv_rs};
    for (int i = 0; i < 3; ++i)
      CWDM_REQUIRE(obs[i] % epv == 0 && obs[i] >= (d->T - 1) * ors[i] + need, CWDM_E_SHAPE,
                   "cwdm_attention_backward: a gradient's batch stride must cover a batch's rows and keep batches "
                   "16-byte aligned");
  }
  const AttnP p = make_params(d);
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(d->dtype, [&](auto tag) -> int {
    using E = decltype(tag);
    return d->ch <= 64    ? launch_bwd<E, 4>(p, (int)d->B, s)
           : d->ch <= 128 ? launch_bwd<E, 8>(p, (int)d->B, s)
                          : launch_bwd<E, 16>(p, (int)d->B, s);
  });
}

extern "C" int64_t cwdm_attn_parts(int64_t T) { return T > 0 ? attn_parts(T) : -1; }

extern "C" int cwdm_attn_linear(const cwdm_attn_linear_desc* d, cwdm_stream_t stream) {
  CWDM_REQUIRE(d, CWDM_E_INVALID, "cwdm_attn_linear: null desc");
  return attn_linear(d->dtype, d->B, d->T, d->K, d->N, d->in, d->gn, d->w, d->bias, d->res, d->out, d->n_out, d->stats,
                     (hipStream_t)stream);
}

extern "C" int cwdm_attn_pack(const float* w, int rows, int cols, int heads, int ch, int legacy, int transpose,
                              int dtype, void* out, cwdm_stream_t stream) {
  return attn_pack(w, rows, cols, heads, ch, legacy, transpose, dtype, out, (hipStream_t)stream);
}
