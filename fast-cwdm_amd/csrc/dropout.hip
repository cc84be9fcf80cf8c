// Dropout of a ResBlock's out_layers (guided_diffusion/unet.py ResBlock: nn.Dropout(p) between
// out_layers' SiLU and its conv), training only.  The keep mask is never stored: forward and backward
// regenerate it from the Philox4x32-10 block function of the sampler (sampler.hpp),
//   blk  = philox4x32_10(ctr = (v lo, v hi, site, b << 16 | c >> 2), key = (seed lo, seed hi))
//   keep = (blk[c & 3] >> 8) >= thr,   thr = floor(p 2^24)
// with v the voxel index inside batch entry b (NDHWC order), c the channel and site the ResBlock's
// ordinal in the plan: one block per 4 channels.  The mask depends on neither the dtype, the values
// nor the batch size.
//   * cwdm_gn_silu_dropout: u = keep ? SiLU(x scale + shift) / (1 - p) : 0, channels-last, one rounding
//   * cwdm_dropout_bwd:     du = keep ? du / (1 - p) : 0, in place (a select, so a dropped Inf / NaN is 0)
// Both stream like cwdm_gn_apply: a thread handles one 8-channel group of VPT voxels a quarter of the
// tensor apart, 16-byte loads and stores, 32-bit item indices (host-checked).
#include "conv3d_kernels.hpp"
#include "sampler.hpp"

namespace cwdm {
namespace {

struct DropArgs {
  unsigned thr;      // floor(p 2^24): a 24-bit draw below it drops
  float inv;         // 1 / (1 - p)
  unsigned k0, k1;   // the seed's halves
  unsigned site;
};

// keep bits of channels c .. c + 7 (bit e = channel c + e) of voxel v in batch entry b: two Philox blocks.
// (v < 2^31 here, so the counter's high voxel word is 0)
__device__ __forceinline__ unsigned drop_keep8(const DropArgs& a, unsigned v, unsigned b, int c) {
  unsigned m = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned ctr[4] = {v, 0u, a.site, (b << 16) | (unsigned)((c >> 2) + h)};
    philox4x32_10(ctr, a.k0, a.k1);
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= ((ctr[e] >> 8) >= a.thr ? 1u : 0u) << (4 * h + e);
  }
  return m;
}

// FWD: out = dropout(SiLU(x sc + sh)); else out = dropout-backward of x (out may be x)
template <typename T, int VPT, bool FWD>
__global__ void __launch_bounds__(256) dropout_kernel(const T* x, const float* __restrict__ gn, T* out, int C,
                                                      FastDiv dvpb, FastDiv dg8, unsigned nvox, unsigned nq,
                                                      DropArgs a) {
  const unsigned i0 = blockIdx.x * 256u + threadIdx.x;   // (voxel slot, group)
  const unsigned vq = fdiv(i0, dg8);                     // voxels vq, vq + nq, ...
  if (vq >= nq) return;
  const int c = (int)(i0 - vq * dg8.d) * 8;
  float xv[VPT][8];
  unsigned vs[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const unsigned v = vq + k * nq < nvox ? vq + k * nq : nvox - 1;
    vs[k] = v;
    const T* src = x + (size_t)v * C + c;
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
    if constexpr (FWD) {
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
    }
    const unsigned keep = drop_keep8(a, v - b * dvpb.d, b, c);
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = FWD ? silu_aff(xv[k][e], sc[e], sh[e]) : xv[k][e];
      y[e] = (keep >> e) & 1u ? f * a.inv : 0.0f;
    }
    T* dst = out + (size_t)v * C + c;
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<u32x4*>(dst) = pack<T>(y);
    } else {
      *reinterpret_cast<u32x4*>(dst) = pack<float>(y);
      *reinterpret_cast<u32x4*>(dst + 4) = pack<float>(y + 4);
    }
  }
}

template <bool FWD>
int dropout_launch(const char* who, const void* x, const float* ss, void* out, int dtype, int64_t B, int64_t V, int C,
                   double p, uint64_t seed, int site, hipStream_t s) {
  const std::string w(who);
  CWDM_REQUIRE(x && out && (!FWD || ss), CWDM_E_INVALID, w + ": null pointer");
  CWDM_REQUIRE(dtype_compute(dtype), CWDM_E_INVALID, w + ": bad dtype");
  CWDM_REQUIRE(p >= 0.0 && p < 1.0, CWDM_E_INVALID, w + ": the drop probability must lie in [0, 1)");
  CWDM_REQUIRE(B > 0 && V > 0 && C > 0 && site >= 0, CWDM_E_SHAPE, w + ": bad shape");
  // the counter's last word holds b << 16 | c >> 2; a thread's 8 channels are one or two 16-byte accesses
  CWDM_REQUIRE(B < 65536 && C % 8 == 0 && C < (1 << 18), CWDM_E_UNSUPPORTED,
               w + ": needs a batch below 65536 and channels a multiple of 8 (below 2^18)");
  CWDM_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0, CWDM_E_INVALID, w + ": tensors must be 16-byte aligned");
  constexpr int VPT = 4;
  const int G8 = C / 8;
  CWDM_REQUIRE(B * V * G8 < (1LL << 31) - 256 * VPT, CWDM_E_UNSUPPORTED,
               w + ": more than 2^31 channel groups in one launch");
  const int64_t nvox = B * V, nq = ceil_div(nvox, VPT);
  const dim3 grid((unsigned)ceil_div(nq * G8, 256));
  const FastDiv dvpb = make_fastdiv((unsigned)V), dg8 = make_fastdiv((unsigned)G8);
  DropArgs a;
  a.thr = (unsigned)(p * 16777216.0);   // floor: p >= 0
  a.inv = 1.0f / (1.0f - (float)p);
  a.k0 = (unsigned)(seed & 0xffffffffu);
  a.k1 = (unsigned)(seed >> 32);
  a.site = (unsigned)site;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((dropout_kernel<T, VPT, FWD>), grid, dim3(256), 0, s, reinterpret_cast<const T*>(x), ss,
                       reinterpret_cast<T*>(out), C, dvpb, dg8, (unsigned)nvox, (unsigned)nq, a);
    CWDM_LAUNCHED();
    return CWDM_OK;
  });
}

}  // namespace
}  // namespace cwdm

using namespace cwdm;

extern "C" int cwdm_gn_silu_dropout(const void* x, const float* scale_shift, void* out, int dtype, int64_t B,
                                    int64_t V, int C, double p, uint64_t seed, int site, cwdm_stream_t stream) {
  return dropout_launch<true>("cwdm_gn_silu_dropout", x, scale_shift, out, dtype, B, V, C, p, seed, site,
                              (hipStream_t)stream);
}

extern "C" int cwdm_dropout_bwd(void* du, int dtype, int64_t B, int64_t V, int C, double p, uint64_t seed, int site,
                                cwdm_stream_t stream) {
  return dropout_launch<false>("cwdm_dropout_bwd", du, nullptr, du, dtype, B, V, C, p, seed, site,
                               (hipStream_t)stream);
}
