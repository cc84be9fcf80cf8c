// Timestep path: sinusoidal embedding -> time_embed MLP
// (guided_diffusion/nn.py:103-121, guided_diffusion/unet.py:534-539, :770) and the
// per-ResBlock emb projections SiLU -> Linear (unet.py:248-254, :295-308) for
// all blocks in one GEMV over the packed, concatenated weights.  The conv1 bias
// of each block is folded into the projection bias, so conv1's epilogue adds a
// single per-(b, c) vector.
#include "internal.hpp"

namespace cwdm {
namespace {

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

// one workgroup per batch element.  label_w (null: no class conditioning) is label_emb.weight
// [num_classes][E] and y int64[B]: the result is time_embed(t) + label_emb[y] (unet.py:763-774), one fp32
// add on the fp32 result of the second Linear.  A label outside [0, num_classes) never indexes the table:
// nothing is added for that sample and CWDM_DEV_E_LABEL is raised in the device error word (err).
__global__ void __launch_bounds__(256) time_embed_kernel(const float* __restrict__ t, int mc,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        float* __restrict__ temb,
                                                        const float* __restrict__ label_w,
                                                        const long long* __restrict__ y, int num_classes,
                                                        unsigned* __restrict__ err) {
  extern __shared__ float sm[];
  const int E = 4 * mc, half = mc / 2;
  float* sin_emb = sm;       // [mc]
  float* hid = sm + mc;      // [E]
  const int b = blockIdx.x;
  const float tv = t[b];
  for (int k = threadIdx.x; k < half; k += blockDim.x) {
    // th.exp(-math.log(10000) * arange(half) / half) in fp32
    const float fr = expf(__fdiv_rn(__fmul_rn(-9.210340371976184f, (float)k), (float)half));
    const float a = __fmul_rn(tv, fr);
    sin_emb[k] = cosf(a);
    sin_emb[k + half] = sinf(a);
  }
  if ((mc & 1) && threadIdx.x == 0) sin_emb[mc - 1] = 0.f;
  __syncthreads();
  for (int o = threadIdx.x; o < E; o += blockDim.x) {
    float acc = b1[o];
    const float* wr = w1 + (long long)o * mc;
    for (int i = 0; i < mc; ++i) acc += wr[i] * sin_emb[i];
    hid[o] = silu_f(acc);
  }
  __syncthreads();
  const float* lrow = nullptr;
  if (label_w) {
    const long long c = y[b];
    if (c >= 0 && c < num_classes) lrow = label_w + c * E;
    else if (threadIdx.x == 0)
      __hip_atomic_fetch_or(err, (unsigned)CWDM_DEV_E_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int o = threadIdx.x; o < E; o += blockDim.x) {
    float acc = b2[o];
    const float* wr = w2 + (long long)o * E;
    for (int i = 0; i < E; ++i) acc += wr[i] * hid[i];
    temb[(long long)b * E + o] = lrow ? acc + lrow[o] : acc;
  }
}

// out[b][r] = bias[r] + W[r, :] . SiLU(temb[b, :]); one wave per row.
__global__ void __launch_bounds__(256) emb_proj_kernel(const float* __restrict__ temb, int E,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      int R, float* __restrict__ out) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv, b = blockIdx.y;
  if (r >= R) return;
  const float* te = temb + (long long)b * E;
  const float* wr = W + (long long)r * E;
  float acc = 0.f;
  for (int i = lane; i < E; i += 64) acc += wr[i] * silu_f(te[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[(long long)b * R + r] = acc + bias[r];
}

}  // namespace

int launch_time_embed(const float* t, int B, int mc, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* temb, const float* label_w, const int64_t* y, int num_classes,
                      hipStream_t s) {
  const size_t sm = (size_t)(mc + 4 * mc) * sizeof(float);
  unsigned* err = nullptr;
  if (label_w) {
    CWDM_REQUIRE(y && num_classes > 0, CWDM_E_INVALID, "time_embed: a label table needs labels");
    if (int rc = dev_err_word(&err)) return rc;
  }
  hipLaunchKernelGGL(time_embed_kernel, dim3(B), dim3(256), sm, s, t, mc, w1, b1, w2, b2, temb, label_w,
                     reinterpret_cast<const long long*>(y), num_classes, err);
  CWDM_LAUNCHED();
  return CWDM_OK;
}

int launch_emb_proj(const float* temb, int B, int E, const float* W, const float* bias, int R, float* out,
                    hipStream_t s) {
  hipLaunchKernelGGL(emb_proj_kernel, dim3((unsigned)ceil_div(R, 4), B), dim3(256), 0, s, temb, E, W, bias, R, out);
  CWDM_LAUNCHED();
  return CWDM_OK;
}

}  // namespace cwdm
