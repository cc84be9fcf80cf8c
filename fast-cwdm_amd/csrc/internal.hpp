// libcwdm's cross-unit interface: every function that one translation unit
// defines and another uses is declared here, once (those whose signature needs
// V4Params / V5Aa: conv3d_v4.hpp), with the two process-wide atomics they share.
// No per-thread state crosses units: what a conv call takes and reports beyond
// its desc travels in a ConvCall.  The defining unit includes this header too,
// so a signature or type that drifts fails to compile.
#pragma once
#include <atomic>
#include <vector>

#include "common.hpp"

namespace cwdm {

// ---- conv routing (cwdm_conv3d_forward, conv3d.hip) -----------------------
// kernel-path policy (cwdm_conv3d_set_path; conv3d_v4.hip) and the diagnostics
// builds' stamp buffer (cwdm_debug_conv_stamps)
extern std::atomic<int> g_conv_path;
extern std::atomic<unsigned long long*> g_stamps;

// What one conv call takes beyond its desc, and what it reports back.  The
// eligibility predicates below are functions of (desc, context): a question
// asked at layout time gets the run-time answer when it passes the same fields.
struct ConvCall {
  // offered by the caller (the defaults: nothing)
  GnFinFuse* gnfin = nullptr;    // a pending GroupNorm finalize of d->a_gn (taken: gnfin->used)
  GbwdFuse* gbwd = nullptr;      // the GroupNorm-backward reduce for a dgrad's epilogue (gbwd->used / nblk)
  GapplyFuse* gapply = nullptr;  // the GroupNorm-backward apply for a 1x1 skip dgrad (gapply->used)
  void* act_keep = nullptr;      // where the GroupNorm pre-pass writes the activated input (null: the workspace)
  // the caller's zeroed sync block (plan_sync_bytes): the small-grid K-split arrival counters -- each
  // K-split launch leaves them zero again -- then the apply-ahead sweep counters; null: from the workspace
  unsigned* sync = nullptr;
  bool fp32x = false;            // a 16-bit small-grid conv may write fp32 (the K-expanded split convs only)
  bool stats_wg = false;         // per-workgroup GroupNorm partials wanted
  ProfHook* prof = nullptr;
  // reported by the call
  bool act_kept = false;         // the pre-pass wrote to act_keep
  int64_t stats_rows = 0;        // rows of per-workgroup partials written (0: the per-tile layout)
};
// cwdm_conv3d_forward with its context
int conv3d_forward(const cwdm_conv3d_desc* d, ConvCall& c, hipStream_t s);

// conv3d.hip: the brick / split-K kernels, and the weight packs as jobs (the public packs'
// checks and error codes; a caller batches its jobs through pack_batch_run)
int legacy_conv3d_forward(const cwdm_conv3d_desc* d, ProfHook* prof, hipStream_t s);
int pack_job(const float* w, int cout, int cin, int ksize, int dtype, void* packed, PackJob& j);
int pack_s2_job(const float* w, int cout, int cin, int dtype, void* packed, int transpose, PackJob& j);
int pack_dgrad_job(const float* w, int cout, int cin, int ksize, int dtype, void* packed, PackJob& j);
int pack_phase_job(const float* w, int cout, int cin, int dtype, void* packed, PackJob& j);
int pack_batch_run(std::vector<PackJob>& jobs, int dtype, PackJob* table, std::vector<PackJob>& cache, hipStream_t s);

// conv3d_head.hip: the output head, its fused sampler step, the split-bf16 preparations
bool head_eligible(const cwdm_conv3d_desc* d);
int head_conv_forward(const cwdm_conv3d_desc* d, ProfHook* prof, hipStream_t s);
bool head_sampler_eligible(const cwdm_conv3d_desc* d, const cwdm_sampler_args* a);
int head_sampler_forward(const cwdm_conv3d_desc* d, const cwdm_sampler_args* a, ProfHook* prof, hipStream_t s);
int head_split3_prep(const float* x, const float* gn, int64_t B, int64_t V, int C, void* x3, hipStream_t s);
int head_split3_pack(const float* w, int cout, int cin, float* tmp, void* out, hipStream_t s, int k);
int split3_prep(const float* x0, int c0, const float* x1, int c1, const float* gn, int64_t B, int64_t V, int cm,
                void* x3, hipStream_t s);

// pointwise.hip: 1x1 convs (pw_gapply_ok: the skip dgrad can take a GapplyFuse)
bool pw_eligible(const cwdm_conv3d_desc* d);
int pw_forward(const cwdm_conv3d_desc* d, ConvCall& c, hipStream_t s);
bool pw_gapply_ok(const cwdm_conv3d_desc* d);
bool pw_split_eligible(const cwdm_conv3d_desc* d);
int pw_split_forward(const cwdm_conv3d_desc* d, ProfHook* prof, hipStream_t s);

// conv3d_v4.hip: the DMA-staged conv and its pre-passes
bool v4_eligible(const cwdm_conv3d_desc* d, const ConvCall& c);
int64_t v4_items(const cwdm_conv3d_desc* d);
int v4_ksplit(const cwdm_conv3d_desc* d, const ConvCall& c);
int64_t v4_workspace_bytes(const cwdm_conv3d_desc* d, const ConvCall& c);
int conv3d_v4_forward(const cwdm_conv3d_desc* d, ConvCall& c, hipStream_t s);
int v4_launch(const cwdm_conv3d_desc* d, const void* a0, int c0, const void* a1, int c1, int a0_cm,
              const void* res, int rmode, void* partial, ConvCall& c, hipStream_t s);
bool gbwd_grid_ok(const cwdm_conv3d_desc* d, const GbwdFuse* g);
bool apply_skip_ok(int dtype, int C, int cout, int64_t B, int64_t vpb);
int gn_apply_skip(const void* x0, int c0, const void* x1, int c1, const float* gn, int64_t B, int64_t vpb, int dtype,
                  const void* wskip, int cout, void* act, void* skip, hipStream_t s);
// run the offered GroupNorm finalize f now if it is pending for d (d->a_gn == its ss)
int gnfin_flush(const cwdm_conv3d_desc* d, GnFinFuse* f, hipStream_t s);

// conv3d_v5.hip: the warp-specialised conv
bool v5_eligible(const cwdm_conv3d_desc* d, bool gn, const ConvCall& c);
int v5_aa_units(const cwdm_conv3d_desc* d, const ConvCall& c, int* lead);
// the phase instance takes this upsampling conv (cwdm_conv3d_desc.a_w_phase; rmode: the residual
// mode after the 1x1 skip pre-pass)
bool v5_phase_ok(const cwdm_conv3d_desc* d, int rmode, const ConvCall& c);

// conv3d_sg.hip: the small-grid conv (fp32x: ConvCall::fp32x)
bool sg_eligible(const cwdm_conv3d_desc* d, bool fp32x);
int sg_ksplit(const cwdm_conv3d_desc* d, bool fp32x);
bool sg_skip_eligible(const cwdm_conv3d_desc* d, bool fp32x);
int sg_skip_ksplit(const cwdm_conv3d_desc* d, bool fp32x);
int sg_skip_launch(const cwdm_conv3d_desc* d, void* out, void* partial, const ConvCall& c, hipStream_t s);
int64_t ksplit_slice_voxels(const cwdm_conv3d_desc* d, bool fp32x);
int64_t sg_sync_bytes(int ksplit);
int64_t plan_sync_bytes();
// the apply-ahead sweep counters of a sync block (ConvCall::sync)
unsigned* plan_aa_counters(unsigned* sync);

// ---- what else the U-Net plan drives --------------------------------------
// embed.hip
int launch_time_embed(const float* t, int B, int mc, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* temb, hipStream_t s);
int launch_emb_proj(const float* temb, int B, int E, const float* W, const float* bias, int R, float* out,
                    hipStream_t s);
// grad.hip
int launch_emb_bwd(const float* dEb, int R, int n, int B, const float* temb, int E, const float* W, float* dw,
                   float* db, float* dcb, float* dsil, hipStream_t s, int acc);
int launch_temb_bwd(const float* t, int B, int mc, const float* w1, const float* b1, const float* w2,
                    const float* temb, const float* dsil, float* dw1, float* db1, float* dw2, float* db2,
                    hipStream_t s);
int gn_silu_bwd_impl(const void* x0, int c0, const void* x1, int c1, const void* du, int du_mode, const float* ss,
                     const float* mr, const float* gamma, int groups, int64_t B, int64_t d, int64_t h, int64_t w,
                     int dtype, void* dx0, int acc0, void* dx1, int acc1, float* dgamma, float* dbeta, void* ws,
                     int64_t ws_bytes, float* chs, int64_t chs_stride, cwdm_stream_t stream, int acc_affine,
                     const float* pre_part = nullptr, int pre_nblk = 0, const float** coef_out = nullptr);
int gb_part_reduce(const float* part, int nblk, int C, int64_t B, int slices, float* out, hipStream_t s);
// wavelet_nd.hip
int haar_nd_synth_add(int dtype, int64_t B, int64_t d, int64_t h, int64_t w, int C, const void* L, int64_t l_vs,
                      float lll, const void* H, int64_t h_vs, float high, void* fine, int acc, hipStream_t s);
int haar_nd_anal_add(int dtype, int64_t B, int64_t d, int64_t h, int64_t w, int C, const void* fine, void* L,
                     int64_t l_vs, float lll, int accL, void* H, int64_t h_vs, float high, int accH, hipStream_t s);
// wavelet2.hip: the two-level sampler step (cwdm_sampler_step, wavelet.hip)
int sampler2_launch(const cwdm_sampler_args* a, hipStream_t s);

}  // namespace cwdm
