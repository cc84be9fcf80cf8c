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
// kernel-path policy (cwdm_conv3d_set_path; conv_route.cpp) and the diagnostics
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

// ---- the route of one conv call (conv_route.cpp) --------------------------
// Everything that is decided about a conv before anything is launched: which
// kernel runs it, how its GroupNorm'd input and its 1x1 skip product are
// prepared, its K split, what it takes of the context's offers, and its
// workspace.  conv_route is the one place that decides; the launch path
// (conv3d.hip, conv3d_v4.hip), cwdm_conv3d_workspace_bytes and the U-Net
// plan's layout read the result.
enum class ConvKernel {
  Head,        // conv3d_head.hip: the output head
  Pointwise,   // pointwise.hip: a pure 1x1
  SmallGrid,   // conv3d_sg.hip (W < kWideMinW)
  V5Phase,     // conv3d_v5.hip, an upsampling conv as eight phase convs
  V5,          // conv3d_v5.hip on raw or pre-activated sources
  V5Gn,        //   ... applying the GroupNorm in LDS
  V5Aa,        //   ... writing the activated copy ahead of its own sweep (aa_units, aa_lead)
  V5Split,     // conv3d_v5s_kernel: fp32 through split-bf16 weights (a_w_split)
  V4,          // conv3d_v4.hpp
  Brick        // conv3d_kernels.hpp: every shape and mode
};
enum class GnInput { None, Apply, FinApply, InKernel };   // the gn_apply / gn_fin_apply pre-pass, or the kernel's own
enum class SkipKernel { None, SmallGrid, Pw, PwSplit, Brick };   // d->b_w beside a 3x3x3 conv: runs first, added as the residual
struct ConvRoute {
  ConvKernel kernel = ConvKernel::Brick;
  GnInput gn = GnInput::None;
  SkipKernel skip = SkipKernel::None;
  int ksplit = 1, skip_ksplit = 1;
  int aa_units = 0, aa_lead = 0;
  bool flush_fin = false;      // an offered GroupNorm finalize (ConvCall::gnfin) runs first, on its own
  bool v4_ok = false;          // the v4 kernel's shape / work rule holds (the fused GroupNorm + skip pass of the plan asks)
  bool ct32 = false, fast = false;   // V4: 32-channel tiles / the 32-bit-offset epilogue
  // what the call takes of its context
  bool takes_gbwd = false, takes_gapply = false, keeps_act = false;
  // workspace regions, in this order: the activated input | the skip product | the K-split slices with their
  // counters | the apply-ahead counters.  Sizes, conservatively: a region is counted where the desc could
  // use it (ws_act for any a_gn, ws_aa likewise), so the total depends on the desc's shape alone.
  int64_t ws_act = 0, ws_skip = 0, ws_ksplit = 0, ws_aa = 0, ws_total = 0;
  bool on_dma() const { return kernel != ConvKernel::Head && kernel != ConvKernel::Pointwise && kernel != ConvKernel::Brick; }
  bool gn_in_lds() const { return gn == GnInput::InKernel && kernel != ConvKernel::V5Aa; }
};
// the preferred route of (d, c), whatever workspace d brings (conv3d_forward demotes to Brick below ws_total)
ConvRoute conv_route(const cwdm_conv3d_desc* d, const ConvCall& c);
// the route of a launch on prepared sources (v4_launch): GroupNorm applied, the skip product, if any,
// in the residual slot (rmode: the residual mode the launch sees) -- the kernel and its K split only
ConvRoute conv_route_prepared(const cwdm_conv3d_desc* d, int rmode, const ConvCall& c);
// cwdm_conv3d_workspace_bytes with the route in hand: the route's regions, or the brick kernels' split-K slices
int64_t conv_workspace_bytes(const cwdm_conv3d_desc* d, const ConvRoute& r);
// the kernel (skip) and K split (skip_ksplit) of a 1x1 skip product e run on its own, as conv_route
// picks them for the skip beside a 3x3x3 conv
ConvRoute conv_route_skip(const cwdm_conv3d_desc* e, const ConvCall& c);
// the 1x1 skip product of d on its own (segment B only, the output written in the compute dtype)
cwdm_conv3d_desc skip_desc(const cwdm_conv3d_desc* d, void* out);
// compute units of the device (256 without one)
int cu_count();
constexpr int kV5AaWords = 4096;   // apply-ahead sweep counters of one launch (conv3d_v5.hip kV5AaCnt)

// conv3d.hip: the brick / split-K kernels, and the weight packs as jobs (the public packs'
// checks and error codes; a caller batches its jobs through pack_batch_run)
int legacy_conv3d_forward(const cwdm_conv3d_desc* d, ProfHook* prof, hipStream_t s);
int pack_job(const float* w, int cout, int cin, int ksize, int dtype, void* packed, PackJob& j);
// a 3x3x3 conv whose packed input channels [cin_real, cin) are zero columns (w is cout x cin_real OIDHW): the
// U-Net's conv_in over an input padded to the K chunk
int pack_zext_job(const float* w, int cout, int cin_real, int cin, int dtype, void* packed, PackJob& j);
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

// pointwise.hip: 1x1 convs (gapply: the launch takes c.gapply, ConvRoute::takes_gapply)
int pw_forward(const cwdm_conv3d_desc* d, ConvCall& c, bool gapply, hipStream_t s);
int pw_split_forward(const cwdm_conv3d_desc* d, ProfHook* prof, hipStream_t s);

// conv3d_v4.hip: the DMA-staged conv and its pre-passes, by the route r
int conv3d_v4_forward(const cwdm_conv3d_desc* d, const ConvRoute& r, ConvCall& c, hipStream_t s);
int v4_launch(const cwdm_conv3d_desc* d, const void* a0, int c0, const void* a1, int c1, int a0_cm,
              const void* res, int rmode, void* partial, const ConvRoute& r, ConvCall& c, hipStream_t s);
bool apply_skip_ok(int dtype, int C, int cout, int64_t B, int64_t vpb);
int gn_apply_skip(const void* x0, int c0, const void* x1, int c1, const float* gn, int64_t B, int64_t vpb, int dtype,
                  const void* wskip, int cout, void* act, void* skip, hipStream_t s);
// the fused finalize + pre-pass takes the offered finalize f (gn_fin_apply)
bool gn_fin_fusable(const GnFinFuse& f, int dtype, int c0, int c1);
// run the offered GroupNorm finalize f now if it is pending for d (d->a_gn == its ss)
int gnfin_flush(const cwdm_conv3d_desc* d, GnFinFuse* f, hipStream_t s);

// conv3d_v5.hip: what of the warp-specialised conv's rules depends on its launch grids.  Both assume
// a conv that kernel takes (conv_route asks them after its own shape rule).
// apply-ahead: the per-chunk share (1..8 steps of 256 lanes) its sweep needs and the sweep lead, or 0
int v5_aa_units(const cwdm_conv3d_desc* d, int* lead);
// the phase instance takes this upsampling conv (cwdm_conv3d_desc.a_w_phase; rmode: the residual
// mode the launch sees)
bool v5_phase_ok(const cwdm_conv3d_desc* d, int rmode, bool stats_wg);

// conv3d_sg.hip: the small-grid conv (ksplit: ConvRoute::ksplit / skip_ksplit)
int sg_skip_launch(const cwdm_conv3d_desc* d, void* out, void* partial, int ksplit, const ConvCall& c, hipStream_t s);
int64_t sg_sync_bytes(int ksplit);
int64_t plan_sync_bytes();
// the apply-ahead sweep counters of a sync block (ConvCall::sync)
unsigned* plan_aa_counters(unsigned* sync);

// ---- what else the U-Net plan drives --------------------------------------
// layout.hip: dst (voxels, c_dst) = [src (voxels, c_src) | zeros], channels-last, both 16-byte aligned with whole
// 16-byte quads of channels; every lane of dst is written on every call
int pad_channels(const void* src, int c_src, void* dst, int c_dst, int dtype, int64_t voxels, hipStream_t s);
// conv3d_v5.hip: the device address of the sticky error word behind cwdm_device_status (looked up once;
// call it outside stream capture first: cwdm_unet_set_labels does)
int dev_err_word(unsigned** word);
// embed.hip (label_w null: no class conditioning; else temb += label_w[y[b]], y int64[B] on the device)
int launch_time_embed(const float* t, int B, int mc, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* temb, const float* label_w, const int64_t* y, int num_classes,
                      hipStream_t s);
int launch_emb_proj(const float* temb, int B, int E, const float* W, const float* bias, int R, float* out,
                    hipStream_t s);
// grad.hip
int launch_emb_bwd(const float* dEb, int R, int n, int B, const float* temb, int E, const float* W, float* dw,
                   float* db, float* dcb, float* dsil, hipStream_t s, int acc);
int launch_temb_bwd(const float* t, int B, int mc, const float* w1, const float* b1, const float* w2,
                    const float* temb, const float* dsil, float* dw1, float* db1, float* dw2, float* db2,
                    hipStream_t s);
// d label_emb.weight[c][:] = sum over b with y[b] == c, b ascending, of dsil[b][:] * SiLU'(temb[b][:]) (the
// gradient of temb launch_temb_bwd consumes); every row written, absent classes as +0.0
int launch_label_emb_bwd(const float* temb, const float* dsil, const int64_t* y, int B, int E, int num_classes,
                         float* dlabel, hipStream_t s);
// a FiLM block's out_layers.0 in gn_silu_bwd_impl: beta (d s needs it), the rows [s | t] and where d s, d t go
// (batch strides in floats), and chs_c (optional): the per-channel sums of the written dx0 over voxels and
// batch entries, added to chs_c[c] in a fixed order -- the bias gradient of the block's conv1
struct GnBwdFilm {
  const float* beta;
  const float* film; int64_t film_bs;
  float* dfilm; int64_t dfilm_bs;
  float* chs_c;
};
int gn_silu_bwd_impl(const void* x0, int c0, const void* x1, int c1, const void* du, int du_mode, const float* ss,
                     const float* mr, const float* gamma, int groups, int64_t B, int64_t d, int64_t h, int64_t w,
                     int dtype, void* dx0, int acc0, void* dx1, int acc1, float* dgamma, float* dbeta, void* ws,
                     int64_t ws_bytes, float* chs, int64_t chs_stride, cwdm_stream_t stream, int acc_affine,
                     const float* pre_part = nullptr, int pre_nblk = 0, const float** coef_out = nullptr,
                     const GnBwdFilm* film = nullptr);
int gb_part_reduce(const float* part, int nblk, int C, int64_t B, int slices, float* out, hipStream_t s);
constexpr int kGbSlices = 64;   // slice sums the plan takes of the fused GroupNorm-backward partials (gb_part_reduce)
// attention.hip: the bottleneck attention block's projections (cwdm_attn_linear / cwdm_attn_pack with
// their arguments spelled out), the adjoint of the legacy row permutation for the qkv gradients
// (dst[source row][c] += src[packed row][c]), and the backward of a GroupNorm without activation:
// dx = (acc ? dx : 0) + add + dGN(dn), dgamma / dbeta accumulated; part: fp32 scratch [B][C][2]
int64_t attn_parts(int64_t T);
int attn_linear(int dtype, int64_t B, int64_t T, int K, int N, const void* in, const float* gn, const void* w,
                const float* bias, const void* res, void* out, void* n_out, float* stats, hipStream_t s);
int attn_pack(const float* w, int rows, int cols, int heads, int ch, int legacy, int transpose, int dtype, void* out,
              hipStream_t s);
int attn_unperm_add(const float* src, float* dst, int rows, int cols, int heads, int ch, hipStream_t s);
int gn_lin_bwd(int dtype, int64_t B, int64_t T, int C, int groups, const void* x, const void* dn, const float* mr,
               const float* gamma, const void* add, void* dx, int acc, float* part, float* dgamma, float* dbeta,
               hipStream_t s);
// wavelet_nd.hip
int haar_nd_synth_add(int dtype, int64_t B, int64_t d, int64_t h, int64_t w, int C, const void* L, int64_t l_vs,
                      float lll, const void* H, int64_t h_vs, float high, void* fine, int acc, hipStream_t s);
int haar_nd_anal_add(int dtype, int64_t B, int64_t d, int64_t h, int64_t w, int C, const void* fine, void* L,
                     int64_t l_vs, float lll, int accL, void* H, int64_t h_vs, float high, int accH, hipStream_t s);
// wavelet2.hip: the two-level sampler step (cwdm_sampler_step, wavelet.hip)
int sampler2_launch(const cwdm_sampler_args* a, hipStream_t s);

}  // namespace cwdm
