// The route of a conv call (ConvRoute, internal.hpp): host code only.  Each kernel's shape rule is a
// file-local predicate here; conv_route applies them in one fixed order and sizes the
// workspace from the same decisions.  What depends on a kernel's launch grid (the CU count, the
// apply-ahead share, the phase instance's statistics rows) is asked of the kernel's own unit.
#include <algorithm>

#include "conv3d_kernels.hpp"
#include "internal.hpp"

namespace cwdm {

// kernel-path policy (cwdm_conv3d_set_path): 0 auto, 1 legacy only, 2 DMA kernels wherever the shape allows,
// 3 as 2 without the warp-specialised kernel
std::atomic<int> g_conv_path{env_int("CWDM_CONV_PATH", 0)};

namespace {

inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }

int64_t src_voxels(const cwdm_conv3d_desc* d) {
  const int64_t V = d->D * d->H * d->W;
  return d->a_mode == 1 ? V / 8 : V;
}

// ---- pointwise.hip -----------------------------------------------------------
// shapes the pointwise kernel takes: a pure 1x1 (segment B only), 16-bit, no
// residual / statistics, output in the compute dtype, channels in 16s
bool pw_eligible(const cwdm_conv3d_desc* d) {
  if (!dtype_half(d->dtype) || d->a_w || !d->b_w || d->res_mode >= 0 || d->stats || d->out_dtype != d->dtype)
    return false;
  const int K = d->b_c0 + d->b_c1;
  if (K % 16 || d->b_c0 % 16 || d->cout % 8 || (d->out1 && d->out_c0 % 4)) return false;
  return d->B * d->D * d->H * d->W < (1LL << 40);
}

// the accurate fast mode's pure 1x1 (a_w_split marks it: the split weights of
// the conv this skip belongs to): fp32, no residual / statistics / second output
bool pw_split_eligible(const cwdm_conv3d_desc* d) {
  if (d->dtype != CWDM_F32 || !d->a_w_split || d->a_w || !d->b_w || d->res_mode >= 0 || d->stats ||
      d->out_dtype != CWDM_F32 || d->out1 || d->accumulate)
    return false;
  const int K = d->b_c0 + d->b_c1;
  return K % 16 == 0 && d->b_c0 % 16 == 0 && d->cout % 32 == 0 && d->B * d->D * d->H * d->W < (1LL << 40);
}

// ---- conv3d_sg.hip -----------------------------------------------------------
// fp32x (ConvCall::fp32x, set by the U-Net plan for the accurate fast mode's K-expanded small-grid
// convs): a 16-bit conv with fp32 output takes this kernel, its residual fp32 too
bool sg_shape_ok(const cwdm_conv3d_desc* d, bool fp32x) {
  if (g_conv_path.load(std::memory_order_relaxed) == 1) return false;
  if (!dtype_half(d->dtype) || d->accumulate || d->out1 || d->cout % 64) return false;
  if (d->out_dtype != d->dtype && !(d->out_dtype == CWDM_F32 && fp32x)) return false;
  // W < kWideMinW (the wide kernels take the rest): 16 x 4 x 4 bricks for W >= 16,
  // 8 x 8 x 4 below (pick_brick's statistics bricks), the last brick of an axis partial
  return d->W >= 1 && d->W < kWideMinW && d->H >= 1 && d->D >= 1;
}

// shapes the small-grid kernel takes: bf16, plain bf16 output (no fp32 / dual /
// accumulating output), same-grid or upsampled source and residual, W = 16
// (16x4x4 statistics bricks) or W = 8 (8x8x4), 32-channel K chunks.  At 8^3
// there are only 32 tiles: K split across workgroups (sg_ksplit), finished by
// the last slice of each tile.
bool sg_eligible(const cwdm_conv3d_desc* d, bool fp32x) {
  if (!sg_shape_ok(d, fp32x) || !d->a_w) return false;
  if (d->a_mode != 0 && d->a_mode != 1) return false;
  if (d->res_mode < -1 || d->res_mode > 1) return false;
  if ((d->a_c0 + d->a_c1) % 32 || d->a_c0 % 16) return false;
  const int64_t V = d->D * d->H * d->W;
  const int64_t SV = d->a_mode == 1 ? V / 8 : V;
  return SV * (d->a_c0 + d->a_c1) * 2 < 0xFFFFE000LL && d->B * (V / 256) * (d->cout / 16) < (1LL << 31);
}

// the 1x1 skip segment alone (segment B of a desc, channels-last sources)
bool sg_skip_eligible(const cwdm_conv3d_desc* d, bool fp32x) {
  if (!sg_shape_ok(d, fp32x) || !d->b_w) return false;
  if ((d->b_c0 + d->b_c1) % 32 || d->b_c0 % 16) return false;
  const int64_t V = d->D * d->H * d->W;
  return V * (d->b_c0 + d->b_c1) * 2 < 0xFFFFE000LL && d->B * (V / 256) * (d->cout / 16) < (1LL << 31);
}

// statistics bricks of a small grid (== cwdm_conv3d_parts, pick_brick)
int64_t sg_parts(const cwdm_conv3d_desc* d) {
  const Brick br = pick_brick(d->D, d->H, d->W);
  return ceil_div(d->W, br.bx) * ceil_div(d->H, br.by) * ceil_div(d->D, br.bz);
}

// K slices of a launch: enough work items for the chip (~256), at least one
// 32-channel chunk per slice (the 16^3 level has 256 tiles: no split)
int sg_split_for(const cwdm_conv3d_desc* d, int cin, bool skip = false) {
  const int64_t tiles = d->B * sg_parts(d) * (d->cout / 16);
  const int nch = cin / 32;
  // work-item target (env CWDM_SG_TARGET, A/B knob; 192 since r04: the 8^3
  // level splits K 4 ways instead of 8, 66.28 -> 66.54 steps/s on one box,
  // config 5 unchanged -- profiles/r04/g_sg_target_ab.txt); the 1x1 skips' own
  // (env CWDM_SG_SKIP_TARGET, A/B knob, default the same)
  static const int64_t target3 = env_ll("CWDM_SG_TARGET", 192);
  static const int64_t target1 = env_ll("CWDM_SG_SKIP_TARGET", target3);
  const int64_t target = skip ? target1 : target3;
  if (tiles >= target || nch < 2) return 1;
  int S = (int)std::min<int64_t>((target + tiles - 1) / tiles, nch);
  const int per = (nch + S - 1) / S;
  S = (nch + per - 1) / per;
  return (tiles * S < (1 << 16) && S > 1) ? S : 1;
}

// voxels per batch of one K-split slice: the small-grid kernel stores whole
// (possibly partial) bricks of 256 voxels, the wide kernel the grid itself
int64_t ksplit_slice_voxels(const cwdm_conv3d_desc* d, bool fp32x) {
  return sg_shape_ok(d, fp32x) ? sg_parts(d) * 256 : d->D * d->H * d->W;
}

// ---- conv3d_v4.hpp -----------------------------------------------------------
int64_t v4_items(const cwdm_conv3d_desc* d) {
  return d->B * ((d->W + 31) / 32) * (d->H / 4) * (d->D / 4) * (d->cout / 64);
}

// work items a launch aims for before it splits K (env CWDM_V4_KSPLIT_TARGET)
int64_t v4_ksplit_target() {
  // 64 (r04; was 128): config 5's 28^3 64-channel down-block convs (49 tiles)
  // then run unsplit on 32-channel tiles: 44 -> 19 us against the split legacy path
  static const int64_t t = env_ll("CWDM_V4_KSPLIT_TARGET", 64);
  return t;
}

// K split of a conv of the DMA path: the small-grid kernel's own (8^3 level), else that of a grid
// with fewer tiles than two workgroups per CU (the 32^3 level): enough K slices for ~512 work items,
// at least two chunks per slice
int dma_ksplit(const cwdm_conv3d_desc* d, bool sg) {
  if (sg) return sg_split_for(d, d->a_c0 + d->a_c1);
  const int ck = ck_of(d->dtype);
  const int nch = (d->a_c0 + d->a_c1) / ck;
  const int64_t nblk = v4_items(d);
  const int64_t target = v4_ksplit_target();
  if (nblk >= target || nch < 2 || nblk == 0) return 1;   // (no tile: a shape none of the wide kernels takes)
  // 16-bit: v4_launch doubles the work items with 32-channel tiles (no finishing
  // passes) -- enough at config 5's 28^3 level (98 -> 196)
  if (dtype_half(d->dtype) && 2 * nblk >= target && d->cout % 64 == 0) return 1;
  int S = (int)std::min<int64_t>((target + nblk - 1) / nblk, nch / 2);
  if (S < 1) S = 1;
  const int per = (nch + S - 1) / S;
  return (nch + per - 1) / per;
}

// the v4 kernel (or, sg: the small-grid kernel behind the same pre-passes) takes the conv
bool v4_eligible(const cwdm_conv3d_desc* d, bool sg, int S) {
  const int path = g_conv_path.load(std::memory_order_relaxed);
  if (path == 1) return false;
  // the 1x1 skip product is added through the residual slot: not both
  if (d->b_w && d->res_mode >= 0) return false;
  if (sg) return true;  // 16^3 / 8^3 levels: conv3d_sg.hip behind the same pre-passes
  if (!dtype_compute(d->dtype)) return false;
  // W >= kWideMinW: the statistics partials follow cwdm_conv3d_parts' 32-wide x tiles (pick_brick)
  if (!d->a_w || d->W < kWideMinW || d->H % 4 || d->D % 4 || d->cout % 64) return false;
  if (d->a_mode != 0 && d->a_mode != 1) return false;
  if (d->res_mode < -1 || d->res_mode > 1) return false;
  if (d->out1 && d->out_c0 % 8) return false;
  const int64_t nblk = v4_items(d);
  // work items: K slices, or (16-bit, no split, < 256 tiles) v4_launch's 32-channel tiles
  const int64_t items = nblk * S * (S == 1 && dtype_half(d->dtype) && nblk < 256 ? 2 : 1);
  if (items < std::min<int64_t>(384, v4_ksplit_target()) && path < 2) return false;  // too few work items even K-split: the brick kernels
  const int esz = dtype_size(d->dtype);
  const int64_t sv = src_voxels(d);
  // the DMA range check works on 32-bit byte offsets per batch
  const int64_t lim = 0xFFFFE000LL;
  if (d->a_gn) return sv * (d->a_c0 + d->a_c1) * esz < lim;
  return sv * d->a_c0 * esz < lim && sv * d->a_c1 * esz < lim;
}

// the U-Net plan's backward: fuse the reduce pass of the SiLU(GroupNorm)
// backward that follows this dgrad conv into its epilogue (GbwdFuse, conv3d_v4.hpp
// V4Params::gx0); taken only by the 16-bit fast epilogue without K split (v4
// only), and only where the conv leaves VALU room -- at 128^3 the
// epilogue's ~13 VALU + 2 transcendentals per output element cost the
// MFMA-bound kernel more (+30 %) than the separate reduce pass it saves; at
// 32^3 it is a net win (same-box kernel traces).  At 64^3 it was too
// against v4's plain dgrad (r03), but the warp-specialised kernel now takes those
// dgrads faster than the fused v4 instance runs: 12 launches 3096 us fused vs 2547 +
// 371 us of separate reduces (r06, profiles/r06/w_gbwd_maxw_ab.txt).  Env
// CWDM_GBWD_MAXW, default 32.  Elsewhere the dgrad is an ordinary conv (v5 may take it).
bool gbwd_grid_ok(const cwdm_conv3d_desc* d, const GbwdFuse* g) {
  static const int gb_maxw = env_int("CWDM_GBWD_MAXW", 32);
  return g && !g->used && dtype_half(d->dtype) && d->W <= gb_maxw && d->a_mode == 0 && d->res_mode < 0 &&
         !d->stats;
}

// ---- conv3d_v5.hip -----------------------------------------------------------
// the warp-specialised kernel takes a conv of the DMA path when it is a 16-bit
// fast-epilogue conv without K split (S) and with at least one tile per CU (CWDM_V5_MIN_TPC)
// (env CWDM_V5: 0 off, 1 GroupNorm'd inputs only, 2 every eligible conv, 3 (default)
// every eligible conv with the GroupNorm applied by the cwdm_gn_apply pre-pass: the
// in-LDS transform costs the helper waves more issue cycles than the MFMA waves
// leave them -- measured 611 vs 588 us on the 64->64 128^3-subband conv)
// gn: with the GroupNorm applied in LDS
bool v5_eligible(const cwdm_conv3d_desc* d, bool gn, bool sg, int S, const ConvCall& c) {
  static const int mode = env_int("CWDM_V5", 3);
  const int path = g_conv_path.load(std::memory_order_relaxed);
  if (d->dtype == CWDM_F32) {
    // the accurate fast mode (conv3d_v5s_kernel): wherever the split weights are
    // given and the shape tiles (no minimum work: it is 8x the exact-fp32 MFMA rate)
    if (!d->a_w_split || path == 1 || path == 3) return false;
    if (d->out_dtype != CWDM_F32 || d->accumulate || d->out1) return false;
    if (d->a_mode != 0 && d->a_mode != 1) return false;
    if (d->a_c0 % 16 || d->a_c1 % 16) return false;   // pairs of 8-channel fp32 chunks, never straddling the sources
    if (d->res_mode < -1 || d->res_mode > 1) return false;
    // the 1x1 skip product is added through the residual slot (conv3d_v4_forward): not both
    if (d->b_w && d->res_mode >= 0) return false;
    if (d->W < kWideMinW || d->H % 4 || d->D % 4 || d->cout % 64) return false;
    // 32-bit buffer offsets per batch: the output, and the sources (raw, or the
    // activated (c0 + c1)-channel copy of the training forward's pre-pass)
    const int64_t lim = 0xFFFFE000LL;
    if (d->D * d->H * d->W * d->cout * 4 >= lim) return false;
    const int64_t sv = src_voxels(d);
    if (d->a_gn ? sv * (d->a_c0 + d->a_c1) * 4 >= lim : (sv * d->a_c0 * 4 >= lim || sv * d->a_c1 * 4 >= lim))
      return false;
    return !(gn && d->a_mode == 1);
  }
  if (mode <= 0 || (mode == 1 && !gn) || path == 1 || path == 3) return false;
  // GroupNorm+SiLU in LDS: not for an upsampling conv (its halo repeats every
  // source voxel 8x: the pre-pass at the half resolution is 8x cheaper), and
  // not in mode 3 (pre-pass + this kernel on the activated copy)
  if (gn && (d->a_mode == 1 || mode == 3)) return false;
  if (!dtype_half(d->dtype) || sg) return false;
  if (path != 2 && S != 1) return false;   // (path 2: forced, no K split of its own)
  if (d->out_dtype != d->dtype || d->accumulate || d->out1) return false;
  if (d->a_mode != 0 && d->a_mode != 1) return false;
  if (d->res_mode < -1 || d->res_mode > 1) return false;
  if (d->W < kWideMinW || d->H % 4 || d->D % 4 || d->cout % 64) return false;
  if (d->D * d->H * d->W * d->cout * 2 >= 0xFFFFE000LL) return false;
  if (d->a_c0 + d->a_c1 < 32) return false;   // >= 2 chunks per tile: a tile's drain spans two chunks
  if (gbwd_grid_ok(d, c.gbwd)) return false;   // the backward's fused dgrad instance is v4's
  // tiles per CU below which v4 (two workgroups per CU) keeps the conv (env
  // CWDM_V5_MIN_TPC, A/B knob; 1 since r04: config 5's 56^3 64-channel convs,
  // 392 tiles, 57 -> 53 us on v5)
  static const double min_tpc = env_double("CWDM_V5_MIN_TPC", 1.0);
  return path == 2 || (double)v4_items(d) >= min_tpc * cu_count();
}

// ---- the launch on prepared sources -----------------------------------------
// what one desc answers to every rule below (each asked once)
struct Facts {
  bool sg;    // the small-grid kernel takes the conv
  int S;      // its K split on the DMA path
  bool v5;    // the warp-specialised kernel takes it (sources raw or pre-activated)
};
Facts facts_of(const cwdm_conv3d_desc* d, const ConvCall& c) {
  Facts f;
  f.sg = sg_eligible(d, c.fp32x);
  f.S = dma_ksplit(d, f.sg);
  f.v5 = v5_eligible(d, false, f.sg, f.S, c);
  return f;
}

// the kernel of a launch whose sources are prepared, in v4_launch's order: small-grid, the phase
// instance, the warp-specialised kernel, v4 (with its tile form and what it takes of c.gbwd)
void route_launch(ConvRoute& r, const cwdm_conv3d_desc* d, int rmode, const Facts& f, const ConvCall& c) {
  r.ksplit = 1;
  if (f.sg) {
    r.kernel = ConvKernel::SmallGrid;
    r.ksplit = f.S;
  } else if (f.v5 && v5_phase_ok(d, rmode, c.stats_wg)) {
    // an upsampling conv as eight phase convs on the source grid, where its phase weights came along
    r.kernel = ConvKernel::V5Phase;
  } else if (f.v5) {   // (refuses the dgrad that takes the fused GroupNorm-backward reduce)
    r.kernel = d->dtype == CWDM_F32 ? ConvKernel::V5Split : ConvKernel::V5;
  } else {
    r.kernel = ConvKernel::V4;
    r.ksplit = f.S;
    const bool out_f32 = d->out_dtype == CWDM_F32 && d->dtype != CWDM_F32;
    // the fast epilogue addresses output / residual through 32-bit buffer offsets per batch
    const bool plain_out = !out_f32 && !d->accumulate && !d->out1 && d->D * d->H * d->W * d->cout * 2 < 0xFFFFE000LL;
    r.fast = plain_out && f.S == 1;   // (K slices are fp32 partials)
    // fewer 64-channel tiles than CUs (the 32^3 level): 32-channel tiles, one
    // z-plane per wave (twice the work items; the statistics bricks are the same)
    static const bool ct32_on = env_not0("CWDM_V4_CT32");
    r.ct32 = ct32_on && dtype_half(d->dtype) && f.S == 1 && plain_out && v4_items(d) < 256;
    // (gbwd_grid_ok: where the fused reduce pays)
    if (gbwd_grid_ok(d, c.gbwd) && (r.ct32 || r.fast) && f.S == 1 && rmode < 0 && !d->stats && d->a_mode == 0) {
      const GbwdFuse& g = *c.gbwd;
      const int nc = r.ct32 ? 32 : 64, C = d->cout;
      const long long need = (long long)d->B * ((d->W + 31) / 32) * (d->H / 4) * (d->D / 4) * C * 8;
      r.takes_gbwd = g.groups > 0 && C % g.groups == 0 && C / g.groups >= 2 && g.c0 % nc == 0 && g.c0 <= C &&
                     (g.c0 == C || g.x1) && need <= g.part_bytes;
    }
  }
}

}  // namespace

cwdm_conv3d_desc skip_desc(const cwdm_conv3d_desc* d, void* out) {
  cwdm_conv3d_desc e = *d;
  e.a0 = nullptr; e.a1 = nullptr; e.a_c0 = 0; e.a_c1 = 0; e.a_gn = nullptr; e.a_w = nullptr; e.a_mode = 0;
  e.bias = nullptr; e.bias_bstride = 0; e.stats = nullptr;
  e.out = out; e.out_dtype = d->dtype; e.out1 = nullptr; e.out_c0 = 0; e.accumulate = 0;
  e.workspace = nullptr; e.ws_bytes = 0;
  return e;
}

ConvRoute conv_route_skip(const cwdm_conv3d_desc* e, const ConvCall& c) {
  ConvRoute r;
  r.skip = sg_skip_eligible(e, c.fp32x) ? SkipKernel::SmallGrid
           : pw_eligible(e)             ? SkipKernel::Pw
           : pw_split_eligible(e)       ? SkipKernel::PwSplit
                                        : SkipKernel::Brick;
  if (r.skip == SkipKernel::SmallGrid) r.skip_ksplit = sg_split_for(e, e->b_c0 + e->b_c1, true);
  return r;
}

ConvRoute conv_route_prepared(const cwdm_conv3d_desc* d, int rmode, const ConvCall& c) {
  ConvRoute r;
  route_launch(r, d, rmode, facts_of(d, c), c);
  return r;
}

// The rules, in order:
//  1. the output head (head_eligible), 2. a pure 1x1 (pw_eligible): neither uses a workspace;
//  3. the DMA path -- v4 or the small-grid kernel could run it, or (fp32 with split weights) the
//     split-bf16 kernel can -- else the brick kernels;
//  on the DMA path
//  4. a GroupNorm'd input: in the warp-specialised kernel's LDS (inference: nothing keeps the copy),
//     else written by that kernel ahead of its sweep (v5_aa_units), else by a pre-pass, which takes
//     an offered finalize where gn_fin_fusable allows;
//  5. the 1x1 skip product first, as the conv's residual: small-grid 1x1, pw, pw_split, brick;
//  6. the kernel: small-grid, the phase instance, v5, v4 (route_launch), with its K split.
ConvRoute conv_route(const cwdm_conv3d_desc* d, const ConvCall& c) {
  ConvRoute r;
  // (an offered GroupNorm finalize runs first on every route but the one whose pre-pass takes it)
  GnFinFuse* fin = (c.gnfin && !c.gnfin->used && d->a_gn && c.gnfin->ss == d->a_gn) ? c.gnfin : nullptr;
  r.flush_fin = fin != nullptr;
  if (head_eligible(d)) {
    r.kernel = ConvKernel::Head;
    if (d->a_gn) r.gn = GnInput::InKernel;
    return r;
  }
  if (pw_eligible(d)) {
    r.kernel = ConvKernel::Pointwise;
    const GapplyFuse* g = c.gapply;
    r.takes_gapply = g && !g->used && d->cout % 8 == 0 && (!d->out1 || d->out_c0 % 8 == 0) &&
                     d->D * d->H * d->W >= 256 && !d->bias;
    return r;
  }
  const Facts f = facts_of(d, c);
  r.v4_ok = v4_eligible(d, f.sg, f.S);
  // (the accurate fast mode's split-bf16 kernel takes fp32 shapes of any size: the same host path)
  if (!(r.v4_ok || (d->a_w_split && f.v5))) return r;   // Brick

  // the workspace: sized by the desc's shape alone (see ConvRoute)
  const int esz = dtype_size(d->dtype);
  int rmode = d->res_mode;
  if (d->a_gn) r.ws_act = align256(d->B * src_voxels(d) * (d->a_c0 + d->a_c1) * esz);
  if (d->b_w) {
    r.ws_skip = align256(d->B * d->D * d->H * d->W * d->cout * esz);
    const cwdm_conv3d_desc e = skip_desc(d, nullptr);
    const ConvRoute k = conv_route_skip(&e, c);
    r.skip = k.skip;
    r.skip_ksplit = k.skip_ksplit;   // (its slices use the conv's K-split region: the skip runs first)
    rmode = 0;
  }
  const int S = std::max(f.S, r.skip_ksplit);
  // (+ the small-grid kernel's K-split arrival counters behind the slices)
  if (S > 1) r.ws_ksplit = align256(S * d->B * ksplit_slice_voxels(d, c.fp32x) * d->cout * 4) + sg_sync_bytes(S);
  // (+ a lone launch's apply-ahead sweep counters, last)
  if (d->a_gn) r.ws_aa = kV5AaWords * 4;
  r.ws_total = r.ws_act + r.ws_skip + r.ws_ksplit + r.ws_aa;

  route_launch(r, d, rmode, f, c);
  if (d->a_gn) {
    // GroupNorm + SiLU inside the warp-specialised conv (no activated copy): inference only -- the
    // training forward keeps the activated input for wgrad; or that conv writes the activated copy
    // itself, ahead of its sweep (apply-ahead: no pre-pass over HBM; the training forward keeps the copy)
    if (!c.act_keep && v5_eligible(d, true, f.sg, f.S, c)) {
      r.kernel = d->dtype == CWDM_F32 ? ConvKernel::V5Split : ConvKernel::V5Gn;
      r.gn = GnInput::InKernel;
      r.ksplit = 1;
    } else if (f.v5 && (r.aa_units = v5_aa_units(d, &r.aa_lead)) > 0) {
      r.kernel = ConvKernel::V5Aa;
      r.gn = GnInput::InKernel;
      r.ksplit = 1;
    } else {
      r.aa_units = r.aa_lead = 0;
      r.gn = fin && gn_fin_fusable(*fin, d->dtype, d->a_c0, d->a_c1) ? GnInput::FinApply : GnInput::Apply;
    }
    if (r.gn == GnInput::FinApply) r.flush_fin = false;
    if (r.kernel != ConvKernel::V4) r.takes_gbwd = r.ct32 = r.fast = false;
    r.keeps_act = c.act_keep && !r.gn_in_lds();
  }
  return r;
}

}  // namespace cwdm

extern "C" int cwdm_conv3d_set_path(int path) {
  CWDM_REQUIRE(path >= 0 && path <= 3, CWDM_E_INVALID, "cwdm_conv3d_set_path: path must be 0, 1, 2 or 3");
  return cwdm::g_conv_path.exchange(path);
}
