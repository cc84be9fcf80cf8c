// U-Net executor: builds the UNetModel topology of the run.sh configuration
// family (guided_diffusion/unet.py:482-725), owns the parameter
// naming contract (state_dict keys/shapes), packs weights into the kernel
// layouts and replays UNetModel.forward (unet.py:754-800) as a fixed list of
// GroupNorm-finalize and fused conv launches on one stream (struct Forward, one
// member per StepKind).
//
// build() also records the model as a list of Blocks, each of one BlockKind:
// the gradient segments of the training backward.  cwdm_unet_backward runs a
// range of them, last block first, through struct Backward, one member per kind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <cstdlib>
#include <utility>
#include <vector>

#include "internal.hpp"

using namespace cwdm;

namespace {

constexpr int64_t kAlign = 256;
inline int64_t align_up(int64_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Param { std::string name; std::vector<int64_t> shape; int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; } };

struct Tensor {
  int level, channels;
  int stats_kind = 0;  // producer of its (sum, sum^2) parts: 0 conv epilogue, 1 / 2 cwdm_haar_nd over its own /
                       // the half grid (analysis / synthesis output), 3 cwdm_skip_avg, 4 cwdm_attn_linear (one row
                       // per 16 voxels), -1 none (never GroupNorm'd)
  bool grad = true;    // the backward keeps a gradient buffer for it (false: a dropout step's output, whose
                       // gradient only passes through the scratch tmp)
};

struct GnStep {
  int src0, src1;       // tensor ids (src1 = -1 if none)
  int gamma_p, beta_p;  // param indices
  int64_t gamma_off, beta_off;
  int channels;
  int level;
  int ss_id;            // scale/shift buffer index
  int film_row = -1;    // use_scale_shift_norm, a ResBlock's out_layers.0: row offset of its emb rows [scale | shift]
                        // (folded into the scale/shift buffer by the finalize), -1: a plain GroupNorm
};

struct ConvStep {
  int a0, a1, amode, gn;        // gn = scale/shift buffer index or -1
  int w_p, b_p;                 // param indices of conv weight / bias
  int64_t w_off;                // packed weight byte offset
  int cin_a;
  int sb0, sb1;                 // 1x1 segment sources (-1 none)
  int ws_p, wsb_p;              // skip weight / bias params
  int64_t wsk_off;
  int cin_b;
  int bias_kind;                // 0 static packed bias, 1 emb-folded rows
  int64_t bias_off;             // packed byte offset (kind 0) or row offset (kind 1)
  int emb_w_p, emb_b_p;         // for kind 1: emb_layers params (pack)
  int res, rmode;
  int out;                      // tensor id, -1 = final fp32 output
  int cout;
  int level;                    // output level
  bool stats;
  int skip_conv = -1;           // conv1 of a block with a 1x1 skip: index of the block's conv2
  int64_t wsplit_off = -1;      // accurate fast mode: split-bf16 packed weights (cwdm_conv3d_pack_split), -1 none
  int64_t hsplit_off = -1;      // accurate fast mode, output head: K-expanded bf16 weights [hi | hi | lo] (head_split3_pack)
  int64_t wphase_off = -1;      // 16-bit upsampling convs: phase weights (cwdm_conv3d_pack_phase), -1 none
  int64_t xsplit_off = -1;      // accurate fast mode, small grids (level >= 2): the same for the bf16 small-grid kernel
  int64_t xsplit_sk_off = -1;   //   and for its 1x1 skip (k = 1)
  int s2 = 0;                   // stride-2 conv (Downsample.op) over a space-to-depth input: cin_a = 8 x its channels
  int cin_w = 0;                // conv_in over the staged input: the weight's own input channels (< cin_a: the packed
                                // columns past them are zero), 0: cin_a
  int w_cin() const { return cin_w ? cin_w : cin_a; }
};

struct S2dStep {  // space-to-depth of a Downsample conv's input (stride2.hip)
  int src, out, level_out, channels;
};

struct PoolStep {  // down-ResBlock pre-pass (cwdm_gn_silu_pool)
  int src, ss_id, out_h, out_x, level_out, channels;
};

struct HaarStep {  // WavUNetModel resampling / input pyramid (cwdm_haar_nd, wavelet_nd.hip)
  int src, high_in, out, high_out;  // tensor ids (-1 none)
  int inverse, all8;
  float lll_scale, high_scale;
  int emb_row;                      // emb projection row offset added after the resampling, -1 none
  bool stats;
  int level;                        // the coarse grid's level
};

// dropout of a ResBlock's out_layers (cwdm_gn_silu_dropout, dropout.hip): out = mask * SiLU(GN(src)) / (1 - p),
// the norm's scale / shift from buffer ss_id; site = the block's ordinal among the plan's ResBlocks
struct DropStep {
  int src, ss_id, out, level, channels, site;
};

struct AvgStep {  // additive skip (cwdm_skip_avg, skip_avg.hip): out = (a + b) / 2
  int a, b, out, level, channels;
};

// the bottleneck AttentionBlock (attention.hip): out = src + proj_out(attention(qkv(GroupNorm(src))))
struct AttnStep {
  int src, out, gn, level;      // tensors, the norm's scale/shift buffer
  int C, heads, ch;
  int qkv_w_p, qkv_b_p, proj_w_p, proj_b_p;                   // param indices
  int64_t qkv_w_off, qkv_b_off, proj_w_off, proj_b_off;       // packed byte offsets ([Q | K | V] row order)
  int64_t qkvT_off = -1, projT_off = -1;                      // packed_bwd: the transposed weights (input gradients)
};

enum StepKind { kGn, kConv, kPool /* pre-pass */, kS2d /* space-to-depth */, kHaar, kAvg /* additive skip */,
                kAttn /* bottleneck attention */, kDrop /* out_layers dropout */, kStage /* zero-padded input */ };
struct Step { StepKind kind; int idx; };

// what one Block is: the backward runs one function per kind (struct Backward)
enum class BlockKind {
  Res,         // ResBlock at one resolution (g1, c1, g2, c2)
  ResUp,       // ResBlock(up=True): nearest x2 of its input folded into conv1's gather and the residual
  ResDown,     // ResBlock(down=True): 2x average pool of SiLU(GN1(x)) and of x ahead of conv1 (pool)
  Downsample,  // resblock_updown=False: the stride-2 conv c1 over the space-to-depth input (s2d)
  Upsample,    // resblock_updown=False: nearest x2 + conv c1
  WavDown,     // WavUNetModel ResBlock that halves the grid by DWT after conv1 (hh, hx)
  WavUp,       // WavUNetModel ResBlock that doubles it by IDWT after conv1 (hh, hx)
  WavPyramid,  // WavUNetModel WaveletDownsample of the input pyramid's level x0: haar, then the conv c1
  Attention    // the bottleneck AttentionBlock: attn, g1 = its norm, x0 = its input
};

// resampling of a ResBlock's input, as the convs' a_mode / res_mode, the wgrad's u_mode, cwdm_resample_add
// and the GroupNorm backward's du_mode number it: 0 none, 1 nearest x2 up, 2 2x average pool down
int resample_mode(BlockKind k) { return k == BlockKind::ResUp ? 1 : (k == BlockKind::ResDown ? 2 : 0); }

// one backward segment: a ResBlock or one of the other BlockKinds, in forward order (the backward runs
// them in reverse).  Every index is -1 where the kind has no such step.
struct Block {
  BlockKind kind = BlockKind::Res;
  int g1 = -1, c1 = -1, g2 = -1, c2 = -1;  // u->gns / u->convs
  int pool = -1;                           // u->pools (ResDown)
  int drop = -1;                           // u->drops (Res / ResUp / ResDown of a plan with dropout): conv2 reads
                                           // its output, already activated, instead of h1 through g2
  int s2d = -1;                            // u->s2ds (Downsample)
  int haar = -1;                           // u->haars (WavPyramid)
  int attn = -1;                           // u->attns (Attention)
  int x0 = -1, x1 = -1;                    // input tensors (x1 = -1 unless decoder concat)
  int p_begin = 0, p_end = 0;              // parameter index range
  int emb_k = -1;                          // index into emb_rows_*
  int hh = -1, hx = -1;                    // u->haars, WavDown / WavUp: the resampling of h (+ emb) and of x (x_upd)
  int avg = -1;                            // u->avgs, additive skips: the step that produced x0 (its adjoint ends
                                           // the block's backward)
};

}  // namespace

struct CopyJob {  // dst[0:n] = a[0:n] (+ b[0:n]): the fp32 parameter copies of a pack, one launch
  float* dst;
  const float* a;
  const float* b;
  long long n, blk0;
};

struct cwdm_unet {
  cwdm_unet_config cfg;
  // device job tables of the batched packs (uploaded when the job list changes)
  cwdm::PackJob* pack_tab = nullptr;
  cwdm::PackJob* bwd_tab = nullptr;
  CopyJob* copy_tab = nullptr;
  size_t pack_cap = 0, bwd_cap = 0, copy_cap = 0;
  std::vector<cwdm::PackJob> pack_cache, bwd_cache;
  std::vector<CopyJob> copy_cache;
  int E = 0;                      // time embed dim
  std::vector<Param> params;
  std::vector<Tensor> tensors;
  std::vector<GnStep> gns;
  std::vector<ConvStep> convs;
  std::vector<PoolStep> pools;
  std::vector<S2dStep> s2ds;
  std::vector<HaarStep> haars;
  std::vector<AvgStep> avgs;
  std::vector<AttnStep> attns;
  std::vector<DropStep> drops;
  uint64_t dropout_seed = 0;      // cwdm_unet_set_dropout_seed: read when a dropout step or its backward is launched
  const int64_t* labels = nullptr;  // cwdm_unet_set_labels: device int64[B], read when the time embedding or the
                                    // table's gradient is launched (class-conditional plans)
  std::vector<Step> steps;
  struct Alias { std::string name; int owner, before; };
  std::vector<Alias> aliases;     // WavUNetModel: second state_dict name of a reused parameter; before = the
                                  // parameter index it precedes in state_dict order
  struct Trace { int tensor, level; };
  std::vector<Trace> trace;       // per topology block: its output tensor (-1 = final output) and level
  int input_tensor = -1;          // pseudo tensor for x
  int stage_tensor = -1;          // in_channels no multiple of the K chunk: x zero-padded to it (the kStage step
                                  // writes every lane on every forward), conv_in's input; -1: conv_in reads x
  int R = 0;                      // emb projection rows
  std::vector<int> emb_rows_w, emb_rows_b, emb_rows_cb;  // per res block: emb weight/bias param, conv1 bias param
                                                         // (-1: the conv bias is not folded, WavUNet up/down)
  std::vector<int> emb_rows_off, emb_rows_n;
  int te_w1, te_b1, te_w2, te_b2;
  int label_w = -1;               // label_emb.weight (num_classes > 0)
  std::vector<Block> blocks;
  int head_g = -1, head_c = -1, head_p_begin = 0;
  std::vector<int64_t> goff;      // flat gradient offset (elements) per parameter
  int64_t grad_numel = 0;
  std::vector<int64_t> dg_off, dgs_off;  // packed dgrad weights per conv (-1 none)
  int64_t packed_bwd_bytes = 0;
  std::vector<char> ginit;        // backward: gradient buffer of tensor written yet
  int64_t off_te_w1, off_te_b1, off_te_w2, off_te_b2, off_emb_w, off_emb_b;
  int64_t off_label = -1;         // the fp32 table as it stands
  int64_t packed_bytes = 0;
  int64_t split3_tmp = -1;      // fp32 staging of head_split3_pack (one region, the packs run in stream order)
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> ev;
  std::vector<double> ev_flops;
  std::vector<cwdm::ProfHook> hooks;  // per conv: the MFMA kernel launches inside it
  int ev_used = 0;

  int add_param(const std::string& n, std::vector<int64_t> s) {
    params.push_back({n, std::move(s)});
    return (int)params.size() - 1;
  }
};

namespace {

int esize(int dtype) { return dtype_size(dtype); }

void build(cwdm_unet* u) {
  const auto& c = u->cfg;
  const int mc = c.model_channels, E = 4 * mc;
  u->E = E;
  u->te_w1 = u->add_param("time_embed.0.weight", {E, mc});
  u->te_b1 = u->add_param("time_embed.0.bias", {E});
  u->te_w2 = u->add_param("time_embed.2.weight", {E, E});
  u->te_b2 = u->add_param("time_embed.2.bias", {E});
  // the reference registers label_emb between time_embed and input_blocks (unet.py:541-542)
  if (c.num_classes > 0) u->label_w = u->add_param("label_emb.weight", {c.num_classes, E});

  auto new_tensor = [&](int level, int ch) {
    u->tensors.push_back({level, ch});
    return (int)u->tensors.size() - 1;
  };
  u->input_tensor = new_tensor(0, c.in_channels);
  auto trace = [&](int tensor, int lvl) { u->trace.push_back({tensor, lvl}); };

  // WavUNetModel's decoder registers one ResBlock under two prefixes
  // (wunet.py:648-687): while alias_from is set, names under it resolve to the
  // parameter of the same suffix under alias_to instead of a new parameter
  std::string alias_from, alias_to;
  auto addp = [&](const std::string& n, std::vector<int64_t> shape) {
    if (alias_from.empty() || n.compare(0, alias_from.size(), alias_from) != 0) return u->add_param(n, std::move(shape));
    const std::string owner = alias_to + n.substr(alias_from.size());
    for (size_t i = 0; i < u->params.size(); ++i)
      if (u->params[i].name == owner) {
        u->aliases.push_back({n, (int)i, (int)u->params.size()});
        return (int)i;
      }
    return -1;  // unreachable: the owner block was built first
  };
  auto conv_params = [&](const std::string& p, int co, int ci, int k, int* wp, int* bp) {
    *wp = addp(p + ".weight", {co, ci, k, k, k});
    *bp = addp(p + ".bias", {co});
  };

  // conv_in
  int h;
  {
    ConvStep cs{};
    conv_params("input_blocks.0.0", mc, c.in_channels, 3, &cs.w_p, &cs.b_p);
    cs.a0 = u->input_tensor; cs.cin_a = c.in_channels;
    // 8 + 8x input channels on 16-channel K chunks: the conv runs over a zero-padded copy of x with zero
    // weight columns (the parameter keeps the model's shape; use_freq plans are aligned, cwdm_unet_create)
    const int ck = ck_of(c.dtype);
    if (c.in_channels % ck) {
      cs.cin_w = c.in_channels;
      cs.cin_a = (c.in_channels + ck - 1) / ck * ck;
      cs.a0 = u->stage_tensor = new_tensor(0, cs.cin_a);
      u->tensors[cs.a0].stats_kind = -1;
      u->tensors[cs.a0].grad = false;
      u->steps.push_back({kStage, 0});
    }
    cs.a1 = -1; cs.amode = 0; cs.gn = -1;
    cs.sb0 = cs.sb1 = -1; cs.ws_p = cs.wsb_p = -1; cs.cin_b = 0;
    cs.bias_kind = 0; cs.res = -1; cs.rmode = -1;
    cs.cout = mc; cs.level = 0; cs.stats = true;
    h = cs.out = new_tensor(0, mc);
    u->convs.push_back(cs);
    u->steps.push_back({kConv, (int)u->convs.size() - 1});
    trace(h, 0);
  }
  std::vector<int> stack{h};
  int level = 0;

  auto gn_step = [&](const std::string& p, int s0, int s1, int lvl) {
    GnStep g{};
    g.src0 = s0; g.src1 = s1;
    g.channels = u->tensors[s0].channels + (s1 >= 0 ? u->tensors[s1].channels : 0);
    g.gamma_p = addp(p + ".weight", {g.channels});
    g.beta_p = addp(p + ".bias", {g.channels});
    g.level = lvl;
    g.ss_id = (int)u->gns.size();
    u->gns.push_back(g);
    u->steps.push_back({kGn, g.ss_id});
    return g.ss_id;
  };

  auto haar_step = [&](const HaarStep& hs) {
    u->haars.push_back(hs);
    u->steps.push_back({kHaar, (int)u->haars.size() - 1});
  };
  auto add_emb_row = [&](Block& blk, int wp, int bp, int cbp, int n) {
    u->emb_rows_w.push_back(wp); u->emb_rows_b.push_back(bp); u->emb_rows_cb.push_back(cbp);
    blk.emb_k = (int)u->emb_rows_off.size();
    u->emb_rows_off.push_back(u->R); u->emb_rows_n.push_back(n);
    const int row = u->R;
    u->R += n;
    return row;
  };

  // ResBlock (unet.py:185-311): returns output tensor.  WavDown / WavUp: the
  // WavUNetModel ResBlock (wunet.py:210-269) that down/upsamples by DWT / IDWT
  // AFTER its first conv; skip_bands = the 7 high bands an up block inverts
  // with, *skip_out = the 7 high bands a down block returns.
  using BK = BlockKind;
  auto resblock = [&](const std::string& p, int x0, int x1, int cout, BlockKind kind, int skip_bands = -1,
                      int* skip_out = nullptr) {
    Block blk{};
    blk.p_begin = (int)u->params.size();
    blk.x0 = x0; blk.x1 = x1; blk.kind = kind;
    const int lin = u->tensors[x0].level;
    const int cin = u->tensors[x0].channels + (x1 >= 0 ? u->tensors[x1].channels : 0);
    const bool down = kind == BK::ResDown || kind == BK::WavDown, up = kind == BK::ResUp || kind == BK::WavUp;
    const int lout = down ? lin + 1 : (up ? lin - 1 : lin);
    int g1 = gn_step(p + ".in_layers.0", x0, x1, lin);
    blk.g1 = g1;
    if (kind == BK::WavDown || kind == BK::WavUp) {
      ConvStep c1{};
      conv_params(p + ".in_layers.2", cout, cin, 3, &c1.w_p, &c1.b_p);
      c1.emb_w_p = addp(p + ".emb_layers.1.weight", {cout, E});
      c1.emb_b_p = addp(p + ".emb_layers.1.bias", {cout});
      c1.a0 = x0; c1.a1 = -1; c1.amode = 0; c1.gn = g1; c1.cin_a = cin;
      c1.sb0 = c1.sb1 = -1; c1.ws_p = c1.wsb_p = -1; c1.cin_b = 0;
      c1.bias_kind = 0; c1.res = -1; c1.rmode = -1; c1.cout = cout; c1.level = lin; c1.stats = false;
      const int h1 = c1.out = new_tensor(lin, cout);
      u->tensors[h1].stats_kind = -1;
      u->convs.push_back(c1);
      blk.c1 = (int)u->convs.size() - 1;
      u->steps.push_back({kConv, blk.c1});
      const int row = add_emb_row(blk, c1.emb_w_p, c1.emb_b_p, -1, cout);
      // h: DWT -> LLL / 3 (+ the 7 high bands as the skip) or IDWT(3 h, skip); then + emb
      HaarStep hh{};
      hh.src = h1; hh.high_in = down ? -1 : skip_bands; hh.inverse = down ? 0 : 1; hh.all8 = 0;
      hh.lll_scale = down ? 1.f / 3.f : 3.f; hh.high_scale = 1.f;
      hh.out = new_tensor(lout, cout);
      u->tensors[hh.out].stats_kind = down ? 1 : 2;
      hh.high_out = -1;
      if (down) {
        hh.high_out = new_tensor(lout, 7 * cout);
        u->tensors[hh.high_out].stats_kind = -1;
      }
      hh.emb_row = row; hh.stats = true; hh.level = down ? lout : lin;
      haar_step(hh);
      blk.hh = (int)u->haars.size() - 1;
      if (skip_out) *skip_out = hh.high_out;
      // x: the same resampling, LLL only / with the same skip bands (x_upd)
      HaarStep hx = hh;
      hx.src = x0; hx.out = new_tensor(lout, cin); hx.high_out = -1; hx.emb_row = -1; hx.stats = false;
      u->tensors[hx.out].stats_kind = -1;
      haar_step(hx);
      blk.hx = (int)u->haars.size() - 1;
      const int g2 = gn_step(p + ".out_layers.0", hh.out, -1, lout);
      blk.g2 = g2;
      ConvStep c2{};
      conv_params(p + ".out_layers.3", cout, cout, 3, &c2.w_p, &c2.b_p);
      c2.a0 = hh.out; c2.a1 = -1; c2.amode = 0; c2.gn = g2; c2.cin_a = cout;
      c2.sb0 = c2.sb1 = -1; c2.ws_p = c2.wsb_p = -1; c2.cin_b = 0;
      c2.res = hx.out; c2.rmode = 0;  // up/down blocks keep the channel count (checked at create)
      c2.bias_kind = 0; c2.cout = cout; c2.level = lout; c2.stats = true;
      const int o = c2.out = new_tensor(lout, cout);
      u->convs.push_back(c2);
      blk.c2 = (int)u->convs.size() - 1;
      u->steps.push_back({kConv, blk.c2});
      blk.p_end = (int)u->params.size();
      u->blocks.push_back(blk);
      return o;
    }
    int xres = x0, xrmode = resample_mode(kind);
    int a_src = x0, a_mode = resample_mode(kind), a_gn = g1;
    if (kind == BK::ResDown) {
      // AvgPool(SiLU(GN(x))) and AvgPool(x) once, at the low resolution
      PoolStep ps{};
      ps.src = x0; ps.ss_id = g1; ps.level_out = lout; ps.channels = cin;
      ps.out_h = new_tensor(lout, cin);
      ps.out_x = new_tensor(lout, cin);
      u->pools.push_back(ps);
      u->steps.push_back({kPool, (int)u->pools.size() - 1});
      blk.pool = (int)u->pools.size() - 1;
      a_src = ps.out_h; a_mode = 0; a_gn = -1;
      xres = ps.out_x; xrmode = 0;
    }
    ConvStep c1{};
    conv_params(p + ".in_layers.2", cout, cin, 3, &c1.w_p, &c1.b_p);
    // use_scale_shift_norm (unet.py ResBlock._forward): emb_out = [scale | shift] is applied after
    // out_layers.0 (FiLM) instead of being added here, so conv1 keeps its own static bias
    const bool film = c.use_scale_shift_norm != 0;
    const int emb_n = film ? 2 * cout : cout;
    c1.emb_w_p = addp(p + ".emb_layers.1.weight", {emb_n, E});
    c1.emb_b_p = addp(p + ".emb_layers.1.bias", {emb_n});
    c1.a0 = a_src; c1.a1 = x1; c1.amode = a_mode; c1.gn = a_gn; c1.cin_a = cin;
    c1.sb0 = c1.sb1 = -1; c1.ws_p = c1.wsb_p = -1; c1.cin_b = 0;
    int film_row = -1;
    if (film) {
      c1.bias_kind = 0;
      film_row = add_emb_row(blk, c1.emb_w_p, c1.emb_b_p, -1, emb_n);
    } else {
      c1.bias_kind = 1; c1.bias_off = add_emb_row(blk, c1.emb_w_p, c1.emb_b_p, c1.b_p, cout);
    }
    c1.res = -1; c1.rmode = -1; c1.cout = cout; c1.level = lout; c1.stats = true;
    int h1 = c1.out = new_tensor(lout, cout);
    u->convs.push_back(c1);
    blk.c1 = (int)u->convs.size() - 1;
    u->steps.push_back({kConv, (int)u->convs.size() - 1});

    int g2 = gn_step(p + ".out_layers.0", h1, -1, lout);
    blk.g2 = g2;
    u->gns[g2].film_row = film_row;
    int a2 = h1, gn2 = g2;
    if (c.dropout > 0.0) {
      // Dropout(p) between out_layers' SiLU and its conv (unet.py:255-262): the finalize runs on its own, one
      // pass writes u = mask * SiLU(GN(h1)) / (1 - p), and conv2 reads u with no prologue (as conv1 reads a
      // ResDown block's pooled input)
      DropStep ds{h1, g2, new_tensor(lout, cout), lout, cout, (int)u->drops.size()};
      u->tensors[ds.out].stats_kind = -1;
      u->tensors[ds.out].grad = false;
      u->drops.push_back(ds);
      u->steps.push_back({kDrop, ds.site});
      blk.drop = ds.site;
      a2 = ds.out; gn2 = -1;
    }
    ConvStep c2{};
    conv_params(p + ".out_layers.3", cout, cout, 3, &c2.w_p, &c2.b_p);
    c2.a0 = a2; c2.a1 = -1; c2.amode = 0; c2.gn = gn2; c2.cin_a = cout;
    c2.sb0 = c2.sb1 = -1; c2.ws_p = c2.wsb_p = -1; c2.cin_b = 0;
    c2.res = -1; c2.rmode = -1;
    if (cin != cout) {
      conv_params(p + ".skip_connection", cout, cin, 1, &c2.ws_p, &c2.wsb_p);
      c2.sb0 = x0; c2.sb1 = x1; c2.cin_b = cin;
      u->convs[blk.c1].skip_conv = (int)u->convs.size();  // c2's index once pushed below
    } else {
      c2.res = xres;
      c2.rmode = xrmode;
    }
    c2.bias_kind = 0; c2.cout = cout; c2.level = lout; c2.stats = true;
    int o = c2.out = new_tensor(lout, cout);
    u->convs.push_back(c2);
    u->steps.push_back({kConv, (int)u->convs.size() - 1});
    blk.c2 = (int)u->convs.size() - 1;
    blk.p_end = (int)u->params.size();
    u->blocks.push_back(blk);
    return o;
  };

  // resblock_updown=False: Downsample(use_conv=True) = a stride-2 conv, run as
  // a stride-1 conv over the space-to-depth input; Upsample(use_conv=True) =
  // nearest x2 folded into the conv's gather (a_mode 1).  unet.py:40-100, :606-612, :700-706.
  auto resample_layer = [&](const std::string& p, int x, int down) {
    Block blk{};
    blk.p_begin = (int)u->params.size();
    blk.x0 = x; blk.kind = down ? BK::Downsample : BK::Upsample;
    const int lin = u->tensors[x].level, chn = u->tensors[x].channels;
    const int lout = down ? lin + 1 : lin - 1;
    ConvStep cs{};
    conv_params(p, chn, chn, 3, &cs.w_p, &cs.b_p);
    cs.a1 = -1; cs.gn = -1; cs.sb0 = cs.sb1 = -1; cs.ws_p = cs.wsb_p = -1; cs.cin_b = 0;
    cs.bias_kind = 0; cs.res = -1; cs.rmode = -1; cs.cout = chn; cs.level = lout; cs.stats = true;
    if (down) {
      S2dStep sd{x, new_tensor(lout, 8 * chn), lout, chn};
      u->s2ds.push_back(sd);
      u->steps.push_back({kS2d, (int)u->s2ds.size() - 1});
      blk.s2d = (int)u->s2ds.size() - 1;
      cs.a0 = sd.out; cs.amode = 0; cs.cin_a = 8 * chn; cs.s2 = 1;
    } else {
      cs.a0 = x; cs.amode = 1; cs.cin_a = chn;
    }
    const int o = cs.out = new_tensor(lout, chn);
    u->convs.push_back(cs);
    u->steps.push_back({kConv, (int)u->convs.size() - 1});
    blk.c1 = (int)u->convs.size() - 1;
    blk.p_end = (int)u->params.size();
    u->blocks.push_back(blk);
    return o;
  };

  int ch = mc, idx = 1;
  const int nl = c.num_levels;
  if (c.use_freq) {
    // WavUNetModel (wunet.py:470-700, forward :754-795): every level ends in a
    // DWT ResBlock and a WaveletDownsample of the input pyramid; the decoder
    // has no concatenation, only the high-band skips into its IDWT ResBlocks
    std::vector<int> skips;
    int pyr = u->input_tensor;
    for (int l = 0; l < nl; ++l) {
      const int mult = c.channel_mult[l];
      for (int r = 0; r < c.num_res_blocks; ++r) {
        h = resblock("input_blocks." + std::to_string(idx) + ".0", h, -1, mult * mc, BK::Res);
        ch = mult * mc;
        trace(h, level);
        ++idx;
      }
      int sk = -1;
      h = resblock("input_blocks." + std::to_string(idx) + ".0", h, -1, ch, BK::WavDown, -1, &sk);
      skips.push_back(sk);
      ++level;
      trace(h, level);
      // WaveletDownsample (:131-145): conv(cat(8 bands) / 3) + h
      const int cp = u->tensors[pyr].channels;
      HaarStep hp{};
      hp.src = pyr; hp.high_in = -1; hp.high_out = -1; hp.inverse = 0; hp.all8 = 1;
      hp.lll_scale = hp.high_scale = 1.f / 3.f; hp.emb_row = -1; hp.stats = false; hp.level = level;
      hp.out = new_tensor(level, 8 * cp);
      u->tensors[hp.out].stats_kind = -1;
      haar_step(hp);
      Block pb{};   // the WaveletDownsample as a backward segment of its own
      pb.kind = BK::WavPyramid; pb.haar = (int)u->haars.size() - 1; pb.x0 = pyr;
      pb.p_begin = (int)u->params.size();
      ConvStep cs{};
      conv_params("input_blocks." + std::to_string(idx + 1) + ".0.conv", ch, 8 * cp, 3, &cs.w_p, &cs.b_p);
      cs.a0 = hp.out; cs.a1 = -1; cs.amode = 0; cs.gn = -1; cs.cin_a = 8 * cp;
      cs.sb0 = cs.sb1 = -1; cs.ws_p = cs.wsb_p = -1; cs.cin_b = 0;
      cs.bias_kind = 0; cs.res = h; cs.rmode = 0; cs.cout = ch; cs.level = level; cs.stats = true;
      h = pyr = cs.out = new_tensor(level, ch);
      u->convs.push_back(cs);
      u->steps.push_back({kConv, (int)u->convs.size() - 1});
      pb.c1 = (int)u->convs.size() - 1;
      pb.p_end = (int)u->params.size();
      u->blocks.push_back(pb);
      trace(h, level);
      idx += 2;
    }
    h = resblock("middle_block.0", h, -1, ch, BK::Res);
    trace(h, level);
    h = resblock("middle_block.1", h, -1, ch, BK::Res);
    trace(h, level);
    idx = 0;
    for (int l = nl - 1; l >= 0; --l) {
      const int mult = c.channel_mult[l];
      const int sk = skips.back();  // popped by the level's first output block (hs.pop() skips the Nones)
      skips.pop_back();
      std::string owner;
      for (int i = 0; i <= c.num_res_blocks; ++i) {
        const std::string p = "output_blocks." + std::to_string(idx);
        if (i != c.num_res_blocks) {
          h = resblock(p + ".0", h, -1, mc * mult, BK::Res);
          ch = mc * mult;
          owner = p + ".0";
        } else {
          // Sequential(<the level's last ResBlock again>, IDWT ResBlock)
          alias_from = p + ".0.";
          alias_to = owner + ".";
          h = resblock(p + ".0", h, -1, ch, BK::Res);
          alias_from.clear();
          h = resblock(p + ".1", h, -1, ch, BK::WavUp, sk);
          --level;
        }
        trace(h, level);
        ++idx;
      }
    }
    for (int i = 0; i < c.num_res_blocks; ++i) {
      h = resblock("out_res." + std::to_string(i) + ".0", h, -1, ch, BK::Res);
      trace(h, level);
    }
  }
  for (int l = 0; l < nl && !c.use_freq; ++l) {
    const int mult = c.channel_mult[l];
    for (int r = 0; r < c.num_res_blocks; ++r) {
      h = resblock("input_blocks." + std::to_string(idx) + ".0", h, -1, mult * mc, BK::Res);
      ch = mult * mc;
      stack.push_back(h);
      trace(h, level);
      ++idx;
    }
    if (l != nl - 1) {
      const std::string p = "input_blocks." + std::to_string(idx) + ".0";
      h = c.resblock_updown ? resblock(p, h, -1, ch, BK::ResDown) : resample_layer(p + ".op", h, 1);
      ++level;
      stack.push_back(h);
      trace(h, level);
      ++idx;
    }
  }
  if (!c.use_freq) {
    h = resblock("middle_block.0", h, -1, ch, BK::Res);
    trace(h, level);
    if (c.bottleneck_attention) {
      // AttentionBlock (unet.py:314-360): norm, qkv, proj_out in state_dict order; the ResBlock after it
      // is then middle_block.2
      Block blk{};
      blk.p_begin = (int)u->params.size();
      blk.x0 = h; blk.kind = BK::Attention;
      AttnStep at{};
      at.src = h; at.level = level; at.C = ch;
      at.heads = c.num_head_channels > 0 ? ch / c.num_head_channels : std::max(c.num_heads, 1);
      at.ch = ch / at.heads;
      blk.g1 = at.gn = gn_step("middle_block.1.norm", h, -1, level);
      at.qkv_w_p = addp("middle_block.1.qkv.weight", {3 * ch, ch, 1});
      at.qkv_b_p = addp("middle_block.1.qkv.bias", {3 * ch});
      at.proj_w_p = addp("middle_block.1.proj_out.weight", {ch, ch, 1});
      at.proj_b_p = addp("middle_block.1.proj_out.bias", {ch});
      h = at.out = new_tensor(level, ch);
      u->tensors[h].stats_kind = 4;
      u->attns.push_back(at);
      u->steps.push_back({kAttn, (int)u->attns.size() - 1});
      blk.attn = (int)u->attns.size() - 1;
      blk.p_end = (int)u->params.size();
      u->blocks.push_back(blk);
      trace(h, level);
    }
    h = resblock(c.bottleneck_attention ? "middle_block.2" : "middle_block.1", h, -1, ch, BK::Res);
    trace(h, level);
    idx = 0;
  }
  for (int l = nl - 1; l >= 0 && !c.use_freq; --l) {
    const int mult = c.channel_mult[l];
    for (int i = 0; i <= c.num_res_blocks; ++i) {
      int skip = stack.back();
      stack.pop_back();
      if (c.additive_skips) {
        // h = (h + skip) / 2, then an ordinary single-source ResBlock to the channels of the next
        // skip left on the stack (unet.py:664-666), so h always matches the skip it is averaged with
        AvgStep as{h, skip, -1, level, u->tensors[skip].channels};
        as.out = new_tensor(level, as.channels);
        u->tensors[as.out].stats_kind = 3;
        u->avgs.push_back(as);
        u->steps.push_back({kAvg, (int)u->avgs.size() - 1});
        ch = stack.empty() ? mc : u->tensors[stack.back()].channels;
        h = resblock("output_blocks." + std::to_string(idx) + ".0", as.out, -1, ch, BK::Res);
        u->blocks.back().avg = (int)u->avgs.size() - 1;
      } else {
        h = resblock("output_blocks." + std::to_string(idx) + ".0", h, skip, mc * mult, BK::Res);
        ch = mc * mult;
      }
      trace(h, level);
      if (l && i == c.num_res_blocks) {
        const std::string p = "output_blocks." + std::to_string(idx) + ".1";
        h = c.resblock_updown ? resblock(p, h, -1, ch, BK::ResUp) : resample_layer(p + ".conv", h, 0);
        --level;
        trace(h, level);
      }
      ++idx;
    }
  }
  // out head
  u->head_p_begin = (int)u->params.size();
  int g = gn_step("out.0", h, -1, 0);
  u->head_g = g;
  ConvStep co{};
  conv_params("out.2", c.out_channels, ch, 3, &co.w_p, &co.b_p);
  co.a0 = h; co.a1 = -1; co.amode = 0; co.gn = g; co.cin_a = ch;
  co.sb0 = co.sb1 = -1; co.ws_p = co.wsb_p = -1; co.cin_b = 0;
  co.bias_kind = 0; co.res = -1; co.rmode = -1; co.cout = c.out_channels; co.level = 0; co.stats = false;
  co.out = -1;
  u->convs.push_back(co);
  u->head_c = (int)u->convs.size() - 1;
  u->steps.push_back({kConv, (int)u->convs.size() - 1});
  trace(-1, 0);

  // packed layout
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off = align_up(off + bytes); return o; };
  u->off_te_w1 = take(u->params[u->te_w1].numel() * 4);
  u->off_te_b1 = take(u->params[u->te_b1].numel() * 4);
  u->off_te_w2 = take(u->params[u->te_w2].numel() * 4);
  u->off_te_b2 = take(u->params[u->te_b2].numel() * 4);
  if (u->label_w >= 0) u->off_label = take(u->params[u->label_w].numel() * 4);
  u->off_emb_w = take((int64_t)u->R * E * 4);
  u->off_emb_b = take((int64_t)u->R * 4);
  int64_t split3_max = 0;
  for (auto& cs : u->convs) {
    cs.w_off = take(cwdm_conv3d_packed_bytes(cs.cout, cs.cin_a, 3, c.dtype));
    if (c.mfma_split && c.dtype == CWDM_F32 && !cs.s2 && cs.cout % 64 == 0 && cs.cin_a % 16 == 0)
      cs.wsplit_off = take(cwdm_conv3d_packed_split_bytes(cs.cout, cs.cin_a));
    // an upsampling conv's phase weights, by the channel rule (whether a forward's grid takes the
    // phase path is decided per launch: cwdm_conv3d_desc.a_w_phase)
    if (dtype_half(c.dtype) && cs.amode == 1 && !cs.s2 && cs.ws_p < 0 && cs.rmode == -1 && cs.cout % 64 == 0 &&
        cs.cin_a % 16 == 0 && cs.cin_a >= 32)
      cs.wphase_off = take(cwdm_conv3d_packed_phase_bytes(cs.cout, cs.cin_a, c.dtype));
    if (c.mfma_split && c.dtype == CWDM_F32 && &cs == &u->convs[u->head_c] && cs.a1 < 0 && cs.amode == 0 &&
        cs.gn >= 0 && cs.cout <= 16 && cs.cin_a % 32 == 0 && 3 * cs.cin_a <= 256) {
      cs.hsplit_off = take(cwdm_conv3d_packed_bytes(cs.cout, 3 * cs.cin_a, 3, CWDM_BF16));
      split3_max = std::max(split3_max, (int64_t)3 * cs.cout * cs.cin_a * 27 * 4);
    }
    // the small grids' K-expanded split convs (unet_forward_impl, xsg_plan): every 3x3x3 conv
    // that can land on a grid below the wide kernels' minimum width
    if (c.mfma_split && c.dtype == CWDM_F32 && !cs.s2 && cs.level >= 2 && cs.amode <= 1 &&
        cs.cout % 64 == 0 && cs.cin_a % 32 == 0) {
      cs.xsplit_off = take(cwdm_conv3d_packed_bytes(cs.cout, 3 * cs.cin_a, 3, CWDM_BF16));
      split3_max = std::max(split3_max, (int64_t)3 * cs.cout * cs.cin_a * 27 * 4);
      if (cs.ws_p >= 0 && cs.cin_b % 32 == 0) {
        cs.xsplit_sk_off = take(cwdm_conv3d_packed_bytes(cs.cout, 3 * cs.cin_b, 1, CWDM_BF16));
        split3_max = std::max(split3_max, (int64_t)3 * cs.cout * cs.cin_b * 4);
      }
    }
    if (cs.ws_p >= 0) cs.wsk_off = take(cwdm_conv3d_packed_bytes(cs.cout, cs.cin_b, 1, c.dtype));
    if (cs.bias_kind == 0) cs.bias_off = take((int64_t)cs.cout * 4);
  }
  for (auto& gs : u->gns) {
    gs.gamma_off = take((int64_t)gs.channels * 4);
    gs.beta_off = take((int64_t)gs.channels * 4);
  }
  const int64_t es_w = dtype_size(c.dtype);
  for (auto& at : u->attns) {
    at.qkv_w_off = take((int64_t)3 * at.C * at.C * es_w);
    at.qkv_b_off = take((int64_t)3 * at.C * 4);
    at.proj_w_off = take((int64_t)at.C * at.C * es_w);
    at.proj_b_off = take((int64_t)at.C * 4);
  }
  if (split3_max > 0) u->split3_tmp = take(split3_max);
  u->packed_bytes = off;

  // flat gradient layout (state_dict order, contiguous)
  int64_t go = 0;
  for (const auto& pr : u->params) { u->goff.push_back(go); go += pr.numel(); }
  u->grad_numel = go;
  // packed dgrad weights (every conv but conv_in, whose input needs no gradient)
  const int ck = ck_of(c.dtype);
  int64_t bo = 0;
  auto takeb = [&](int64_t bytes) { int64_t o = bo; bo = align_up(bo + bytes); return o; };
  for (size_t i = 0; i < u->convs.size(); ++i) {
    const auto& cs = u->convs[i];
    const int cpad = (int)((cs.cout + ck - 1) / ck * ck);
    u->dg_off.push_back(i == 0 ? -1 : takeb(cwdm_conv3d_packed_bytes(cs.cin_a, cpad, 3, c.dtype)));
    u->dgs_off.push_back(cs.ws_p >= 0 ? takeb(cwdm_conv3d_packed_bytes(cs.cin_b, cpad, 1, c.dtype)) : -1);
  }
  for (auto& at : u->attns) {
    at.qkvT_off = takeb((int64_t)3 * at.C * at.C * es_w);
    at.projT_off = takeb((int64_t)at.C * at.C * es_w);
  }
  u->packed_bwd_bytes = bo;
}

// shape-only descriptor of one conv step (pointers filled in by Forward::conv_desc)
cwdm_conv3d_desc conv_shape(const cwdm_unet* u, const ConvStep& cs, int64_t B, int64_t D, int64_t H, int64_t W) {
  cwdm_conv3d_desc d{};
  d.dtype = u->cfg.dtype;
  d.B = B; d.D = D >> cs.level; d.H = H >> cs.level; d.W = W >> cs.level;
  d.cout = cs.cout;
  d.a_c0 = u->tensors[cs.a0].channels;
  d.a_c1 = cs.a1 >= 0 ? u->tensors[cs.a1].channels : 0;
  d.a_mode = cs.amode;
  // presence flags only: they select the kernel path and size its workspace
  // (the DMA-staged kernel needs room for the GroupNorm+SiLU'd input and the skip)
  d.a_w = reinterpret_cast<const void*>(1);
  if (cs.gn >= 0) d.a_gn = reinterpret_cast<const float*>(1);
  if (cs.ws_p >= 0) {
    d.b_c0 = u->tensors[cs.sb0].channels;
    d.b_c1 = cs.sb1 >= 0 ? u->tensors[cs.sb1].channels : 0;
    d.b_w = reinterpret_cast<const void*>(1);  // presence flag only
  }
  d.res_mode = cs.rmode;
  d.out_dtype = cs.out < 0 ? CWDM_F32 : u->cfg.dtype;
  if (cs.wsplit_off >= 0) d.a_w_split = reinterpret_cast<const void*>(1);   // presence flags only
  if (cs.wphase_off >= 0) d.a_w_phase = reinterpret_cast<const void*>(1);
  return d;
}
// voxels per batch of such a conv's source grid: half the output's edges under the nearest x2 gather (a_mode 1)
int64_t src_voxels(const cwdm_conv3d_desc& d) {
  return d.a_mode == 1 ? (d.D / 2) * (d.H / 2) * (d.W / 2) : d.D * d.H * d.W;
}
// the 1x1 skip of conv d alone, as an fp32 product: no 3x3x3 operand, bias, statistics or residual
// (not cwdm::skip_desc, which keeps the residual and the conv's output dtype)
cwdm_conv3d_desc skip_only_desc(const cwdm_conv3d_desc& d) {
  cwdm_conv3d_desc k = d;
  k.a0 = k.a1 = nullptr; k.a_c0 = k.a_c1 = 0; k.a_gn = nullptr; k.a_w = nullptr; k.a_mode = 0;
  k.bias = nullptr; k.bias_bstride = 0; k.stats = nullptr; k.res = nullptr; k.res_mode = -1;
  k.out_dtype = CWDM_F32;
  return k;
}

// the accurate fast mode on a small grid: the fp32 conv d (GroupNorm+SiLU'd or plain input, optional 1x1
// skip) as ONE bf16 small-grid conv over the K-expanded split input [hi | lo | hi] of SiLU(GN(x))
// (cwdm::split3_prep, chunk-major) against the weights [hi | hi | lo] (cs.xsplit_off): the three
// products hi.hi + lo.hi + hi.lo of the split kernels, fp32 output and residual.  The 1x1 skip,
// if any, runs first into an fp32 residual buffer: the same K expansion on the small-grid kernel's
// 1x1 form (channels-last split of the raw input, cs.xsplit_sk_off), else pw_split.
// Workspace: x3 (the conv's or the skip's split input) | skip | K-split slices.
struct XsgPlan {
  bool ok = false;
  bool sk_sg = false;        // the skip on the small-grid kernel (sk_ksplit: its K split)
  bool sk_pw_split = false;  // else: on pw_split (false: through cwdm::conv3d_forward)
  int sk_ksplit = 1;
  cwdm_conv3d_desc e{};      // the bf16 desc (pointers filled in by the forward)
  cwdm_conv3d_desc ek{};     //   and the skip's
  cwdm::ConvRoute er;        // the route of e's launch: the small-grid kernel and its K split
  int64_t x3_bytes = 0, skip_bytes = 0, total = 0;
};
XsgPlan xsg_plan(const ConvStep& cs, const cwdm_conv3d_desc& d) {
  XsgPlan x;
  if (cs.xsplit_off < 0 || d.res_mode > 1 || (d.b_w && d.res_mode >= 0)) return x;
  const int C = d.a_c0 + d.a_c1;
  cwdm_conv3d_desc e = d;
  e.dtype = CWDM_BF16;
  e.a_c0 = 3 * C; e.a_c1 = 0; e.a_gn = nullptr; e.a_w_split = nullptr;
  e.b_c0 = e.b_c1 = 0; e.b_w = nullptr;
  if (d.b_w) e.res_mode = 0;
  e.out_dtype = CWDM_F32;
  // (the forward runs these convs with ConvCall::fp32x set)
  cwdm::ConvCall cx;
  cx.fp32x = true;
  x.er = cwdm::conv_route_prepared(&e, e.res_mode, cx);
  if (x.er.kernel != cwdm::ConvKernel::SmallGrid) return x;
  x.e = e;
  x.x3_bytes = align_up(d.B * src_voxels(d) * 3 * C * 2);
  x.skip_bytes = d.b_w ? align_up(d.B * d.D * d.H * d.W * d.cout * 4) : 0;
  // a K-split slice holds the grid's whole 256-voxel statistics bricks
  const int64_t slice = d.B * cwdm_conv3d_parts(e.dtype, d.D, d.H, d.W, d.cout) * 256 * d.cout * 4;
  int64_t part = x.er.ksplit > 1 ? x.er.ksplit * slice : 0;
  if (d.b_w) {
    // the skip alone: K-expanded on the small-grid kernel's 1x1 form where its weights were packed, else as fp32
    cwdm_conv3d_desc k = skip_only_desc(d);
    x.sk_pw_split = cwdm::conv_route_skip(&k, cx).skip == cwdm::SkipKernel::PwSplit;
    k.dtype = CWDM_BF16;
    k.a_w_split = nullptr;
    k.b_c0 = 3 * (d.b_c0 + d.b_c1); k.b_c1 = 0; k.b1 = nullptr;
    const cwdm::ConvRoute kr = cwdm::conv_route_skip(&k, cx);
    if (cs.xsplit_sk_off >= 0 && kr.skip == cwdm::SkipKernel::SmallGrid) {
      x.sk_sg = true;
      x.sk_ksplit = kr.skip_ksplit;
      x.ek = k;
      x.x3_bytes = std::max(x.x3_bytes, align_up(d.B * d.D * d.H * d.W * k.b_c0 * 2));
      if (kr.skip_ksplit > 1) part = std::max(part, kr.skip_ksplit * slice);
    }
  }
  x.total = x.x3_bytes + x.skip_bytes + part;
  x.ok = true;
  return x;
}

// how the forward runs one conv step, decided in layout(); Forward::conv dispatches to the member named here
enum class ConvKind {
  Plain,       // conv_plain: cwdm::conv3d_forward with the plan's context
  SkipPass,    // conv_skip_pass: conv1 of a skip block behind the fused GroupNorm + 1x1-skip pass (cwdm::gn_apply_skip)
  SkipTaken,   // conv2 of that block: its skip product came from conv1's pass, so conv() rewrites the desc to a
               // plain residual and runs conv_plain
  HeadSplit,   // conv_head_split: the accurate fast mode's head over the K-expanded split input
  Xsg          // conv_xsg: the accurate fast mode on a small grid (XsgPlan)
};
struct ConvPlan {
  cwdm::ConvRoute route;   // of the conv's shape in the plan's context, nothing offered
  cwdm::ConvRoute pass;    // SkipPass: of the launch on the pass's activated copy
  // with an inference-sized workspace / a training-sized one (which keeps the activated inputs)
  ConvKind kind = ConvKind::Plain, kind_keep = ConvKind::Plain;
  int xsg = -1;            // Xsg: its XsgPlan in Layout::xsg
};

struct Layout {
  int64_t temb, ebias, split, split_bytes, sync;
  int64_t skipbuf = 0;          // conv2 residual written by the fused GroupNorm + 1x1-skip pass
  std::vector<ConvPlan> conv;   // per conv step
  std::vector<XsgPlan> xsg;     // of the convs the accurate fast mode can rearrange on a small grid
  std::vector<int64_t> t_off, s_off, s_parts;
  std::vector<int64_t> ss_off, mr_off;
  int64_t total;
  // training: the activated input (GroupNorm+SiLU, chunk-major) of every conv
  // whose forward pre-pass writes one, kept past the inference total for the
  // DMA-staged wgrad (cwdm_unet_train_workspace_bytes); -1 = not kept
  std::vector<int64_t> keep_off;
  // the attention block: its qkv projection (B, T, 3 C) and attention output (B, T, C); a training-sized
  // workspace also keeps the rows' log-sum-exp (fp32 [B][heads][T]) and the normalised input (B, T, C)
  int64_t attn_qkv = -1, attn_a = -1, attn_L = -1, attn_n = -1;
  int64_t train_total;
};

// what both passes read of one call (the base of struct Forward and struct Backward): the plan, the layout
// of the forward's workspace for the call's grid, the base pointers, and the lookups over them
struct PlanView {
  cwdm_unet* u;
  const Layout& L;
  const unsigned char* pk;   // packed parameters (forward form)
  unsigned char* wb;         // the forward's workspace (the backward only reads it)
  const void* x;             // the model input
  int64_t B, D, H, W;
  cwdm_stream_t stream;
  // derived from the above
  hipStream_t s = (hipStream_t)stream;
  int dt = u->cfg.dtype;

  const float* P(int64_t off) const { return reinterpret_cast<const float*>(pk + off); }
  const void* act(int id) const { return id < 0 ? nullptr : (id == u->input_tensor ? x : wb + L.t_off[id]); }
  int nch(int id) const { return id < 0 ? 0 : u->tensors[id].channels; }
  int64_t vox(int lv) const { return (D >> lv) * (H >> lv) * (W >> lv); }
  const float* ss_of(int g) const { return reinterpret_cast<const float*>(wb + L.ss_off[g]); }
  const float* mr_of(int g) const { return reinterpret_cast<const float*>(wb + L.mr_off[g]); }
};

// statistics partial rows per tensor: the per-tile layout, or the rows of a warp-specialised conv
// that summed them per workgroup (ConvCall::stats_rows; env CWDM_STATS_WG=0: per tile everywhere)
bool plan_stats_wg() {
  static const bool on = env_not0("CWDM_STATS_WG");
  return on;
}

Layout layout(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  Layout L;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off = align_up(off + bytes); return o; };
  L.sync = take(cwdm::plan_sync_bytes());   // first: a memset block at a 256-byte boundary
  L.temb = take(B * u->E * 4);
  L.ebias = take(B * (int64_t)u->R * 4);
  const int es = esize(u->cfg.dtype);
  for (size_t i = 0; i < u->tensors.size(); ++i) {
    const auto& t = u->tensors[i];
    const int64_t d = D >> t.level, h = H >> t.level, w = W >> t.level;
    if ((int)i == u->input_tensor) {
      L.t_off.push_back(-1); L.s_off.push_back(-1); L.s_parts.push_back(0);
      continue;
    }
    L.t_off.push_back(take(B * d * h * w * t.channels * es));
    const int64_t parts = t.stats_kind < 0    ? 0
                          : t.stats_kind == 1 ? cwdm_haar_nd_parts(d, h, w)
                          : t.stats_kind == 2 ? cwdm_haar_nd_parts(d / 2, h / 2, w / 2)
                          : t.stats_kind == 3 ? cwdm_skip_avg_parts(d * h * w)
                          : t.stats_kind == 4 ? cwdm::attn_parts(d * h * w)
                                              : cwdm_conv3d_parts(u->cfg.dtype, d, h, w, t.channels);
    L.s_parts.push_back(parts);
    L.s_off.push_back(take(B * parts * t.channels * 2 * 4));
  }
  for (const auto& g : u->gns) L.ss_off.push_back(take(B * (int64_t)g.channels * 2 * 4));
  for (size_t i = 0; i < u->gns.size(); ++i) L.mr_off.push_back(take(B * (int64_t)u->cfg.num_groups * 2 * 4));
  // every conv's route, once: what the forward runs and what the regions below are sized for
  const size_t nc = u->convs.size();
  L.conv.resize(nc);
  cwdm::ConvCall lc;
  lc.stats_wg = plan_stats_wg();
  int64_t split = 0;
  for (size_t i = 0; i < nc; ++i) {
    const auto& cs = u->convs[i];
    const cwdm_conv3d_desc d = conv_shape(u, cs, B, D, H, W);
    ConvPlan& cp = L.conv[i];
    cp.route = cwdm::conv_route(&d, lc);
    split = std::max(split, cwdm::conv_workspace_bytes(&d, cp.route));
    if (cs.xsplit_off < 0) continue;
    const XsgPlan xp = xsg_plan(cs, d);
    if (!xp.ok) continue;
    split = std::max(split, xp.total);
    cp.xsg = (int)L.xsg.size();
    L.xsg.push_back(xp);
  }
  L.split_bytes = split;
  L.split = take(split);
  // ResBlocks with a 1x1 skip whose convs run on the DMA kernel: GN1 and the
  // skip read x in one pass (cwdm::gn_apply_skip).  A conv1 that applies GroupNorm
  // in its own LDS (conv3d_v5, inference) reads x raw: the pass would only write an
  // activated copy nobody reads; conv2 then runs the 1x1 skip itself
  int64_t skipb = 0;
  const bool fuse = env_not0("CWDM_SKIP_FUSE");  // "0": A/B switch for the fused pass (read per plan)
  for (size_t i = 0; fuse && i < nc; ++i) {
    const auto& c1 = u->convs[i];
    if (c1.skip_conv < 0 || c1.gn < 0 || c1.amode != 0) continue;
    const auto& c2 = u->convs[c1.skip_conv];
    const cwdm_conv3d_desc d1 = conv_shape(u, c1, B, D, H, W);
    const int64_t vpb = d1.D * d1.H * d1.W;
    ConvPlan& cp = L.conv[i];
    if (!cp.route.v4_ok || !L.conv[c1.skip_conv].route.v4_ok ||
        !cwdm::apply_skip_ok(u->cfg.dtype, c1.cin_a, c2.cout, B, vpb))
      continue;
    cp.kind_keep = ConvKind::SkipPass;
    if (!cp.route.gn_in_lds()) cp.kind = ConvKind::SkipPass;
    cp.pass = cwdm::conv_route_prepared(&d1, d1.res_mode, lc);
    skipb = std::max(skipb, B * vpb * c2.cout * es);
  }
  L.skipbuf = take(skipb);
  for (const auto& at : u->attns) {
    const int64_t T = (D >> at.level) * (H >> at.level) * (W >> at.level);
    L.attn_qkv = take(B * T * 3 * at.C * es);
    L.attn_a = take(B * T * at.C * es);
  }
  for (size_t i = 0; i < nc; ++i) {
    const auto& cs = u->convs[i];
    ConvPlan& cp = L.conv[i];
    if (cp.kind_keep == ConvKind::SkipPass) continue;
    const bool after_c1 = cs.ws_p >= 0 && i > 0 && u->convs[i - 1].skip_conv == (int)i;
    if (after_c1 && L.conv[i - 1].kind_keep == ConvKind::SkipPass) cp.kind_keep = ConvKind::SkipTaken;
    // (the accurate fast mode's rearranged convs: inference only, and never a conv2 of a fused pass --
    // that pass needs the wide grids, these the output head and the small ones)
    const cwdm_conv3d_desc d = conv_shape(u, cs, B, D, H, W);
    if (after_c1 && L.conv[i - 1].kind == ConvKind::SkipPass) cp.kind = ConvKind::SkipTaken;
    else if (cs.hsplit_off >= 0 && cs.gn >= 0 && B * d.D * d.H * d.W * 3 * d.a_c0 * 2 <= split) cp.kind = ConvKind::HeadSplit;
    else if (cp.xsg >= 0 && L.xsg[cp.xsg].total <= split) cp.kind = ConvKind::Xsg;
  }
  L.total = off;
  L.keep_off.assign(nc, -1);
  for (size_t i = 0; i < nc; ++i) {
    const auto& cs = u->convs[i];
    if (!dtype_half(u->cfg.dtype) || cs.gn < 0 || cs.amode > 1 || cs.s2 || !L.conv[i].route.v4_ok) continue;
    const cwdm_conv3d_desc d = conv_shape(u, cs, B, D, H, W);
    const int64_t sv = src_voxels(d), cin = d.a_c0 + d.a_c1;
    if (sv * cin * 2 >= (1LL << 31)) continue;  // the DMA wgrad's per-batch buffer range
    L.keep_off[i] = take(B * sv * cin * es);
  }
  for (const auto& at : u->attns) {
    const int64_t T = (D >> at.level) * (H >> at.level) * (W >> at.level);
    L.attn_L = take(B * at.heads * T * 4);
    L.attn_n = take(B * T * at.C * es);
  }
  L.train_total = off;
  return L;
}

}  // namespace

namespace cwdm {
namespace {
__global__ void __launch_bounds__(256) copy_batch_kernel(const CopyJob* __restrict__ jobs, int njobs) {
  const long long bid = blockIdx.x;
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= bid) lo = mid;
    else hi = mid - 1;
  }
  const CopyJob j = jobs[lo];
  const long long base = (bid - j.blk0) * 1024;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // 4 independent gathers in flight per thread
    const long long i = base + k * 256 + threadIdx.x;
    if (i < j.n) j.dst[i] = j.b ? j.a[i] + j.b[i] : j.a[i];
  }
}

__global__ void vec_add_kernel(const float* a, const float* b, float* o, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}
}  // namespace
int launch_vec_add(const float* a, const float* b, float* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(vec_add_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, a, b, out, n);
  CWDM_LAUNCHED();
  return CWDM_OK;
}
}  // namespace cwdm

extern "C" int cwdm_unet_create(const cwdm_unet_config* cfg, cwdm_unet** plan) {
  CWDM_REQUIRE(cfg && plan, CWDM_E_INVALID, "cwdm_unet_create: null pointer");
  CWDM_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 8, CWDM_E_INVALID, "cwdm_unet_create: 1..8 levels");
  CWDM_REQUIRE(cfg->model_channels > 0 && cfg->in_channels > 0 && cfg->out_channels > 0 && cfg->num_res_blocks >= 1,
               CWDM_E_INVALID, "cwdm_unet_create: bad channel config");
  CWDM_REQUIRE(dtype_compute(cfg->dtype), CWDM_E_INVALID, "cwdm_unet_create: bad dtype");
  CWDM_REQUIRE(cfg->num_groups > 0, CWDM_E_INVALID, "cwdm_unet_create: bad num_groups");
  const int ck = ck_of(cfg->dtype);
  // 8 wavelet channels per volume (the image and each condition); a UNetModel plan pads them to the K chunk
  // itself (stage_tensor), WavUNetModel's pyramid reads the input tensor as it is
  CWDM_REQUIRE(cfg->in_channels % 8 == 0, CWDM_E_UNSUPPORTED, "cwdm_unet_create: in_channels must be a multiple of 8");
  CWDM_REQUIRE(!cfg->use_freq || cfg->in_channels % ck == 0, CWDM_E_UNSUPPORTED,
               "cwdm_unet_create: use_freq: in_channels must be a multiple of " + std::to_string(ck));
  for (int l = 0; l < cfg->num_levels; ++l) {
    const int ch = cfg->channel_mult[l] * cfg->model_channels;
    CWDM_REQUIRE(ch > 0 && ch % ck == 0 && (ch % 64 == 0 || ch % 32 == 0), CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: level channels must be multiples of 32 (and of the chunk)");
    CWDM_REQUIRE(ch % cfg->num_groups == 0, CWDM_E_INVALID, "cwdm_unet_create: channels not divisible by groups");
  }
  CWDM_REQUIRE(!(cfg->additive_skips && cfg->use_freq), CWDM_E_UNSUPPORTED,
               "cwdm_unet_create: additive_skips with use_freq (WavUNetModel has no concatenation to replace)");
  CWDM_REQUIRE(!(cfg->use_scale_shift_norm && cfg->use_freq), CWDM_E_UNSUPPORTED,
               "cwdm_unet_create: use_scale_shift_norm with use_freq (WavUNetModel's ResBlocks are not covered)");
  CWDM_REQUIRE(cfg->dropout >= 0.0 && cfg->dropout < 1.0, CWDM_E_INVALID,
               "cwdm_unet_create: dropout must lie in [0, 1)");
  CWDM_REQUIRE(!(cfg->dropout > 0.0 && cfg->use_freq), CWDM_E_UNSUPPORTED,
               "cwdm_unet_create: dropout with use_freq (WavUNetModel's ResBlocks are not covered)");
  CWDM_REQUIRE(cfg->num_classes >= 0, CWDM_E_INVALID, "cwdm_unet_create: num_classes must not be negative");
  CWDM_REQUIRE(!(cfg->num_classes > 0 && cfg->use_freq), CWDM_E_UNSUPPORTED,
               "cwdm_unet_create: num_classes with use_freq (WavUNetModel's class conditioning is not covered)");
  if (cfg->bottleneck_attention) {
    CWDM_REQUIRE(!cfg->use_freq, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: bottleneck_attention with use_freq (WavUNetModel's middle block is not covered)");
    const int C = cfg->channel_mult[cfg->num_levels - 1] * cfg->model_channels;
    const int heads = cfg->num_head_channels > 0 ? C / cfg->num_head_channels : std::max(cfg->num_heads, 1);
    CWDM_REQUIRE(heads >= 1 && C % heads == 0 && (cfg->num_head_channels <= 0 || C % cfg->num_head_channels == 0),
                 CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: bottleneck attention: " + std::to_string(C) + " channels not divisible into heads");
    const int ch = C / heads;
    CWDM_REQUIRE(ch % 16 == 0, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: bottleneck attention: head channels must be a multiple of 16, got " +
                     std::to_string(ch));
    CWDM_REQUIRE(ch <= 256, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: bottleneck attention: at most 256 head channels, got " + std::to_string(ch));
    CWDM_REQUIRE(C / cfg->num_groups <= 256, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: bottleneck attention: at most 256 channels per GroupNorm group");
  }
  if (cfg->use_freq) {
    // WavUNetModel as script_util.create_model builds it (:268-292)
    CWDM_REQUIRE(cfg->resblock_updown, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: use_freq needs resblock_updown=1 (wunet.Downsample with use_freq ignores its conv)");
    CWDM_REQUIRE(cfg->channel_mult[0] == 1, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: use_freq: the output head takes model_channels (wunet.py:713), channel_mult[0] = 1");
    CWDM_REQUIRE(cfg->in_channels % 8 == 0 && cfg->in_channels <= 2048, CWDM_E_UNSUPPORTED,
                 "cwdm_unet_create: use_freq: the wavelet pyramid needs in_channels a multiple of 8");
    // the decoder re-runs each level's last ResBlock on its own output (wunet.py:648-687): that block must keep
    // its channel count, i.e. num_res_blocks >= 2 or no channel change into the level
    for (int l = 0; l < cfg->num_levels && cfg->num_res_blocks == 1; ++l) {
      const int prev = l == cfg->num_levels - 1 ? cfg->channel_mult[l] : cfg->channel_mult[l + 1];
      CWDM_REQUIRE(prev == cfg->channel_mult[l], CWDM_E_UNSUPPORTED,
                   "cwdm_unet_create: use_freq with num_res_blocks=1 needs equal channel_mult across levels "
                   "(the reused decoder ResBlock would see the wrong channel count, as in the reference)");
    }
  }
  auto* u = new cwdm_unet();
  u->cfg = *cfg;
  build(u);
  *plan = u;
  return CWDM_OK;
}

extern "C" void cwdm_unet_destroy(cwdm_unet* u) {
  if (!u) return;
  for (auto e : u->ev) (void)hipEventDestroy(e);
  (void)hipFree(u->pack_tab);
  (void)hipFree(u->bwd_tab);
  (void)hipFree(u->copy_tab);
  delete u;
}

extern "C" int cwdm_unet_set_dropout_seed(cwdm_unet* u, uint64_t seed) {
  CWDM_REQUIRE(u, CWDM_E_INVALID, "cwdm_unet_set_dropout_seed: null plan");
  u->dropout_seed = seed;
  return CWDM_OK;
}

extern "C" int cwdm_unet_set_labels(cwdm_unet* u, const int64_t* y_dev) {
  CWDM_REQUIRE(u, CWDM_E_INVALID, "cwdm_unet_set_labels: null plan");
  CWDM_REQUIRE(u->cfg.num_classes > 0, CWDM_E_INVALID,
               "cwdm_unet_set_labels: the plan has no classes (num_classes = 0)");
  CWDM_REQUIRE(y_dev, CWDM_E_INVALID, "cwdm_unet_set_labels: null labels");
  // (the error word's address is looked up here, never inside a stream capture)
  unsigned* err = nullptr;
  if (int rc = cwdm::dev_err_word(&err)) return rc;
  u->labels = y_dev;
  return CWDM_OK;
}

extern "C" int cwdm_unet_num_params(const cwdm_unet* u) { return u ? (int)u->params.size() : -1; }

extern "C" int cwdm_unet_param_info(const cwdm_unet* u, int i, char* name, int cap, int64_t* shape, int* ndim) {
  CWDM_REQUIRE(u && i >= 0 && i < (int)u->params.size(), CWDM_E_INVALID, "cwdm_unet_param_info: bad index");
  const auto& p = u->params[i];
  if (name && cap > 0) {
    std::strncpy(name, p.name.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (ndim) *ndim = (int)p.shape.size();
  if (shape)
    for (size_t k = 0; k < p.shape.size() && k < 5; ++k) shape[k] = p.shape[k];
  return CWDM_OK;
}

extern "C" int cwdm_unet_num_aliases(const cwdm_unet* u) { return u ? (int)u->aliases.size() : -1; }

extern "C" int cwdm_unet_alias_info(const cwdm_unet* u, int i, char* name, int cap, int* owner, int* before) {
  CWDM_REQUIRE(u && i >= 0 && i < (int)u->aliases.size(), CWDM_E_INVALID, "cwdm_unet_alias_info: bad index");
  if (name && cap > 0) {
    std::strncpy(name, u->aliases[i].name.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (owner) *owner = u->aliases[i].owner;
  if (before) *before = u->aliases[i].before;
  return CWDM_OK;
}

extern "C" int64_t cwdm_unet_packed_bytes(const cwdm_unet* u) { return u ? u->packed_bytes : -1; }

// device table of n jobs (grown when needed)
template <typename J>
static int ensure_table(J*& tab, size_t& cap, size_t n) {
  if (n <= cap) return CWDM_OK;
  if (tab) CWDM_HIP(hipFree(tab));
  tab = nullptr;
  CWDM_HIP(hipMalloc(reinterpret_cast<void**>(&tab), n * sizeof(J)));
  cap = n;
  return CWDM_OK;
}

static int copy_batch_run(cwdm_unet* u, std::vector<CopyJob>& jobs, hipStream_t s) {
  if (jobs.empty()) return CWDM_OK;
  long long blk = 0;
  for (auto& j : jobs) {
    j.blk0 = blk;
    blk += (j.n + 1023) / 1024;
  }
  int rc;
  if ((rc = ensure_table(u->copy_tab, u->copy_cap, jobs.size()))) return rc;
  if (u->copy_cache.size() != jobs.size() ||
      std::memcmp(u->copy_cache.data(), jobs.data(), jobs.size() * sizeof(CopyJob))) {
    CWDM_HIP(hipMemcpyAsync(u->copy_tab, jobs.data(), jobs.size() * sizeof(CopyJob), hipMemcpyHostToDevice, s));
    CWDM_HIP(hipStreamSynchronize(s));
    u->copy_cache = jobs;
  }
  hipLaunchKernelGGL(cwdm::copy_batch_kernel, dim3((unsigned)blk), dim3(256), 0, s, u->copy_tab, (int)jobs.size());
  CWDM_LAUNCHED();
  return CWDM_OK;
}

// (the packs and the fp32 parameter copies each go out as one batched launch;
// one launch per parameter / conv cost ~2.5 ms per training step in copies,
// vec-adds and pack kernels)
extern "C" int cwdm_unet_pack(const cwdm_unet* uc, const float* const* P, void* packed, cwdm_stream_t stream) {
  CWDM_REQUIRE(uc && P && packed, CWDM_E_INVALID, "cwdm_unet_pack: null pointer");
  cwdm_unet* u = const_cast<cwdm_unet*>(uc);  // only the job-table cache changes
  hipStream_t s = (hipStream_t)stream;
  auto* base = reinterpret_cast<unsigned char*>(packed);
  std::vector<CopyJob> cj;
  auto cp = [&](int pi, int64_t off) {
    cj.push_back(CopyJob{reinterpret_cast<float*>(base + off), P[pi], nullptr, u->params[pi].numel(), 0});
  };
  cp(u->te_w1, u->off_te_w1);
  cp(u->te_b1, u->off_te_b1);
  cp(u->te_w2, u->off_te_w2);
  cp(u->te_b2, u->off_te_b2);
  if (u->label_w >= 0) cp(u->label_w, u->off_label);
  float* ew = reinterpret_cast<float*>(base + u->off_emb_w);
  float* eb = reinterpret_cast<float*>(base + u->off_emb_b);
  for (size_t k = 0; k < u->emb_rows_w.size(); ++k) {
    const int64_t o = u->emb_rows_off[k], n = u->emb_rows_n[k];
    cj.push_back(CopyJob{ew + o * u->E, P[u->emb_rows_w[k]], nullptr, n * u->E, 0});
    cj.push_back(CopyJob{eb + o, P[u->emb_rows_b[k]], u->emb_rows_cb[k] < 0 ? nullptr : P[u->emb_rows_cb[k]], n, 0});
  }
  // the convs' packs, collected for one launch (pack_batch_run below)
  std::vector<cwdm::PackJob> jobs;
  cwdm::PackJob j;
  int rc;
  for (const auto& cs : u->convs) {
    if ((rc = cs.s2      ? cwdm::pack_s2_job(P[cs.w_p], cs.cout, cs.cin_a / 8, u->cfg.dtype, base + cs.w_off, 0, j)
              : cs.cin_w ? cwdm::pack_zext_job(P[cs.w_p], cs.cout, cs.cin_w, cs.cin_a, u->cfg.dtype, base + cs.w_off, j)
                         : cwdm::pack_job(P[cs.w_p], cs.cout, cs.cin_a, 3, u->cfg.dtype, base + cs.w_off, j)))
      return rc;
    jobs.push_back(j);
    if (cs.wphase_off >= 0) {
      if ((rc = cwdm::pack_phase_job(P[cs.w_p], cs.cout, cs.cin_a, u->cfg.dtype, base + cs.wphase_off, j))) return rc;
      jobs.push_back(j);
    }
    if (cs.wsplit_off >= 0 &&
        (rc = cwdm_conv3d_pack_split(P[cs.w_p], cs.cout, cs.cin_a, base + cs.wsplit_off, stream)))
      return rc;
    if (cs.ws_p >= 0) {
      if ((rc = cwdm::pack_job(P[cs.ws_p], cs.cout, cs.cin_b, 1, u->cfg.dtype, base + cs.wsk_off, j))) return rc;
      jobs.push_back(j);
    }
    if (cs.bias_kind == 0)
      cj.push_back(CopyJob{reinterpret_cast<float*>(base + cs.bias_off), P[cs.b_p],
                           cs.wsb_p >= 0 ? P[cs.wsb_p] : nullptr, cs.cout, 0});
  }
  // the accurate fast mode's K-expanded weights (head, small grids): bf16, so packed now, outside the
  // batch (which packs in the model's dtype)
  for (const auto& cs : u->convs) {
    float* tmp = reinterpret_cast<float*>(base + u->split3_tmp);
    for (const int64_t o : {cs.hsplit_off, cs.xsplit_off})
      if (o >= 0 && (rc = cwdm::head_split3_pack(P[cs.w_p], cs.cout, cs.cin_a, tmp, base + o, s, 3))) return rc;
    if (cs.xsplit_sk_off >= 0 &&
        (rc = cwdm::head_split3_pack(P[cs.ws_p], cs.cout, cs.cin_b, tmp, base + cs.xsplit_sk_off, s, 1)))
      return rc;
  }
  for (const auto& g : u->gns) {
    cp(g.gamma_p, g.gamma_off);
    cp(g.beta_p, g.beta_off);
  }
  // the attention block's projections: row-major in the plan dtype, the qkv rows (and bias) permuted to
  // [Q | K | V] when the model keeps the legacy per-head order
  for (const auto& at : u->attns) {
    const int legacy = u->cfg.attn_new_order ? 0 : 1;
    if ((rc = cwdm::attn_pack(P[at.qkv_w_p], 3 * at.C, at.C, at.heads, at.ch, legacy, 0, u->cfg.dtype,
                              base + at.qkv_w_off, s)))
      return rc;
    if ((rc = cwdm::attn_pack(P[at.qkv_b_p], 3 * at.C, 1, at.heads, at.ch, legacy, 0, CWDM_F32, base + at.qkv_b_off, s)))
      return rc;
    if ((rc = cwdm::attn_pack(P[at.proj_w_p], at.C, at.C, at.heads, at.ch, 0, 0, u->cfg.dtype, base + at.proj_w_off, s)))
      return rc;
    cp(at.proj_b_p, at.proj_b_off);
  }
  if ((rc = copy_batch_run(u, cj, s))) return rc;
  if ((rc = ensure_table(u->pack_tab, u->pack_cap, jobs.size()))) return rc;
  return cwdm::pack_batch_run(jobs, u->cfg.dtype, u->pack_tab, u->pack_cache, s);
}

extern "C" int64_t cwdm_unet_workspace_bytes(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  if (!u || B <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
  return layout(u, B, D, H, W).total;
}

extern "C" int64_t cwdm_unet_train_workspace_bytes(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  const int64_t n = cwdm_unet_workspace_bytes(u, B, D, H, W);
  if (n < 0) return n;
  return layout(u, B, D, H, W).train_total;
}

extern "C" double cwdm_unet_flops(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  if (!u) return -1;
  double f = 0;
  for (const auto& cs : u->convs) {
    const double v = (double)B * (D >> cs.level) * (H >> cs.level) * (W >> cs.level);
    // algorithmic (stride-2: 27 C taps; conv_in: the model's input channels, not the padded ones)
    f += 2.0 * v * cs.cout * (27.0 * (cs.s2 ? cs.cin_a / 8 : cs.w_cin()) + cs.cin_b);
  }
  for (const auto& at : u->attns) {   // the qkv and proj GEMMs, q k^T and P v
    const double T = (double)(D >> at.level) * (H >> at.level) * (W >> at.level);
    f += 2.0 * B * T * at.C * (4.0 * at.C + 2.0 * T);
  }
  return f;
}

// the attention block's descriptor, forward part: q, k, v side by side in the rows of qkv (B, T, 3 C), the
// output rows in a (B, T, C), the rows' log-sum-exp in lse (nullptr: not kept)
static cwdm_attention_desc attn_desc(const AttnStep& at, int dt, int64_t B, int64_t T, const unsigned char* qkv,
                                     void* a, float* lse) {
  const int64_t C = at.C, es = esize(dt);
  cwdm_attention_desc ad{};
  ad.dtype = dt; ad.B = B; ad.T = T; ad.heads = at.heads; ad.ch = at.ch;
  ad.q = qkv; ad.k = qkv + C * es; ad.v = qkv + 2 * C * es;
  ad.q_rs = ad.k_rs = ad.v_rs = 3 * C; ad.q_bs = ad.k_bs = ad.v_bs = T * 3 * C;
  ad.o = a; ad.o_rs = C; ad.o_bs = T * C; ad.L = lse;
  return ad;
}

namespace {

// One forward call: UNetModel.forward as the plan's step list on one stream.  run() dispatches each step to
// the member of its StepKind (pool, s2d, haar, dropout, avg, attention, gn, conv); conv() fills the step's
// desc (conv_desc) and dispatches to the member of its ConvKind (conv_plain, conv_skip_pass, conv_head_split,
// conv_xsg), or to conv_head_sampler where the output head can fuse the sampling step.
// The pending GroupNorm finalize: gn() only notes its norm in fin_pend (cwdm::GnFinFuse: at the small grids
// the consumer conv's pre-pass computes it), flush_fin() runs it as its own launch, offer_fin() hands it to a
// conv that reads that norm and must then take it.  The rule, in run(): a pending finalize whose consumer is
// not the next step runs before that step.  Env CWDM_GNFIN=0: every finalize as its own launch (A/B switch).
struct Forward : PlanView {
  float* out; const float* t;
  bool keep;                       // a training-sized workspace: keep the convs' activated inputs for the backward
  const cwdm_sampler_args* samp;   // cwdm_unet_forward_step: run the sampling step on the output, fused into the
  int* fused;                      // output head where it qualifies (*fused = 1), else by the caller afterwards
  // derived from the above
  float* temb = reinterpret_cast<float*>(wb + L.temb);
  float* ebias = reinterpret_cast<float*>(wb + L.ebias);
  unsigned* sync = reinterpret_cast<unsigned*>(wb + L.sync);   // the zeroed sync block (ConvCall::sync)
  // statistics partial rows per tensor: the per-tile layout, or a conv's per-workgroup rows (plan_stats_wg)
  std::vector<int64_t> srows = L.s_parts;
  int fin_pend = -1;   // the norm whose finalize is pending, -1 none
  int conv_i = 0;      // the profiling cursor: conv steps run so far (u->hooks, u->ev_used)

  void* dst(int id) const { return wb + L.t_off[id]; }
  float* stats(int id) const { return reinterpret_cast<float*>(wb + L.s_off[id]); }
  void* kept(int ci) const { return keep && L.keep_off[ci] >= 0 ? wb + L.keep_off[ci] : nullptr; }

  int begin() {
    CWDM_HIP(hipMemsetAsync(sync, 0, cwdm::plan_sync_bytes(), s));
    if (int rc = launch_time_embed(t, (int)B, u->cfg.model_channels, P(u->off_te_w1), P(u->off_te_b1), P(u->off_te_w2),
                                   P(u->off_te_b2), temb, u->label_w >= 0 ? P(u->off_label) : nullptr, u->labels,
                                   u->cfg.num_classes, s))
      return rc;
    if (int rc = launch_emb_proj(temb, (int)B, u->E, P(u->off_emb_w), P(u->off_emb_b), u->R, ebias, s)) return rc;
    return u->profiling ? prof_begin() : CWDM_OK;
  }
  // four events per conv: the MFMA kernel launches inside it (cwdm::ProfHook)
  int prof_begin() {
    const size_t need = u->convs.size() * 4;
    while (u->ev.size() < need) {
      hipEvent_t e;
      CWDM_HIP(hipEventCreate(&e));
      u->ev.push_back(e);
    }
    u->ev_flops.assign(u->convs.size(), 0.0);
    u->hooks.assign(u->convs.size(), cwdm::ProfHook{});
    for (size_t i = 0; i < u->convs.size(); ++i)
      for (int k = 0; k < 4; ++k) u->hooks[i].ev[k >> 1][k & 1] = u->ev[4 * i + k];
    u->ev_used = 0;
    return CWDM_OK;
  }

  int run() {
    int rc = CWDM_OK;
    for (const auto& st : u->steps) {
      if (fin_pend >= 0 && !(st.kind == kConv && u->convs[st.idx].gn == u->gns[fin_pend].ss_id) && (rc = flush_fin()))
        return rc;
      switch (st.kind) {
        case kGn: rc = gn(st.idx); break;
        case kConv: rc = conv(st.idx); break;
        case kPool: rc = pool(u->pools[st.idx]); break;
        case kS2d: rc = s2d(u->s2ds[st.idx]); break;
        case kHaar: rc = haar(u->haars[st.idx]); break;
        case kAvg: rc = avg(u->avgs[st.idx]); break;
        case kAttn: rc = attention(u->attns[st.idx]); break;
        case kDrop: rc = dropout(u->drops[st.idx]); break;
        case kStage: rc = stage(); break;
      }
      if (rc) return rc;
    }
    return flush_fin();
  }

  // ---- the pending GroupNorm finalize
  int gn(int gi) {
    static const bool fin_on = env_not0("CWDM_GNFIN");
    fin_pend = gi;
    return fin_on ? CWDM_OK : flush_fin();
  }
  // the pending finalize's arguments (not yet used); it is pending no longer
  cwdm::GnFinFuse take_fin() {
    const auto& g = u->gns[std::exchange(fin_pend, -1)];
    cwdm::GnFinFuse f{};
    f.s0 = stats(g.src0); f.p0 = srows[g.src0]; f.c0 = nch(g.src0);
    f.s1 = g.src1 >= 0 ? stats(g.src1) : nullptr;
    f.p1 = g.src1 >= 0 ? srows[g.src1] : 0; f.c1 = nch(g.src1);
    f.gamma = P(g.gamma_off); f.beta = P(g.beta_off); f.groups = u->cfg.num_groups;
    f.voxels = vox(g.level); f.eps = 1e-5f; f.B = B;
    f.ss = reinterpret_cast<float*>(wb + L.ss_off[g.ss_id]); f.mr = reinterpret_cast<float*>(wb + L.mr_off[g.ss_id]);
    f.film = g.film_row >= 0 ? ebias + g.film_row : nullptr;
    f.film_bs = u->R;
    return f;
  }
  int flush_fin() {
    if (fin_pend < 0) return CWDM_OK;
    const cwdm::GnFinFuse f = take_fin();
    if (f.film)
      return cwdm_gn_finalize_film(f.s0, f.p0, f.c0, f.s1, f.p1, f.c1, f.gamma, f.beta, f.groups, B, f.voxels, f.eps,
                                   f.ss, f.mr, f.film, f.film_bs, stream);
    return cwdm_gn_finalize(f.s0, f.p0, f.c0, f.s1, f.p1, f.c1, f.gamma, f.beta, f.groups, B, f.voxels, f.eps, f.ss,
                            f.mr, stream);
  }
  // conv ci = d through cwdm::conv3d_forward, offered the pending finalize (in ff) if it is of the norm d reads:
  // the conv must then take it; any other pending finalize runs first
  int offer_fin(int ci, const cwdm_conv3d_desc& d, cwdm::ConvCall& cc, cwdm::GnFinFuse& ff) {
    const bool offer = fin_pend >= 0 && d.a_gn == ss_of(u->gns[fin_pend].ss_id);
    if (offer) {
      ff = take_fin();
      cc.gnfin = &ff;
    } else if (int rc = flush_fin()) {
      return rc;
    }
    if (int rc = cwdm::conv3d_forward(&d, cc, s)) return rc;
    CWDM_REQUIRE(!offer || ff.used, CWDM_E_INVALID,
                 "cwdm_unet_forward: conv " + std::to_string(ci) + " did not take its GroupNorm finalize");
    return CWDM_OK;
  }

  // ---- the steps that are one launch (dropout and attention read a norm no conv takes: run() flushed it)
  // x, dense (B, D, H, W, in_channels), into its zero-padded copy: real zeros in the padded lanes whatever the
  // workspace held (the backward's weight gradient reads the copy too)
  int stage() {
    return cwdm::pad_channels(x, u->cfg.in_channels, dst(u->stage_tensor), nch(u->stage_tensor), dt, B * vox(0), s);
  }
  int pool(const PoolStep& ps) {
    const int lv = ps.level_out;
    return cwdm_gn_silu_pool(act(ps.src), ps.channels, ss_of(ps.ss_id), B, D >> lv, H >> lv, W >> lv, dt,
                             dst(ps.out_h), dst(ps.out_x), stream);
  }
  int s2d(const S2dStep& sd) {
    const int lv = sd.level_out;
    return cwdm_space_to_depth(act(sd.src), sd.channels, B, D >> lv, H >> lv, W >> lv, dt, dst(sd.out), 1, 0, stream);
  }
  int haar(const HaarStep& hs) {
    const int lv = hs.level;
    cwdm_haar_nd_desc a{};
    a.dtype = dt; a.B = B; a.d = D >> lv; a.h = H >> lv; a.w = W >> lv; a.C = nch(hs.src);
    a.inverse = hs.inverse; a.all8 = hs.all8;
    a.src = act(hs.src); a.high_in = act(hs.high_in);
    a.lll_scale = hs.lll_scale; a.high_scale = hs.high_scale;
    a.out = dst(hs.out); a.high_out = hs.high_out >= 0 ? dst(hs.high_out) : nullptr;
    a.bias = hs.emb_row >= 0 ? ebias + hs.emb_row : nullptr; a.bias_bstride = u->R;
    a.stats = hs.stats ? stats(hs.out) : nullptr;
    return cwdm_haar_nd(&a, stream);
  }
  int dropout(const DropStep& ds) {
    return cwdm_gn_silu_dropout(act(ds.src), ss_of(ds.ss_id), dst(ds.out), dt, B, vox(ds.level), ds.channels,
                                u->cfg.dropout, u->dropout_seed, ds.site, stream);
  }
  int avg(const AvgStep& as) {
    return cwdm_skip_avg(act(as.a), act(as.b), dst(as.out), stats(as.out), dt, B, vox(as.level), as.channels, stream);
  }
  // qkv(GroupNorm(src)), attention, src + proj_out; a training-sized workspace keeps the normalised input and
  // the rows' log-sum-exp
  int attention(const AttnStep& at) {
    const int64_t T = vox(at.level);
    const int C = at.C;
    unsigned char* qkv = wb + L.attn_qkv;
    void* a = wb + L.attn_a;
    int rc;
    if ((rc = cwdm::attn_linear(dt, B, T, C, 3 * C, act(at.src), ss_of(at.gn), pk + at.qkv_w_off, P(at.qkv_b_off),
                                nullptr, qkv, keep ? wb + L.attn_n : nullptr, nullptr, s)))
      return rc;
    const cwdm_attention_desc ad =
        attn_desc(at, dt, B, T, qkv, a, keep ? reinterpret_cast<float*>(wb + L.attn_L) : nullptr);
    if ((rc = cwdm_attention_forward(&ad, stream))) return rc;
    return cwdm::attn_linear(dt, B, T, C, C, a, nullptr, pk + at.proj_w_off, P(at.proj_b_off), act(at.src),
                             dst(at.out), nullptr, stats(at.out), s);
  }

  // ---- a conv step
  cwdm_conv3d_desc conv_desc(int ci) const {
    const auto& cs = u->convs[ci];
    // (conv_shape set the channel counts, a_mode, res_mode and out_dtype; its presence flags become pointers)
    cwdm_conv3d_desc d = conv_shape(u, cs, B, D, H, W);
    d.a0 = act(cs.a0); d.a1 = act(cs.a1);
    d.workspace = wb + L.split; d.ws_bytes = L.split_bytes;
    d.a_gn = cs.gn >= 0 ? ss_of(cs.gn) : nullptr;
    d.a_w = pk + cs.w_off;
    d.a_w_split = cs.wsplit_off >= 0 ? pk + cs.wsplit_off : nullptr;
    d.a_w_phase = cs.wphase_off >= 0 ? pk + cs.wphase_off : nullptr;
    if (cs.ws_p >= 0) { d.b0 = act(cs.sb0); d.b1 = act(cs.sb1); d.b_w = pk + cs.wsk_off; }
    if (cs.bias_kind == 0) { d.bias = P(cs.bias_off); d.bias_bstride = 0; }
    else { d.bias = ebias + cs.bias_off; d.bias_bstride = u->R; }
    d.res = act(cs.res);
    d.out = cs.out < 0 ? out : dst(cs.out);
    d.stats = (cs.stats && cs.out >= 0) ? stats(cs.out) : nullptr;
    return d;
  }
  int conv(int ci) {
    const auto& cs = u->convs[ci];
    cwdm_conv3d_desc d = conv_desc(ci);
    // this conv's context: the plan's zeroed sync block, per-workgroup statistics, the profiling hook
    cwdm::ConvCall cc;
    cc.sync = sync; cc.stats_wg = plan_stats_wg();
    if (u->profiling) cc.prof = &u->hooks[conv_i];
    ConvKind kind = keep ? L.conv[ci].kind_keep : L.conv[ci].kind;
    if (kind == ConvKind::SkipTaken) {
      // the skip was computed in conv1's GroupNorm pass: a plain residual here
      d.b0 = d.b1 = nullptr; d.b_c0 = d.b_c1 = 0; d.b_w = nullptr;
      d.res = wb + L.skipbuf; d.res_mode = 0;
      kind = ConvKind::Plain;
    }
    int rc = CWDM_OK;
    // (the output head fuses the sampling step where the step's arguments allow: a run-time question)
    if (kind != ConvKind::SkipPass && samp && cs.out < 0 && cwdm::head_sampler_eligible(&d, samp))
      rc = conv_head_sampler(d, cc);
    else switch (kind) {
      case ConvKind::Plain:
      case ConvKind::SkipTaken: rc = conv_plain(ci, d, cc); break;   // (SkipTaken: rewritten above)
      case ConvKind::SkipPass: rc = conv_skip_pass(ci, d, cc); break;
      case ConvKind::HeadSplit: rc = conv_head_split(ci, d, cc); break;
      case ConvKind::Xsg: rc = conv_xsg(ci, d, cc); break;
    }
    if (rc) return rc;
    if (cc.stats_rows > 0 && cs.out >= 0) srows[cs.out] = cc.stats_rows;
    if (u->profiling) u->ev_used = conv_i + 1;
    ++conv_i;
    return CWDM_OK;
  }
  int conv_plain(int ci, const cwdm_conv3d_desc& d, cwdm::ConvCall& cc) {
    cc.act_keep = kept(ci);
    cwdm::GnFinFuse ff{};
    if (int rc = offer_fin(ci, d, cc, ff)) return rc;
    CWDM_REQUIRE(!cc.act_keep || cc.act_kept, CWDM_E_INVALID,
                 "cwdm_unet_forward: conv " + std::to_string(ci) + " did not keep its activated input");
    return CWDM_OK;
  }
  int conv_head_sampler(const cwdm_conv3d_desc& d, cwdm::ConvCall& cc) {
    if (int rc = flush_fin()) return rc;
    if (int rc = cwdm::head_sampler_forward(&d, samp, cc.prof, s)) return rc;
    if (fused) *fused = 1;
    return CWDM_OK;
  }
  // conv1 of a skip block: SiLU(GN1(x)) for this conv and W_skip . x for conv2 in one pass
  int conv_skip_pass(int ci, const cwdm_conv3d_desc& d, cwdm::ConvCall& cc) {
    const auto& c2 = u->convs[u->convs[ci].skip_conv];
    const ConvPlan& cp = L.conv[ci];
    void* ain = kept(ci) ? kept(ci) : wb + L.split;
    int rc;
    if ((rc = flush_fin())) return rc;
    if ((rc = cwdm::gn_apply_skip(d.a0, d.a_c0, d.a1, d.a_c1, d.a_gn, B, d.D * d.H * d.W, dt, pk + c2.wsk_off, c2.cout,
                                  ain, wb + L.skipbuf, s)))
      return rc;
    void* part = wb + L.split + cp.route.ws_act;   // (the K-split slices follow the activated input)
    return cwdm::v4_launch(&d, ain, d.a_c0 + d.a_c1, nullptr, 0, 1, d.res, d.res_mode, part, cp.pass, cc, s);
  }
  // the accurate fast mode's head: a bf16 head over the K-expanded split input (head_split3_prep)
  int conv_head_split(int ci, const cwdm_conv3d_desc& d, cwdm::ConvCall& cc) {
    if (int rc = flush_fin()) return rc;
    void* x3 = wb + L.split;
    if (int rc = cwdm::head_split3_prep(reinterpret_cast<const float*>(d.a0), d.a_gn, B, d.D * d.H * d.W, d.a_c0, x3, s))
      return rc;
    cwdm_conv3d_desc e = d;
    e.dtype = CWDM_BF16;
    e.a0 = x3; e.a_c0 = 3 * d.a_c0; e.a1 = nullptr; e.a_c1 = 0;
    e.a_gn = nullptr; e.a_w = pk + u->convs[ci].hsplit_off; e.a_w_split = nullptr;
    e.workspace = nullptr; e.ws_bytes = 0;
    return cwdm::conv3d_forward(&e, cc, s);
  }
  // the accurate fast mode on a small grid: one bf16 small-grid conv over the K-expanded split input, its
  // 1x1 skip first (XsgPlan; workspace x3 | skip | K-split slices)
  int conv_xsg(int ci, const cwdm_conv3d_desc& d, cwdm::ConvCall& cc) {
    const auto& cs = u->convs[ci];
    const XsgPlan& xp = L.xsg[L.conv[ci].xsg];
    int rc;
    if ((rc = flush_fin())) return rc;
    unsigned char* x3 = wb + L.split;
    const void* res = d.res;   // (the skip's product instead, where there is one)
    int rmode = d.res_mode;
    cc.fp32x = true;
    void* part = x3 + xp.x3_bytes + xp.skip_bytes;
    if (d.b_w) {
      if ((rc = xsg_skip(cs, d, xp, part, cc))) return rc;
      res = x3 + xp.x3_bytes; rmode = 0;
    }
    if ((rc = cwdm::split3_prep(reinterpret_cast<const float*>(d.a0), d.a_c0, reinterpret_cast<const float*>(d.a1),
                                d.a_c1, d.a_gn, B, src_voxels(d), 1, x3, s)))
      return rc;
    cwdm_conv3d_desc e = xp.e;
    e.a0 = x3; e.a1 = nullptr; e.a_w = pk + cs.xsplit_off;
    e.bias = d.bias; e.bias_bstride = d.bias_bstride;
    e.res = res; e.res_mode = rmode;
    e.out = d.out; e.stats = d.stats;
    e.workspace = nullptr; e.ws_bytes = 0;
    if (xp.er.ksplit <= 1) part = nullptr;
    return cwdm::v4_launch(&e, x3, e.a_c0, nullptr, 0, 1, res, rmode, part, xp.er, cc, s);
  }
  // its 1x1 skip into the fp32 residual behind x3
  int xsg_skip(const ConvStep& cs, const cwdm_conv3d_desc& d, const XsgPlan& xp, void* part, cwdm::ConvCall& cc) {
    unsigned char* x3 = wb + L.split;
    if (xp.sk_sg) {
      // the K-expanded split of the raw input on the small-grid kernel
      if (int rc = cwdm::split3_prep(reinterpret_cast<const float*>(d.b0), d.b_c0, reinterpret_cast<const float*>(d.b1),
                                     d.b_c1, nullptr, B, d.D * d.H * d.W, 0, x3, s))
        return rc;
      cwdm_conv3d_desc k = xp.ek;
      k.b0 = x3; k.b_w = pk + cs.xsplit_sk_off;
      return cwdm::sg_skip_launch(&k, x3 + xp.x3_bytes, xp.sk_ksplit > 1 ? part : nullptr, xp.sk_ksplit, cc, s);
    }
    // pw_split: the split products of the 1x1 weights
    cwdm_conv3d_desc k = skip_only_desc(d);
    k.out = x3 + xp.x3_bytes;
    k.workspace = nullptr; k.ws_bytes = 0;
    return xp.sk_pw_split ? cwdm::pw_split_forward(&k, cc.prof, s) : cwdm::conv3d_forward(&k, cc, s);
  }
};

}  // namespace

static int unet_forward_impl(cwdm_unet* u, const void* packed, const void* x, const float* t, float* out,
                             int64_t B, int64_t D, int64_t H, int64_t W, void* ws, int64_t ws_bytes,
                             cwdm_stream_t stream, const cwdm_sampler_args* samp, int* fused) {
  CWDM_REQUIRE(u && packed && x && t && out && ws, CWDM_E_INVALID, "cwdm_unet_forward: null pointer");
  CWDM_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, CWDM_E_SHAPE, "cwdm_unet_forward: empty grid");
  CWDM_REQUIRE(u->cfg.num_classes == 0 || u->labels, CWDM_E_INVALID,
               "cwdm_unet_forward: a class-conditional plan needs its labels (cwdm_unet_set_labels)");
  const int64_t div = int64_t(1) << (u->cfg.num_levels - (u->cfg.use_freq ? 0 : 1));
  CWDM_REQUIRE(D % div == 0 && H % div == 0 && W % div == 0, CWDM_E_SHAPE,
               "cwdm_unet_forward: every subband edge must be divisible by " + std::to_string(div));
  Layout L = layout(u, B, D, H, W);
  CWDM_REQUIRE(ws_bytes >= L.total, CWDM_E_WORKSPACE,
               "cwdm_unet_forward: workspace too small (need " + std::to_string(L.total) + " bytes)");
  // a training-sized workspace keeps the convs' activated inputs for the backward
  const bool keep = L.train_total > L.total && ws_bytes >= L.train_total;
  Forward fw{{u, L, reinterpret_cast<const unsigned char*>(packed), reinterpret_cast<unsigned char*>(ws), x, B, D, H, W,
              stream}, out, t, keep, samp, fused};
  if (int rc = fw.begin()) return rc;
  return fw.run();
}

extern "C" int cwdm_unet_forward(cwdm_unet* u, const void* packed, const void* x, const float* t, float* out,
                                 int64_t B, int64_t D, int64_t H, int64_t W, void* ws, int64_t ws_bytes,
                                 cwdm_stream_t stream) {
  return unet_forward_impl(u, packed, x, t, out, B, D, H, W, ws, ws_bytes, stream, nullptr, nullptr);
}

extern "C" int cwdm_unet_forward_step(cwdm_unet* u, const void* packed, const void* x, const float* t_model,
                                      const cwdm_sampler_args* step, int64_t B, int64_t D, int64_t H, int64_t W,
                                      void* ws, int64_t ws_bytes, int* fused, cwdm_stream_t stream) {
  CWDM_REQUIRE(step && step->model_out, CWDM_E_INVALID, "cwdm_unet_forward_step: null step / model_out");
  CWDM_REQUIRE(u && step->d == D && step->h == H && step->w == W && step->B == B &&
                   (step->levels == 2 || u->cfg.out_channels == 8),
               CWDM_E_SHAPE, "cwdm_unet_forward_step: the step's grid must be the forward's");
  int did = 0;
  int rc = unet_forward_impl(u, packed, x, t_model, const_cast<float*>(step->model_out), B, D, H, W, ws, ws_bytes,
                             stream, step, &did);
  if (fused) *fused = did;
  if (rc || did) return rc;
  return cwdm_sampler_step(step, stream);
}

extern "C" int cwdm_unet_trace_count(const cwdm_unet* u) { return u ? (int)u->trace.size() : -1; }

extern "C" int cwdm_unet_trace_info(const cwdm_unet* u, int i, int64_t B, int64_t D, int64_t H, int64_t W,
                                    int64_t* off, int* ch, int* level) {
  CWDM_REQUIRE(u && i >= 0 && i < (int)u->trace.size(), CWDM_E_INVALID, "cwdm_unet_trace_info: bad index");
  const int id = u->trace[i].tensor;
  Layout L = layout(u, B, D, H, W);
  if (off) *off = id >= 0 ? L.t_off[id] : -1;
  if (ch) *ch = id >= 0 ? u->tensors[id].channels : u->cfg.out_channels;
  if (level) *level = u->trace[i].level;
  return CWDM_OK;
}

extern "C" int cwdm_unet_set_profiling(cwdm_unet* u, int on) {
  CWDM_REQUIRE(u, CWDM_E_INVALID, "cwdm_unet_set_profiling: null plan");
  u->profiling = on != 0;
  return CWDM_OK;
}

extern "C" int cwdm_unet_profile_read(cwdm_unet* u, double* ms, double* flops, int* n) {
  CWDM_REQUIRE(u, CWDM_E_INVALID, "cwdm_unet_profile_read: null plan");
  double tot = 0, fl = 0;
  int launches = 0;
  for (int i = 0; i < u->ev_used; ++i) {
    const cwdm::ProfHook& h = u->hooks[i];
    for (int k = 0; k < h.n; ++k) {
      float m = 0;
      CWDM_HIP(hipEventElapsedTime(&m, h.ev[k][0], h.ev[k][1]));
      tot += m;
      fl += h.flops[k];
      ++launches;
    }
  }
  if (ms) *ms = tot;
  if (flops) *flops = fl;
  if (n) *n = launches;
  return CWDM_OK;
}

// ============================================================================
// Backward (training): the reverse of the launch list above, as torch autograd
// differentiates UNetModel.forward inside TrainLoop.forward_backward
// (guided_diffusion/train_util.py:396-462).  Per ResBlock, in reverse:
//   conv2: bias grad (channel sums), wgrad (input = SiLU(GN2(h1)) recomputed
//          in the staging), skip 1x1 wgrad + dgrad or residual adjoint,
//          dgrad (flipped/transposed weights, same implicit-GEMM kernel);
//          with dropout the wgrad reads the stored u, and cwdm_dropout_bwd masks the dgrad's output
//   GN2:   SiLU/GroupNorm backward -> dh1
//   conv1: emb-projection grads (per-batch channel sums), wgrad, dgrad
//   GN1:   SiLU/GroupNorm backward with the up/down resample adjoint -> dx
// Gradient buffers live in grad_ws (one per forward tensor, compute dtype);
// the first writer of a buffer stores, later writers accumulate.
// Segment 0 is the output head, then one per Block from the last to the first
// (by BlockKind, the members of struct Backward), then conv_in + time_embed.
// ============================================================================
namespace {

struct GLayout {
  std::vector<int64_t> g_off;
  int64_t sync, tmp, dout, deb, dsil, gnws, gnws_bytes, split, split_bytes, wgws, wgws_bytes, dwe, chs, chs_bytes;
  int64_t gbp, gbp_bytes;   // fused GroupNorm-backward partials ([B][tiles][C][2]) + their slice sums
  // the attention block: d qkv (B, T, 3 C), d a and d n (B, T, C), D (fp32 [B][heads][T]), the GroupNorm
  // backward's per-(batch, channel) sums, and the packed-order qkv weight / bias gradient before its rows
  // go back to the legacy order
  int64_t at_dqkv = -1, at_da = -1, at_dn = -1, at_D = -1, at_part = -1, at_dw = -1;
  int64_t total;
};

int ckpad(const cwdm_unet* u, int c) {
  const int ck = ck_of(u->cfg.dtype);
  return (c + ck - 1) / ck * ck;
}

// dgrad conv of conv step i as a forward conv descriptor (shape only)
cwdm_conv3d_desc dgrad_shape(const cwdm_unet* u, int i, int64_t B, int64_t D, int64_t H, int64_t W) {
  const auto& cs = u->convs[i];
  cwdm_conv3d_desc d{};
  d.dtype = u->cfg.dtype;
  d.B = B; d.D = D >> cs.level; d.H = H >> cs.level; d.W = W >> cs.level;
  d.cout = cs.cin_a;
  d.a_c0 = ckpad(u, cs.cout);
  d.a_mode = 0;
  d.a_w = reinterpret_cast<const void*>(1);
  d.res_mode = -1;
  d.out_dtype = u->cfg.dtype;
  return d;
}

// conv_in's weight gradient where its input channels are no multiple of the wgrad kernels' 32 (8 + 8x channels) or
// are padded ones: the input padded to 32s, then the gradient over the padded columns, both in the dgrads' scratch
// tmp, which is free by the last segment (Backward::stem copies the real columns out)
struct StemPad {
  int cw = 0;   // the wgrad's input channels, 0: conv_in's wgrad writes the parameter's gradient directly
  int64_t x_bytes = 0, dw_bytes = 0;
};
StemPad stem_pad(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  const auto& c0 = u->convs[0];
  StemPad p;
  if (c0.cin_a % 32 == 0 && !c0.cin_w) return p;
  p.cw = (c0.cin_a + 31) / 32 * 32;
  p.x_bytes = p.cw == c0.cin_a ? 0 : align_up(B * D * H * W * p.cw * esize(u->cfg.dtype));
  p.dw_bytes = (int64_t)c0.cout * p.cw * 27 * 4;
  return p;
}

GLayout glayout(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  GLayout G;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { int64_t o = off; off = align_up(off + bytes); return o; };
  const int es = esize(u->cfg.dtype);
  G.sync = take(cwdm::plan_sync_bytes());
  for (size_t i = 0; i < u->tensors.size(); ++i) {
    const auto& t = u->tensors[i];
    if ((int)i == u->input_tensor || !t.grad) { G.g_off.push_back(-1); continue; }
    G.g_off.push_back(take(B * (D >> t.level) * (H >> t.level) * (W >> t.level) * t.channels * es));
  }
  int64_t tmp = 0, split = 0, gnws = 0, wgws = 0;
  for (const auto& cs : u->convs) {
    wgws = std::max(wgws, cwdm_conv3d_wgrad_workspace_bytes(cs.cout, cs.cin_a, 3));
    if (cs.ws_p >= 0) wgws = std::max(wgws, cwdm_conv3d_wgrad_workspace_bytes(cs.cout, cs.cin_b, 1));
  }
  for (const auto& at : u->attns) wgws = std::max(wgws, cwdm_conv3d_wgrad_workspace_bytes(3 * at.C, at.C, 1));
  for (size_t i = 1; i < u->convs.size(); ++i) {
    const auto& cs = u->convs[i];
    const int64_t v = B * (D >> cs.level) * (H >> cs.level) * (W >> cs.level);
    tmp = std::max(tmp, v * cs.cin_a * es);
    cwdm_conv3d_desc d = dgrad_shape(u, (int)i, B, D, H, W);
    split = std::max(split, (int64_t)cwdm_conv3d_workspace_bytes(&d));
  }
  for (const auto& g : u->gns) {
    const int lv = g.level;
    gnws = std::max(gnws, cwdm_gn_silu_bwd_workspace_bytes(g.channels, B, D >> lv, H >> lv, W >> lv));
  }
  if (const StemPad sp = stem_pad(u, B, D, H, W); sp.cw) {
    tmp = std::max(tmp, sp.x_bytes + sp.dw_bytes);
    wgws = std::max(wgws, cwdm_conv3d_wgrad_workspace_bytes(u->convs[0].cout, sp.cw, 3));
  }
  G.tmp = take(tmp);
  G.dout = take(B * D * H * W * ckpad(u, u->cfg.out_channels) * es);
  G.deb = take(B * (int64_t)u->R * 4);
  G.dsil = take(B * (int64_t)u->E * 4);
  G.gnws_bytes = gnws;
  G.gnws = take(gnws);
  G.split_bytes = split;
  G.split = take(split);
  G.wgws = take(wgws);
  G.wgws_bytes = wgws;
  int64_t dwe = 0;   // expanded weight gradient of a stride-2 conv before folding
  for (const auto& cs : u->convs)
    if (cs.s2) dwe = std::max(dwe, (int64_t)cs.cout * cs.cin_a * 27 * 4);
  G.dwe = take(dwe);
  int64_t chs = 0;   // per-workgroup partials of the bias-gradient channel sums (fixed-order finish)
  for (const auto& cs : u->convs)
    chs = std::max(chs, cwdm_channel_sum_workspace_bytes(B, (D >> cs.level) * (H >> cs.level) * (W >> cs.level),
                                                         std::max(cs.cout, 8)));
  for (const auto& at : u->attns)
    chs = std::max(chs, cwdm_channel_sum_workspace_bytes(B, (D >> at.level) * (H >> at.level) * (W >> at.level),
                                                         3 * at.C));
  G.chs_bytes = chs;
  G.chs = take(chs);
  for (const auto& at : u->attns) {
    const int64_t T = (D >> at.level) * (H >> at.level) * (W >> at.level);
    G.at_dqkv = take(B * T * 3 * at.C * es);
    G.at_da = take(B * T * at.C * es);
    G.at_dn = take(B * T * at.C * es);
    G.at_D = take(B * at.heads * T * 4);
    G.at_part = take(B * (int64_t)at.C * 2 * 4);
    G.at_dw = take(((int64_t)3 * at.C * at.C + 3 * at.C) * 4);
  }
  // the dgrad epilogue's GroupNorm-backward partials: one row per 32x4x4 tile
  // of the DMA conv (cwdm::GbwdFuse), then kGbSlices slice sums of them
  int64_t gbp = 0;
  for (const auto& g : u->gns) {
    const int lv = g.level;
    const int64_t tiles = ceil_div(W >> lv, 32) * ceil_div(H >> lv, 4) * ceil_div(D >> lv, 4);
    gbp = std::max(gbp, B * tiles * g.channels * 8 + align_up(B * (int64_t)kGbSlices * g.channels * 8));
  }
  G.gbp_bytes = gbp;
  G.gbp = take(gbp);
  G.total = off;
  return G;
}

}  // namespace

extern "C" int64_t cwdm_unet_packed_bwd_bytes(const cwdm_unet* u) { return u ? u->packed_bwd_bytes : -1; }

extern "C" int cwdm_unet_pack_bwd(const cwdm_unet* uc, const float* const* P, void* packed_bwd, cwdm_stream_t stream) {
  CWDM_REQUIRE(uc && P && packed_bwd, CWDM_E_INVALID, "cwdm_unet_pack_bwd: null pointer");
  cwdm_unet* u = const_cast<cwdm_unet*>(uc);  // only the job-table cache changes
  auto* base = reinterpret_cast<unsigned char*>(packed_bwd);
  int rc;
  std::vector<cwdm::PackJob> jobs;
  cwdm::PackJob j;
  for (size_t i = 0; i < u->convs.size(); ++i) {
    const auto& cs = u->convs[i];
    if (u->dg_off[i] >= 0) {
      if ((rc = cs.s2 ? cwdm::pack_s2_job(P[cs.w_p], cs.cout, cs.cin_a / 8, u->cfg.dtype, base + u->dg_off[i], 1, j)
                      : cwdm::pack_dgrad_job(P[cs.w_p], cs.cout, cs.cin_a, 3, u->cfg.dtype, base + u->dg_off[i], j)))
        return rc;
      jobs.push_back(j);
    }
    if (u->dgs_off[i] >= 0) {
      if ((rc = cwdm::pack_dgrad_job(P[cs.ws_p], cs.cout, cs.cin_b, 1, u->cfg.dtype, base + u->dgs_off[i], j)))
        return rc;
      jobs.push_back(j);
    }
  }
  for (const auto& at : u->attns) {   // W^T of the two projections: their input gradients are row-major GEMMs too
    if ((rc = cwdm::attn_pack(P[at.qkv_w_p], 3 * at.C, at.C, at.heads, at.ch, u->cfg.attn_new_order ? 0 : 1, 1,
                              u->cfg.dtype, base + at.qkvT_off, (hipStream_t)stream)))
      return rc;
    if ((rc = cwdm::attn_pack(P[at.proj_w_p], at.C, at.C, at.heads, at.ch, 0, 1, u->cfg.dtype, base + at.projT_off,
                              (hipStream_t)stream)))
      return rc;
  }
  if ((rc = ensure_table(u->bwd_tab, u->bwd_cap, jobs.size()))) return rc;
  return cwdm::pack_batch_run(jobs, u->cfg.dtype, u->bwd_tab, u->bwd_cache, (hipStream_t)stream);
}

extern "C" int64_t cwdm_unet_grad_workspace_bytes(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  if (!u || B <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
  return glayout(u, B, D, H, W).total;
}

extern "C" int cwdm_unet_backward_segments(const cwdm_unet* u) { return u ? (int)u->blocks.size() + 2 : -1; }

extern "C" int cwdm_unet_segment_range(const cwdm_unet* u, int seg, int64_t* off, int64_t* n) {
  CWDM_REQUIRE(u && seg >= 0 && seg < (int)u->blocks.size() + 2, CWDM_E_INVALID, "cwdm_unet_segment_range: bad seg");
  const int nb = (int)u->blocks.size();
  int pb, pe;
  if (seg == 0) { pb = u->head_p_begin; pe = (int)u->params.size(); }
  else if (seg <= nb) { const auto& b = u->blocks[nb - seg]; pb = b.p_begin; pe = b.p_end; }
  else { pb = 0; pe = u->blocks[0].p_begin; }
  const int64_t o = u->goff[pb];
  const int64_t e = pe < (int)u->params.size() ? u->goff[pe] : u->grad_numel;
  if (off) *off = o;
  if (n) *n = e - o;
  return CWDM_OK;
}

extern "C" double cwdm_unet_backward_flops(const cwdm_unet* u, int64_t B, int64_t D, int64_t H, int64_t W) {
  if (!u) return -1;
  double f = 0;
  for (size_t i = 0; i < u->convs.size(); ++i) {
    const auto& cs = u->convs[i];
    const double v = (double)B * (D >> cs.level) * (H >> cs.level) * (W >> cs.level);
    const double fwd = 2.0 * v * cs.cout * (27.0 * (cs.s2 ? cs.cin_a / 8 : cs.w_cin()) + cs.cin_b);
    f += i == 0 ? fwd : 2 * fwd;  // wgrad (+ dgrad)
  }
  return f;
}

namespace {

// the reduce pass of a GroupNorm backward that a dgrad conv's epilogue took (Backward::dgrad_gn): its partials
struct Pre { const float* part = nullptr; int nblk = 0; };
// what Backward::gn_bwd does beyond the plain backward
struct GnBwdOpt {
  float* chs = nullptr; int64_t chs_stride = 0;   // per-batch channel sums of the written dx0, in the same pass
  const cwdm::GnBwdFilm* film = nullptr;   // a FiLM block's out_layers.0
  const float** coef_out = nullptr;        // reduce / finalize only: the apply pass's coefficients for a GapplyFuse
  bool keep_acc = false;                   // with coef_out: leave the store / accumulate state to the conv that applies
};

// One cwdm_unet_backward call: what its launches read, the calls they share, and one member per kind of
// segment.  Everything goes out on one stream and shares the scratch regions tmp (a dgrad's output = the
// GroupNorm backward's input), G.chs, G.gnws, G.wgws and G.split, so a segment's launch order is part of its
// result.  The store / accumulate state of the gradient buffers (u->ginit, take_acc) lives in the plan: it
// carries over between calls that each run a range of segments.
struct Backward : PlanView {
  const GLayout& G;
  const unsigned char* pb;   // packed parameters, backward form
  unsigned char* gb;         // the gradient workspace
  const float *t, *dout; float* grads;
  bool kept;   // the forward ran on a training-sized workspace: the convs' activated inputs are there
  // derived from the above
  int es = esize(dt);
  unsigned* sync = reinterpret_cast<unsigned*>(gb + G.sync);   // the zeroed sync block (ConvCall::sync)
  const float* temb = reinterpret_cast<const float*>(wb + L.temb);
  float* deb = reinterpret_cast<float*>(gb + G.deb);     // d emb projection rows [B][R]
  float* dsil = reinterpret_cast<float*>(gb + G.dsil);   // d SiLU(time embedding) [B][E]
  void* tmp = gb + G.tmp;
  float* gbp = reinterpret_cast<float*>(gb + G.gbp);

  float* GR(int pi) const { return grads + u->goff[pi]; }
  void* grd(int id) const { return id < 0 ? nullptr : gb + G.g_off[id]; }
  // first writer stores, later writers accumulate
  int take_acc(int id) { return id < 0 ? 0 : (std::exchange(u->ginit[id], char(1)) ? 1 : 0); }

  // bias gradient of a conv / linear layer: the channel sums of its output gradient dy (B, voxels of level,
  // stride channels, the first C of them summed) into db, and into db2 (a folded-in second bias) if given
  int bias_grad(const void* dy, int level, int C, float* db, float* db2 = nullptr, int stride = 0) {
    return cwdm_channel_sum(dy, dt, B, vox(level), C, stride ? stride : C, nullptr, 0, db, db2, gb + G.chs,
                            G.chs_bytes, stream);
  }
  // the gradient of tensor id (at level lv) takes src through the adjoint of resample mode
  int resample_add(int id, const void* src, int C, int lv, int mode) {
    return cwdm_resample_add(grd(id), src, C, B, D >> lv, H >> lv, W >> lv, mode, take_acc(id), dt, stream);
  }
  // weight gradient dw of a conv (u_cm: u0 is an activated input in the chunk-major form a forward conv kept)
  int wgrad(int level, int ksize, const void* u0, int uc0, const void* u1, int uc1, int umode, const float* ugn,
            const void* dy, int dy_cs, int cout, float* dw, int u_cm = 0) {
    cwdm_wgrad_desc d{};
    d.dtype = dt; d.B = B; d.D = D >> level; d.H = H >> level; d.W = W >> level; d.ksize = ksize;
    d.u0 = u0; d.u_c0 = uc0; d.u1 = u1; d.u_c1 = uc1; d.u_mode = umode; d.u_gn = ugn; d.u_cm = u_cm;
    d.dy = dy; d.dy_cs = dy_cs; d.cout = cout; d.dw = dw;
    d.workspace = gb + G.wgws; d.ws_bytes = G.wgws_bytes;
    return cwdm_conv3d_wgrad(&d, stream);
  }
  // conv ci's wgrad from the activated input its forward kept (training
  // workspace), else recomputed from the sources by the staging code
  int wgrad_c(int ci, int level, const void* u0, int uc0, const void* u1, int uc1, int umode, const float* ugn,
              const void* dy, int dy_cs, int cout, float* dw) {
    if (!kept || L.keep_off[ci] < 0) return wgrad(level, 3, u0, uc0, u1, uc1, umode, ugn, dy, dy_cs, cout, dw);
    return wgrad(level, 3, wb + L.keep_off[ci], uc0 + uc1, nullptr, 0, umode, nullptr, dy, dy_cs, cout, dw, 1);
  }
  // input gradient of conv ci into tmp
  int dgrad(int ci, const void* dy, cwdm::GbwdFuse* gbwd = nullptr) {
    cwdm_conv3d_desc d = dgrad_shape(u, ci, B, D, H, W);
    d.a0 = dy; d.a_w = pb + u->dg_off[ci]; d.out = tmp;
    d.workspace = gb + G.split; d.ws_bytes = G.split_bytes;
    cwdm::ConvCall cc;
    cc.sync = sync; cc.gbwd = gbwd;
    return cwdm::conv3d_forward(&d, cc, s);
  }
  // dgrad conv ci whose output du (tmp) feeds the SiLU(GroupNorm gi) backward at
  // the same grid, input x = (xid0, xid1): the conv's epilogue takes the reduce
  // pass of that backward when its kernel can (cwdm::GbwdFuse: 16-bit DMA conv,
  // no K split); pre then names the partials for gn_bwd
  int dgrad_gn(int ci, const void* dy, int gi, int xid0, int xid1, Pre& pre) {
    pre = Pre{};
    static const bool gb_on = env_not0("CWDM_GBWD_FUSE");
    if (!gb_on || G.gbp_bytes <= 0) return dgrad(ci, dy);
    const auto& g = u->gns[gi];
    cwdm::GbwdFuse f{};
    f.x0 = act(xid0); f.x1 = act(xid1); f.c0 = nch(xid0);
    f.ss = ss_of(gi); f.mr = mr_of(gi); f.groups = u->cfg.num_groups; f.part = gbp;
    f.part_bytes = G.gbp_bytes - align_up(B * (int64_t)kGbSlices * g.channels * 8);
    const int r = dgrad(ci, dy, &f);
    if (r || !f.used) return r;
    if (f.nblk <= 512) {   // few tiles: gn_bwd_finalize reads them directly
      pre.part = gbp; pre.nblk = f.nblk;
      return CWDM_OK;
    }
    float* sl = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(gbp) + f.part_bytes);
    if (int rc2 = gb_part_reduce(gbp, f.nblk, g.channels, B, kGbSlices, sl, s)) return rc2;
    pre.part = sl; pre.nblk = kGbSlices;
    return CWDM_OK;
  }
  // SiLU(GroupNorm gi) backward of du = tmp (du_mode: resample_mode of the block) into the gradients of the
  // norm's input (x0, x1), its reduce pass in pre if the dgrad took it; the only gn_silu_bwd_impl call here
  int gn_bwd(int gi, int x0, int x1, int du_mode, const Pre& pre, const GnBwdOpt& o = {}) {
    const auto& g = u->gns[gi];
    const int lv = g.level;
    const int a0 = o.keep_acc ? 0 : take_acc(x0), a1 = o.keep_acc ? 0 : take_acc(x1);
    // affine gradients accumulate (zeroed at segment 0): a reused WavUNetModel block adds its second use
    return gn_silu_bwd_impl(act(x0), nch(x0), act(x1), nch(x1), tmp, du_mode, ss_of(gi), mr_of(gi), P(g.gamma_off),
                            u->cfg.num_groups, B, D >> lv, H >> lv, W >> lv, dt, grd(x0), a0, grd(x1), a1,
                            GR(g.gamma_p), GR(g.beta_p), gb + G.gnws, G.gnws_bytes, o.chs, o.chs_stride, stream, 1,
                            pre.part, pre.nblk, o.coef_out, o.film);
  }
  // d(emb rows k) in deb -> the emb projection's gradients (and a folded-in conv bias's), d SiLU(time embedding)
  int emb_bwd(int k) {
    const int roff = u->emb_rows_off[k];
    return launch_emb_bwd(deb + roff, u->R, u->emb_rows_n[k], (int)B, temb, u->E,
                          P(u->off_emb_w) + (int64_t)roff * u->E, GR(u->emb_rows_w[k]), GR(u->emb_rows_b[k]),
                          u->emb_rows_cb[k] >= 0 ? GR(u->emb_rows_cb[k]) : nullptr, dsil, s, 1);
  }

  // ---- segment 0: zero the gradients, then the output head (out.0 GroupNorm, out.2 conv)
  int head() {
    int rc;
    u->ginit.assign(u->tensors.size(), 0);
    CWDM_HIP(hipMemsetAsync(grads, 0, u->grad_numel * 4, s));
    CWDM_HIP(hipMemsetAsync(deb, 0, B * (int64_t)u->R * 4, s));
    CWDM_HIP(hipMemsetAsync(dsil, 0, B * (int64_t)u->E * 4, s));
    // dout -> padded compute-dtype buffer
    const int oc = u->cfg.out_channels, ocp = ckpad(u, oc);
    const int64_t V0 = D * H * W;
    void* d16 = gb + G.dout;
    CWDM_HIP(hipMemsetAsync(d16, 0, B * V0 * ocp * es, s));
    const int64_t ss_[3] = {V0 * oc, 1, oc}, ds_[3] = {V0 * ocp, 1, ocp};
    if ((rc = cwdm_copy3(dout, CWDM_F32, ss_, d16, dt, ds_, B, oc, V0, stream))) return rc;
    const auto& co = u->convs[u->head_c];
    const auto& hg = u->gns[u->head_g];
    if ((rc = bias_grad(d16, 0, oc, GR(co.b_p), nullptr, ocp))) return rc;
    if ((rc = wgrad(0, 3, act(co.a0), co.cin_a, nullptr, 0, 0, ss_of(u->head_g), d16, ocp, oc, GR(co.w_p))))
      return rc;
    Pre pre;
    if ((rc = dgrad_gn(u->head_c, d16, u->head_g, hg.src0, -1, pre))) return rc;
    return gn_bwd(u->head_g, hg.src0, -1, 0, pre);
  }

  // ---- the bottleneck AttentionBlock: y = x + proj_out(attention(qkv(GroupNorm(x))))
  int attention(const Block& bk) {
    const auto& at = u->attns[bk.attn];
    const auto& g = u->gns[at.gn];
    CWDM_REQUIRE(kept, CWDM_E_WORKSPACE,
                 "cwdm_unet_backward: the attention block needs the forward's training workspace "
                 "(cwdm_unet_train_workspace_bytes: it keeps the log-sum-exp rows and the normalised input)");
    const int C = at.C, lv = at.level, o = at.out, xt = at.src;
    const int64_t T = vox(lv);
    unsigned char* dqkv = gb + G.at_dqkv;
    void *da = gb + G.at_da, *dn = gb + G.at_dn;
    int rc;
    // ---- proj_out: bias, weight, input gradient
    if ((rc = bias_grad(grd(o), lv, C, GR(at.proj_b_p)))) return rc;
    if ((rc = wgrad(lv, 1, wb + L.attn_a, C, nullptr, 0, 0, nullptr, grd(o), C, C, GR(at.proj_w_p)))) return rc;
    if ((rc = cwdm::attn_linear(dt, B, T, C, C, grd(o), nullptr, pb + at.projT_off, nullptr, nullptr, da, nullptr,
                                nullptr, s)))
      return rc;
    // ---- softmax(q k^T) v
    cwdm_attention_desc ad = attn_desc(at, dt, B, T, wb + L.attn_qkv, const_cast<unsigned char*>(wb + L.attn_a),
                                       const_cast<float*>(reinterpret_cast<const float*>(wb + L.attn_L)));
    ad.D = reinterpret_cast<float*>(gb + G.at_D);
    ad.d_o = da; ad.do_rs = C; ad.do_bs = T * C;
    ad.dq = dqkv; ad.dk = dqkv + (int64_t)C * es; ad.dv = dqkv + (int64_t)2 * C * es;
    ad.dq_rs = ad.dk_rs = ad.dv_rs = 3 * C; ad.dq_bs = ad.dk_bs = ad.dv_bs = T * 3 * C;
    if ((rc = cwdm_attention_backward(&ad, stream))) return rc;
    // ---- qkv: bias, weight (rows back to the model's order), input gradient
    const bool legacy = !u->cfg.attn_new_order;
    float* dwp = legacy ? reinterpret_cast<float*>(gb + G.at_dw) : GR(at.qkv_w_p);
    float* dbp = legacy ? dwp + (int64_t)3 * C * C : GR(at.qkv_b_p);
    if (legacy) CWDM_HIP(hipMemsetAsync(dwp, 0, ((int64_t)3 * C * C + 3 * C) * 4, s));
    if ((rc = bias_grad(dqkv, lv, 3 * C, dbp))) return rc;
    if ((rc = wgrad(lv, 1, wb + L.attn_n, C, nullptr, 0, 0, nullptr, dqkv, 3 * C, 3 * C, dwp))) return rc;
    if (legacy) {
      if ((rc = cwdm::attn_unperm_add(dwp, GR(at.qkv_w_p), 3 * C, C, at.heads, at.ch, s))) return rc;
      if ((rc = cwdm::attn_unperm_add(dbp, GR(at.qkv_b_p), 3 * C, 1, at.heads, at.ch, s))) return rc;
    }
    if ((rc = cwdm::attn_linear(dt, B, T, 3 * C, C, dqkv, nullptr, pb + at.qkvT_off, nullptr, nullptr, dn, nullptr,
                                nullptr, s)))
      return rc;
    // ---- the norm (no activation) and the residual: dx = dy + dGN(dn)
    return cwdm::gn_lin_bwd(dt, B, T, C, u->cfg.num_groups, act(xt), dn, mr_of(at.gn), P(g.gamma_off), grd(o),
                            grd(xt), take_acc(xt), reinterpret_cast<float*>(gb + G.at_part), GR(g.gamma_p),
                            GR(g.beta_p), s);
  }

  // ---- WavUNetModel WaveletDownsample (wunet.py:131-145): out = conv(cat(DWT(pyr)) / 3) + h
  int wav_pyramid(const Block& bk) {
    const auto& cs = u->convs[bk.c1];
    const auto& hp = u->haars[bk.haar];
    const int o = cs.out, lv = cs.level;
    int rc;
    if ((rc = bias_grad(grd(o), lv, cs.cout, GR(cs.b_p)))) return rc;
    if ((rc = wgrad(lv, 3, act(hp.out), cs.cin_a, nullptr, 0, 0, nullptr, grd(o), cs.cout, cs.cout, GR(cs.w_p))))
      return rc;
    if ((rc = resample_add(cs.res, grd(o), cs.cout, lv, 0))) return rc;
    if (hp.src == u->input_tensor) return CWDM_OK;   // the level-0 pyramid is the model input: no gradient
    if ((rc = dgrad(bk.c1, grd(o)))) return rc;
    const int cp = u->tensors[hp.src].channels;
    return haar_nd_synth_add(dt, B, D >> lv, H >> lv, W >> lv, cp, tmp, 8LL * cp, hp.lll_scale,
                             reinterpret_cast<unsigned char*>(tmp) + (int64_t)cp * es, 8LL * cp, hp.high_scale,
                             grd(hp.src), take_acc(hp.src), s);
  }

  // ---- WavUNetModel ResBlock that resamples by DWT / IDWT after its first conv (wunet.py:210-269)
  int wav_resblock(const Block& bk) {
    const bool down = bk.kind == BlockKind::WavDown;
    const auto& c1 = u->convs[bk.c1];
    const auto& c2 = u->convs[bk.c2];
    const auto& hh = u->haars[bk.hh];
    const auto& hx = u->haars[bk.hx];
    const int lout = c2.level, lin = c1.level, o = c2.out, h1 = c1.out, cout = c2.cout, cin = nch(bk.x0);
    int rc;
    // ---- conv2 + the residual x_upd
    if ((rc = bias_grad(grd(o), lout, cout, GR(c2.b_p)))) return rc;
    if ((rc = wgrad_c(bk.c2, lout, act(hh.out), cout, nullptr, 0, 0, ss_of(bk.g2), grd(o), cout, cout, GR(c2.w_p))))
      return rc;
    if ((rc = resample_add(hx.out, grd(o), cout, lout, 0))) return rc;
    Pre pre2;
    if ((rc = dgrad_gn(bk.c2, grd(o), bk.g2, hh.out, -1, pre2))) return rc;
    // ---- GN2 -> d(h + emb), with its channel sums = the emb projection's gradient
    const GnBwdOpt g2{deb + u->emb_rows_off[bk.emb_k], u->R};
    if ((rc = gn_bwd(bk.g2, hh.out, -1, 0, pre2, g2))) return rc;
    if ((rc = emb_bwd(bk.emb_k))) return rc;
    // ---- the resampling adjoints (orthonormal Haar: analysis <-> synthesis)
    const int lc = down ? lout : lin;   // the coarse grid of this block's DWT / IDWT
    const int64_t dc = D >> lc, hc = H >> lc, wc = W >> lc;
    if (down) {
      // h = DWT(h1): LLL / 3 (+ emb) continues, the 7 high bands are the skip
      const int sk = hh.high_out;
      const void* dsk = u->ginit[sk] ? grd(sk) : nullptr;   // (no later user: zero)
      if ((rc = haar_nd_synth_add(dt, B, dc, hc, wc, cout, grd(hh.out), cout, hh.lll_scale, dsk, 7LL * cout,
                                  hh.high_scale, grd(h1), take_acc(h1), s)))
        return rc;
      if ((rc = haar_nd_synth_add(dt, B, dc, hc, wc, cin, grd(hx.out), cin, hx.lll_scale, nullptr, 0, 0.f,
                                  grd(bk.x0), take_acc(bk.x0), s)))
        return rc;
    } else {
      // h = IDWT(3 h1, skip) (+ emb), x_upd = IDWT(3 x, skip): both feed the skip bands' gradient
      const int sk = hh.high_in;
      const int a_h1 = take_acc(h1), a_sk = take_acc(sk);
      if ((rc = haar_nd_anal_add(dt, B, dc, hc, wc, cout, grd(hh.out), grd(h1), cout, hh.lll_scale, a_h1, grd(sk),
                                 7LL * cout, hh.high_scale, a_sk, s)))
        return rc;
      const int a_x0 = take_acc(bk.x0), a_sk2 = take_acc(sk);
      if ((rc = haar_nd_anal_add(dt, B, dc, hc, wc, cin, grd(hx.out), grd(bk.x0), cin, hx.lll_scale, a_x0, grd(sk),
                                 7LL * cin, hx.high_scale, a_sk2, s)))
        return rc;
    }
    // ---- conv1 (own bias; the emb is added after the resampling) and GN1
    if ((rc = bias_grad(grd(h1), lin, cout, GR(c1.b_p)))) return rc;
    if ((rc = wgrad_c(bk.c1, lin, act(bk.x0), cin, nullptr, 0, 0, ss_of(bk.g1), grd(h1), cout, cout, GR(c1.w_p))))
      return rc;
    Pre pre1;
    if ((rc = dgrad_gn(bk.c1, grd(h1), bk.g1, bk.x0, -1, pre1))) return rc;
    return gn_bwd(bk.g1, bk.x0, -1, 0, pre1);
  }

  // ---- Downsample stride-2 conv / Upsample nearest + conv (resblock_updown=False)
  int resample_layer(const Block& bk) {
    const auto& cs = u->convs[bk.c1];
    const int o = cs.out, xt = bk.x0, lv = cs.level;
    const int chn = u->tensors[xt].channels, lx = u->tensors[xt].level;
    int rc;
    if ((rc = bias_grad(grd(o), lv, cs.cout, GR(cs.b_p)))) return rc;
    if (bk.kind == BlockKind::Upsample) {
      if ((rc = wgrad(lv, 3, act(xt), chn, nullptr, 0, 1, nullptr, grd(o), cs.cout, cs.cout, GR(cs.w_p)))) return rc;
      if ((rc = dgrad(bk.c1, grd(o)))) return rc;
      return resample_add(xt, tmp, chn, lx, 1);
    }
    const auto& sd = u->s2ds[bk.s2d];
    float* dwe = reinterpret_cast<float*>(gb + G.dwe);
    CWDM_HIP(hipMemsetAsync(dwe, 0, (int64_t)cs.cout * cs.cin_a * 27 * 4, s));
    if ((rc = wgrad(lv, 3, act(sd.out), cs.cin_a, nullptr, 0, 0, nullptr, grd(o), cs.cout, cs.cout, dwe))) return rc;
    if ((rc = cwdm_conv3d_s2_fold_dw(dwe, cs.cout, chn, GR(cs.w_p), 1, stream))) return rc;
    if ((rc = dgrad(bk.c1, grd(o)))) return rc;
    return cwdm_space_to_depth(tmp, chn, B, D >> lv, H >> lv, W >> lv, dt, grd(xt), 0, take_acc(xt), stream);
  }

  // ---- ResBlock (Res / ResUp / ResDown), in the stages of the comment above
  // 1x1 skip dgrad into dx0 / dx1 (dual output)
  cwdm_conv3d_desc skip_dgrad_desc(const Block& bk) const {
    const auto& c2 = u->convs[bk.c2];
    cwdm_conv3d_desc d{};
    d.dtype = dt; d.B = B; d.D = D >> c2.level; d.H = H >> c2.level; d.W = W >> c2.level;
    d.cout = nch(c2.sb0) + nch(c2.sb1); d.res_mode = -1;
    d.b0 = grd(c2.out); d.b_c0 = c2.cout; d.b_w = pb + u->dgs_off[bk.c2];
    d.out = grd(c2.sb0); d.out_dtype = dt;
    if (c2.sb1 >= 0) { d.out1 = grd(c2.sb1); d.out_c0 = nch(c2.sb0); }
    return d;
  }
  // (its route would take an offered apply)
  bool skip_takes_gapply(const Block& bk) const {
    const cwdm_conv3d_desc d = skip_dgrad_desc(bk);
    cwdm::GapplyFuse probe{};
    cwdm::ConvCall cc;
    cc.gapply = &probe;
    return cwdm::conv_route(&d, cc).takes_gapply;
  }
  int skip_dgrad(const Block& bk, cwdm::GapplyFuse* gf) {
    const auto& c2 = u->convs[bk.c2];
    cwdm_conv3d_desc d = skip_dgrad_desc(bk);
    // equalise the store/accumulate state of the two outputs
    int a0 = take_acc(c2.sb0), a1 = c2.sb1 >= 0 ? take_acc(c2.sb1) : a0;
    if (a0 != a1) {
      const int zid = a0 ? c2.sb1 : c2.sb0;
      const auto& zt = u->tensors[zid];
      CWDM_HIP(hipMemsetAsync(grd(zid), 0, B * vox(zt.level) * zt.channels * es, s));
      a0 = a1 = 1;
    }
    d.accumulate = a0;
    d.workspace = gb + G.split; d.ws_bytes = G.split_bytes;
    cwdm::ConvCall cc;
    cc.sync = sync; cc.gapply = gf;
    if (int r = cwdm::conv3d_forward(&d, cc, s)) return r;
    CWDM_REQUIRE(!gf || gf->used, CWDM_E_UNSUPPORTED, "train plan: skip dgrad did not take the fused apply");
    return CWDM_OK;
  }
  // additive skips: the block's input is (h + skip) / 2; once its gradient is complete, the adjoint
  // hands half of it to h and to the skip (whose encoder consumer runs later and accumulates)
  int avg_bwd(const Block& bk) {
    if (bk.avg < 0) return CWDM_OK;
    const auto& as = u->avgs[bk.avg];
    const int aa = take_acc(as.a), ab = take_acc(as.b);
    return cwdm_skip_avg_bwd(grd(as.out), grd(as.a), aa, grd(as.b), ab, dt, B, vox(as.level), as.channels, stream);
  }
  // GN2 -> dh1, with the per-channel sums of dh1 (the emb projection's
  // gradient) taken in the same pass when dh1 is written, not accumulated
  int resblock_gn2(const Block& bk, const Pre& pre2) {
    const auto& c1 = u->convs[bk.c1];
    const auto& g = u->gns[bk.g2];
    const int h1 = c1.out, cout = c1.cout, roff = u->emb_rows_off[bk.emb_k];
    const bool fuse_sum = !u->ginit[h1], film = g.film_row >= 0;
    // FiLM: the finalize writes d scale / d shift into the block's rows; conv1 has its own bias, whose
    // gradient (the sum of dh1 over voxels and batch) is the apply pass's channel sums finished per channel
    const float* ebias = reinterpret_cast<const float*>(wb + L.ebias);
    const cwdm::GnBwdFilm gf{P(g.beta_off), ebias + roff, u->R, deb + roff, u->R, fuse_sum ? GR(c1.b_p) : nullptr};
    GnBwdOpt o;
    if (film) o.film = &gf;
    else if (fuse_sum) { o.chs = deb + roff; o.chs_stride = u->R; }
    if (int rc = gn_bwd(bk.g2, h1, -1, 0, pre2, o)) return rc;
    if (fuse_sum) return CWDM_OK;
    // dh1 was accumulated: its sums (conv1's bias gradient / the emb rows') in a pass of their own
    if (film) return bias_grad(grd(h1), c1.level, cout, GR(c1.b_p));
    return cwdm_channel_sum(grd(h1), dt, B, vox(c1.level), cout, cout, deb + roff, u->R, nullptr, nullptr,
                            gb + G.chs, G.chs_bytes, stream);
  }
  int resblock(const Block& bk) {
    const auto& c1 = u->convs[bk.c1];
    const auto& c2 = u->convs[bk.c2];
    const int lout = c2.level, o = c2.out, h1 = c1.out, cout = c2.cout, mode = resample_mode(bk.kind);
    int rc;
    // ---- conv2 (+ skip / residual)
    if ((rc = bias_grad(grd(o), lout, cout, GR(c2.b_p), c2.wsb_p >= 0 ? GR(c2.wsb_p) : nullptr))) return rc;
    // (a dropout block's conv2 read u = the dropout step's output, activated and masked already)
    const DropStep* ds = bk.drop >= 0 ? &u->drops[bk.drop] : nullptr;
    if (ds) rc = wgrad(lout, 3, act(ds->out), cout, nullptr, 0, 0, nullptr, grd(o), cout, cout, GR(c2.w_p));
    else rc = wgrad_c(bk.c2, lout, act(h1), cout, nullptr, 0, 0, ss_of(bk.g2), grd(o), cout, cout, GR(c2.w_p));
    if (rc) return rc;
    // with skip_gapply the GroupNorm-1 backward's apply pass rides in the skip dgrad's epilogue
    // (GapplyFuse), so that conv runs after GN1's reduce / finalize below
    static const bool gapply_on = env_not0("CWDM_GAPPLY_FUSE");
    const bool skip_gapply = c2.ws_p >= 0 && gapply_on && bk.kind == BlockKind::Res && c2.sb0 == bk.x0 &&
                             c2.sb1 == bk.x1 && skip_takes_gapply(bk);
    if (c2.ws_p >= 0) {
      if ((rc = wgrad(lout, 1, act(c2.sb0), nch(c2.sb0), act(c2.sb1), nch(c2.sb1), 0, nullptr, grd(o), cout, cout,
                      GR(c2.ws_p))))
        return rc;
      if (!skip_gapply && (rc = skip_dgrad(bk, nullptr))) return rc;
    } else {
      // identity residual (possibly through the block's resampling)
      if ((rc = resample_add(bk.x0, grd(o), cout, u->tensors[bk.x0].level, mode))) return rc;
    }
    Pre pre2;
    if (ds) {
      // du = conv2's plain input gradient, masked and scaled in place by the regenerated mask; the GroupNorm
      // backward then takes its own reduce pass (a dgrad epilogue's partials would be of the unmasked gradient)
      if ((rc = dgrad(bk.c2, grd(o)))) return rc;
      if ((rc = cwdm_dropout_bwd(tmp, dt, B, vox(lout), cout, u->cfg.dropout, u->dropout_seed, ds->site, stream)))
        return rc;
    } else if ((rc = dgrad_gn(bk.c2, grd(o), bk.g2, h1, -1, pre2))) {
      return rc;
    }
    if ((rc = resblock_gn2(bk, pre2))) return rc;
    // ---- conv1: emb projection, wgrad, dgrad
    if ((rc = emb_bwd(bk.emb_k))) return rc;
    if (bk.kind == BlockKind::ResDown) {
      const auto& ps = u->pools[bk.pool];
      if ((rc = wgrad(lout, 3, act(ps.out_h), ps.channels, nullptr, 0, 0, nullptr, grd(h1), cout, cout, GR(c1.w_p))))
        return rc;
    } else if ((rc = wgrad_c(bk.c1, lout, act(bk.x0), nch(bk.x0), act(bk.x1), nch(bk.x1), mode, ss_of(bk.g1), grd(h1),
                             cout, cout, GR(c1.w_p)))) {
      return rc;
    }
    // ---- GN1 (+ resample adjoint) -> dx0 / dx1 (the reduce in the dgrad's epilogue
    // when the GroupNorm's grid is the conv's: no resampling in between)
    Pre pre1;
    rc = bk.kind == BlockKind::Res ? dgrad_gn(bk.c1, grd(h1), bk.g1, bk.x0, bk.x1, pre1) : dgrad(bk.c1, grd(h1));
    if (rc) return rc;
    if (skip_gapply) {
      // GN1 reduce / finalize, then the skip dgrad applying it: dx = skip + GN1 backward
      const float* coef = nullptr;
      GnBwdOpt g1;
      g1.coef_out = &coef; g1.keep_acc = true;
      if ((rc = gn_bwd(bk.g1, bk.x0, bk.x1, 0, pre1, g1))) return rc;
      cwdm::GapplyFuse gf{};
      gf.x0 = act(bk.x0); gf.x1 = act(bk.x1); gf.du = tmp; gf.ss = ss_of(bk.g1); gf.coef = coef;
      if ((rc = skip_dgrad(bk, &gf))) return rc;
    } else if ((rc = gn_bwd(bk.g1, bk.x0, bk.x1, mode, pre1))) {
      return rc;
    }
    return avg_bwd(bk);
  }

  // ---- the last segment: conv_in + time_embed
  // conv_in's weight gradient: of the model's own input channels only, whatever the kernels ran on (StemPad)
  int stem_wgrad() {
    const auto& c0 = u->convs[0];
    const void* xin = act(c0.a0);   // x, or the forward's staged copy
    const StemPad sp = stem_pad(u, B, D, H, W);
    if (!sp.cw) return wgrad(0, 3, xin, c0.cin_a, nullptr, 0, 0, nullptr, grd(c0.out), c0.cout, c0.cout, GR(c0.w_p));
    int rc;
    unsigned char* scratch = reinterpret_cast<unsigned char*>(tmp);
    if (sp.x_bytes) {
      if ((rc = cwdm::pad_channels(xin, c0.cin_a, scratch, sp.cw, dt, B * vox(0), s))) return rc;
      xin = scratch;
    }
    float* dwp = reinterpret_cast<float*>(scratch + sp.x_bytes);
    CWDM_HIP(hipMemsetAsync(dwp, 0, sp.dw_bytes, s));
    if ((rc = wgrad(0, 3, xin, sp.cw, nullptr, 0, 0, nullptr, grd(c0.out), c0.cout, c0.cout, dwp))) return rc;
    // dw[co][ci][tap] for ci < the parameter's input channels (the rest: zero inputs' columns, dropped)
    const int ci = c0.w_cin();
    const int64_t ss_[3] = {(int64_t)sp.cw * 27, 27, 1}, ds_[3] = {(int64_t)ci * 27, 27, 1};
    return cwdm_copy3(dwp, CWDM_F32, ss_, GR(c0.w_p), CWDM_F32, ds_, c0.cout, ci, 27, stream);
  }
  int stem() {
    const auto& c0 = u->convs[0];
    int rc;
    if ((rc = bias_grad(grd(c0.out), 0, c0.cout, GR(c0.b_p)))) return rc;
    if ((rc = stem_wgrad())) return rc;
    if ((rc = launch_temb_bwd(t, (int)B, u->cfg.model_channels, P(u->off_te_w1), P(u->off_te_b1), P(u->off_te_w2), temb,
                              dsil, GR(u->te_w1), GR(u->te_b1), GR(u->te_w2), GR(u->te_b2), s)))
      return rc;
    // class conditioning: emb = time_embed(t) + label_emb[y], so the table's rows collect the same gradient
    if (u->label_w < 0) return CWDM_OK;
    return launch_label_emb_bwd(temb, dsil, u->labels, (int)B, u->E, u->cfg.num_classes, GR(u->label_w), s);
  }
};

}  // namespace

extern "C" int cwdm_unet_backward(cwdm_unet* u, const void* packed, const void* packed_bwd, const void* x,
                                  const float* t, const float* dout, float* grads, int64_t B, int64_t D, int64_t H,
                                  int64_t W, const void* ws, int64_t ws_bytes, void* gws, int64_t gws_bytes,
                                  int seg_begin, int seg_end, cwdm_stream_t stream) {
  CWDM_REQUIRE(u && packed && packed_bwd && x && t && dout && grads && ws && gws, CWDM_E_INVALID,
               "cwdm_unet_backward: null pointer");
  const int nb = (int)u->blocks.size(), nseg = nb + 2;
  CWDM_REQUIRE(0 <= seg_begin && seg_begin <= seg_end && seg_end <= nseg, CWDM_E_INVALID,
               "cwdm_unet_backward: bad segment range");
  CWDM_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, CWDM_E_SHAPE, "cwdm_unet_backward: empty grid");
  CWDM_REQUIRE(u->cfg.num_classes == 0 || u->labels, CWDM_E_INVALID,
               "cwdm_unet_backward: a class-conditional plan needs its labels (cwdm_unet_set_labels)");
  const int64_t div = int64_t(1) << (u->cfg.num_levels - (u->cfg.use_freq ? 0 : 1));
  CWDM_REQUIRE(D % div == 0 && H % div == 0 && W % div == 0, CWDM_E_SHAPE,
               "cwdm_unet_backward: every subband edge must be divisible by " + std::to_string(div));
  const Layout L = layout(u, B, D, H, W);
  const GLayout G = glayout(u, B, D, H, W);
  CWDM_REQUIRE(ws_bytes >= L.total, CWDM_E_WORKSPACE, "cwdm_unet_backward: forward workspace too small");
  CWDM_REQUIRE(gws_bytes >= G.total, CWDM_E_WORKSPACE,
               "cwdm_unet_backward: grad workspace too small (need " + std::to_string(G.total) + " bytes)");
  CWDM_REQUIRE(seg_begin == 0 || (int)u->ginit.size() == (int)u->tensors.size(), CWDM_E_INVALID,
               "cwdm_unet_backward: segment 0 must run first");
  using UC = unsigned char;
  Backward bw{{u, L, reinterpret_cast<const UC*>(packed), static_cast<UC*>(const_cast<void*>(ws)), x, B, D, H, W, stream},
              G, reinterpret_cast<const UC*>(packed_bwd), reinterpret_cast<UC*>(gws), t, dout, grads,
              L.train_total > L.total && ws_bytes >= L.train_total};
  // (every call: a caller may run segments on a fresh grad workspace)
  CWDM_HIP(hipMemsetAsync(bw.sync, 0, cwdm::plan_sync_bytes(), bw.s));
  // segment 0 the output head, then the blocks last to first, then conv_in + time_embed
  for (int seg = seg_begin; seg < seg_end; ++seg) {
    int rc = CWDM_OK;
    if (seg == 0) rc = bw.head();
    else if (seg > nb) rc = bw.stem();
    else switch (const Block& bk = u->blocks[nb - seg]; bk.kind) {
      case BlockKind::Attention: rc = bw.attention(bk); break;
      case BlockKind::WavPyramid: rc = bw.wav_pyramid(bk); break;
      case BlockKind::WavDown:
      case BlockKind::WavUp: rc = bw.wav_resblock(bk); break;
      case BlockKind::Downsample:
      case BlockKind::Upsample: rc = bw.resample_layer(bk); break;
      case BlockKind::Res:
      case BlockKind::ResUp:
      case BlockKind::ResDown: rc = bw.resblock(bk); break;
    }
    if (rc) return rc;
  }
  return CWDM_OK;
}
