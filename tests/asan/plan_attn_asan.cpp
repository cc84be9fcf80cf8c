// Host-side AddressSanitizer / UBSan check of the attention plans (no GPU): the
// U-Net plan builder with bottleneck_attention for the config-1 and production
// topologies, both qkv row orders, one grid each -- parameter contract and
// order around the block, aliases, inference / training / gradient workspace
// sizes, traces, backward segments, FLOPs -- and the refusals of
// cwdm_unet_create and of the attention entry points' argument checks.  A
// stand-alone program (its own main) linked against the sanitized objects of
// tests/asan/build.sh by tests/test_asan_attn_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cwdm.h"

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                      \
    }                                                               \
  } while (0)

static cwdm_unet_config cfg(int mc, int nrb, std::vector<int> mult, int dtype, int groups, int heads, int head_ch,
                            int new_order) {
  cwdm_unet_config c;
  std::memset(&c, 0, sizeof(c));
  c.in_channels = 32; c.model_channels = mc; c.out_channels = 8; c.num_res_blocks = nrb;
  c.num_levels = (int)mult.size();
  for (size_t i = 0; i < mult.size(); ++i) c.channel_mult[i] = mult[i];
  c.num_groups = groups; c.dtype = dtype; c.resblock_updown = 1;
  c.bottleneck_attention = 1; c.num_heads = heads; c.num_head_channels = head_ch; c.attn_new_order = new_order;
  return c;
}

static void exercise(const cwdm_unet_config& c, int64_t n) {
  cwdm_unet* u = nullptr;
  cwdm_unet* plain = nullptr;
  cwdm_unet_config off = c;
  off.bottleneck_attention = 0;
  CHECK(cwdm_unet_create(&c, &u) == CWDM_OK && u);
  CHECK(cwdm_unet_create(&off, &plain) == CWDM_OK && plain);
  if (!u || !plain) { std::fprintf(stderr, "  %s\n", cwdm_last_error()); return; }
  const int C = c.channel_mult[c.num_levels - 1] * c.model_channels;
  const int np = cwdm_unet_num_params(u);
  CHECK(np == cwdm_unet_num_params(plain) + 6);
  char name[256];
  int64_t shape[5];
  int nd = 0, first = -1;
  int64_t numel = 0, before = 0;
  const char* want[6] = {"middle_block.1.norm.weight", "middle_block.1.norm.bias", "middle_block.1.qkv.weight",
                         "middle_block.1.qkv.bias", "middle_block.1.proj_out.weight", "middle_block.1.proj_out.bias"};
  for (int i = 0; i < np; ++i) {
    CHECK(cwdm_unet_param_info(u, i, name, sizeof(name), shape, &nd) == CWDM_OK);
    if (first < 0 && std::strcmp(name, want[0]) == 0) { first = i; before = numel; }
    int64_t k = 1;
    for (int d = 0; d < nd; ++d) k *= shape[d];
    numel += k;
  }
  CHECK(first > 0 && first + 6 < np);
  for (int j = 0; first > 0 && j < 6; ++j) {
    CHECK(cwdm_unet_param_info(u, first + j, name, sizeof(name), shape, &nd) == CWDM_OK);
    CHECK(std::strcmp(name, want[j]) == 0);
    if (j == 2) CHECK(nd == 3 && shape[0] == 3 * C && shape[1] == C && shape[2] == 1);
    if (j == 4) CHECK(nd == 3 && shape[0] == C && shape[1] == C && shape[2] == 1);
  }
  if (first > 0) {
    CHECK(cwdm_unet_param_info(u, first - 1, name, sizeof(name), shape, &nd) == CWDM_OK);
    CHECK(std::strncmp(name, "middle_block.0.", 15) == 0);
    CHECK(cwdm_unet_param_info(u, first + 6, name, sizeof(name), shape, &nd) == CWDM_OK);
    CHECK(std::strncmp(name, "middle_block.2.", 15) == 0);
  }
  CHECK(cwdm_unet_num_aliases(u) == 0);
  CHECK(cwdm_unet_alias_info(u, 0, name, sizeof(name), nullptr, nullptr) != CWDM_OK);
  CHECK(cwdm_unet_packed_bytes(u) > cwdm_unet_packed_bytes(plain));
  CHECK(cwdm_unet_packed_bwd_bytes(u) > cwdm_unet_packed_bwd_bytes(plain));
  const int64_t div = int64_t(1) << (c.num_levels - 1);
  const int64_t T = (n / div) * (n / div) * (2 * n / div);
  for (int64_t b : {1, 2}) {
    const int64_t ws = cwdm_unet_workspace_bytes(u, b, n, n, 2 * n);
    const int64_t tws = cwdm_unet_train_workspace_bytes(u, b, n, n, 2 * n);
    CHECK(ws > cwdm_unet_workspace_bytes(plain, b, n, n, 2 * n));
    CHECK(tws > ws);   // the log-sum-exp rows and the normalised input
    CHECK(tws - ws >= cwdm_unet_train_workspace_bytes(plain, b, n, n, 2 * n) - cwdm_unet_workspace_bytes(plain, b, n, n, 2 * n));
    CHECK(cwdm_unet_grad_workspace_bytes(u, b, n, n, 2 * n) > cwdm_unet_grad_workspace_bytes(plain, b, n, n, 2 * n));
    const double df = cwdm_unet_flops(u, b, n, n, 2 * n) - cwdm_unet_flops(plain, b, n, n, 2 * n);
    const double wantf = 2.0 * b * T * C * (4.0 * C + 2.0 * T);
    CHECK(df > 0 && df > wantf * (1 - 1e-9) && df < wantf * (1 + 1e-9));
    CHECK(cwdm_unet_backward_flops(u, b, n, n, 2 * n) > 0);
    const int tc = cwdm_unet_trace_count(u);
    CHECK(tc == cwdm_unet_trace_count(plain) + 1);
    for (int i = 0; i < tc; ++i) {
      int64_t o = 0;
      int ch = 0, lv = 0;
      CHECK(cwdm_unet_trace_info(u, i, b, n, n, 2 * n, &o, &ch, &lv) == CWDM_OK);
      CHECK(o < ws && ch > 0 && lv >= 0 && lv < c.num_levels);
    }
  }
  const int ns = cwdm_unet_backward_segments(u);
  CHECK(ns == cwdm_unet_backward_segments(plain) + 1);
  int64_t total = 0;
  bool own = false;
  for (int s = 0; s < ns; ++s) {
    int64_t o = -1, cnt = -1;
    CHECK(cwdm_unet_segment_range(u, s, &o, &cnt) == CWDM_OK);
    CHECK(o >= 0 && cnt >= 0 && o + cnt <= numel);
    total += cnt;
    if (o == before && cnt == (int64_t)4 * C * C + 6 * C) own = true;
  }
  CHECK(total == numel);
  CHECK(own);   // the block's parameters are one segment
  CHECK(cwdm_unet_segment_range(u, ns, nullptr, nullptr) != CWDM_OK);
  cwdm_unet_destroy(u);
  cwdm_unet_destroy(plain);
}

int main() {
  for (int dt : {CWDM_F32, CWDM_BF16, CWDM_F16})
    for (int order : {0, 1}) {
      exercise(cfg(32, 1, {1, 2}, dt, 8, 4, 0, order), 16);              // config 1, 4 heads of 16: T = 8 x 8 x 16
      exercise(cfg(64, 2, {1, 2, 2, 4, 4}, dt, 32, 0, 64, order), 112);  // production, 64-channel heads: T = 7 x 7 x 14
    }
  exercise(cfg(64, 2, {1, 2, 2, 4, 4}, CWDM_BF16, 32, 0, 0, 0), 128);    // num_heads 0 reads as one head of 256
  // refusals: each with a message, never a crash
  cwdm_unet* u = nullptr;
  auto bad = cfg(32, 1, {1, 3}, CWDM_BF16, 8, 0, 24, 0);                  // ch = 24
  CHECK(cwdm_unet_create(&bad, &u) == CWDM_E_UNSUPPORTED && std::strstr(cwdm_last_error(), "multiple of 16"));
  bad = cfg(32, 1, {1, 2}, CWDM_BF16, 8, 3, 0, 0);                        // 64 channels, 3 heads
  CHECK(cwdm_unet_create(&bad, &u) == CWDM_E_UNSUPPORTED && std::strstr(cwdm_last_error(), "not divisible"));
  bad = cfg(32, 1, {1, 2}, CWDM_BF16, 8, 0, 48, 0);                       // 64 % 48
  CHECK(cwdm_unet_create(&bad, &u) == CWDM_E_UNSUPPORTED);
  bad = cfg(64, 2, {1, 8}, CWDM_BF16, 32, 1, 0, 0);                       // one head of 512
  CHECK(cwdm_unet_create(&bad, &u) == CWDM_E_UNSUPPORTED && std::strstr(cwdm_last_error(), "256"));
  bad = cfg(32, 2, {1, 2}, CWDM_BF16, 8, 1, 0, 0);
  bad.use_freq = 1;                                                       // WavUNetModel
  CHECK(cwdm_unet_create(&bad, &u) == CWDM_E_UNSUPPORTED && std::strstr(cwdm_last_error(), "use_freq"));
  CHECK(u == nullptr);
  // the entry points' argument checks return before any launch
  CHECK(cwdm_attention_forward(nullptr, nullptr) == CWDM_E_INVALID);
  cwdm_attention_desc d;
  std::memset(&d, 0, sizeof(d));
  d.dtype = CWDM_BF16; d.B = 1; d.T = 16; d.heads = 1; d.ch = 24;
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_UNSUPPORTED && std::strstr(cwdm_last_error(), "multiple of 16"));
  d.ch = 272;
  CHECK(cwdm_attention_backward(&d, nullptr) == CWDM_E_UNSUPPORTED);
  d.ch = 64; d.T = 0;
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_SHAPE);
  d.T = 16;
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_INVALID);           // null q / k / v / o
  // batch strides (B > 1): refused before anything is launched, so the pointers only need to look aligned
  d.B = 2;
  d.q = d.k = d.v = reinterpret_cast<const void*>(uintptr_t(4096));
  d.o = reinterpret_cast<void*>(uintptr_t(8192));
  d.q_rs = d.k_rs = d.v_rs = d.o_rs = 64;
  d.q_bs = d.k_bs = d.v_bs = d.o_bs = 16 * 64;
  d.k_bs = 16 * 64 + 4;                                                   // batch 1 of k not 16-byte aligned
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_SHAPE && std::strstr(cwdm_last_error(), "batch stride"));
  d.k_bs = 16 * 64;
  d.o_bs = 0;                                                             // both batches would write the same rows
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_SHAPE && std::strstr(cwdm_last_error(), "batch stride"));
  d.o_bs = 15 * 64 + 32;                                                  // batch 1 would start inside batch 0's last row
  CHECK(cwdm_attention_forward(&d, nullptr) == CWDM_E_SHAPE);
  cwdm_attn_linear_desc l;
  std::memset(&l, 0, sizeof(l));
  l.dtype = CWDM_F32; l.B = 1; l.T = 4; l.K = 24; l.N = 64;
  CHECK(cwdm_attn_linear(&l, nullptr) == CWDM_E_INVALID);                 // null pointers
  CHECK(cwdm_attn_linear(nullptr, nullptr) == CWDM_E_INVALID);
  CHECK(cwdm_attn_pack(nullptr, 4, 4, 1, 4, 0, 0, CWDM_F32, nullptr, nullptr) == CWDM_E_INVALID);
  CHECK(cwdm_attn_parts(512) == 32 && cwdm_attn_parts(343) == 22 && cwdm_attn_parts(1) == 1 && cwdm_attn_parts(0) < 0);
  if (fails) {
    std::fprintf(stderr, "%d contract checks failed\n", fails);
    return 1;
  }
  std::printf("plan_attn_asan: ok\n");
  return 0;
}
