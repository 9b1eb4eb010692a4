// NesT (nest.py:150-216): patch embedding (Rearrange + 1x1 Conv2D, i.e. unfold + Dense, :178-181); per hierarchy level the block partition
// 'b (b1 h) (b2 w) c -> (b b1 b2) h w c' fused with the positional add (:140-142,209), block_repeats[i] transformer blocks on the (b * blocks^2)
// independent sequences (one ViT engine per level whose vitx_config.nest_block is set: to_out always kept, plain small-head attention kernels,
// engine.hip), the inverse partition (:211) and -- except at the last level -- Aggregate (:111-123): Conv2D 3x3 'SAME' with bias as im2col rows
// (cct_tok.hip) times the HWIO kernel viewed as [9 Cin, Cout] in image chunks, the channel LayerNorm (eps 1e-5), MaxPool2D 3/2 'SAME'
// (nest_ops.hip); then LayerNorm, the mean over the map and Dense (:196-200).  Every 1x1 Conv2D of the reference is a Dense over the channel axis.
// Everything outside the engines keeps fp32 storage; in the bf16 / bf16x3 modes its large GEMMs take the split-operand (hi + lo bf16) MFMA path.
// The composite owns the public parameter / gradient arenas in its own table order and copies them to / from the engines.
// Only the deterministic path exists (dropout 0).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

constexpr int NEST_MAX_LEVELS = 8;

// one entry of nest_layers (nest.py:187-194) with the geometry of its map and of the aggregation behind it
struct NestLevel {
  int d = 0, heads = 0, dh = 0, inner = 0, depth = 0;   // layer_dims / layer_heads (:171-172), dim_head = d // heads (:80), block_repeats[i]
  int nb = 1, f = 0;                                    // block grid 2^(H-1-i) per side (:208); map extent fmap / 2^i
  int dn = 0, K = 0, Kp = 0, chunk = 1;                 // aggregation (not at the last level): filters, 9 * d, its row stride, images per pass
  int64_t pos = -1, conv_w = -1, conv_b = -1, ag_g = -1, ag_b = -1;   // arena offsets
  vitx_engine* eng = nullptr;                           // depth > 0
  std::vector<ArenaMap> maps;                           // the level's block tensors -> the engine's
  float *x_in = nullptr, *out = nullptr;                // [B, f, f, d]: the level's input map (embedded / the pooled map below) and its output
  float *conv = nullptr, *ln = nullptr, *pooled = nullptr, *mean = nullptr, *rstd = nullptr;   // [B, f, f, dn] x 2, [B, f/2, f/2, dn], [B f f] x 2
};

}  // namespace

struct vitx_nest {
  vitx_nest_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<NestLevel> lv;
  vitx_engine* prof_eng = nullptr;   // the composite's own launches are booked on the first engine
  int64_t emb_w = -1, emb_b = -1, head_g = -1, head_b = -1, fc_w = -1, fc_b = -1;
  int fmap = 0, hb = 0, n = 0, pd = 0, nc = 0, B = 0, x3 = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *patches = nullptr, *dpatches = nullptr, *tok_a = nullptr, *tok_b = nullptr, *rows = nullptr, *drows = nullptr, *gw_part = nullptr, *gw_slices = nullptr;
  float *xn = nullptr, *mean = nullptr, *rstd = nullptr, *pooled = nullptr, *dpooled = nullptr, *g[3] = {nullptr, nullptr, nullptr};
  float *dpos_part = nullptr, *ws = nullptr;
  bool have_fwd = false;
  int b = 0;
};

namespace {

// levels and their geometry (nest.py:163-176); "" or what is wrong with the configuration
std::string nest_geometry(const vitx_nest_config& c, std::vector<NestLevel>& out) {
  out.clear();
  if (c.image_size <= 0 || c.patch_size <= 0 || c.num_classes <= 0 || c.dim <= 0 || c.heads <= 0 || c.num_hierarchies <= 0 || c.mlp_mult <= 0)
    return "invalid NesT configuration";
  if (c.num_hierarchies > NEST_MAX_LEVELS) return "num_hierarchies must be <= 8";
  if (c.image_size % c.patch_size) return "Image dimensions must be divisible by the patch size.";   // nest.py:163
  const int H = c.num_hierarchies, fmap = c.image_size / c.patch_size, blocks = 1 << (H - 1);
  if (fmap % blocks)
    return "the feature map (image_size / patch_size = " + std::to_string(fmap) + ") must be divisible by 2^(num_hierarchies - 1) = " +
           std::to_string(blocks) + " (the reference fails there inside its block rearrange, nest.py:209)";
  if ((int64_t)c.dim << (H - 1) > 4096) return "dim * 2^(num_hierarchies - 1) must be <= 4096";
  for (int i = 0; i < H; ++i) {
    if (c.block_repeats[i] < 0) return "block_repeats must be >= 0";
    NestLevel L;
    L.d = c.dim << i; L.heads = c.heads << i; L.dh = L.d / L.heads; L.inner = L.dh * L.heads; L.depth = c.block_repeats[i];
    if (L.dh <= 0) return "dim must be >= heads (dim_head = dim // heads, nest.py:80)";
    L.nb = 1 << (H - 1 - i); L.f = fmap >> i;
    if (i < H - 1) { L.dn = c.dim << (i + 1); L.K = 9 * L.d; L.Kp = (int)round_up(L.K, 64); }
    out.push_back(L);
  }
  return "";
}

}  // namespace

// Table of NesT's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string nest_param_table(const vitx_nest_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_nest* m = nullptr) {
  out.clear();
  std::vector<NestLevel> lv;
  const std::string e = nest_geometry(c, lv);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  const int64_t pd = (int64_t)c.patch_size * c.patch_size * 3, mult = c.mlp_mult;
  const int64_t hb = (c.image_size / c.patch_size) >> (c.num_hierarchies - 1), seq_len = hb * hb;
  const int64_t ew = tb.add("patch_embedding.kernel", {1, 1, pd, c.dim}), eb = tb.add("patch_embedding.bias", {c.dim});
  for (size_t i = 0; i < lv.size(); ++i) {
    NestLevel& L = lv[i];
    const int64_t d = L.d, inner = L.inner;
    const std::string pre = "nest_layers." + std::to_string(i);
    L.pos = tb.add(pre + ".transformer.pos_emb", {seq_len});
    for (int l = 0; l < L.depth; ++l) {
      const std::string p = pre + ".transformer." + std::to_string(l);
      tb.add(p + ".attn.norm.g", {1, 1, 1, d}); tb.add(p + ".attn.norm.b", {1, 1, 1, d});
      tb.add(p + ".attn.to_qkv.kernel", {1, 1, d, 3 * inner});
      tb.add(p + ".attn.to_out.kernel", {1, 1, inner, d}); tb.add(p + ".attn.to_out.bias", {d});
      tb.add(p + ".ff.norm.g", {1, 1, 1, d}); tb.add(p + ".ff.norm.b", {1, 1, 1, d});
      tb.add(p + ".ff.fc1.kernel", {1, 1, d, d * mult}); tb.add(p + ".ff.fc1.bias", {d * mult});
      tb.add(p + ".ff.fc2.kernel", {1, 1, d * mult, d}); tb.add(p + ".ff.fc2.bias", {d});
    }
    if (i + 1 < lv.size()) {
      L.conv_w = tb.add(pre + ".aggregate.conv.kernel", {3, 3, d, L.dn}); L.conv_b = tb.add(pre + ".aggregate.conv.bias", {L.dn});
      L.ag_g = tb.add(pre + ".aggregate.norm.g", {1, 1, 1, L.dn}); L.ag_b = tb.add(pre + ".aggregate.norm.b", {1, 1, 1, L.dn});
    }
  }
  const int64_t dl = lv.back().d;
  const int64_t hg = tb.add("mlp_head.norm.g", {1, 1, 1, dl}), hbt = tb.add("mlp_head.norm.b", {1, 1, 1, dl});
  const int64_t fw = tb.add("mlp_head.kernel", {dl, c.num_classes}), fb = tb.add("mlp_head.bias", {c.num_classes});
  if (m) {
    m->lv = lv;
    m->emb_w = ew; m->emb_b = eb; m->head_g = hg; m->head_b = hbt; m->fc_w = fw; m->fc_b = fb;
    m->fmap = c.image_size / c.patch_size; m->hb = (int)hb; m->n = (int)seq_len; m->pd = (int)pd; m->nc = c.num_classes;
  }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config nest_engine_config(const vitx_nest_config& c, const NestLevel& L, int n) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.image_h = 1; ec.image_w = n; ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.num_classes = 1; ec.dim = L.d; ec.depth = L.depth; ec.heads = L.heads; ec.dim_head = L.dh;
  ec.mlp_dim = L.d * c.mlp_mult; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.max_batch = c.max_batch * L.nb * L.nb; ec.device_id = c.device_id;
  ec.nest_block = 1;
  return ec;
}

// everything a configuration can be refused for without a device
int nest_check(const vitx_nest_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_nest probe;
  const std::string e = nest_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  if ((int64_t)c.max_batch * probe.lv[0].nb * probe.lv[0].nb > (1 << 24)) { err = "max_batch * blocks^2 too large"; return VITX_ERR_INVALID; }
  for (const NestLevel& L : probe.lv) {
    if (L.depth == 0) continue;
    if (c.compute == VITX_COMPUTE_BF16 && (L.d % 64 || L.inner % 64 || (L.d * c.mlp_mult) % 64)) {
      err = "BF16 compute needs every level's dim, heads * (dim // heads) and dim * mlp_mult to be multiples of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    std::vector<ParamDesc> et;
    const std::string ee = build_param_table(nest_engine_config(c, L, probe.n), et);
    if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
  }
  return VITX_OK;
}

#define NALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void nest_destroy(vitx_nest* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (NestLevel& L : m->lv)
    if (L.eng) engine_destroy(L.eng);
  if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

int nest_create(const vitx_nest_config& cin, vitx_nest** out, std::string& err) {
  vitx_nest_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-5f;   // nest.py:29
  int rc = nest_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_nest* m = new vitx_nest();
  m->cfg = c;
  auto fail = [&](int code) { nest_destroy(m); return code; };
  nest_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // one engine per level with blocks; all of them run on the first one's stream
  static const char* PAIRS[][2] = {{"attn.norm.g", "attn.norm.gamma"}, {"attn.norm.b", "attn.norm.beta"}, {"attn.to_qkv.kernel", "attn.to_qkv.kernel"},
                                   {"attn.to_out.kernel", "attn.to_out.kernel"}, {"attn.to_out.bias", "attn.to_out.bias"},
                                   {"ff.norm.g", "mlp.norm.gamma"}, {"ff.norm.b", "mlp.norm.beta"}, {"ff.fc1.kernel", "mlp.fc1.kernel"},
                                   {"ff.fc1.bias", "mlp.fc1.bias"}, {"ff.fc2.kernel", "mlp.fc2.kernel"}, {"ff.fc2.bias", "mlp.fc2.bias"}};
  for (size_t i = 0; i < m->lv.size(); ++i) {
    NestLevel& L = m->lv[i];
    if (L.depth == 0) continue;
    if ((rc = engine_create(nest_engine_config(c, L, m->n), &L.eng, err)) != VITX_OK) return fail(rc);
    // the fp32 FMA form measured slower than the materialised path at the usage shape, the bf16 MFMA form faster
    L.eng->small_attn = c.small_attn > 0 || (c.small_attn == 0 && c.compute == VITX_COMPUTE_BF16);
    if (!m->prof_eng) { m->prof_eng = L.eng; m->stream = L.eng->stream; }
    for (int l = 0; l < L.depth; ++l)
      for (const auto& pr : PAIRS)
        if ((rc = add_arena_map(L.maps, m->table, "nest_layers." + std::to_string(i) + ".transformer." + std::to_string(l) + "." + pr[0], L.eng->table,
                                "transformer." + std::to_string(l) + "." + pr[1], err)) != VITX_OK) return fail(rc);
  }
  if (!m->stream) {   // no level has blocks: the composite runs alone
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { err = "no HIP device visible (there is no CPU fallback)"; return fail(VITX_ERR_HIP); }
    if (hipSetDevice(c.device_id) != hipSuccess || hipStreamCreate(&m->stream) != hipSuccess) { err = "hipStreamCreate failed"; return fail(VITX_ERR_HIP); }
    m->own_stream = true;
  }
  // buffers
  const int64_t B = m->B;
  NALLOC(m->params, m->n_arena);
  NALLOC(m->grads, m->n_arena);
  int64_t rows_max = 1, gw_max = 1, map_max = 1, seq_max = 1;
  for (size_t i = 0; i < m->lv.size(); ++i) {
    NestLevel& L = m->lv[i];
    const int64_t px = (int64_t)L.f * L.f;
    map_max = std::max(map_max, B * px * std::max(L.d, L.dn));
    seq_max = std::max(seq_max, B * L.nb * L.nb * (int64_t)m->n);
    if (i > 0) L.x_in = m->lv[i - 1].pooled; else NALLOC(L.x_in, B * px * L.d);
    NALLOC(L.out, B * px * L.d);
    if (L.dn) {
      const int64_t per_image = px * L.Kp;
      L.chunk = (int)std::min<int64_t>(B, c.conv_chunk > 0 ? c.conv_chunk : std::max<int64_t>(1, IM2COL_BUDGET / per_image));
      rows_max = std::max(rows_max, (int64_t)L.chunk * per_image);
      gw_max = std::max(gw_max, (int64_t)L.Kp * L.dn);
      NALLOC(L.conv, B * px * L.dn); NALLOC(L.ln, B * px * L.dn); NALLOC(L.mean, B * px); NALLOC(L.rstd, B * px);
      NALLOC(L.pooled, B * (px / 4) * L.dn);
    }
  }
  const NestLevel& last = m->lv.back();
  const int64_t img_elems = B * c.image_size * c.image_size * 3, last_rows = B * last.f * last.f;
  NALLOC(m->img, img_elems); NALLOC(m->dimg, img_elems);
  NALLOC(m->logits, B * m->nc); NALLOC(m->dlogits, B * m->nc);
  NALLOC(m->patches, B * m->fmap * m->fmap * m->pd); NALLOC(m->dpatches, B * m->fmap * m->fmap * m->pd);
  NALLOC(m->tok_a, map_max); NALLOC(m->tok_b, map_max);
  NALLOC(m->rows, rows_max); NALLOC(m->drows, rows_max); NALLOC(m->gw_part, gw_max); NALLOC(m->gw_slices, CONV_WGRAD_SLICES * gw_max);
  NALLOC(m->xn, last_rows * last.d); NALLOC(m->mean, last_rows); NALLOC(m->rstd, last_rows);
  NALLOC(m->pooled, B * last.d); NALLOC(m->dpooled, B * last.d);
  for (float*& g : m->g) NALLOC(g, map_max);
  NALLOC(m->dpos_part, seq_max);
  const int dmax = m->lv.back().d;
  NALLOC(m->ws, std::max<int64_t>(layernorm_bwd_ws_elems(dmax), colsum_ws_elems(std::max(dmax, m->nc))) + 64);
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

int push_params(vitx_nest* m, std::string& err) {
  int rc;
  for (NestLevel& L : m->lv) {
    if (!L.eng) continue;
    if ((rc = copy_maps(m->params, L.eng->params, L.maps, true, m->stream, err)) != VITX_OK) return rc;
    L.eng->params_dirty = true;
  }
  return VITX_OK;
}
std::vector<vitx_engine*> nest_engines(vitx_nest* m) {
  std::vector<vitx_engine*> v;
  for (NestLevel& L : m->lv) if (L.eng) v.push_back(L.eng);
  return v;
}

int nest_forward(vitx_nest* m, const float* img_dev, int b, std::string& err) {
  const vitx_nest_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  const int n = m->n, hb = m->hb, f0 = m->fmap;
  {   // patch embedding (nest.py:178-181): the (p1 p2 c) feature order of launch_unfold is the reference's Rearrange
    CompositeProf pr(m->prof_eng, "nest_embed");
    launch_unfold(img_dev, m->patches, 0, b, c.image_size, c.image_size, 3, c.patch_size, c.patch_size, m->pd, s);
    dense_fwd(m->patches, m->pd, P + m->emb_w, P + m->emb_b, m->lv[0].x_in, b * f0 * f0, c.dim, m->pd, s, m->x3);
  }
  for (size_t i = 0; i < m->lv.size(); ++i) {
    NestLevel& L = m->lv[i];
    const int nseq = b * L.nb * L.nb;
    { CompositeProf pr(m->prof_eng, "nest_blocks"); launch_nest_to_blocks(L.x_in, P + L.pos, m->tok_a, b, L.nb, hb, hb, L.d, s); }   // :209 and :140-142
    const float* tok = m->tok_a;
    if (L.eng) {
      L.eng->stream = s;
      int rc;
      if ((rc = engine_transformer_forward(L.eng, m->tok_a, nseq, n, 0, 0, m->tok_b, err)) != VITX_OK) return rc;   // :144-146
      tok = m->tok_b;
    }
    { CompositeProf pr(m->prof_eng, "nest_blocks"); launch_nest_from_blocks(tok, L.out, b, L.nb, hb, hb, L.d, s); }                  // :211
    if (!L.dn) continue;
    // Aggregate (:111-123): conv in image chunks, LayerNorm, max-pool over the whole batch
    const int64_t in_img = (int64_t)L.f * L.f * L.d, out_img = (int64_t)L.f * L.f * L.dn;
    for (int b0 = 0; b0 < b; b0 += L.chunk) {
      const int nb = std::min(L.chunk, b - b0);
      { CompositeProf pr(m->prof_eng, "nest_im2col"); launch_cct_im2col(L.out + b0 * in_img, m->rows, nb, L.f, L.f, L.d, 3, 1, L.Kp, s); }
      CompositeProf pr(m->prof_eng, "nest_conv_gemm");
      dense_fwd(m->rows, L.Kp, P + L.conv_w, P + L.conv_b, L.conv + b0 * out_img, nb * L.f * L.f, L.dn, L.K, s, m->x3);
    }
    launch_layernorm_fwd(L.conv, L.dn, P + L.ag_g, P + L.ag_b, L.ln, 0, L.dn, L.mean, L.rstd, b * L.f * L.f, L.dn, c.ln_eps, s);
    CompositeProf pr(m->prof_eng, "nest_maxpool_fwd");
    launch_nest_maxpool_fwd(L.ln, L.pooled, b, L.f, L.f, L.dn, 3, 2, s);
  }
  // mlp_head (:196-200)
  const NestLevel& last = m->lv.back();
  CompositeProf pr(m->prof_eng, "nest_head");
  launch_layernorm_fwd(last.out, last.d, P + m->head_g, P + m->head_b, m->xn, 0, last.d, m->mean, m->rstd, b * last.f * last.f, last.d, c.ln_eps, s);
  launch_mean_pool(m->xn, b, last.f * last.f, last.d, m->pooled, s);
  dense_fwd(m->pooled, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and, when dimg_dev is given, d(img)
int nest_backward(vitx_nest* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  const vitx_nest_config& c = m->cfg;
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b, n = m->n, hb = m->hb, f0 = m->fmap;
  launch_fill_zero(G, m->n_arena * 4, s);
  int cur = 0;   // m->g[cur] holds d(level output map)
  {
    const NestLevel& last = m->lv.back();
    const int ntok = last.f * last.f, d = last.d;
    CompositeProf pr(m->prof_eng, "nest_head");
    dense_dw(m->pooled, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dpooled, b, m->nc, d, s);
    launch_mean_pool_bwd(m->dpooled, b, ntok, d, m->g[1], s);
    launch_layernorm_bwd(m->g[1], 0, d, last.out, d, m->mean, m->rstd, P + m->head_g, nullptr, 0, m->g[0], d, nullptr, 0, m->ws, G + m->head_g, G + m->head_b,
                         nullptr, b * ntok, d, s);
  }
  for (int i = (int)m->lv.size() - 1; i >= 0; --i) {
    NestLevel& L = m->lv[(size_t)i];
    const int nseq = b * L.nb * L.nb;
    const int a1 = (cur + 1) % 3, a2 = (cur + 2) % 3;
    // the partition's VJP is its inverse map and the other way round
    { CompositeProf pr(m->prof_eng, "nest_blocks"); launch_nest_to_blocks(m->g[cur], nullptr, m->g[a1], b, L.nb, hb, hb, L.d, s); }
    const float* dtok = m->g[a1];
    if (L.eng) {
      L.eng->stream = s;
      int rc;
      if ((rc = engine_transformer_backward(L.eng, m->g[a1], m->g[a2], err)) != VITX_OK) return rc;
      if ((rc = copy_maps(m->grads, L.eng->grads, L.maps, false, m->stream, err)) != VITX_OK) return rc;
      dtok = m->g[a2];
    }
    float* dxin = const_cast<float*>(dtok) == m->g[a1] ? m->g[a2] : m->g[a1];
    {
      CompositeProf pr(m->prof_eng, "nest_blocks");
      launch_nest_dpos(dtok, m->dpos_part, G + L.pos, nseq, n, L.d, s);
      launch_nest_from_blocks(dtok, dxin, b, L.nb, hb, hb, L.d, s);
    }
    if (i == 0) {   // patch embedding
      CompositeProf pr(m->prof_eng, "nest_embed");
      const int rows = b * f0 * f0;
      dense_dw(m->patches, m->pd, dxin, G + m->emb_w, rows, c.dim, m->pd, s, m->x3);
      launch_colsum(dxin, 0, c.dim, rows, c.dim, m->ws, G + m->emb_b, s);
      if (dimg_dev) {
        dense_dx(dxin, P + m->emb_w, m->dpatches, rows, c.dim, m->pd, s, m->x3);
        launch_fold_add(m->dpatches, m->pd, dimg_dev, b, c.image_size, c.image_size, 3, c.patch_size, c.patch_size, s);
      }
      break;
    }
    // Aggregate of the level below: dxin is d(its pooled map)
    NestLevel& A = m->lv[(size_t)i - 1];
    const int px = A.f * A.f;
    float* dln = m->g[cur];                                      // (d(level output) has been consumed)
    float* dconv = const_cast<float*>(dtok);                     // (so has d(tokens))
    { CompositeProf pr(m->prof_eng, "nest_maxpool_bwd"); launch_nest_maxpool_bwd(A.ln, dxin, dln, b, A.f, A.f, A.dn, 3, 2, s); }
    launch_layernorm_bwd(dln, 0, A.dn, A.conv, A.dn, A.mean, A.rstd, P + A.ag_g, nullptr, 0, dconv, A.dn, nullptr, 0, m->ws, G + A.ag_g, G + A.ag_b, nullptr,
                         b * px, A.dn, s);
    launch_colsum(dconv, 0, A.dn, b * px, A.dn, m->ws, G + A.conv_b, s);
    float* dout = dxin;                                          // d(the lower level's output map) [b, f, f, d]
    const int64_t in_img = (int64_t)px * A.d, out_img = (int64_t)px * A.dn;
    for (int b0 = 0; b0 < b; b0 += A.chunk) {
      const int nb = std::min(A.chunk, b - b0);
      const int rows = nb * px;
      const float* dy = dconv + b0 * out_img;
      { CompositeProf pr(m->prof_eng, "nest_im2col"); launch_cct_im2col(A.out + b0 * in_img, m->rows, nb, A.f, A.f, A.d, 3, 1, A.Kp, s); }
      {
        CompositeProf pr(m->prof_eng, "nest_conv_gemm");
        conv_wgrad(m->rows, A.Kp, dy, m->gw_part, m->gw_slices, rows, A.dn, m->x3, s);
        const int64_t nw = (int64_t)A.K * A.dn;
        hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + A.conv_w, (const float*)m->gw_part, nw, b0 == 0 ? 1 : 0);
        dense_dx(dy, P + A.conv_w, m->drows, rows, A.dn, A.K, s, m->x3);
      }
      CompositeProf pr(m->prof_eng, "nest_col2im");
      launch_extract_patches_bwd(m->drows, dout + b0 * in_img, nb, A.f, A.f, A.d, 3, 1, s);
    }
    cur = (int)(dout == m->g[0] ? 0 : dout == m->g[1] ? 1 : 2);
  }
  return VITX_OK;
}

}  // namespace

extern "C" {

int32_t vitx_nest_param_table_size(const vitx_nest_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, nest_param_table);
}
int32_t vitx_nest_param_table_entry(const vitx_nest_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                    int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, nest_param_table);
}
int32_t vitx_nest_create(const vitx_nest_config* cfg, vitx_nest_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, nest_create);
}
int32_t vitx_nest_destroy(vitx_nest_handle m) {
  CAPI_TRY
  nest_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_nest, "blob size does not match the NesT parameter table")
int32_t vitx_nest_forward_dev(vitx_nest_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  std::string err;
  int rc = nest_forward(m, img_dev, b, err);   // (the image is read once: the VJP works from the unfolded patches)
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_nest_forward(vitx_nest_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_size * m->cfg.image_size * 3, b, logits_host,
                                [&](std::string& err) { return nest_forward(m, m->img, b, err); });
}
int32_t vitx_nest_backward_dev(vitx_nest_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = nest_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_nest_backward(vitx_nest_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_size * m->cfg.image_size * 3,
                                 [&](float* dimg_dev, std::string& err) { return nest_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_nest_profile_begin(vitx_nest_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(nest_engines(m));
}
int32_t vitx_nest_profile_end(vitx_nest_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(nest_engines(m), out, cap, n_out);
}
int32_t vitx_nest_read(vitx_nest_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const float* src = nullptr;
  int64_t n = 0;
  const int64_t b = m->b;
  auto level_of = [&](const std::string& prefix) -> int {
    if (w.compare(0, prefix.size(), prefix) != 0 || w.size() == prefix.size()) return -1;
    for (size_t k = prefix.size(); k < w.size(); ++k) if (w[k] < '0' || w[k] > '9') return -1;
    const long v = std::strtol(w.c_str() + prefix.size(), nullptr, 10);
    return v < (long)m->lv.size() ? (int)v : -1;
  };
  int i;
  if (w == "embedded") { src = m->lv[0].x_in; n = b * m->fmap * m->fmap * m->cfg.dim; }
  else if (w == "pooled") { src = m->pooled; n = b * m->lv.back().d; }
  else if ((i = level_of("level.")) >= 0) { const NestLevel& L = m->lv[(size_t)i]; src = L.out; n = b * L.f * L.f * L.d; }
  else if ((i = level_of("aggregated.")) >= 0 && m->lv[(size_t)i].dn) { const NestLevel& L = m->lv[(size_t)i]; src = L.pooled; n = b * (L.f / 2) * (L.f / 2) * L.dn; }
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
