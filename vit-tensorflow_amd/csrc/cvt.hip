// CvT (cvt.py:149-202): per stage Conv2D(emb_dim, emb_kernel, 'SAME', emb_stride) with bias (:187) as im2col rows (cct_tok.hip) times the HWIO
// kernel viewed as [k*k*Cin, Cout] in image chunks, the channel LayerNorm (:30-43,188), and a Transformer (:129-147) of `depth` layers
// x + Attention(LN x), x + MLP(LN x): the conv_proj block form of the engine (vitx_config.conv_proj_kernel / _stride) on b sequences of the
// whole map -- q and kv through a depthwise 'SAME' convolution + BatchNormalization (cvt_ops.hip) and a pointwise Dense, heads of 64, to_out
// always.  Then the mean over the map and Dense (:195-198).  A stage owns one engine (none at depth 0).
// Embeddings, their LayerNorm and the head keep fp32 storage in every compute mode; in the bf16 / bf16x3 modes their GEMMs take the split-operand
// MFMA path.  The composite owns the public parameter / gradient arenas in its own table order and copies them to / from
// the engines; a block's tensors have the same order in both tables.
// BatchNormalization: a training forward uses the statistics of the call's whole batch (the engine sees all b images at once: nothing here
// chunks what it normalises); an inference forward the moving statistics of the table, and has no VJP.  Nothing updates the moving statistics.
// Only the deterministic path exists (dropout 0).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

constexpr int CV_STAGES = 3, CV_DIM_HEAD = 64;   // cvt.py:130: CvT never passes dim_head
// what fused_attn = 0 means for at most 64 keys (attn_fewkey) and for 65 .. MANYKEY_MAX keys (attn_manykey): DESIGN.md section 22
constexpr bool CV_FEWKEY_DEFAULT = true, CV_MANYKEY_DEFAULT = true;

struct CvtStage {
  int d = 0, ek = 0, es = 0, pk = 0, ks = 0, heads = 0, depth = 0, mult = 0;   // s{i}_emb_dim, _emb_kernel, _emb_stride, _proj_kernel, _kv_proj_stride, _heads, _depth, _mlp_mult
  int cin = 0, K = 0, Kp = 0, chunk = 1;                                       // input channels, k * k * cin, its row stride, images per im2col pass
  int Hin = 0, Win = 0, H = 0, W = 0, Hk = 0, Wk = 0;                          // the stage's input map, its own, and the kv map
  int64_t emb_w = -1, emb_b = -1, ln_g = -1, ln_b = -1;                        // arena offsets
  vitx_engine* eng = nullptr;
  std::vector<ArenaMap> maps;
  float *x_in = nullptr, *conv = nullptr, *mean = nullptr, *rstd = nullptr, *emb = nullptr, *out = nullptr;
};

}  // namespace

struct vitx_cvt {
  vitx_cvt_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<CvtStage> st;
  vitx_engine* prof_eng = nullptr;   // the composite's own launches are booked on the first engine
  int64_t fc_w = -1, fc_b = -1;
  int nc = 0, B = 0, x3 = 0;
  hipStream_t stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *rows = nullptr, *drows = nullptr, *gw_part = nullptr, *gw_slices = nullptr, *ga = nullptr, *gb = nullptr, *tap = nullptr;
  float *pooled = nullptr, *dpooled = nullptr, *ws = nullptr;
  bool have_fwd = false, inference = false;
  int b = 0;
};

namespace {

// stages and, when the configuration names an image, their maps; "" or what is wrong with the configuration
std::string cvt_geometry(const vitx_cvt_config& c, std::vector<CvtStage>& out) {
  out.clear();
  if (c.num_classes <= 0) return "num_classes must be positive";
  if (c.image_h < 0 || c.image_w < 0 || (c.image_h == 0) != (c.image_w == 0)) return "invalid image size";
  int H = c.image_h, W = c.image_w, cin = 3;
  for (int i = 0; i < CV_STAGES; ++i) {
    CvtStage S;
    S.d = c.emb_dim[i]; S.ek = c.emb_kernel[i]; S.es = c.emb_stride[i]; S.pk = c.proj_kernel[i]; S.ks = c.kv_proj_stride[i];
    S.heads = c.heads[i]; S.depth = c.depth[i]; S.mult = c.mlp_mult[i];
    const std::string sn = "s" + std::to_string(i + 1);
    if (S.d <= 0 || S.ek <= 0 || S.es <= 0 || S.pk <= 0 || S.ks <= 0 || S.heads <= 0 || S.mult <= 0)
      return sn + ": emb_dim, emb_kernel, emb_stride, proj_kernel, kv_proj_stride, heads and mlp_mult must be positive";
    if (S.depth < 0) return sn + "_depth must be >= 0";
    if (S.d > 4096) return sn + "_emb_dim must be <= 4096";
    if (S.pk > 255 || S.ks > 32767 || S.ek > 255) return sn + ": emb_kernel and proj_kernel must be <= 255, kv_proj_stride <= 32767";
    S.cin = cin; S.K = S.ek * S.ek * cin; S.Kp = (int)round_up(S.K, 64);
    if (H > 0) {
      S.Hin = H; S.Win = W;
      H = (int)ceil_div(H, S.es); W = (int)ceil_div(W, S.es);   // 'SAME'
      S.H = H; S.W = W;
      S.Hk = (int)ceil_div(H, S.ks); S.Wk = (int)ceil_div(W, S.ks);
      if ((int64_t)S.H * S.W > (1 << 24)) return sn + ": the map is too large";
    }
    cin = S.d;
    out.push_back(S);
  }
  return "";
}

}  // namespace

// Table of CvT's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string cvt_param_table(const vitx_cvt_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_cvt* m = nullptr) {
  out.clear();
  std::vector<CvtStage> st;
  const std::string e = cvt_geometry(c, st);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  for (size_t i = 0; i < st.size(); ++i) {
    CvtStage& S = st[i];
    const int64_t d = S.d, inner = (int64_t)S.heads * CV_DIM_HEAD, pk = S.pk, hid = d * S.mult;
    const std::string pre = "cvt_layers." + std::to_string(i);
    S.emb_w = tb.add(pre + ".embed.kernel", {S.ek, S.ek, S.cin, d}); S.emb_b = tb.add(pre + ".embed.bias", {d});
    S.ln_g = tb.add(pre + ".norm.g", {1, 1, 1, d}); S.ln_b = tb.add(pre + ".norm.b", {1, 1, 1, d});
    for (int l = 0; l < S.depth; ++l) {
      const std::string q = pre + ".transformer." + std::to_string(l);
      tb.add(q + ".attn.norm.g", {1, 1, 1, d}); tb.add(q + ".attn.norm.b", {1, 1, 1, d});
      for (int pj = 0; pj < 2; ++pj) {
        const std::string p = q + (pj ? ".attn.to_kv" : ".attn.to_q");
        tb.add(p + ".dw.kernel", {pk, pk, 1, d});
        tb.add(p + ".bn.gamma", {d}); tb.add(p + ".bn.beta", {d}); tb.add(p + ".bn.moving_mean", {d}); tb.add(p + ".bn.moving_variance", {d});
        tb.add(p + ".pw.kernel", {1, 1, d, pj ? 2 * inner : inner});
      }
      tb.add(q + ".attn.to_out.kernel", {1, 1, inner, d}); tb.add(q + ".attn.to_out.bias", {d});
      tb.add(q + ".ff.norm.g", {1, 1, 1, d}); tb.add(q + ".ff.norm.b", {1, 1, 1, d});
      tb.add(q + ".ff.fc1.kernel", {1, 1, d, hid}); tb.add(q + ".ff.fc1.bias", {hid});
      tb.add(q + ".ff.fc2.kernel", {1, 1, hid, d}); tb.add(q + ".ff.fc2.bias", {d});
    }
  }
  const int64_t dl = st.back().d;
  const int64_t fw = tb.add("head.kernel", {dl, c.num_classes}), fb = tb.add("head.bias", {c.num_classes});
  if (m) { m->st = st; m->fc_w = fw; m->fc_b = fb; m->nc = c.num_classes; }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config cvt_engine_config(const vitx_cvt_config& c, const CvtStage& S) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.image_h = S.H; ec.image_w = S.W; ec.max_batch = c.max_batch;
  ec.num_classes = 1; ec.dim = S.d; ec.depth = S.depth; ec.heads = S.heads; ec.dim_head = CV_DIM_HEAD;
  ec.mlp_dim = S.d * S.mult; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.device_id = c.device_id;
  ec.nest_block = 1;
  ec.conv_proj_kernel = (int16_t)S.pk; ec.conv_proj_stride = (int16_t)S.ks;
  return ec;
}

// everything a configuration can be refused for without a device
int cvt_check(const vitx_cvt_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_cvt probe;
  const std::string e = cvt_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.image_h <= 0) { err = "vitx_cvt_create needs the image size"; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  for (const CvtStage& S : probe.st) {
    if (c.compute == VITX_COMPUTE_BF16 && S.d % 64) {
      err = "BF16 compute needs every stage's emb_dim to be a multiple of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    if (!S.depth) continue;
    std::vector<ParamDesc> et;
    const std::string ee = build_param_table(cvt_engine_config(c, S), et);
    if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
  }
  return VITX_OK;
}

#define CVALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void cvt_destroy(vitx_cvt* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (CvtStage& S : m->st) if (S.eng) engine_destroy(S.eng);
  delete m;
}

// parameter maps of one stage: the composite's tensors of its blocks -> the engine's, same order in both; adjacent runs are merged
int cvt_maps(vitx_cvt* m, size_t si, std::string& err) {
  CvtStage& S = m->st[si];
  static const char* NAMES[][2] = {
      {"attn.norm.g", "attn.norm.gamma"}, {"attn.norm.b", "attn.norm.beta"},
      {"attn.to_q.dw.kernel", "attn.to_q.dw.kernel"}, {"attn.to_q.bn.gamma", "attn.to_q.bn.gamma"}, {"attn.to_q.bn.beta", "attn.to_q.bn.beta"},
      {"attn.to_q.bn.moving_mean", "attn.to_q.bn.moving_mean"}, {"attn.to_q.bn.moving_variance", "attn.to_q.bn.moving_variance"},
      {"attn.to_q.pw.kernel", "attn.to_q.pw.kernel"},
      {"attn.to_kv.dw.kernel", "attn.to_kv.dw.kernel"}, {"attn.to_kv.bn.gamma", "attn.to_kv.bn.gamma"}, {"attn.to_kv.bn.beta", "attn.to_kv.bn.beta"},
      {"attn.to_kv.bn.moving_mean", "attn.to_kv.bn.moving_mean"}, {"attn.to_kv.bn.moving_variance", "attn.to_kv.bn.moving_variance"},
      {"attn.to_kv.pw.kernel", "attn.to_kv.pw.kernel"},
      {"attn.to_out.kernel", "attn.to_out.kernel"}, {"attn.to_out.bias", "attn.to_out.bias"},
      {"ff.norm.g", "mlp.norm.gamma"}, {"ff.norm.b", "mlp.norm.beta"}, {"ff.fc1.kernel", "mlp.fc1.kernel"}, {"ff.fc1.bias", "mlp.fc1.bias"},
      {"ff.fc2.kernel", "mlp.fc2.kernel"}, {"ff.fc2.bias", "mlp.fc2.bias"}};
  int rc = VITX_OK;
  for (int l = 0; l < S.depth && rc == VITX_OK; ++l) {
    const std::string q = "cvt_layers." + std::to_string(si) + ".transformer." + std::to_string(l) + ".";
    const std::string eq = "transformer." + std::to_string(l) + ".";
    for (const auto& pr : NAMES)
      if ((rc = add_arena_map(S.maps, m->table, q + pr[0], S.eng->table, eq + pr[1], err)) != VITX_OK) break;
  }
  return rc;
}

int cvt_create(const vitx_cvt_config& cin, vitx_cvt** out, std::string& err) {
  vitx_cvt_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-5f;   // cvt.py:31
  if (c.bn_eps <= 0.f) c.bn_eps = 1e-5f;   // cvt.py:85
  int rc = cvt_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_cvt* m = new vitx_cvt();
  m->cfg = c;
  auto fail = [&](int code) { cvt_destroy(m); return code; };
  cvt_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // one engine per stage with blocks; all of them run on the first one's stream
  for (size_t i = 0; i < m->st.size(); ++i) {
    CvtStage& S = m->st[i];
    if (!S.depth) continue;
    if ((rc = engine_create(cvt_engine_config(c, S), &S.eng, err)) != VITX_OK) return fail(rc);
    // fused_attn 0: the measured default per key-count class
    S.eng->fewkey_attn = c.fused_attn > 0 || (c.fused_attn == 0 && CV_FEWKEY_DEFAULT);
    S.eng->manykey_attn = c.fused_attn > 0 || (c.fused_attn == 0 && CV_MANYKEY_DEFAULT);
    S.eng->bn_eps = c.bn_eps;
    if (!m->prof_eng) { m->prof_eng = S.eng; m->stream = S.eng->stream; }
    if ((rc = cvt_maps(m, i, err)) != VITX_OK) return fail(rc);
  }
  const int64_t B = m->B;
  CVALLOC(m->params, m->n_arena);
  CVALLOC(m->grads, m->n_arena);
  int64_t map_max = 1, rows_max = 1, gw_max = 1;
  int dmax = 1;
  for (size_t i = 0; i < m->st.size(); ++i) {
    CvtStage& S = m->st[i];
    const int64_t px = (int64_t)S.H * S.W, per_image = px * S.Kp;
    map_max = std::max({map_max, B * px * S.d, B * (int64_t)S.Hin * S.Win * S.cin});
    S.chunk = (int)std::min<int64_t>(B, std::max<int64_t>(1, IM2COL_BUDGET / per_image));
    rows_max = std::max(rows_max, (int64_t)S.chunk * per_image);
    gw_max = std::max(gw_max, (int64_t)S.Kp * S.d);
    dmax = std::max(dmax, S.d);
    CVALLOC(S.conv, B * px * S.d); CVALLOC(S.mean, B * px); CVALLOC(S.rstd, B * px); CVALLOC(S.emb, B * px * S.d);
    if (S.eng) CVALLOC(S.out, B * px * S.d); else S.out = S.emb;
    if (i > 0) S.x_in = m->st[i - 1].out;
  }
  const int64_t img_elems = B * c.image_h * c.image_w * 3;
  CVALLOC(m->img, img_elems); CVALLOC(m->dimg, img_elems);
  CVALLOC(m->logits, B * m->nc); CVALLOC(m->dlogits, B * m->nc);
  CVALLOC(m->rows, rows_max); CVALLOC(m->drows, rows_max); CVALLOC(m->gw_part, gw_max); CVALLOC(m->gw_slices, CONV_WGRAD_SLICES * gw_max);
  CVALLOC(m->ga, map_max); CVALLOC(m->gb, map_max); CVALLOC(m->tap, map_max);
  CVALLOC(m->pooled, B * m->st.back().d); CVALLOC(m->dpooled, B * m->st.back().d);
  CVALLOC(m->ws, std::max<int64_t>(layernorm_bwd_ws_elems(dmax), colsum_ws_elems(std::max(dmax, m->nc))) + 64);
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

int push_params(vitx_cvt* m, std::string& err) {
  int rc;
  for (CvtStage& S : m->st) {
    if (!S.eng) continue;
    if ((rc = copy_maps(m->params, S.eng->params, S.maps, true, m->stream, err)) != VITX_OK) return rc;
    S.eng->params_dirty = true;
  }
  return VITX_OK;
}

int cvt_forward(vitx_cvt* m, const float* img_dev, int b, int training, std::string& err) {
  const vitx_cvt_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  m->inference = !training;
  int rc;
  for (size_t i = 0; i < m->st.size(); ++i) {
    CvtStage& S = m->st[i];
    const float* x_in = i == 0 ? img_dev : S.x_in;
    const int px = S.H * S.W;
    const int64_t in_img = (int64_t)S.Hin * S.Win * S.cin, out_img = (int64_t)px * S.d;
    // Conv2D 'SAME' with bias (cvt.py:187) in image chunks, then the channel LayerNorm (:188)
    for (int b0 = 0; b0 < b; b0 += S.chunk) {
      const int nb = std::min(S.chunk, b - b0);
      { CompositeProf pr(m->prof_eng, "cvt_im2col"); launch_cct_im2col(x_in + b0 * in_img, m->rows, nb, S.Hin, S.Win, S.cin, S.ek, S.es, S.Kp, s); }
      CompositeProf pr(m->prof_eng, "cvt_conv_gemm");
      dense_fwd(m->rows, S.Kp, P + S.emb_w, P + S.emb_b, S.conv + b0 * out_img, nb * px, S.d, S.K, s, m->x3);
    }
    {
      CompositeProf pr(m->prof_eng, "cvt_embed_norm");
      launch_layernorm_fwd(S.conv, S.d, P + S.ln_g, P + S.ln_b, S.emb, 0, S.d, S.mean, S.rstd, b * px, S.d, c.ln_eps, s);
    }
    if (!S.eng) continue;
    S.eng->stream = s;
    S.eng->bn_inference = !training;
    if ((rc = engine_transformer_forward(S.eng, S.emb, b, px, 0, 0, S.out, err)) != VITX_OK) return rc;   // :189-191
  }
  // GlobalAvgPool2D + Dense (:195-198)
  const CvtStage& last = m->st.back();
  CompositeProf pr(m->prof_eng, "cvt_head");
  launch_mean_pool(last.out, b, last.H * last.W, last.d, m->pooled, s);
  dense_fwd(m->pooled, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten; the moving statistics' entries are zeros) and, when dimg_dev is
// given, d(img)
int cvt_backward(vitx_cvt* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  if (m->inference) {
    err = "the last forward ran with training == 0: BatchNormalization on the moving statistics is forward only (no VJP is built)";
    return VITX_ERR_UNSUPPORTED;
  }
  const vitx_cvt_config& c = m->cfg;
  (void)c;
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b;
  launch_fill_zero(G, m->n_arena * 4, s);
  float *g = m->ga, *g2 = m->gb;   // g holds d(stage output map)
  {
    const CvtStage& last = m->st.back();
    const int d = last.d;
    CompositeProf pr(m->prof_eng, "cvt_head");
    dense_dw(m->pooled, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dpooled, b, m->nc, d, s);
    launch_mean_pool_bwd(m->dpooled, b, last.H * last.W, d, g, s);
  }
  int rc;
  for (int i = (int)m->st.size() - 1; i >= 0; --i) {
    CvtStage& S = m->st[(size_t)i];
    const int px = S.H * S.W, rows_all = b * px;
    const int64_t in_img = (int64_t)S.Hin * S.Win * S.cin, out_img = (int64_t)px * S.d;
    if (S.eng) {
      S.eng->stream = s;
      if ((rc = engine_transformer_backward(S.eng, g, g, err)) != VITX_OK) return rc;
      if ((rc = copy_maps(m->grads, S.eng->grads, S.maps, false, s, err)) != VITX_OK) return rc;
    }
    {   // g = d(emb) -> g2 = d(conv)
      CompositeProf pr(m->prof_eng, "cvt_embed_norm");
      launch_layernorm_bwd(g, 0, S.d, S.conv, S.d, S.mean, S.rstd, P + S.ln_g, nullptr, 0, g2, S.d, nullptr, 0, m->ws, G + S.ln_g, G + S.ln_b, nullptr, rows_all,
                           S.d, s);
      launch_colsum(g2, 0, S.d, rows_all, S.d, m->ws, G + S.emb_b, s);
    }
    const float* x_in = i == 0 ? m->img : S.x_in;
    const bool want_dx = i > 0 || dimg_dev;
    float* dxin = i == 0 ? dimg_dev : g;   // (d(emb) has been consumed)
    for (int b0 = 0; b0 < b; b0 += S.chunk) {
      const int nb = std::min(S.chunk, b - b0);
      const int rows = nb * px;
      const float* dy = g2 + b0 * out_img;
      { CompositeProf pr(m->prof_eng, "cvt_im2col"); launch_cct_im2col(x_in + b0 * in_img, m->rows, nb, S.Hin, S.Win, S.cin, S.ek, S.es, S.Kp, s); }
      {
        CompositeProf pr(m->prof_eng, "cvt_conv_gemm");
        conv_wgrad(m->rows, S.Kp, dy, m->gw_part, m->gw_slices, rows, S.d, m->x3, s);
        const int64_t nw = (int64_t)S.K * S.d;
        hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + S.emb_w, (const float*)m->gw_part, nw, b0 == 0 ? 1 : 0);
        if (want_dx) dense_dx(dy, P + S.emb_w, m->drows, rows, S.d, S.K, s, m->x3);
      }
      if (!want_dx) continue;
      CompositeProf pr(m->prof_eng, "cvt_col2im");
      launch_extract_patches_bwd(m->drows, dxin + b0 * in_img, nb, S.Hin, S.Win, S.cin, S.ek, S.es, s);
    }
    // g now holds d(the previous stage's output); g2 is free again
  }
  return VITX_OK;
}

std::vector<vitx_engine*> cvt_engines(vitx_cvt* m) {
  std::vector<vitx_engine*> v;
  for (CvtStage& S : m->st) if (S.eng) v.push_back(S.eng);
  return v;
}

}  // namespace

extern "C" {

int32_t vitx_cvt_param_table_size(const vitx_cvt_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, cvt_param_table);
}
int32_t vitx_cvt_param_table_entry(const vitx_cvt_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, cvt_param_table);
}
int32_t vitx_cvt_create(const vitx_cvt_config* cfg, vitx_cvt_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, cvt_create);
}
int32_t vitx_cvt_destroy(vitx_cvt_handle m) {
  CAPI_TRY
  cvt_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_cvt, "blob size does not match the CvT parameter table")
int32_t vitx_cvt_forward_dev(vitx_cvt_handle m, const float* img_dev, int32_t b, int32_t training, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  // (the embedding's weight gradient re-reads the image: the handle keeps its own copy)
  CAPI_HIP(hipMemcpyAsync(m->img, img_dev, (size_t)b * m->cfg.image_h * m->cfg.image_w * 3 * 4, hipMemcpyDeviceToDevice, m->stream));
  std::string err;
  int rc = cvt_forward(m, m->img, b, training, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_cvt_forward(vitx_cvt_handle m, const float* img_host, int32_t b, int32_t training, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_h * m->cfg.image_w * 3, b, logits_host,
                                [&](std::string& err) { return cvt_forward(m, m->img, b, training, err); });
}
int32_t vitx_cvt_backward_dev(vitx_cvt_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = cvt_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_cvt_backward(vitx_cvt_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_h * m->cfg.image_w * 3,
                                 [&](float* dimg_dev, std::string& err) { return cvt_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_cvt_profile_begin(vitx_cvt_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(cvt_engines(m));
}
int32_t vitx_cvt_profile_end(vitx_cvt_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(cvt_engines(m), out, cap, n_out);
}
int32_t vitx_cvt_read(vitx_cvt_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const float* src = nullptr;
  int64_t n = 0;
  const int64_t b = m->b;
  // "<prefix><s>" or "<prefix><s>.<l>" with one-digit s and a decimal l; -1 where the name is not of that form
  auto parse = [&](const std::string& prefix, bool with_layer, int* layer) -> int {
    if (w.compare(0, prefix.size(), prefix) != 0 || w.size() < prefix.size() + 1) return -1;
    const int v = w[prefix.size()] - '0';
    if (v < 0 || v >= (int)m->st.size()) return -1;
    if (!with_layer) return w.size() == prefix.size() + 1 ? v : -1;
    if (w.size() < prefix.size() + 3 || w[prefix.size() + 1] != '.') return -1;
    int l = 0;
    for (size_t k = prefix.size() + 2; k < w.size(); ++k) {
      if (w[k] < '0' || w[k] > '9' || l > 100000) return -1;
      l = l * 10 + (w[k] - '0');
    }
    if (l >= m->st[(size_t)v].depth) return -1;
    *layer = l;
    return v;
  };
  int i, l = 0;
  if (w == "pooled") { src = m->pooled; n = b * m->st.back().d; }
  else if ((i = parse("embedded.", false, nullptr)) >= 0) { const CvtStage& S = m->st[(size_t)i]; src = S.emb; n = b * S.H * S.W * S.d; }
  else if ((i = parse("stage.", false, nullptr)) >= 0) { const CvtStage& S = m->st[(size_t)i]; src = S.out; n = b * S.H * S.W * S.d; }
  else if ((i = parse("q_in.", true, &l)) >= 0 || (i = parse("kv_in.", true, &l)) >= 0) {
    const CvtStage& S = m->st[(size_t)i];
    const bool kv = w[0] == 'k';
    const BlockActs& ba = S.eng->stages[0].ba[(size_t)l];
    const int64_t rows = kv ? b * S.Hk * S.Wk : b * S.H * S.W;
    n = rows * S.d;
    if (n > cap) return capi_fail(VITX_ERR_INVALID, "output buffer too small");
    launch_to_f32(kv ? ba.ctx : ba.qin, S.eng->bf16, S.d, m->tap, S.d, (int)rows, S.d, m->stream);
    src = m->tap;
  }
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
