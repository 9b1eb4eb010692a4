// CrossFormer (crossformer.py:205-257): per stage a CrossEmbedLayer (:30-48) -- one Conv2D 'SAME' with bias per kernel size (sorted, :34; widths
// int(dim / 2^i), the last takes the rest, :38-39) as im2col rows (cct_tok.hip) times the HWIO kernel viewed as [k*k*Cin, w_i] in image chunks, each
// into its column block of the stage input -- and a Transformer (:182-203) of `depth` layers of a SHORT pair (attention inside contiguous
// local x local windows + MLP) and a LONG pair (attention inside the dilated global x global windows of :146 + MLP).  Attention and MLP are
// position-wise outside the attention itself, so a whole pair runs in window layout between one partition and its inverse: the block form of a
// vitx_config.nest_block engine (heads of 32, :105) on the (b * windows) sequences the partition gives -- nest_ops.hip's for the short windows,
// crossformer_ops.hip's for the long ones.  A stage owns one engine of each kind with one block per layer, run a layer at a time through the layer
// range of the transformer entry.  Every attention adds its DynamicPositionBias (:51-71,159-165) to the scaled scores: the network is evaluated
// by crossformer_ops.hip whenever the parameters change and reaches the small-head kernels' BIAS form (attn_lsa.hip) through vitx_engine::attn_bias.
// The reference cuts the bias from the tape (:163, .numpy()): the dpb.* gradients are exact zeros and the attention VJP needs the bias only to
// recompute P.  Then the mean over the map and Dense (:245-248).
// Embeddings, bias network and head keep fp32 storage in every compute mode; in the bf16 / bf16x3 modes the embedding GEMMs take the split-operand
// MFMA path.  The composite owns the public parameter / gradient arenas in its own table order and copies them to / from
// the engines.  Only the deterministic path exists (ff_dropout 0; attn_dropout is unused by the reference).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

// what window_attn = 0 means: the one-wave-per-window kernels (attn_window.hip) for at most 64 tokens in the bf16 mode -- DESIGN.md section 23
// (on: 740 against 790 ms per step at the usage shape, batch 256; the attention classes 9.8 against 45.6 ms)
constexpr bool CF_WINDOW_ATTN_DEFAULT = true;
constexpr int CF_STAGES = 4, CF_DIM_HEAD = 32, CF_MULT = 4, CF_WINDOW_MAX = LSA_N_MAX;   // crossformer.py:105,90; the small-head kernels' n

struct CfScale { int k = 0, w = 0, col0 = 0, K = 0, Kp = 0, chunk = 1; int64_t kern = -1, bias = -1; };
struct CfAttn { int64_t dpb[14]; float* bias = nullptr; };

struct CfStage {
  int d = 0, depth = 0, g = 0, lw = 0, stride = 0, heads = 0, d4 = 0;
  int cin = 0, Hin = 0, Win = 0, H = 0, W = 0;
  std::vector<CfScale> sc;
  std::vector<CfAttn> sht_a, lng_a;   // per layer
  vitx_engine *sht = nullptr, *lng = nullptr;
  std::vector<ArenaMap> sht_maps, lng_maps;
  float *x_in = nullptr, *emb = nullptr, *out = nullptr;
};

}  // namespace

struct vitx_crossformer {
  vitx_crossformer_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<CfStage> st;
  vitx_engine* prof_eng = nullptr;   // the composite's own launches are booked on the first engine
  int64_t fc_w = -1, fc_b = -1;
  int nc = 0, B = 0, x3 = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *rows = nullptr, *drows = nullptr, *scale_y = nullptr, *gw_part = nullptr, *gw_slices = nullptr;
  float *tok_a = nullptr, *tok_b = nullptr, *ga = nullptr, *gb = nullptr, *gc = nullptr;
  float *pooled = nullptr, *dpooled = nullptr, *ws = nullptr, *dvec = nullptr, *dpb_ws = nullptr;
  bool have_fwd = false;
  int b = 0;
};

namespace {

// stages and, when the configuration names an image, their maps; "" or what is wrong with the configuration
std::string cf_geometry(const vitx_crossformer_config& c, std::vector<CfStage>& out) {
  out.clear();
  if (c.num_classes <= 0) return "num_classes must be positive";
  if (c.image_h < 0 || c.image_w < 0 || (c.image_h == 0) != (c.image_w == 0)) return "invalid image size";
  int H = c.image_h, W = c.image_w, cin = 3;
  for (int i = 0; i < CF_STAGES; ++i) {
    CfStage S;
    S.d = c.dim[i]; S.depth = c.depth[i]; S.g = c.global_window_size[i]; S.lw = c.local_window_size[i]; S.stride = c.strides[i];
    const std::string sn = "stage " + std::to_string(i + 1);
    if (S.d < CF_DIM_HEAD)
      return sn + ": dim must be >= 32 (heads = dim // 32 would be 0, crossformer.py:109), got " + std::to_string(S.d);
    if (S.d > 4096) return sn + ": dim must be <= 4096";
    if (S.depth < 0) return sn + ": depth must be >= 0";
    if (S.g <= 0 || S.lw <= 0 || S.stride <= 0) return sn + ": global_window_size, local_window_size and cross_embed_strides must be positive";
    if (S.g * S.g > CF_WINDOW_MAX || S.lw * S.lw > CF_WINDOW_MAX)
      return sn + ": a window of more than 288 tokens is not built (global_window_size " + std::to_string(S.g) + ", local_window_size " +
             std::to_string(S.lw) + ")";
    const int ns = c.n_kernels[i];
    if (ns < 1 || ns > VITX_CF_MAX_SCALES) return sn + ": 1 to 8 cross_embed_kernel_sizes";
    std::vector<int> ks(c.kernel_sizes[i], c.kernel_sizes[i] + ns);
    std::sort(ks.begin(), ks.end());   // :34
    S.heads = S.d / CF_DIM_HEAD; S.d4 = S.d / 4; S.cin = cin;
    int used = 0;
    for (int j = 0; j < ns; ++j) {
      CfScale Q;
      Q.k = ks[(size_t)j];
      if (Q.k <= 0 || Q.k > 255) return sn + ": cross_embed_kernel_sizes must be in 1 .. 255";
      Q.w = j + 1 < ns ? (int)((double)S.d / (double)(1 << (j + 1))) : S.d - used;   // :38-39
      if (Q.w <= 0) return sn + ": a scale of the cross-scale embedding would have no channels (dim " + std::to_string(S.d) + ", " + std::to_string(ns) + " kernel sizes)";
      Q.col0 = used; used += Q.w;
      Q.K = Q.k * Q.k * cin; Q.Kp = (int)round_up(Q.K, 64);
      S.sc.push_back(Q);
    }
    if (H > 0) {
      S.Hin = H; S.Win = W;
      H = (int)ceil_div(H, S.stride); W = (int)ceil_div(W, S.stride);   // 'SAME'
      S.H = H; S.W = W;
      if (S.depth > 0 && (H % S.lw || W % S.lw))
        return sn + ": the map (" + std::to_string(H) + " x " + std::to_string(W) + ") must be divisible by local_window_size = " + std::to_string(S.lw) +
               " (the reference's window rearrange, crossformer.py:144, fails there)";
      if (S.depth > 0 && (H % S.g || W % S.g))
        return sn + ": the map (" + std::to_string(H) + " x " + std::to_string(W) + ") must be divisible by global_window_size = " + std::to_string(S.g) +
               " (the reference's window rearrange, crossformer.py:146, fails there)";
    }
    cin = S.d;
    out.push_back(S);
  }
  return "";
}

}  // namespace

// Table of CrossFormer's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string crossformer_param_table(const vitx_crossformer_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena,
                                    vitx_crossformer* m = nullptr) {
  out.clear();
  std::vector<CfStage> st;
  const std::string e = cf_geometry(c, st);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  for (size_t i = 0; i < st.size(); ++i) {
    CfStage& S = st[i];
    const int64_t d = S.d, inner = (int64_t)S.heads * CF_DIM_HEAD, d4 = S.d4, hid = d * CF_MULT;
    const std::string pre = "crossformer_layers." + std::to_string(i);
    for (size_t j = 0; j < S.sc.size(); ++j) {
      CfScale& Q = S.sc[j];
      const std::string q = pre + ".cel.convs." + std::to_string(j);
      Q.kern = tb.add(q + ".kernel", {Q.k, Q.k, S.cin, Q.w}); Q.bias = tb.add(q + ".bias", {Q.w});
    }
    auto attn = [&](const std::string& q, CfAttn& A) {
      tb.add(q + ".norm.g", {1, 1, 1, d}); tb.add(q + ".norm.b", {1, 1, 1, d});
      tb.add(q + ".to_qkv.kernel", {1, 1, d, 3 * inner});
      tb.add(q + ".to_out.kernel", {1, 1, inner, d}); tb.add(q + ".to_out.bias", {d});
      for (int t = 0; t < 3; ++t) {   // Dense, LayerNormalization (, ReLU) x 3 (:55-64)
        const std::string ts = std::to_string(t);
        A.dpb[4 * t] = tb.add(q + ".dpb.dense." + ts + ".kernel", {t ? d4 : 2, d4}); A.dpb[4 * t + 1] = tb.add(q + ".dpb.dense." + ts + ".bias", {d4});
        A.dpb[4 * t + 2] = tb.add(q + ".dpb.norm." + ts + ".gamma", {d4}); A.dpb[4 * t + 3] = tb.add(q + ".dpb.norm." + ts + ".beta", {d4});
      }
      A.dpb[12] = tb.add(q + ".dpb.dense.3.kernel", {d4, 1}); A.dpb[13] = tb.add(q + ".dpb.dense.3.bias", {1});   // :65
    };
    auto ff = [&](const std::string& q) {
      tb.add(q + ".norm.g", {1, 1, 1, d}); tb.add(q + ".norm.b", {1, 1, 1, d});
      tb.add(q + ".fc1.kernel", {1, 1, d, hid}); tb.add(q + ".fc1.bias", {hid});
      tb.add(q + ".fc2.kernel", {1, 1, hid, d}); tb.add(q + ".fc2.bias", {d});
    };
    S.sht_a.resize((size_t)S.depth); S.lng_a.resize((size_t)S.depth);
    for (int l = 0; l < S.depth; ++l) {
      const std::string q = pre + ".transformer." + std::to_string(l);
      attn(q + ".short_attn", S.sht_a[(size_t)l]); ff(q + ".short_ff");
      attn(q + ".long_attn", S.lng_a[(size_t)l]); ff(q + ".long_ff");
    }
  }
  const int64_t dl = st.back().d;
  const int64_t fw = tb.add("to_logits.kernel", {dl, c.num_classes}), fb = tb.add("to_logits.bias", {c.num_classes});
  if (m) { m->st = st; m->fc_w = fw; m->fc_b = fb; m->nc = c.num_classes; }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

int64_t cf_windows(const CfStage& S, bool lng) { const int w = lng ? S.g : S.lw; return (int64_t)(S.H / w) * (S.W / w); }

vitx_config cf_engine_config(const vitx_crossformer_config& c, const CfStage& S, bool lng) {
  const int w = lng ? S.g : S.lw;
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.image_h = 1; ec.image_w = w * w; ec.max_batch = (int32_t)(c.max_batch * cf_windows(S, lng));
  ec.num_classes = 1; ec.dim = S.d; ec.depth = S.depth; ec.heads = S.heads; ec.dim_head = CF_DIM_HEAD;
  ec.mlp_dim = S.d * CF_MULT; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.device_id = c.device_id;
  ec.nest_block = 1;
  return ec;
}

// everything a configuration can be refused for without a device
int cf_check(const vitx_crossformer_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_crossformer probe;
  const std::string e = crossformer_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.image_h <= 0) { err = "vitx_crossformer_create needs the image size"; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  for (const CfStage& S : probe.st) {
    if (c.compute == VITX_COMPUTE_BF16 && S.d % 64) {
      err = "BF16 compute needs every stage's dim to be a multiple of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    if ((int64_t)S.H * S.W > (1 << 24)) { err = "the map is too large"; return VITX_ERR_INVALID; }
    if (!S.depth) continue;
    for (int g = 0; g < 2; ++g) {
      // (the attention kernels take one (sequence, head, row tile) per workgroup with the sequence on the grid's z axis)
      if ((int64_t)c.max_batch * cf_windows(S, g == 1) > 65535) { err = "max_batch * windows of a stage must be <= 65535"; return VITX_ERR_INVALID; }
      std::vector<ParamDesc> et;
      const std::string ee = build_param_table(cf_engine_config(c, S, g == 1), et);
      if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
    }
  }
  return VITX_OK;
}

#define CFALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void cf_destroy(vitx_crossformer* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (CfStage& S : m->st) {
    if (S.sht) engine_destroy(S.sht);
    if (S.lng) engine_destroy(S.lng);
  }
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  delete m;
}

// parameter maps of one stage: composite tensor -> engine tensor, block l of both engines = layer l of the stage
int cf_maps(vitx_crossformer* m, size_t si, std::string& err) {
  CfStage& S = m->st[si];
  static const char* ATTN[][2] = {{"norm.g", "attn.norm.gamma"}, {"norm.b", "attn.norm.beta"}, {"to_qkv.kernel", "attn.to_qkv.kernel"},
                                  {"to_out.kernel", "attn.to_out.kernel"}, {"to_out.bias", "attn.to_out.bias"}};
  static const char* FF[][2] = {{"norm.g", "mlp.norm.gamma"}, {"norm.b", "mlp.norm.beta"}, {"fc1.kernel", "mlp.fc1.kernel"}, {"fc1.bias", "mlp.fc1.bias"},
                                {"fc2.kernel", "mlp.fc2.kernel"}, {"fc2.bias", "mlp.fc2.bias"}};
  for (int l = 0; l < S.depth; ++l) {
    const std::string q = "crossformer_layers." + std::to_string(si) + ".transformer." + std::to_string(l);
    const std::string eq = "transformer." + std::to_string(l) + ".";
    for (int g = 0; g < 2; ++g) {
      vitx_engine* eng = g ? S.lng : S.sht;
      std::vector<ArenaMap>& maps = g ? S.lng_maps : S.sht_maps;
      const std::string a = q + (g ? ".long_attn." : ".short_attn."), f = q + (g ? ".long_ff." : ".short_ff.");
      for (const auto& pr : ATTN) if (add_arena_map(maps, m->table, a + pr[0], eng->table, eq + pr[1], err) != VITX_OK) return VITX_ERR_INVALID;
      for (const auto& pr : FF) if (add_arena_map(maps, m->table, f + pr[0], eng->table, eq + pr[1], err) != VITX_OK) return VITX_ERR_INVALID;
    }
  }
  return VITX_OK;
}

int cf_create(const vitx_crossformer_config& cin, vitx_crossformer** out, std::string& err) {
  vitx_crossformer_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-5f;   // crossformer.py:75
  int rc = cf_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_crossformer* m = new vitx_crossformer();
  m->cfg = c;
  auto fail = [&](int code) { cf_destroy(m); return code; };
  crossformer_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // two engines per stage with layers; all of them run on the first one's stream
  for (size_t i = 0; i < m->st.size(); ++i) {
    CfStage& S = m->st[i];
    if (!S.depth) continue;
    if ((rc = engine_create(cf_engine_config(c, S, false), &S.sht, err)) != VITX_OK) return fail(rc);
    if ((rc = engine_create(cf_engine_config(c, S, true), &S.lng, err)) != VITX_OK) return fail(rc);
    // window_attn 0: the measured default
    S.sht->window_attn = S.lng->window_attn = c.window_attn > 0 || (c.window_attn == 0 && CF_WINDOW_ATTN_DEFAULT);
    if (!m->prof_eng) { m->prof_eng = S.sht; m->stream = S.sht->stream; }
    if ((rc = cf_maps(m, i, err)) != VITX_OK) return fail(rc);
  }
  if (!m->stream) {   // no stage has layers: a stream of the handle's own
    if (hipSetDevice(c.device_id) != hipSuccess || hipStreamCreate(&m->own_stream) != hipSuccess) { err = "hipStreamCreate failed"; return fail(VITX_ERR_HIP); }
    m->stream = m->own_stream;
  }
  const int64_t B = m->B;
  CFALLOC(m->params, m->n_arena);
  CFALLOC(m->grads, m->n_arena);
  int64_t map_max = 1, rows_max = 1, drows_max = 1, y_max = 1, gw_max = 1, dpb_max = 1;
  int dmax = 1;
  for (size_t i = 0; i < m->st.size(); ++i) {
    CfStage& S = m->st[i];
    const int64_t px = (int64_t)S.H * S.W;
    map_max = std::max({map_max, B * px * S.d, B * (int64_t)S.Hin * S.Win * S.cin});
    dmax = std::max(dmax, S.d);
    for (CfScale& Q : S.sc) {
      const int64_t per_image = px * Q.Kp;
      Q.chunk = (int)std::min<int64_t>(B, std::max<int64_t>(1, IM2COL_BUDGET / per_image));
      rows_max = std::max(rows_max, (int64_t)Q.chunk * per_image);
      drows_max = std::max(drows_max, (int64_t)Q.chunk * px * Q.K);
      y_max = std::max(y_max, (int64_t)Q.chunk * px * Q.w);
      gw_max = std::max(gw_max, (int64_t)Q.Kp * Q.w);
    }
    CFALLOC(S.emb, B * px * S.d);
    if (S.depth) CFALLOC(S.out, B * px * S.d); else S.out = S.emb;
    if (i > 0) S.x_in = m->st[i - 1].out;
    // one bias buffer per attention, handed to the engines block by block
    for (int g = 0; g < 2 && S.depth; ++g) {
      const int w = g ? S.g : S.lw, n = w * w;
      vitx_engine* eng = g ? S.lng : S.sht;
      dpb_max = std::max(dpb_max, cf_dpb_ws_elems(w));
      eng->attn_bias_n = n;
      for (int l = 0; l < S.depth; ++l) {
        CfAttn& A = (g ? S.lng_a : S.sht_a)[(size_t)l];
        CFALLOC(A.bias, (int64_t)n * n);
        eng->attn_bias.push_back(A.bias);
      }
    }
  }
  const int64_t img_elems = B * c.image_h * c.image_w * 3;
  CFALLOC(m->img, img_elems); CFALLOC(m->dimg, img_elems);
  CFALLOC(m->logits, B * m->nc); CFALLOC(m->dlogits, B * m->nc);
  CFALLOC(m->rows, rows_max); CFALLOC(m->drows, drows_max); CFALLOC(m->scale_y, y_max);
  CFALLOC(m->gw_part, gw_max); CFALLOC(m->gw_slices, CONV_WGRAD_SLICES * gw_max);
  CFALLOC(m->tok_a, map_max); CFALLOC(m->tok_b, map_max); CFALLOC(m->ga, map_max); CFALLOC(m->gb, map_max); CFALLOC(m->gc, map_max);
  CFALLOC(m->pooled, B * m->st.back().d); CFALLOC(m->dpooled, B * m->st.back().d);
  CFALLOC(m->ws, colsum_ws_elems(std::max(dmax, m->nc)) + 64);
  CFALLOC(m->dvec, dmax);
  CFALLOC(m->dpb_ws, dpb_max);
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

// the composite's arena to the engines, and every attention's position bias from the new parameters
int push_params(vitx_crossformer* m, std::string& err) {
  int rc;
  const float* P = m->params;
  for (CfStage& S : m->st) {
    if (!S.depth) continue;
    if ((rc = copy_maps(m->params, S.sht->params, S.sht_maps, true, m->stream, err)) != VITX_OK) return rc;
    S.sht->params_dirty = true;
    if ((rc = copy_maps(m->params, S.lng->params, S.lng_maps, true, m->stream, err)) != VITX_OK) return rc;
    S.lng->params_dirty = true;
    CompositeProf pr(m->prof_eng, "cf_dpb_bias");
    for (int g = 0; g < 2; ++g)
      for (CfAttn& A : (g ? S.lng_a : S.sht_a)) {
        CfDpbParams dp;
        for (int t = 0; t < 14; ++t) dp.t[t] = P + A.dpb[t];
        launch_cf_dpb_bias(dp, S.d4, g ? S.g : S.lw, m->dpb_ws, A.bias, m->stream);   // (one workspace: the launches are ordered on the stream)
      }
  }
  return VITX_OK;
}

// one layer of a stage: the short pair on the contiguous windows, then the long pair on the dilated ones; in -> S.out; scratch: tok_a, tok_b
int cf_layer_fwd(vitx_crossformer* m, CfStage& S, int l, const float* in, int b, std::string& err) {
  hipStream_t s = m->stream;
  int rc;
  const int gy = S.H / S.lw, gx = S.W / S.lw;
  { CompositeProf pr(m->prof_eng, "cf_windows"); launch_nest_to_blocks(in, nullptr, m->tok_a, b, gy, S.lw, S.lw, S.d, s, gx); }          // crossformer.py:144
  S.sht->stream = s;
  if ((rc = engine_transformer_forward(S.sht, m->tok_a, b * gy * gx, S.lw * S.lw, 0, 0, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;   // :198-199
  {
    CompositeProf pr(m->prof_eng, "cf_windows");
    launch_nest_from_blocks(m->tok_b, m->tok_a, b, gy, S.lw, S.lw, S.d, s, gx);                                                           // :176
    launch_cf_to_dilated(m->tok_a, m->tok_b, b, S.H, S.W, S.g, S.d, s);                                                                   // :146
  }
  S.lng->stream = s;
  if ((rc = engine_transformer_forward(S.lng, m->tok_b, b * (S.H / S.g) * (S.W / S.g), S.g * S.g, 0, 0, m->tok_a, err, l, l + 1)) != VITX_OK) return rc;   // :200-201
  { CompositeProf pr(m->prof_eng, "cf_windows"); launch_cf_from_dilated(m->tok_a, S.out, b, S.H, S.W, S.g, S.d, s); }                      // :178
  return VITX_OK;
}

// d(out) in g (overwritten with d(in)); scratch: tok_a, tok_b.  The VJP of a partition is its inverse map and the other way round.
int cf_layer_bwd(vitx_crossformer* m, CfStage& S, int l, float* g, int b, std::string& err) {
  hipStream_t s = m->stream;
  int rc;
  const int gy = S.H / S.lw, gx = S.W / S.lw;
  { CompositeProf pr(m->prof_eng, "cf_windows"); launch_cf_to_dilated(g, m->tok_a, b, S.H, S.W, S.g, S.d, s); }
  S.lng->stream = s;
  if ((rc = engine_transformer_backward(S.lng, m->tok_a, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;
  {
    CompositeProf pr(m->prof_eng, "cf_windows");
    launch_cf_from_dilated(m->tok_b, g, b, S.H, S.W, S.g, S.d, s);
    launch_nest_to_blocks(g, nullptr, m->tok_a, b, gy, S.lw, S.lw, S.d, s, gx);
  }
  S.sht->stream = s;
  if ((rc = engine_transformer_backward(S.sht, m->tok_a, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;
  { CompositeProf pr(m->prof_eng, "cf_windows"); launch_nest_from_blocks(m->tok_b, g, b, gy, S.lw, S.lw, S.d, s, gx); }
  return VITX_OK;
}

int cf_forward(vitx_crossformer* m, const float* img_dev, int b, std::string& err) {
  const vitx_crossformer_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  int rc;
  for (size_t i = 0; i < m->st.size(); ++i) {
    CfStage& S = m->st[i];
    const float* x_in = i == 0 ? img_dev : S.x_in;
    const int px = S.H * S.W;
    const int64_t in_img = (int64_t)S.Hin * S.Win * S.cin, out_img = (int64_t)px * S.d;
    // CrossEmbedLayer (crossformer.py:45-48): every scale's Conv2D 'SAME' with bias in image chunks, into its column block
    for (const CfScale& Q : S.sc)
      for (int b0 = 0; b0 < b; b0 += Q.chunk) {
        const int nb = std::min(Q.chunk, b - b0);
        { CompositeProf pr(m->prof_eng, "cf_im2col"); launch_cct_im2col(x_in + b0 * in_img, m->rows, nb, S.Hin, S.Win, S.cin, Q.k, S.stride, Q.Kp, s); }
        CompositeProf pr(m->prof_eng, "cf_conv_gemm");
        dense_fwd(m->rows, Q.Kp, P + Q.kern, P + Q.bias, m->scale_y, nb * px, Q.w, Q.K, s, m->x3);
        launch_cf_cols_put(m->scale_y, S.emb + b0 * out_img, (int64_t)nb * px, Q.w, S.d, Q.col0, s);
      }
    const float* cur = S.emb;
    for (int l = 0; l < S.depth; ++l) {
      if ((rc = cf_layer_fwd(m, S, l, cur, b, err)) != VITX_OK) return rc;
      cur = S.out;
    }
  }
  // Reduce('b h w c -> b c', 'mean') + Dense (:245-248)
  const CfStage& last = m->st.back();
  CompositeProf pr(m->prof_eng, "cf_head");
  launch_mean_pool(last.out, b, last.H * last.W, last.d, m->pooled, s);
  dense_fwd(m->pooled, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten; the dpb.* entries are zeros) and, when dimg_dev is given, d(img)
int cf_backward(vitx_crossformer* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b;
  launch_fill_zero(G, m->n_arena * 4, s);
  float *g = m->ga, *g2 = m->gb;   // g holds d(stage output map)
  {
    const CfStage& last = m->st.back();
    const int d = last.d;
    CompositeProf pr(m->prof_eng, "cf_head");
    dense_dw(m->pooled, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dpooled, b, m->nc, d, s);
    launch_mean_pool_bwd(m->dpooled, b, last.H * last.W, d, g, s);
  }
  int rc;
  for (int i = (int)m->st.size() - 1; i >= 0; --i) {
    CfStage& S = m->st[(size_t)i];
    const int px = S.H * S.W, rows_all = b * px;
    const int64_t in_img = (int64_t)S.Hin * S.Win * S.cin, out_img = (int64_t)px * S.d;
    for (int l = S.depth - 1; l >= 0; --l)
      if ((rc = cf_layer_bwd(m, S, l, g, b, err)) != VITX_OK) return rc;
    if (S.depth) {
      if ((rc = copy_maps(G, S.sht->grads, S.sht_maps, false, s, err)) != VITX_OK) return rc;
      if ((rc = copy_maps(G, S.lng->grads, S.lng_maps, false, s, err)) != VITX_OK) return rc;
    }
    // CrossEmbedLayer: g = d(concatenated maps).  The bias gradients are the column sums, cut by scale.
    {
      CompositeProf pr(m->prof_eng, "cf_conv_gemm");
      launch_colsum(g, 0, S.d, rows_all, S.d, m->ws, m->dvec, s);
      for (const CfScale& Q : S.sc) HIPCHK(hipMemcpyAsync(G + Q.bias, m->dvec + Q.col0, (size_t)Q.w * 4, hipMemcpyDeviceToDevice, s));
    }
    const float* x_in = i == 0 ? m->img : S.x_in;
    const bool want_dx = i > 0 || dimg_dev;
    float* dxin = i == 0 ? dimg_dev : g2;   // d(input) of the scales, summed in scale order (g is read by every scale)
    for (size_t j = 0; j < S.sc.size(); ++j) {
      const CfScale& Q = S.sc[j];
      for (int b0 = 0; b0 < b; b0 += Q.chunk) {
        const int nb = std::min(Q.chunk, b - b0);
        const int rows = nb * px;
        { CompositeProf pr(m->prof_eng, "cf_im2col"); launch_cct_im2col(x_in + b0 * in_img, m->rows, nb, S.Hin, S.Win, S.cin, Q.k, S.stride, Q.Kp, s); }
        {
          CompositeProf pr(m->prof_eng, "cf_conv_gemm");
          launch_cf_cols_get(g + b0 * out_img, m->scale_y, rows, Q.w, S.d, Q.col0, s);
          conv_wgrad(m->rows, Q.Kp, m->scale_y, m->gw_part, m->gw_slices, rows, Q.w, m->x3, s);
          const int64_t nw = (int64_t)Q.K * Q.w;
          hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + Q.kern, (const float*)m->gw_part, nw, b0 == 0 ? 1 : 0);
          if (want_dx) dense_dx(m->scale_y, P + Q.kern, m->drows, rows, Q.w, Q.K, s, m->x3);
        }
        if (!want_dx) continue;
        CompositeProf pr(m->prof_eng, "cf_col2im");
        const int64_t nx = (int64_t)nb * in_img;
        if (j == 0) launch_extract_patches_bwd(m->drows, dxin + b0 * in_img, nb, S.Hin, S.Win, S.cin, Q.k, S.stride, s);
        else {
          launch_extract_patches_bwd(m->drows, m->gc, nb, S.Hin, S.Win, S.cin, Q.k, S.stride, s);
          hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nx)), dim3(256), 0, s, dxin + b0 * in_img, (const float*)m->gc, nx, 0);
        }
      }
    }
    if (i > 0) std::swap(g, g2);   // g now holds d(the previous stage's output)
  }
  return VITX_OK;
}

std::vector<vitx_engine*> cf_engines(vitx_crossformer* m) {
  std::vector<vitx_engine*> v;
  for (CfStage& S : m->st) { if (S.sht) v.push_back(S.sht); if (S.lng) v.push_back(S.lng); }
  return v;
}

}  // namespace

extern "C" {

int32_t vitx_crossformer_param_table_size(const vitx_crossformer_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, crossformer_param_table);
}
int32_t vitx_crossformer_param_table_entry(const vitx_crossformer_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4],
                                           int32_t* rank, int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, crossformer_param_table);
}
int32_t vitx_crossformer_create(const vitx_crossformer_config* cfg, vitx_crossformer_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, cf_create);
}
int32_t vitx_crossformer_destroy(vitx_crossformer_handle m) {
  CAPI_TRY
  cf_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_crossformer, "blob size does not match the CrossFormer parameter table")
int32_t vitx_crossformer_forward_dev(vitx_crossformer_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  // (the embedding's weight gradient re-reads the image: the handle keeps its own copy)
  CAPI_HIP(hipMemcpyAsync(m->img, img_dev, (size_t)b * m->cfg.image_h * m->cfg.image_w * 3 * 4, hipMemcpyDeviceToDevice, m->stream));
  std::string err;
  int rc = cf_forward(m, m->img, b, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossformer_forward(vitx_crossformer_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_h * m->cfg.image_w * 3, b, logits_host,
                                [&](std::string& err) { return cf_forward(m, m->img, b, err); });
}
int32_t vitx_crossformer_backward_dev(vitx_crossformer_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = cf_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossformer_backward(vitx_crossformer_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_h * m->cfg.image_w * 3,
                                 [&](float* dimg_dev, std::string& err) { return cf_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_crossformer_profile_begin(vitx_crossformer_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(cf_engines(m));
}
int32_t vitx_crossformer_profile_end(vitx_crossformer_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(cf_engines(m), out, cap, n_out);
}
int32_t vitx_crossformer_read(vitx_crossformer_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const int64_t b = m->b;
  auto stage_of = [&](const std::string& prefix, size_t at) -> int {
    if (w.compare(0, prefix.size(), prefix) != 0 || w.size() <= at) return -1;
    const int v = w[at] - '0';
    return v >= 0 && v < (int)m->st.size() ? v : -1;
  };
  int i;
  if (w == "pooled") return composite_read_tail(m->pooled, b * m->st.back().d, out_host, cap, n_elems, m->stream);
  if (w.size() == 10 && (i = stage_of("embedded.", 9)) >= 0) { const CfStage& S = m->st[(size_t)i]; return composite_read_tail(S.emb, b * S.H * S.W * S.d, out_host, cap, n_elems, m->stream); }
  if (w.size() == 7 && (i = stage_of("stage.", 6)) >= 0) { const CfStage& S = m->st[(size_t)i]; return composite_read_tail(S.out, b * S.H * S.W * S.d, out_host, cap, n_elems, m->stream); }
  if ((i = stage_of("bias.", 5)) >= 0 && w.size() > 7 && w[6] == '.') {   // bias.<s>.<l>.short | .long
    const CfStage& S = m->st[(size_t)i];
    const size_t dot = w.find('.', 7);
    if (dot != std::string::npos && dot > 7 && dot - 7 <= 6) {
      int l = 0;
      bool ok = true;
      for (size_t k = 7; k < dot; ++k) { if (w[k] < '0' || w[k] > '9') ok = false; else l = l * 10 + (w[k] - '0'); }
      const std::string kind = w.substr(dot + 1);
      if (ok && l < S.depth && (kind == "short" || kind == "long")) {
        const bool lng = kind == "long";
        const int n = lng ? S.g * S.g : S.lw * S.lw;
        return composite_read_tail((lng ? S.lng_a : S.sht_a)[(size_t)l].bias, (int64_t)n * n, out_host, cap, n_elems, m->stream);
      }
    }
  }
  return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  CAPI_CATCH
}
int32_t vitx_crossformer_window_attn(vitx_crossformer_handle m, const float* qkv_host, const float* d_o_host, const float* bias_host, int32_t b, int32_t n,
                                     int32_t h, int32_t tail_rows, float tail_value, int32_t window_kernel, float* o_host, float* lse_host, float* dqkv_host) {
  CAPI_TRY
  if (!m || !qkv_host || !d_o_host || !bias_host || !o_host || !lse_host || !dqkv_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || h <= 0 || tail_rows < 0 || (int64_t)b * h > 65535) return capi_fail(VITX_ERR_INVALID, "invalid shape");
  if (window_kernel ? !attn_window_supported(n, CF_DIM_HEAD) : !attn_small_supported(n, CF_DIM_HEAD)) return capi_fail(VITX_ERR_UNSUPPORTED, "n is outside the kernel's range");
  const int64_t inner = (int64_t)h * CF_DIM_HEAD, live = (int64_t)b * n, rows = live + tail_rows;
  auto to_bf16 = [](float f) -> uint16_t {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  };
  auto to_f32 = [](uint16_t v) -> float { const uint32_t u = (uint32_t)v << 16; float f; std::memcpy(&f, &u, 4); return f; };
  // host images: the live rows from the caller, the tail rows (inputs AND outputs) filled with tail_value
  std::vector<uint16_t> hq((size_t)(rows * 3 * inner), to_bf16(tail_value)), hg((size_t)(rows * inner), to_bf16(tail_value)), ho(hg), hd(hq);
  for (int64_t i = 0; i < live * 3 * inner; ++i) hq[(size_t)i] = to_bf16(qkv_host[i]);
  for (int64_t i = 0; i < live * inner; ++i) hg[(size_t)i] = to_bf16(d_o_host[i]);
  bf16_t *dq = nullptr, *dg = nullptr, *dout = nullptr, *dd = nullptr;
  float *dlse = nullptr, *dsum = nullptr, *dbias = nullptr;
  std::vector<void*> owned;
  auto alloc = [&](void** p, size_t bytes) { if (hipMalloc(p, std::max<size_t>(bytes, 16)) != hipSuccess) return false; owned.push_back(*p); return true; };
  auto release = [&]() { for (void* p : owned) (void)hipFree(p); };
  const size_t stat = (size_t)b * h * n * 4;
  if (!alloc((void**)&dq, hq.size() * 2) || !alloc((void**)&dg, hg.size() * 2) || !alloc((void**)&dout, ho.size() * 2) || !alloc((void**)&dd, hd.size() * 2) ||
      !alloc((void**)&dlse, stat) || !alloc((void**)&dsum, stat) || !alloc((void**)&dbias, (size_t)n * n * 4)) { release(); return capi_fail(VITX_ERR_HIP, "hipMalloc failed"); }
  hipStream_t s = m->stream;
  const float scale = 1.0f / std::sqrt((float)CF_DIM_HEAD);
  hipError_t e = hipMemcpyAsync(dq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dg, hg.data(), hg.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dout, ho.data(), ho.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dd, hd.data(), hd.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dbias, bias_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    if (window_kernel) {
      launch_attn_window_fwd(dq, dout, dlse, dbias, b, n, h, scale, s);
      launch_attn_window_bwd(dq, dout, dg, dlse, dd, dbias, b, n, h, scale, s);
    } else {
      launch_attn_small_fwd(dq, dout, dlse, 1, b, n, h, CF_DIM_HEAD, scale, s, dbias);
      launch_attn_small_bwd(dq, dout, dg, dlse, dsum, dd, 1, b, n, h, CF_DIM_HEAD, scale, s, dbias);
    }
    e = hipMemcpyAsync(ho.data(), dout, ho.size() * 2, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hd.data(), dd, hd.size() * 2, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(lse_host, dlse, stat, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  release();
  if (e != hipSuccess) return capi_fail(VITX_ERR_HIP, hipGetErrorString(e));
  for (size_t i = 0; i < ho.size(); ++i) o_host[i] = to_f32(ho[i]);
  for (size_t i = 0; i < hd.size(); ++i) dqkv_host[i] = to_f32(hd[i]);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossformer_partition(vitx_crossformer_handle m, const float* in_host, float* out_host, int32_t b, int32_t H, int32_t W, int32_t g,
                                   int32_t c, int32_t inverse) {
  CAPI_TRY
  if (!m || !in_host || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || H <= 0 || W <= 0 || g <= 0 || c <= 0 || H % g || W % g) return capi_fail(VITX_ERR_INVALID, "the window must divide the map");
  const size_t bytes = (size_t)b * H * W * c * 4;
  float *src = nullptr, *dst = nullptr;
  CAPI_HIP(hipMalloc(&src, bytes));
  if (hipMalloc(&dst, bytes) != hipSuccess) { (void)hipFree(src); return capi_fail(VITX_ERR_HIP, "hipMalloc failed"); }
  hipError_t e = hipMemcpyAsync(src, in_host, bytes, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) {
    if (inverse) launch_cf_from_dilated(src, dst, b, H, W, g, c, m->stream); else launch_cf_to_dilated(src, dst, b, H, W, g, c, m->stream);
    e = hipMemcpyAsync(out_host, dst, bytes, hipMemcpyDeviceToHost, m->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  (void)hipFree(src); (void)hipFree(dst);
  if (e != hipSuccess) return capi_fail(VITX_ERR_HIP, hipGetErrorString(e));
  return VITX_OK;
  CAPI_CATCH
}

}  // extern "C"
