// TwinsSVT (twins_svt.py:215-268): per stage PatchEmbedding (:94-106: the '(c p1 p2)' Rearrange as a gather of its own, twins_ops.hip, + Dense),
// Transformer(depth 1), PEG (:108-115, one kernel each way in twins_ops.hip), Transformer(depth s_depth); then the mean over the map and Dense
// (:261-264).  A Transformer layer (:199-213) is a LOCAL pair -- attention inside local_patch_size windows + MLP (:117-156,78-92): the block form
// of a vitx_config.nest_block engine on the (b * windows) sequences the window partition gives (nest_ops.hip, rectangular grids), with
// to_qkv = [to_q | to_kv] column-wise -- and a GLOBAL pair -- attention of every map position against the global_k-strided reduction of the map
// + MLP (:158-190): a vitx_config.global_k engine on b sequences of the whole map (bf16 mode, at most 64 keys: the few-key kernels, attn_fewkey.hip).  A stage owns one engine of each kind, with one block per layer
// of its two Transformers (layer 0 in front of the PEG, the others behind it), and runs them a layer at a time through the layer range of the
// transformer entry.  The last stage has no local pairs (has_local=False, :255,258).
// Embeddings, PEG and head keep fp32 storage in every compute mode; in the bf16 / bf16x3 modes their GEMMs take the split-operand MFMA path.
// The composite owns the public parameter / gradient arenas in its own table order and copies them to / from the engines.
// Only the deterministic path exists (dropout 0).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"

namespace {

constexpr int TW_STAGES = 4, TW_HEADS = 8, TW_DIM_HEAD = 64, TW_INNER = TW_HEADS * TW_DIM_HEAD, TW_MULT = 4;   // twins_svt.py:79,118,159

struct TwinsStage {
  int d = 0, p = 0, lp = 0, gk = 0, depth = 0, has_local = 0;   // s{i}_emb_dim, _patch_size, _local_patch_size, _global_k, _depth
  int cin = 0, pd = 0, L = 1;                                   // input channels, cin * p * p, layers of both Transformers (1 + depth)
  int Hin = 0, Win = 0, H = 0, W = 0;                           // the stage's input map and its own
  int64_t emb_w = -1, emb_b = -1, peg_w = -1, peg_b = -1;       // arena offsets
  vitx_engine *loc = nullptr, *glb = nullptr;
  std::vector<ArenaMap> loc_maps, glb_maps;
  float *x_in = nullptr, *patches = nullptr, *emb = nullptr, *pre_peg = nullptr, *peg_out = nullptr, *out = nullptr;
};

}  // namespace

struct vitx_twins {
  vitx_twins_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<TwinsStage> st;
  vitx_engine* prof_eng = nullptr;   // the composite's own launches are booked on the first engine
  int64_t fc_w = -1, fc_b = -1;
  int nc = 0, B = 0, x3 = 0, kp = 0;
  hipStream_t stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *tok_a = nullptr, *tok_b = nullptr, *ga = nullptr, *gb = nullptr, *dpatches = nullptr, *pooled = nullptr, *dpooled = nullptr, *ws = nullptr;
  bool have_fwd = false;
  int b = 0;
};

namespace {

// stages and, when the configuration names an image, their maps; "" or what is wrong with the configuration
std::string twins_geometry(const vitx_twins_config& c, std::vector<TwinsStage>& out) {
  out.clear();
  if (c.num_classes <= 0) return "num_classes must be positive";
  if (c.peg_kernel_size <= 0 || c.peg_kernel_size % 2 == 0)
    return "peg_kernel_size must be odd (an even 'SAME' kernel pads unevenly; it is not built)";
  if (c.image_h < 0 || c.image_w < 0 || (c.image_h == 0) != (c.image_w == 0)) return "invalid image size";
  int H = c.image_h, W = c.image_w, cin = 3;
  for (int i = 0; i < TW_STAGES; ++i) {
    TwinsStage S;
    S.d = c.emb_dim[i]; S.p = c.patch_size[i]; S.lp = c.local_patch_size[i]; S.gk = c.global_k[i]; S.depth = c.depth[i];
    S.has_local = i != TW_STAGES - 1;   // twins_svt.py:248,255
    const std::string sn = "s" + std::to_string(i + 1);
    if (S.d <= 0 || S.p <= 0 || S.lp <= 0 || S.gk <= 0) return sn + ": emb_dim, patch_size, local_patch_size and global_k must be positive";
    if (S.depth < 0) return sn + "_depth must be >= 0";
    if (S.d > 4096) return sn + "_emb_dim must be <= 4096";
    S.cin = cin; S.pd = cin * S.p * S.p; S.L = 1 + S.depth;
    if (H > 0) {
      S.Hin = H; S.Win = W;
      if (H % S.p || W % S.p)
        return sn + ": the map (" + std::to_string(H) + " x " + std::to_string(W) + ") must be divisible by " + sn + "_patch_size = " + std::to_string(S.p) +
               " (the reference's Rearrange, twins_svt.py:103, fails there)";
      H /= S.p; W /= S.p;
      S.H = H; S.W = W;
      if (S.has_local && (H % S.lp || W % S.lp))
        return sn + ": the map (" + std::to_string(H) + " x " + std::to_string(W) + ") must be divisible by " + sn + "_local_patch_size = " +
               std::to_string(S.lp) + " (the reference's window Rearrange, twins_svt.py:141, fails there)";
      if (H % S.gk || W % S.gk)
        return sn + ": the map (" + std::to_string(H) + " x " + std::to_string(W) + ") must be divisible by " + sn + "_global_k = " + std::to_string(S.gk) +
               " (the reference's 'valid' to_kv convolution, twins_svt.py:168, silently drops the rows and columns past the last whole window; that is refused here)";
    }
    cin = S.d;
    out.push_back(S);
  }
  return "";
}

}  // namespace

// Table of TwinsSVT's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string twins_param_table(const vitx_twins_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_twins* m = nullptr) {
  out.clear();
  std::vector<TwinsStage> st;
  const std::string e = twins_geometry(c, st);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  const int64_t kp = c.peg_kernel_size, inner = TW_INNER;
  for (size_t i = 0; i < st.size(); ++i) {
    TwinsStage& S = st[i];
    const int64_t d = S.d, gk = S.gk;
    const std::string pre = "svt_layers." + std::to_string(i);
    S.emb_w = tb.add(pre + ".patch_embedding.proj.kernel", {1, 1, S.pd, d}); S.emb_b = tb.add(pre + ".patch_embedding.proj.bias", {d});
    auto attn = [&](const std::string& q, int64_t k) {
      tb.add(q + ".norm.g", {1, 1, 1, d}); tb.add(q + ".norm.b", {1, 1, 1, d});
      tb.add(q + ".to_q.kernel", {1, 1, d, inner}); tb.add(q + ".to_kv.kernel", {k, k, d, 2 * inner});
      tb.add(q + ".to_out.kernel", {1, 1, inner, d}); tb.add(q + ".to_out.bias", {d});
    };
    auto ff = [&](const std::string& q) {
      tb.add(q + ".norm.g", {1, 1, 1, d}); tb.add(q + ".norm.b", {1, 1, 1, d});
      tb.add(q + ".fc1.kernel", {1, 1, d, d * TW_MULT}); tb.add(q + ".fc1.bias", {d * TW_MULT});
      tb.add(q + ".fc2.kernel", {1, 1, d * TW_MULT, d}); tb.add(q + ".fc2.bias", {d});
    };
    auto transformer = [&](int t, int n) {
      for (int l = 0; l < n; ++l) {
        const std::string q = pre + ".transformer." + std::to_string(t) + "." + std::to_string(l);
        if (S.has_local) { attn(q + ".local_attn", 1); ff(q + ".ff1"); }
        attn(q + ".global_attn", gk); ff(q + ".ff2");
      }
    };
    transformer(0, 1);
    S.peg_w = tb.add(pre + ".peg.kernel", {kp, kp, 1, d}); S.peg_b = tb.add(pre + ".peg.bias", {d});
    transformer(1, S.depth);
  }
  const int64_t dl = st.back().d;
  const int64_t fw = tb.add("head.kernel", {dl, c.num_classes}), fb = tb.add("head.bias", {c.num_classes});
  if (m) { m->st = st; m->fc_w = fw; m->fc_b = fb; m->nc = c.num_classes; m->kp = (int)kp; }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config twins_engine_config(const vitx_twins_config& c, const TwinsStage& S, bool global) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  if (global) { ec.image_h = S.H; ec.image_w = S.W; ec.global_k = S.gk; ec.max_batch = c.max_batch; }
  else { ec.image_h = 1; ec.image_w = S.lp * S.lp; ec.max_batch = c.max_batch * (S.H / S.lp) * (S.W / S.lp); }
  ec.num_classes = 1; ec.dim = S.d; ec.depth = S.L; ec.heads = TW_HEADS; ec.dim_head = TW_DIM_HEAD;
  ec.mlp_dim = S.d * TW_MULT; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.device_id = c.device_id;
  ec.nest_block = 1;
  return ec;
}

// everything a configuration can be refused for without a device
int twins_check(const vitx_twins_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_twins probe;
  const std::string e = twins_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.image_h <= 0) { err = "vitx_twins_create needs the image size"; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  for (const TwinsStage& S : probe.st) {
    if (c.compute == VITX_COMPUTE_BF16 && S.d % 64) {
      err = "BF16 compute needs every stage's emb_dim to be a multiple of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    if (S.has_local && (int64_t)c.max_batch * (S.H / S.lp) * (S.W / S.lp) > (1 << 24)) { err = "max_batch * windows too large"; return VITX_ERR_INVALID; }
    for (int g = S.has_local ? 0 : 1; g < 2; ++g) {
      std::vector<ParamDesc> et;
      const std::string ee = build_param_table(twins_engine_config(c, S, g == 1), et);
      if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
    }
  }
  return VITX_OK;
}

#define TALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void twins_destroy(vitx_twins* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (TwinsStage& S : m->st) {
    if (S.loc) engine_destroy(S.loc);
    if (S.glb) engine_destroy(S.glb);
  }
  delete m;
}

// parameter maps of one stage: composite tensor -> engine tensor, block l of the engines = layer l of the stage (0: transformer.0.0, l >= 1: transformer.1.(l - 1))
int twins_maps(vitx_twins* m, size_t si, std::string& err) {
  TwinsStage& S = m->st[si];
  static const char* COMMON[][2] = {{"norm.g", "attn.norm.gamma"}, {"norm.b", "attn.norm.beta"}, {"to_out.kernel", "attn.to_out.kernel"}, {"to_out.bias", "attn.to_out.bias"}};
  static const char* FF[][2] = {{"norm.g", "mlp.norm.gamma"}, {"norm.b", "mlp.norm.beta"}, {"fc1.kernel", "mlp.fc1.kernel"}, {"fc1.bias", "mlp.fc1.bias"},
                                {"fc2.kernel", "mlp.fc2.kernel"}, {"fc2.bias", "mlp.fc2.bias"}};
  for (int l = 0; l < S.L; ++l) {
    const std::string q = "svt_layers." + std::to_string(si) + ".transformer." + (l == 0 ? std::string("0.0") : "1." + std::to_string(l - 1));
    const std::string eq = "transformer." + std::to_string(l) + ".";
    for (int g = S.has_local ? 0 : 1; g < 2; ++g) {
      vitx_engine* eng = g ? S.glb : S.loc;
      std::vector<ArenaMap>& maps = g ? S.glb_maps : S.loc_maps;
      const std::string a = q + (g ? ".global_attn." : ".local_attn."), f = q + (g ? ".ff2." : ".ff1.");
      auto add = [&](const std::string& cn, const std::string& en, int64_t col0 = 0, int64_t width = -1) {
        return add_arena_map(maps, m->table, cn, eng->table, en, err, col0, width) == VITX_OK;
      };
      for (const auto& pr : COMMON) if (!add(a + pr[0], eq + pr[1])) return VITX_ERR_INVALID;
      for (const auto& pr : FF) if (!add(f + pr[0], eq + pr[1])) return VITX_ERR_INVALID;
      if (g) {
        if (!add(a + "to_q.kernel", eq + "attn.to_q.kernel") || !add(a + "to_kv.kernel", eq + "attn.to_kv.kernel")) return VITX_ERR_INVALID;
      } else {
        // to_qkv = [to_q | to_kv] column-wise (twins_svt.py:142-144 against nest.py:99): d rows of inner and 2 * inner floats into rows of 3 * inner
        if (!add(a + "to_q.kernel", eq + "attn.to_qkv.kernel", 0, TW_INNER) || !add(a + "to_kv.kernel", eq + "attn.to_qkv.kernel", TW_INNER, 2 * TW_INNER))
          return VITX_ERR_INVALID;
      }
    }
  }
  return VITX_OK;
}

int twins_create(const vitx_twins_config& cin, vitx_twins** out, std::string& err) {
  vitx_twins_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-5f;   // twins_svt.py:46
  int rc = twins_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_twins* m = new vitx_twins();
  m->cfg = c;
  auto fail = [&](int code) { twins_destroy(m); return code; };
  twins_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // two engines per stage (one at the last); all of them run on the first one's stream
  for (size_t i = 0; i < m->st.size(); ++i) {
    TwinsStage& S = m->st[i];
    if (S.has_local && (rc = engine_create(twins_engine_config(c, S, false), &S.loc, err)) != VITX_OK) return fail(rc);
    if ((rc = engine_create(twins_engine_config(c, S, true), &S.glb, err)) != VITX_OK) return fail(rc);
    S.glb->fewkey_attn = c.fused_global_attn >= 0;   // (0: the measured default -- on)
    if (!m->prof_eng) { m->prof_eng = S.loc ? S.loc : S.glb; m->stream = m->prof_eng->stream; }
    if ((rc = twins_maps(m, i, err)) != VITX_OK) return fail(rc);
  }
  const int64_t B = m->B;
  TALLOC(m->params, m->n_arena);
  TALLOC(m->grads, m->n_arena);
  int64_t map_max = 1, patch_max = 1;
  int dmax = 1;
  for (size_t i = 0; i < m->st.size(); ++i) {
    TwinsStage& S = m->st[i];
    const int64_t px = (int64_t)S.H * S.W;
    map_max = std::max({map_max, B * px * S.d, B * (int64_t)S.Hin * S.Win * S.cin});
    patch_max = std::max(patch_max, B * px * S.pd);
    dmax = std::max(dmax, S.d);
    TALLOC(S.patches, B * px * S.pd); TALLOC(S.emb, B * px * S.d); TALLOC(S.pre_peg, B * px * S.d); TALLOC(S.peg_out, B * px * S.d);
    if (S.depth > 0) TALLOC(S.out, B * px * S.d); else S.out = S.peg_out;
    if (i > 0) S.x_in = m->st[i - 1].out;
  }
  const int64_t img_elems = B * c.image_h * c.image_w * 3;
  TALLOC(m->img, img_elems); TALLOC(m->dimg, img_elems);
  TALLOC(m->logits, B * m->nc); TALLOC(m->dlogits, B * m->nc);
  TALLOC(m->tok_a, map_max); TALLOC(m->tok_b, map_max); TALLOC(m->ga, map_max); TALLOC(m->gb, map_max);
  TALLOC(m->dpatches, patch_max);
  TALLOC(m->pooled, B * m->st.back().d); TALLOC(m->dpooled, B * m->st.back().d);
  TALLOC(m->ws, std::max<int64_t>(twins_peg_ws_elems(dmax, m->kp), colsum_ws_elems(std::max(dmax, m->nc))) + 64);
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

int push_params(vitx_twins* m, std::string& err) {
  int rc;
  for (TwinsStage& S : m->st) {
    if (S.loc) { if ((rc = copy_maps(m->params, S.loc->params, S.loc_maps, true, m->stream, err)) != VITX_OK) return rc; S.loc->params_dirty = true; }
    if ((rc = copy_maps(m->params, S.glb->params, S.glb_maps, true, m->stream, err)) != VITX_OK) return rc;
    S.glb->params_dirty = true;
  }
  return VITX_OK;
}

// one layer of a stage: the local pair on the window sequences (when the stage has one), then the global pair on the map; in == out is allowed
int twins_layer_fwd(vitx_twins* m, TwinsStage& S, int l, const float* in, float* out, int b, std::string& err) {
  hipStream_t s = m->stream;
  int rc;
  const float* cur = in;
  if (S.loc) {
    const int gy = S.H / S.lp, gx = S.W / S.lp;
    { CompositeProf pr(m->prof_eng, "twins_windows"); launch_nest_to_blocks(cur, nullptr, m->tok_a, b, gy, S.lp, S.lp, S.d, s, gx); }   // twins_svt.py:141
    S.loc->stream = s;
    if ((rc = engine_transformer_forward(S.loc, m->tok_a, b * gy * gx, S.lp * S.lp, 0, 0, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;
    { CompositeProf pr(m->prof_eng, "twins_windows"); launch_nest_from_blocks(m->tok_b, m->tok_a, b, gy, S.lp, S.lp, S.d, s, gx); }       // :153
    cur = m->tok_a;
  }
  S.glb->stream = s;
  return engine_transformer_forward(S.glb, cur, b, S.H * S.W, 0, 0, out, err, l, l + 1);
}

// d(out) in g (overwritten with d(in)); scratch: tok_a, tok_b
int twins_layer_bwd(vitx_twins* m, TwinsStage& S, int l, float* g, int b, std::string& err) {
  hipStream_t s = m->stream;
  int rc;
  S.glb->stream = s;
  if ((rc = engine_transformer_backward(S.glb, g, g, err, l, l + 1)) != VITX_OK) return rc;
  if (S.loc) {
    const int gy = S.H / S.lp, gx = S.W / S.lp;
    // the partition's VJP is its inverse map and the other way round
    { CompositeProf pr(m->prof_eng, "twins_windows"); launch_nest_to_blocks(g, nullptr, m->tok_a, b, gy, S.lp, S.lp, S.d, s, gx); }
    S.loc->stream = s;
    if ((rc = engine_transformer_backward(S.loc, m->tok_a, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;
    { CompositeProf pr(m->prof_eng, "twins_windows"); launch_nest_from_blocks(m->tok_b, g, b, gy, S.lp, S.lp, S.d, s, gx); }
  }
  return VITX_OK;
}

int twins_forward(vitx_twins* m, const float* img_dev, int b, std::string& err) {
  const vitx_twins_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  int rc;
  for (size_t i = 0; i < m->st.size(); ++i) {
    TwinsStage& S = m->st[i];
    const float* x_in = i == 0 ? img_dev : S.x_in;
    const int rows = b * S.H * S.W;
    {   // PatchEmbedding (twins_svt.py:101-106)
      CompositeProf pr(m->prof_eng, "twins_embed");
      launch_twins_patch_gather(x_in, S.patches, b, S.Hin, S.Win, S.cin, S.p, S.pd, s);
      dense_fwd(S.patches, S.pd, P + S.emb_w, P + S.emb_b, S.emb, rows, S.d, S.pd, s, m->x3);
    }
    if ((rc = twins_layer_fwd(m, S, 0, S.emb, S.pre_peg, b, err)) != VITX_OK) return rc;   // Transformer(depth = 1)
    { CompositeProf pr(m->prof_eng, "twins_peg_fwd"); launch_twins_peg_fwd(S.pre_peg, P + S.peg_w, P + S.peg_b, S.peg_out, b, S.H, S.W, S.d, m->kp, s); }
    for (int l = 1; l < S.L; ++l)                                                          // Transformer(depth = s_depth)
      if ((rc = twins_layer_fwd(m, S, l, l == 1 ? S.peg_out : S.out, S.out, b, err)) != VITX_OK) return rc;
  }
  // GlobalAvgPool2D + Dense (:261-264)
  const TwinsStage& last = m->st.back();
  CompositeProf pr(m->prof_eng, "twins_head");
  launch_mean_pool(last.out, b, last.H * last.W, last.d, m->pooled, s);
  dense_fwd(m->pooled, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and, when dimg_dev is given, d(img)
int twins_backward(vitx_twins* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b;
  launch_fill_zero(G, m->n_arena * 4, s);
  float *g = m->ga, *g2 = m->gb;   // g holds d(stage output map)
  {
    const TwinsStage& last = m->st.back();
    const int d = last.d;
    CompositeProf pr(m->prof_eng, "twins_head");
    dense_dw(m->pooled, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dpooled, b, m->nc, d, s);
    launch_mean_pool_bwd(m->dpooled, b, last.H * last.W, d, g, s);
  }
  int rc;
  for (int i = (int)m->st.size() - 1; i >= 0; --i) {
    TwinsStage& S = m->st[(size_t)i];
    const int rows = b * S.H * S.W;
    for (int l = S.L - 1; l >= 1; --l)
      if ((rc = twins_layer_bwd(m, S, l, g, b, err)) != VITX_OK) return rc;
    {   // PEG: g = d(peg_out) -> g2 = d(pre_peg)
      CompositeProf pr(m->prof_eng, "twins_peg_bwd");
      launch_colsum(g, 0, S.d, rows, S.d, m->ws, G + S.peg_b, s);
      launch_twins_peg_bwd_dkern(S.pre_peg, g, m->ws, G + S.peg_w, b, S.H, S.W, S.d, m->kp, s);
      launch_twins_peg_bwd_dx(g, P + S.peg_w, g2, b, S.H, S.W, S.d, m->kp, s);
      std::swap(g, g2);
    }
    if ((rc = twins_layer_bwd(m, S, 0, g, b, err)) != VITX_OK) return rc;
    if (S.loc && (rc = copy_maps(G, S.loc->grads, S.loc_maps, false, s, err)) != VITX_OK) return rc;
    if ((rc = copy_maps(G, S.glb->grads, S.glb_maps, false, s, err)) != VITX_OK) return rc;
    // PatchEmbedding: g = d(emb)
    CompositeProf pr(m->prof_eng, "twins_embed");
    dense_dw(S.patches, S.pd, g, G + S.emb_w, rows, S.d, S.pd, s, m->x3);
    launch_colsum(g, 0, S.d, rows, S.d, m->ws, G + S.emb_b, s);
    if (i == 0 && !dimg_dev) break;
    dense_dx(g, P + S.emb_w, m->dpatches, rows, S.d, S.pd, s, m->x3);
    launch_twins_patch_scatter(m->dpatches, S.pd, i == 0 ? dimg_dev : g2, b, S.Hin, S.Win, S.cin, S.p, s);
    std::swap(g, g2);
  }
  return VITX_OK;
}

std::vector<vitx_engine*> twins_engines(vitx_twins* m) {
  std::vector<vitx_engine*> v;
  for (TwinsStage& S : m->st) { if (S.loc) v.push_back(S.loc); v.push_back(S.glb); }
  return v;
}

}  // namespace

extern "C" {

int32_t vitx_twins_param_table_size(const vitx_twins_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, twins_param_table);
}
int32_t vitx_twins_param_table_entry(const vitx_twins_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                     int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, twins_param_table);
}
int32_t vitx_twins_create(const vitx_twins_config* cfg, vitx_twins_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, twins_create);
}
int32_t vitx_twins_destroy(vitx_twins_handle m) {
  CAPI_TRY
  twins_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_twins, "blob size does not match the TwinsSVT parameter table")
int32_t vitx_twins_forward_dev(vitx_twins_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  std::string err;
  int rc = twins_forward(m, img_dev, b, err);   // (the image is read once: the VJP works from the gathered patches)
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_twins_forward(vitx_twins_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_h * m->cfg.image_w * 3, b, logits_host,
                                [&](std::string& err) { return twins_forward(m, m->img, b, err); });
}
int32_t vitx_twins_backward_dev(vitx_twins_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = twins_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_twins_backward(vitx_twins_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_h * m->cfg.image_w * 3,
                                 [&](float* dimg_dev, std::string& err) { return twins_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_twins_profile_begin(vitx_twins_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(twins_engines(m));
}
int32_t vitx_twins_profile_end(vitx_twins_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(twins_engines(m), out, cap, n_out);
}
int32_t vitx_twins_read(vitx_twins_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const float* src = nullptr;
  int64_t n = 0;
  const int64_t b = m->b;
  auto stage_of = [&](const std::string& prefix) -> int {
    if (w.compare(0, prefix.size(), prefix) != 0 || w.size() != prefix.size() + 1) return -1;
    const int v = w[prefix.size()] - '0';
    return v >= 0 && v < (int)m->st.size() ? v : -1;
  };
  int i;
  if (w == "pooled") { src = m->pooled; n = b * m->st.back().d; }
  else if ((i = stage_of("embedded.")) >= 0) src = m->st[(size_t)i].emb;
  else if ((i = stage_of("pre_peg.")) >= 0) src = m->st[(size_t)i].pre_peg;
  else if ((i = stage_of("peg.")) >= 0) src = m->st[(size_t)i].peg_out;
  else if ((i = stage_of("stage.")) >= 0) src = m->st[(size_t)i].out;
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  if (w != "pooled") { const TwinsStage& S = m->st[(size_t)i]; n = b * S.H * S.W * S.d; }
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
