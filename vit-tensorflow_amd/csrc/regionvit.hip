// RegionViT (regionvit.py:184-263).  Two maps travel through four stages: the LOCAL map (Conv2D 8x8 stride 4 'SAME', or three 3x3 convolutions with
// Keras LayerNormalization and exact GELU between them, :210-221) and the REGION map (the (c p1 p2) patches of local_patch_size * window_size pixels
// -- twins_ops.hip's gather -- through a 1x1 convolution, :223-226).  A stage is a Downsample (Conv2D 3x3 stride 2 'SAME', stages 2-4) applied to
// BOTH maps with the same kernel and bias (:258), an optional PEG on the local map (twins_ops.hip), and an R2LTransformer (:118-182): per layer
//     region = attn(region) + region                        on the b sequences of rh * rw region tokens, no bias
//     x = [region token | window's local tokens]            per (lh / rh) x (lw / rw) window (regionvit_ops.hip)
//     x = attn(x, bias) + x;  x = ff(x) + x                 THE SAME attn as above; bias: the stage's Embedding, per head, zero for the region token
//     region, local = x[:, :1], x[:, 1:]
// The convolutions are im2col rows (cct_tok.hip) times the HWIO kernel on the GEMM launchers, in image chunks.  A stage with layers owns two
// vitx_config.nest_block engines with one block per layer, run a layer at a time: `win` over the (b * windows) sequences of 1 + wh * ww tokens,
// whose blocks are the whole pair (attention with the per-head bias through vitx_engine::attn_bias / attn_bias_hs, then the MLP), and `reg` over the
// region sequences, whose blocks stop behind the attention (BlockActs::skip_mlp).  Both receive the layer's attention parameters; the gradient of
// norm, to_qkv and to_out is the SUM of the two engines' (copy of win's, then reg's added).  Downsample's gradient is the sum over the two maps
// in the same way.  The embedding is a variable: every window block's backward adds its sum over the sequences of dS into the stage's
// [4, n, n] accumulator (vitx_engine::attn_dbias, attn_lsa.hip's launch_attn_dbias), gathered onto the table once per stage.
// The reference as written (and the fixtures): the local tokens behind the last layer reach nothing, so that layer gives its embedding a gradient
// of exactly zero -- here the zero d(local) simply runs through; nothing is skipped.  A stage without layers never touches its embedding.
// Encoders, Downsample, PEG and head keep fp32 storage in every compute mode; in the bf16 / bf16x3 modes their GEMMs take the split-operand MFMA
// path.  Table order: DESIGN.md section 26.  Only the deterministic path exists (ff_dropout 0; attn_dropout is unused by the reference).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

// what window_attn = 0 means: the one-wave-per-window kernels (attn_window.hip) for window sequences of at most 64 tokens in the bf16 mode
// 
constexpr bool RV_WINDOW_ATTN_DEFAULT = true;
constexpr int RV_STAGES = 4, RV_DIM_HEAD = 32, RV_HEADS = 4, RV_INNER = RV_HEADS * RV_DIM_HEAD, RV_MULT = 4, RV_N_MAX = LSA_N_MAX;   // regionvit.py:80,65

struct RvConv { int k = 0, st = 1, cin = 0, cout = 0, K = 0, Kp = 0; int64_t kern = -1, bias = -1; };   // a 'SAME' Conv2D with bias

RvConv rv_conv(int k, int st, int cin, int cout) {
  RvConv Q;
  Q.k = k; Q.st = st; Q.cin = cin; Q.cout = cout; Q.K = k * k * cin; Q.Kp = (int)round_up(Q.K, 64);
  return Q;
}

struct RvStage {
  int d = 0, depth = 0, cin = 0;
  int lh_in = 0, lw_in = 0, rh_in = 0, rw_in = 0;        // the maps in front of the Downsample
  int lh = 0, lw = 0, rh = 0, rw = 0, wh = 0, ww = 0, n = 0;   // behind it; the window and its tokens + 1
  bool has_down = false, has_peg = false;
  RvConv down;
  int64_t peg_w = -1, peg_b = -1, emb = -1;
  vitx_engine *win = nullptr, *reg = nullptr;
  std::vector<ArenaMap> win_maps, reg_maps;
  float *bias = nullptr, *dbias = nullptr;               // [4, n, n]
  float *loc_dn = nullptr, *reg_dn = nullptr, *loc_peg = nullptr, *loc_out = nullptr, *reg_out = nullptr;
};

}  // namespace

struct vitx_regionvit {
  vitx_regionvit_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<RvStage> st;
  bool conv3 = false;
  RvConv enc[3];                    // local encoder: enc[0] alone (8x8 stride 4), or the three 3x3 convolutions
  int64_t enc_g[2] = {-1, -1}, enc_b[2] = {-1, -1};
  int eh[3] = {0, 0, 0}, ew[3] = {0, 0, 0};   // output maps of the encoder's convolutions
  float *enc_c[2] = {nullptr, nullptr}, *enc_n[2] = {nullptr, nullptr}, *enc_a[2] = {nullptr, nullptr}, *enc_mean[2] = {nullptr, nullptr},
        *enc_rstd[2] = {nullptr, nullptr};
  int p = 0, pd = 0;                // region patch and its row length 3 p p
  int64_t renc_w = -1, renc_b = -1, head_g = -1, head_b = -1, fc_w = -1, fc_b = -1;
  float *loc0 = nullptr, *reg0 = nullptr;
  vitx_engine* prof_eng = nullptr;  // the composite's own launches are booked on the first engine
  int nc = 0, B = 0, x3 = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *rows = nullptr, *drows = nullptr, *gw_part = nullptr, *gw_slices = nullptr;
  float *tok_a = nullptr, *tok_b = nullptr, *reg_tmp = nullptr, *gl[2] = {nullptr, nullptr}, *gr[2] = {nullptr, nullptr};
  float *pooled = nullptr, *yh = nullptr, *mean_h = nullptr, *rstd_h = nullptr, *dyh = nullptr, *dpooled = nullptr, *ws = nullptr, *dvec = nullptr,
        *dbias_ws = nullptr;
  bool have_fwd = false;
  int b = 0;
};

namespace {

// stages and, when the configuration names an image, their maps; "" or what is wrong with the configuration
std::string rv_geometry(const vitx_regionvit_config& c, std::vector<RvStage>& out) {
  out.clear();
  if (c.num_classes <= 0) return "num_classes must be positive";
  if (c.image_h < 0 || c.image_w < 0 || (c.image_h == 0) != (c.image_w == 0)) return "invalid image size";
  if (c.window_size <= 0 || c.window_size > 64) return "window_size must be in 1 .. 64";
  if (c.local_patch_size <= 0 || c.local_patch_size > 256) return "local_patch_size must be in 1 .. 256";
  const int p = c.local_patch_size * c.window_size;
  if (c.image_h > 0 && (c.image_h % p || c.image_w % p))
    return "height and width must be divisible by region patch size (" + std::to_string(p) + "; regionvit.py:251)";
  int lh = (int)ceil_div(c.image_h, 4), lw = (int)ceil_div(c.image_w, 4), rh = c.image_h / p, rw = c.image_w / p, cin = c.dim[0];   // (the local encoder is stride 4 whatever local_patch_size says)
  for (int i = 0; i < RV_STAGES; ++i) {
    RvStage S;
    S.d = c.dim[i]; S.depth = c.depth[i]; S.cin = cin;
    const std::string sn = "stage " + std::to_string(i + 1);
    if (S.d <= 0 || S.d > 4096) return sn + ": dim must be in 1 .. 4096";
    if (S.depth < 0) return sn + ": depth must be >= 0";
    S.has_down = i > 0; S.has_peg = i > 0 && c.use_peg;
    if (S.has_down) S.down = rv_conv(3, 2, cin, S.d);
    if (c.image_h > 0) {
      S.lh_in = lh; S.lw_in = lw; S.rh_in = rh; S.rw_in = rw;
      if (S.has_down) { lh = (int)ceil_div(lh, 2); lw = (int)ceil_div(lw, 2); rh = (int)ceil_div(rh, 2); rw = (int)ceil_div(rw, 2); }
      S.lh = lh; S.lw = lw; S.rh = rh; S.rw = rw;
      const std::string maps = "the region map (" + std::to_string(rh) + " x " + std::to_string(rw) + ") and the local map (" + std::to_string(lh) + " x " +
                               std::to_string(lw) + ")";
      if (lh % rh || lw % rw || lh / rh == 0 || lw / rw == 0 || lh / (lh / rh) != rh || lw / (lw / rw) != rw)
        return sn + ": " + maps + " do not cut into windows (the reference's rearrange, regionvit.py:164, fails there)";
      S.wh = lh / rh; S.ww = lw / rw; S.n = 1 + S.wh * S.ww;
      if (S.depth > 0) {
        if (S.wh > c.window_size || S.ww > c.window_size)
          return sn + ": a " + std::to_string(S.wh) + " x " + std::to_string(S.ww) + " window leaves the position table of window_size = " + std::to_string(c.window_size);
        if (S.n > RV_N_MAX) return sn + ": a window plus its region token of more than 288 tokens is not built";
        if (rh * rw > RV_N_MAX) return sn + ": a region sequence of more than 288 tokens is not built (" + std::to_string(rh * rw) + ")";
      }
    }
    cin = S.d;
    out.push_back(S);
  }
  return "";
}

}  // namespace

// Table of RegionViT's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string regionvit_param_table(const vitx_regionvit_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_regionvit* m = nullptr) {
  out.clear();
  std::vector<RvStage> st;
  const std::string e = rv_geometry(c, st);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  const int64_t d0 = c.dim[0];
  RvConv enc[3];
  int64_t eg[2] = {-1, -1}, eb[2] = {-1, -1};
  if (c.tokenize_local_3_conv) {
    static const int idx[3] = {0, 3, 6}, strides[3] = {2, 2, 1};   // positions in the reference's Sequential (:211-219)
    for (int j = 0; j < 3; ++j) {
      enc[j] = rv_conv(3, strides[j], j ? (int)d0 : 3, (int)d0);
      const std::string q = "local_encoder." + std::to_string(idx[j]);
      enc[j].kern = tb.add(q + ".kernel", {3, 3, enc[j].cin, d0}); enc[j].bias = tb.add(q + ".bias", {d0});
      if (j < 2) {
        const std::string qn = "local_encoder." + std::to_string(idx[j] + 1);
        eg[j] = tb.add(qn + ".gamma", {d0}); eb[j] = tb.add(qn + ".beta", {d0});
      }
    }
  } else {
    enc[0] = rv_conv(8, 4, 3, (int)d0);
    enc[0].kern = tb.add("local_encoder.kernel", {8, 8, 3, d0}); enc[0].bias = tb.add("local_encoder.bias", {d0});
  }
  const int64_t p = (int64_t)c.local_patch_size * c.window_size, pd = 3 * p * p;
  const int64_t rw_ = tb.add("region_encoder.1.kernel", {1, 1, pd, d0}), rb_ = tb.add("region_encoder.1.bias", {d0});
  const int64_t side = 2 * c.window_size - 1;
  for (size_t i = 0; i < st.size(); ++i) {
    RvStage& S = st[i];
    const int64_t d = S.d, hid = d * RV_MULT;
    const std::string pre = "region_layers." + std::to_string(i);
    if (S.has_down) { S.down.kern = tb.add(pre + ".down.conv.kernel", {3, 3, S.cin, d}); S.down.bias = tb.add(pre + ".down.conv.bias", {d}); }
    if (S.has_peg) { S.peg_w = tb.add(pre + ".peg.proj.kernel", {3, 3, 1, d}); S.peg_b = tb.add(pre + ".peg.proj.bias", {d}); }
    S.emb = tb.add(pre + ".transformer.local_rel_pos_bias", {side * side, RV_HEADS});
    for (int l = 0; l < S.depth; ++l) {
      const std::string q = pre + ".transformer." + std::to_string(l);
      tb.add(q + ".attn.norm.gamma", {d}); tb.add(q + ".attn.norm.beta", {d});
      tb.add(q + ".attn.to_qkv.kernel", {d, 3 * RV_INNER});
      tb.add(q + ".attn.to_out.kernel", {RV_INNER, d}); tb.add(q + ".attn.to_out.bias", {d});
      tb.add(q + ".ff.norm.gamma", {d}); tb.add(q + ".ff.norm.beta", {d});
      tb.add(q + ".ff.fc1.kernel", {d, hid}); tb.add(q + ".ff.fc1.bias", {hid});
      tb.add(q + ".ff.fc2.kernel", {hid, d}); tb.add(q + ".ff.fc2.bias", {d});
    }
  }
  const int64_t dl = st.back().d;
  const int64_t hg = tb.add("to_logits.norm.gamma", {dl}), hb = tb.add("to_logits.norm.beta", {dl});
  const int64_t fw = tb.add("to_logits.kernel", {dl, c.num_classes}), fb = tb.add("to_logits.bias", {c.num_classes});
  if (m) {
    m->st = st; m->conv3 = c.tokenize_local_3_conv != 0;
    for (int j = 0; j < 3; ++j) m->enc[j] = enc[j];
    for (int j = 0; j < 2; ++j) { m->enc_g[j] = eg[j]; m->enc_b[j] = eb[j]; }
    m->p = (int)p; m->pd = (int)pd; m->renc_w = rw_; m->renc_b = rb_;
    m->head_g = hg; m->head_b = hb; m->fc_w = fw; m->fc_b = fb; m->nc = c.num_classes;
  }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config rv_engine_config(const vitx_regionvit_config& c, const RvStage& S, bool region) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.image_h = 1; ec.image_w = region ? S.rh * S.rw : S.n;
  ec.max_batch = region ? c.max_batch : (int32_t)((int64_t)c.max_batch * S.rh * S.rw);
  ec.num_classes = 1; ec.dim = S.d; ec.depth = S.depth; ec.heads = RV_HEADS; ec.dim_head = RV_DIM_HEAD;
  ec.mlp_dim = S.d * RV_MULT; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.device_id = c.device_id;
  ec.nest_block = 1;
  return ec;
}

// everything a configuration can be refused for without a device
int rv_check(const vitx_regionvit_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_regionvit probe;
  const std::string e = regionvit_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.image_h <= 0) { err = "vitx_regionvit_create needs the image size"; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  if ((int64_t)c.image_h * c.image_w > (1 << 24)) { err = "the image is too large"; return VITX_ERR_INVALID; }
  for (const RvStage& S : probe.st) {
    if (c.compute == VITX_COMPUTE_BF16 && S.d % 64) {
      err = "BF16 compute needs every stage's dim to be a multiple of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    if (!S.depth) continue;
    // (the attention kernels take one (sequence, head, row tile) per workgroup with the sequence on the grid's z axis)
    if ((int64_t)c.max_batch * S.rh * S.rw > 65535) { err = "max_batch * windows of a stage must be <= 65535"; return VITX_ERR_INVALID; }
    for (int g = 0; g < 2; ++g) {
      std::vector<ParamDesc> et;
      const std::string ee = build_param_table(rv_engine_config(c, S, g == 1), et);
      if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
    }
  }
  return VITX_OK;
}

#define RVALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void rv_destroy(vitx_regionvit* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (RvStage& S : m->st) {
    if (S.win) engine_destroy(S.win);
    if (S.reg) engine_destroy(S.reg);
  }
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  delete m;
}

// parameter maps of one stage: block l of the window engine = layer l (attention and MLP), block l of the region engine = layer l's attention
int rv_maps(vitx_regionvit* m, size_t si, std::string& err) {
  RvStage& S = m->st[si];
  static const char* ATTN[][2] = {{"norm.gamma", "attn.norm.gamma"}, {"norm.beta", "attn.norm.beta"}, {"to_qkv.kernel", "attn.to_qkv.kernel"},
                                  {"to_out.kernel", "attn.to_out.kernel"}, {"to_out.bias", "attn.to_out.bias"}};
  static const char* FF[][2] = {{"norm.gamma", "mlp.norm.gamma"}, {"norm.beta", "mlp.norm.beta"}, {"fc1.kernel", "mlp.fc1.kernel"}, {"fc1.bias", "mlp.fc1.bias"},
                                {"fc2.kernel", "mlp.fc2.kernel"}, {"fc2.bias", "mlp.fc2.bias"}};
  for (int l = 0; l < S.depth; ++l) {
    const std::string q = "region_layers." + std::to_string(si) + ".transformer." + std::to_string(l);
    const std::string eq = "transformer." + std::to_string(l) + ".";
    for (const auto& pr : ATTN) {
      if (add_arena_map(S.win_maps, m->table, q + ".attn." + pr[0], S.win->table, eq + pr[1], err) != VITX_OK) return VITX_ERR_INVALID;
      if (add_arena_map(S.reg_maps, m->table, q + ".attn." + pr[0], S.reg->table, eq + pr[1], err) != VITX_OK) return VITX_ERR_INVALID;
    }
    for (const auto& pr : FF) if (add_arena_map(S.win_maps, m->table, q + ".ff." + pr[0], S.win->table, eq + pr[1], err) != VITX_OK) return VITX_ERR_INVALID;
  }
  return VITX_OK;
}

int64_t rv_conv_chunk(const RvConv& Q, int B, int H, int W) {
  const int64_t per_image = ceil_div(H, Q.st) * ceil_div(W, Q.st) * Q.Kp;
  return std::min<int64_t>(B, std::max<int64_t>(1, IM2COL_BUDGET / per_image));
}

int rv_create(const vitx_regionvit_config& cin, vitx_regionvit** out, std::string& err) {
  vitx_regionvit_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-3f;   // Keras LayerNormalization's default (regionvit.py:69,87,213,245)
  int rc = rv_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_regionvit* m = new vitx_regionvit();
  m->cfg = c;
  auto fail = [&](int code) { rv_destroy(m); return code; };
  regionvit_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // two engines per stage with layers; all of them run on the first one's stream
  for (size_t i = 0; i < m->st.size(); ++i) {
    RvStage& S = m->st[i];
    if (!S.depth) continue;
    if ((rc = engine_create(rv_engine_config(c, S, false), &S.win, err)) != VITX_OK) return fail(rc);
    if ((rc = engine_create(rv_engine_config(c, S, true), &S.reg, err)) != VITX_OK) return fail(rc);
    S.win->window_attn = c.window_attn > 0 || (c.window_attn == 0 && RV_WINDOW_ATTN_DEFAULT);
    for (BlockActs& ba : S.reg->stages[0].ba) { ba.skip_mlp = true; ba.x_out = ba.x_mid; }   // region = attn(region) + region: the block stops there
    if (!m->prof_eng) { m->prof_eng = S.win; m->stream = S.win->stream; }
    if ((rc = rv_maps(m, i, err)) != VITX_OK) return fail(rc);
  }
  if (!m->stream) {   // no stage has layers: a stream of the handle's own
    if (hipSetDevice(c.device_id) != hipSuccess || hipStreamCreate(&m->own_stream) != hipSuccess) { err = "hipStreamCreate failed"; return fail(VITX_ERR_HIP); }
    m->stream = m->own_stream;
  }
  const int64_t B = m->B;
  RVALLOC(m->params, m->n_arena);
  RVALLOC(m->grads, m->n_arena);
  int64_t loc_max = 1, reg_max = 1, tok_max = 1, rows_max = 1, drows_max = 1, gw_max = 1, dbias_max = 1;
  int dmax = 1;
  auto conv_use = [&](const RvConv& Q, int H, int W) {   // workspaces of one use of a convolution on an H x W map
    const int64_t ch = rv_conv_chunk(Q, (int)B, H, W), px = ceil_div(H, Q.st) * ceil_div(W, Q.st);
    rows_max = std::max(rows_max, ch * px * Q.Kp);
    drows_max = std::max(drows_max, ch * px * Q.K);
    gw_max = std::max(gw_max, (int64_t)Q.Kp * Q.cout);
  };
  // local encoder
  {
    int H = c.image_h, W = c.image_w;
    for (int j = 0; j < (m->conv3 ? 3 : 1); ++j) {
      conv_use(m->enc[j], H, W);
      H = (int)ceil_div(H, m->enc[j].st); W = (int)ceil_div(W, m->enc[j].st);
      m->eh[j] = H; m->ew[j] = W;
      if (m->conv3 && j < 2) {
        const int64_t el = B * H * W * c.dim[0];
        RVALLOC(m->enc_c[j], el); RVALLOC(m->enc_n[j], el); RVALLOC(m->enc_a[j], el);
        RVALLOC(m->enc_mean[j], B * H * W); RVALLOC(m->enc_rstd[j], B * H * W);
        loc_max = std::max(loc_max, el);
      }
    }
  }
  const RvStage& S0 = m->st[0];
  RVALLOC(m->loc0, B * S0.lh * S0.lw * S0.d);
  RVALLOC(m->reg0, B * S0.rh * S0.rw * S0.d);
  rows_max = std::max(rows_max, B * S0.rh * S0.rw * m->pd);
  drows_max = std::max(drows_max, B * S0.rh * S0.rw * m->pd);
  for (size_t i = 0; i < m->st.size(); ++i) {
    RvStage& S = m->st[i];
    const int64_t le = B * S.lh * S.lw * S.d, re = B * S.rh * S.rw * S.d;
    loc_max = std::max({loc_max, le, B * S.lh_in * S.lw_in * S.cin});
    reg_max = std::max({reg_max, re, B * S.rh_in * S.rw_in * S.cin});
    tok_max = std::max(tok_max, B * S.rh * S.rw * S.n * S.d);
    dmax = std::max(dmax, S.d);
    if (S.has_down) {
      conv_use(S.down, S.lh_in, S.lw_in); conv_use(S.down, S.rh_in, S.rw_in);
      RVALLOC(S.loc_dn, le); RVALLOC(S.reg_dn, re);
    } else { S.loc_dn = m->loc0; S.reg_dn = m->reg0; }
    if (S.has_peg) RVALLOC(S.loc_peg, le); else S.loc_peg = S.loc_dn;
    if (S.depth) {
      RVALLOC(S.loc_out, le); RVALLOC(S.reg_out, re);
      RVALLOC(S.bias, (int64_t)RV_HEADS * S.n * S.n); RVALLOC(S.dbias, (int64_t)RV_HEADS * S.n * S.n);
      dbias_max = std::max(dbias_max, attn_dbias_ws_elems((int)(B * S.rh * S.rw), S.n, RV_HEADS));
      S.win->attn_bias_n = S.n;
      S.win->attn_bias_hs = (int64_t)S.n * S.n;
      for (int l = 0; l < S.depth; ++l) S.win->attn_bias.push_back(S.bias);   // one bias per stage, shared by its layers (:126)
      S.win->attn_dbias = S.dbias;
    } else { S.loc_out = S.loc_peg; S.reg_out = S.reg_dn; }
  }
  const int64_t img_elems = B * c.image_h * c.image_w * 3;
  loc_max = std::max(loc_max, img_elems);   // (d(img) of the local encoder passes through a gradient buffer)
  RVALLOC(m->img, img_elems); RVALLOC(m->dimg, img_elems);
  RVALLOC(m->logits, B * m->nc); RVALLOC(m->dlogits, B * m->nc);
  RVALLOC(m->rows, rows_max); RVALLOC(m->drows, drows_max);
  RVALLOC(m->gw_part, gw_max); RVALLOC(m->gw_slices, CONV_WGRAD_SLICES * gw_max);
  RVALLOC(m->tok_a, tok_max); RVALLOC(m->tok_b, tok_max); RVALLOC(m->reg_tmp, reg_max);
  for (int j = 0; j < 2; ++j) { RVALLOC(m->gl[j], loc_max); RVALLOC(m->gr[j], reg_max); }
  const int dl = m->st.back().d;
  RVALLOC(m->pooled, B * dl); RVALLOC(m->yh, B * dl); RVALLOC(m->mean_h, B); RVALLOC(m->rstd_h, B); RVALLOC(m->dyh, B * dl); RVALLOC(m->dpooled, B * dl);
  RVALLOC(m->ws, std::max<int64_t>({layernorm_bwd_ws_elems(dmax), colsum_ws_elems(std::max(dmax, m->nc)), twins_peg_ws_elems(dmax, 3)}) + 64);
  RVALLOC(m->dvec, dmax);
  RVALLOC(m->dbias_ws, dbias_max);
  for (RvStage& S : m->st) if (S.win) S.win->attn_dbias_ws = m->dbias_ws;
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

// the composite's arena to the engines, and every stage's position bias from its embedding table
int push_params(vitx_regionvit* m, std::string& err) {
  int rc;
  for (RvStage& S : m->st) {
    if (!S.depth) continue;
    if ((rc = copy_maps(m->params, S.win->params, S.win_maps, true, m->stream, err)) != VITX_OK) return rc;
    S.win->params_dirty = true;
    if ((rc = copy_maps(m->params, S.reg->params, S.reg_maps, true, m->stream, err)) != VITX_OK) return rc;
    S.reg->params_dirty = true;
    CompositeProf pr(m->prof_eng, "rv_bias");
    launch_rv_bias_build(m->params + S.emb, S.bias, m->cfg.window_size, S.wh, S.ww, RV_HEADS, m->stream);
  }
  return VITX_OK;
}

// y [b, ceil(H / st), ceil(W / st), cout] = Conv2D 'SAME' of x [b, H, W, cin], in image chunks
void rv_conv_fwd(vitx_regionvit* m, const RvConv& Q, const float* x, int b, int H, int W, float* y) {
  hipStream_t s = m->stream;
  const float* P = m->params;
  const int px = (int)(ceil_div(H, Q.st) * ceil_div(W, Q.st));
  const int64_t in_img = (int64_t)H * W * Q.cin, out_img = (int64_t)px * Q.cout;
  const int chunk = (int)rv_conv_chunk(Q, m->B, H, W);
  for (int b0 = 0; b0 < b; b0 += chunk) {
    const int nb = std::min(chunk, b - b0);
    { CompositeProf pr(m->prof_eng, "rv_im2col"); launch_cct_im2col(x + b0 * in_img, m->rows, nb, H, W, Q.cin, Q.k, Q.st, Q.Kp, s); }
    CompositeProf pr(m->prof_eng, "rv_conv_gemm");
    dense_fwd(m->rows, Q.Kp, P + Q.kern, P + Q.bias, y + b0 * out_img, nb * px, Q.cout, Q.K, s, m->x3);
  }
}

// its VJP for dy: the kernel's and the bias's gradient (accumulate: ADDED to what the arena holds -- the second use of a shared convolution) and,
// when dx is given, d(x) (every element written)
void rv_conv_bwd(vitx_regionvit* m, const RvConv& Q, const float* x, const float* dy, int b, int H, int W, float* dx, bool accumulate) {
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int px = (int)(ceil_div(H, Q.st) * ceil_div(W, Q.st));
  const int64_t in_img = (int64_t)H * W * Q.cin, out_img = (int64_t)px * Q.cout, nw = (int64_t)Q.K * Q.cout;
  {
    CompositeProf pr(m->prof_eng, "rv_conv_gemm");
    launch_colsum(dy, 0, Q.cout, b * px, Q.cout, m->ws, accumulate ? m->dvec : G + Q.bias, s);
    if (accumulate) launch_rv_add(G + Q.bias, m->dvec, Q.cout, s);
  }
  const int chunk = (int)rv_conv_chunk(Q, m->B, H, W);
  for (int b0 = 0; b0 < b; b0 += chunk) {
    const int nb = std::min(chunk, b - b0);
    const int rows = nb * px;
    { CompositeProf pr(m->prof_eng, "rv_im2col"); launch_cct_im2col(x + b0 * in_img, m->rows, nb, H, W, Q.cin, Q.k, Q.st, Q.Kp, s); }
    {
      CompositeProf pr(m->prof_eng, "rv_conv_gemm");
      conv_wgrad(m->rows, Q.Kp, dy + b0 * out_img, m->gw_part, m->gw_slices, rows, Q.cout, m->x3, s);
      hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + Q.kern, (const float*)m->gw_part, nw, b0 == 0 && !accumulate ? 1 : 0);
      if (dx) dense_dx(dy + b0 * out_img, P + Q.kern, m->drows, rows, Q.cout, Q.K, s, m->x3);
    }
    if (!dx) continue;
    CompositeProf pr(m->prof_eng, "rv_col2im");
    launch_extract_patches_bwd(m->drows, dx + b0 * in_img, nb, H, W, Q.cin, Q.k, Q.st, s);
  }
}

int rv_forward(vitx_regionvit* m, const float* img_dev, int b, std::string& err) {
  const vitx_regionvit_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  int rc;
  const int d0 = c.dim[0];
  // local encoder (:210-221)
  if (m->conv3) {
    const float* x = img_dev;
    int H = c.image_h, W = c.image_w;
    for (int j = 0; j < 2; ++j) {
      rv_conv_fwd(m, m->enc[j], x, b, H, W, m->enc_c[j]);
      H = m->eh[j]; W = m->ew[j];
      CompositeProf pr(m->prof_eng, "rv_encoder");
      launch_layernorm_fwd(m->enc_c[j], d0, P + m->enc_g[j], P + m->enc_b[j], m->enc_n[j], 0, d0, m->enc_mean[j], m->enc_rstd[j], b * H * W, d0, c.ln_eps, s);
      launch_rv_gelu_fwd(m->enc_n[j], m->enc_a[j], (int64_t)b * H * W * d0, s);
      x = m->enc_a[j];
    }
    rv_conv_fwd(m, m->enc[2], x, b, H, W, m->loc0);
  } else {
    rv_conv_fwd(m, m->enc[0], img_dev, b, c.image_h, c.image_w, m->loc0);
  }
  // region encoder (:223-226)
  {
    const RvStage& S0 = m->st[0];
    CompositeProf pr(m->prof_eng, "rv_encoder");
    launch_twins_patch_gather(img_dev, m->rows, b, c.image_h, c.image_w, 3, m->p, m->pd, s);
    dense_fwd(m->rows, m->pd, P + m->renc_w, P + m->renc_b, m->reg0, b * S0.rh * S0.rw, d0, m->pd, s, m->x3);
  }
  const float *loc = m->loc0, *reg = m->reg0;
  for (size_t i = 0; i < m->st.size(); ++i) {
    RvStage& S = m->st[i];
    if (S.has_down) {   // :258, one kernel for both maps
      rv_conv_fwd(m, S.down, loc, b, S.lh_in, S.lw_in, S.loc_dn);
      rv_conv_fwd(m, S.down, reg, b, S.rh_in, S.rw_in, S.reg_dn);
    }
    if (S.has_peg) { CompositeProf pr(m->prof_eng, "rv_peg"); launch_twins_peg_fwd(S.loc_dn, P + S.peg_w, P + S.peg_b, S.loc_peg, b, S.lh, S.lw, S.d, 3, s); }
    loc = S.loc_peg; reg = S.reg_dn;
    for (int l = 0; l < S.depth; ++l) {
      S.reg->stream = s;
      if ((rc = engine_transformer_forward(S.reg, reg, b, S.rh * S.rw, 0, 0, m->reg_tmp, err, l, l + 1)) != VITX_OK) return rc;                   // :159
      { CompositeProf pr(m->prof_eng, "rv_windows"); launch_rv_join(m->reg_tmp, loc, m->tok_a, b, S.rh, S.rw, S.wh, S.ww, S.d, s); }                   // :163-168
      S.win->stream = s;
      if ((rc = engine_transformer_forward(S.win, m->tok_a, b * S.rh * S.rw, S.n, 0, 0, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;          // :169-172
      { CompositeProf pr(m->prof_eng, "rv_windows"); launch_rv_split(m->tok_b, S.reg_out, S.loc_out, b, S.rh, S.rw, S.wh, S.ww, S.d, s); }            // :175-177
      loc = S.loc_out; reg = S.reg_out;
    }
  }
  // Reduce('b h w c -> b c', 'mean'), LayerNormalization, Dense (:243-247) on the REGION map
  const RvStage& last = m->st.back();
  CompositeProf pr(m->prof_eng, "rv_head");
  launch_mean_pool(last.reg_out, b, last.rh * last.rw, last.d, m->pooled, s);
  launch_layernorm_fwd(m->pooled, last.d, P + m->head_g, P + m->head_b, m->yh, 0, last.d, m->mean_h, m->rstd_h, b, last.d, c.ln_eps, s);
  dense_fwd(m->yh, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and, when dimg_dev is given, d(img)
int rv_backward(vitx_regionvit* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  const vitx_regionvit_config& c = m->cfg;
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b, d0 = c.dim[0];
  launch_fill_zero(G, m->n_arena * 4, s);
  float *gl = m->gl[0], *gl2 = m->gl[1], *gr = m->gr[0], *gr2 = m->gr[1];   // d(local map), d(region map) of the stage output
  {
    const RvStage& last = m->st.back();
    const int d = last.d;
    CompositeProf pr(m->prof_eng, "rv_head");
    dense_dw(m->yh, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dyh, b, m->nc, d, s);
    launch_layernorm_bwd(m->dyh, 0, d, m->pooled, d, m->mean_h, m->rstd_h, P + m->head_g, nullptr, 0, m->dpooled, d, nullptr, 0, m->ws, G + m->head_g,
                         G + m->head_b, nullptr, b, d, s);
    launch_mean_pool_bwd(m->dpooled, b, last.rh * last.rw, d, gr, s);
    launch_fill_zero(gl, round_up((int64_t)b * last.lh * last.lw * d, 4) * 4, s);   // the last local map reaches nothing (:262)
  }
  int rc;
  for (int i = (int)m->st.size() - 1; i >= 0; --i) {
    RvStage& S = m->st[(size_t)i];
    if (S.depth) launch_fill_zero(S.dbias, round_up((int64_t)RV_HEADS * S.n * S.n, 4) * 4, s);
    for (int l = S.depth - 1; l >= 0; --l) {
      { CompositeProf pr(m->prof_eng, "rv_windows"); launch_rv_join(gr, gl, m->tok_a, b, S.rh, S.rw, S.wh, S.ww, S.d, s); }
      S.win->stream = s;
      if ((rc = engine_transformer_backward(S.win, m->tok_a, m->tok_b, err, l, l + 1)) != VITX_OK) return rc;
      { CompositeProf pr(m->prof_eng, "rv_windows"); launch_rv_split(m->tok_b, gr, gl, b, S.rh, S.rw, S.wh, S.ww, S.d, s); }
      S.reg->stream = s;
      if ((rc = engine_transformer_backward(S.reg, gr, gr, err, l, l + 1)) != VITX_OK) return rc;
    }
    if (S.depth) {
      // norm, to_qkv, to_out ran twice per layer: the window engine's gradients, then the region engine's added
      if ((rc = copy_maps(G, S.win->grads, S.win_maps, false, s, err)) != VITX_OK) return rc;
      CompositeProf pr(m->prof_eng, "rv_bias");
      for (const ArenaMap& t : S.reg_maps) launch_rv_add(G + t.c, S.reg->grads + t.e, t.width, s);
      launch_rv_table_grad(S.dbias, G + S.emb, c.window_size, S.wh, S.ww, RV_HEADS, s);
    }
    if (S.has_peg) {   // gl = d(peg output) -> gl2 = d(its input)
      CompositeProf pr(m->prof_eng, "rv_peg");
      launch_colsum(gl, 0, S.d, b * S.lh * S.lw, S.d, m->ws, G + S.peg_b, s);
      launch_twins_peg_bwd_dkern(S.loc_dn, gl, m->ws, G + S.peg_w, b, S.lh, S.lw, S.d, 3, s);
      launch_twins_peg_bwd_dx(gl, P + S.peg_w, gl2, b, S.lh, S.lw, S.d, 3, s);
      std::swap(gl, gl2);
    }
    if (S.has_down) {   // one kernel, two maps: the local map's gradient, then the region map's added
      const RvStage& Pv = m->st[(size_t)i - 1];
      rv_conv_bwd(m, S.down, Pv.loc_out, gl, b, S.lh_in, S.lw_in, gl2, false);
      rv_conv_bwd(m, S.down, Pv.reg_out, gr, b, S.rh_in, S.rw_in, gr2, true);
      std::swap(gl, gl2); std::swap(gr, gr2);
    }
  }
  // region encoder: gr = d(reg0)
  {
    const RvStage& S0 = m->st[0];
    const int rows = b * S0.rh * S0.rw;
    CompositeProf pr(m->prof_eng, "rv_encoder");
    launch_twins_patch_gather(m->img, m->rows, b, c.image_h, c.image_w, 3, m->p, m->pd, s);
    dense_dw(m->rows, m->pd, gr, G + m->renc_w, rows, d0, m->pd, s, m->x3);
    launch_colsum(gr, 0, d0, rows, d0, m->ws, G + m->renc_b, s);
    if (dimg_dev) {
      dense_dx(gr, P + m->renc_w, m->drows, rows, d0, m->pd, s, m->x3);
      launch_twins_patch_scatter(m->drows, m->pd, dimg_dev, b, c.image_h, c.image_w, 3, m->p, s);
    }
  }
  // local encoder: gl = d(loc0); its d(img) is added to the region encoder's
  if (m->conv3) {
    rv_conv_bwd(m, m->enc[2], m->enc_a[1], gl, b, m->eh[1], m->ew[1], gl2, false);
    std::swap(gl, gl2);
    for (int j = 1; j >= 0; --j) {
      const int H = m->eh[j], W = m->ew[j];
      {
        CompositeProf pr(m->prof_eng, "rv_encoder");
        launch_rv_gelu_bwd(m->enc_n[j], gl, gl2, (int64_t)b * H * W * d0, s);
        launch_layernorm_bwd(gl2, 0, d0, m->enc_c[j], d0, m->enc_mean[j], m->enc_rstd[j], P + m->enc_g[j], nullptr, 0, gl, d0, nullptr, 0, m->ws, G + m->enc_g[j],
                             G + m->enc_b[j], nullptr, b * H * W, d0, s);
      }
      const float* x = j ? m->enc_a[0] : m->img;
      const int Hi = j ? m->eh[0] : c.image_h, Wi = j ? m->ew[0] : c.image_w;
      rv_conv_bwd(m, m->enc[j], x, gl, b, Hi, Wi, (j || dimg_dev) ? gl2 : nullptr, false);
      std::swap(gl, gl2);
    }
  } else {
    rv_conv_bwd(m, m->enc[0], m->img, gl, b, c.image_h, c.image_w, dimg_dev ? gl2 : nullptr, false);
    std::swap(gl, gl2);
  }
  if (dimg_dev) { CompositeProf pr(m->prof_eng, "rv_encoder"); launch_rv_add(dimg_dev, gl, (int64_t)b * c.image_h * c.image_w * 3, s); }
  return VITX_OK;
}

std::vector<vitx_engine*> rv_engines(vitx_regionvit* m) {
  std::vector<vitx_engine*> v;
  for (RvStage& S : m->st) { if (S.win) v.push_back(S.win); if (S.reg) v.push_back(S.reg); }
  return v;
}

uint16_t rv_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
float rv_to_f32(uint16_t v) { const uint32_t u = (uint32_t)v << 16; float f; std::memcpy(&f, &u, 4); return f; }

}  // namespace

extern "C" {

int32_t vitx_regionvit_param_table_size(const vitx_regionvit_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, regionvit_param_table);
}
int32_t vitx_regionvit_param_table_entry(const vitx_regionvit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                         int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, regionvit_param_table);
}
int32_t vitx_regionvit_create(const vitx_regionvit_config* cfg, vitx_regionvit_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, rv_create);
}
int32_t vitx_regionvit_destroy(vitx_regionvit_handle m) {
  CAPI_TRY
  rv_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_regionvit, "blob size does not match the RegionViT parameter table")
int32_t vitx_regionvit_forward_dev(vitx_regionvit_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  // (the encoders' weight gradients re-read the image: the handle keeps its own copy)
  CAPI_HIP(hipMemcpyAsync(m->img, img_dev, (size_t)b * m->cfg.image_h * m->cfg.image_w * 3 * 4, hipMemcpyDeviceToDevice, m->stream));
  std::string err;
  int rc = rv_forward(m, m->img, b, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_regionvit_forward(vitx_regionvit_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_h * m->cfg.image_w * 3, b, logits_host,
                                [&](std::string& err) { return rv_forward(m, m->img, b, err); });
}
int32_t vitx_regionvit_backward_dev(vitx_regionvit_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = rv_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_regionvit_backward(vitx_regionvit_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_h * m->cfg.image_w * 3,
                                 [&](float* dimg_dev, std::string& err) { return rv_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_regionvit_profile_begin(vitx_regionvit_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(rv_engines(m));
}
int32_t vitx_regionvit_profile_end(vitx_regionvit_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(rv_engines(m), out, cap, n_out);
}
int32_t vitx_regionvit_read(vitx_regionvit_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const int64_t b = m->b;
  auto stage_of = [&](const std::string& prefix) -> int {
    if (w.size() != prefix.size() + 1 || w.compare(0, prefix.size(), prefix) != 0) return -1;
    const int v = w[prefix.size()] - '0';
    return v >= 0 && v < (int)m->st.size() ? v : -1;
  };
  int i;
  if (w == "pooled") return composite_read_tail(m->pooled, b * m->st.back().d, out_host, cap, n_elems, m->stream);
  if ((i = stage_of("local.")) >= 0) { const RvStage& S = m->st[(size_t)i]; return composite_read_tail(S.loc_out, b * S.lh * S.lw * S.d, out_host, cap, n_elems, m->stream); }
  if ((i = stage_of("region.")) >= 0) { const RvStage& S = m->st[(size_t)i]; return composite_read_tail(S.reg_out, b * S.rh * S.rw * S.d, out_host, cap, n_elems, m->stream); }
  if ((i = stage_of("bias.")) >= 0 && m->st[(size_t)i].depth) {
    const RvStage& S = m->st[(size_t)i];
    return composite_read_tail(S.bias, (int64_t)RV_HEADS * S.n * S.n, out_host, cap, n_elems, m->stream);
  }
  return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  CAPI_CATCH
}
int32_t vitx_regionvit_attn(vitx_regionvit_handle m, const float* qkv_host, const float* d_o_host, const float* bias_host, int32_t b, int32_t n, int32_t h,
                            int32_t tail_rows, float tail_value, int32_t window_kernel, float* o_host, float* lse_host, float* dqkv_host,
                            float* dbias_host) {
  CAPI_TRY
  if (!m || !qkv_host || !d_o_host || !bias_host || !o_host || !lse_host || !dqkv_host || !dbias_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || h <= 0 || tail_rows < 0 || (int64_t)b * h > 65535 || b > 65535) return capi_fail(VITX_ERR_INVALID, "invalid shape");
  if (window_kernel ? !attn_window_supported(n, RV_DIM_HEAD) : !attn_small_supported(n, RV_DIM_HEAD)) return capi_fail(VITX_ERR_UNSUPPORTED, "n is outside the kernel's range");
  const int64_t inner = (int64_t)h * RV_DIM_HEAD, live = (int64_t)b * n, rows = live + tail_rows, nb = (int64_t)h * n * n;
  // host images: the live rows from the caller, the tail rows (inputs AND outputs) filled with tail_value
  std::vector<uint16_t> hq((size_t)(rows * 3 * inner), rv_to_bf16(tail_value)), hg((size_t)(rows * inner), rv_to_bf16(tail_value)), ho(hg), hd(hq);
  for (int64_t i = 0; i < live * 3 * inner; ++i) hq[(size_t)i] = rv_to_bf16(qkv_host[i]);
  for (int64_t i = 0; i < live * inner; ++i) hg[(size_t)i] = rv_to_bf16(d_o_host[i]);
  bf16_t *dq = nullptr, *dg = nullptr, *dout = nullptr, *dd = nullptr;
  float *dlse = nullptr, *dsum = nullptr, *dbias = nullptr, *dacc = nullptr, *dws = nullptr;
  std::vector<void*> owned;
  auto alloc = [&](void** p, size_t bytes) { if (hipMalloc(p, std::max<size_t>(bytes, 16)) != hipSuccess) return false; owned.push_back(*p); return true; };
  auto release = [&]() { for (void* p : owned) (void)hipFree(p); };
  const size_t stat = (size_t)b * h * n * 4;
  if (!alloc((void**)&dq, hq.size() * 2) || !alloc((void**)&dg, hg.size() * 2) || !alloc((void**)&dout, ho.size() * 2) || !alloc((void**)&dd, hd.size() * 2) ||
      !alloc((void**)&dlse, stat) || !alloc((void**)&dsum, stat) || !alloc((void**)&dbias, (size_t)nb * 4) || !alloc((void**)&dacc, (size_t)nb * 4) ||
      !alloc((void**)&dws, (size_t)attn_dbias_ws_elems(b, n, h) * 4)) { release(); return capi_fail(VITX_ERR_HIP, "hipMalloc failed"); }
  hipStream_t s = m->stream;
  const float scale = 1.0f / std::sqrt((float)RV_DIM_HEAD);
  hipError_t e = hipMemcpyAsync(dq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dg, hg.data(), hg.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dout, ho.data(), ho.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dd, hd.data(), hd.size() * 2, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dbias, bias_host, (size_t)nb * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(dacc, 0, (size_t)nb * 4, s);
  if (e == hipSuccess) {
    const int64_t hs = (int64_t)n * n;
    if (window_kernel) {
      launch_attn_window_fwd(dq, dout, dlse, dbias, b, n, h, scale, s, hs);
      launch_attn_window_bwd(dq, dout, dg, dlse, dd, dbias, b, n, h, scale, s, hs);
    } else {
      launch_attn_small_fwd(dq, dout, dlse, 1, b, n, h, RV_DIM_HEAD, scale, s, dbias, hs);
      launch_attn_small_bwd(dq, dout, dg, dlse, dsum, dd, 1, b, n, h, RV_DIM_HEAD, scale, s, dbias, hs);
    }
    launch_attn_dbias(dq, dout, dg, dlse, 1, b, n, h, scale, dbias, hs, dws, dacc, s);
    e = hipMemcpyAsync(ho.data(), dout, ho.size() * 2, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hd.data(), dd, hd.size() * 2, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(lse_host, dlse, stat, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dbias_host, dacc, (size_t)nb * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  release();
  if (e != hipSuccess) return capi_fail(VITX_ERR_HIP, hipGetErrorString(e));
  for (size_t i = 0; i < ho.size(); ++i) o_host[i] = rv_to_f32(ho[i]);
  for (size_t i = 0; i < hd.size(); ++i) dqkv_host[i] = rv_to_f32(hd[i]);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_regionvit_partition(vitx_regionvit_handle m, float* region_host, float* local_host, float* tokens_host, int32_t b, int32_t rh, int32_t rw,
                                 int32_t wh, int32_t ww, int32_t c, int32_t inverse) {
  CAPI_TRY
  if (!m || !region_host || !local_host || !tokens_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || rh <= 0 || rw <= 0 || wh <= 0 || ww <= 0 || c <= 0) return capi_fail(VITX_ERR_INVALID, "invalid shape");
  const size_t rb = (size_t)b * rh * rw * c * 4, lb = rb * wh * ww, tb = rb + lb;
  float *dr = nullptr, *dl = nullptr, *dt = nullptr;
  CAPI_HIP(hipMalloc(&dr, rb));
  if (hipMalloc(&dl, lb) != hipSuccess) { (void)hipFree(dr); return capi_fail(VITX_ERR_HIP, "hipMalloc failed"); }
  if (hipMalloc(&dt, tb) != hipSuccess) { (void)hipFree(dr); (void)hipFree(dl); return capi_fail(VITX_ERR_HIP, "hipMalloc failed"); }
  hipStream_t s = m->stream;
  hipError_t e;
  if (inverse) {
    e = hipMemcpyAsync(dt, tokens_host, tb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      launch_rv_split(dt, dr, dl, b, rh, rw, wh, ww, c, s);
      e = hipMemcpyAsync(region_host, dr, rb, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(local_host, dl, lb, hipMemcpyDeviceToHost, s);
  } else {
    e = hipMemcpyAsync(dr, region_host, rb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dl, local_host, lb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      launch_rv_join(dr, dl, dt, b, rh, rw, wh, ww, c, s);
      e = hipMemcpyAsync(tokens_host, dt, tb, hipMemcpyDeviceToHost, s);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(dr); (void)hipFree(dl); (void)hipFree(dt);
  if (e != hipSuccess) return capi_fail(VITX_ERR_HIP, hipGetErrorString(e));
  return VITX_OK;
  CAPI_CATCH
}

}  // extern "C"
