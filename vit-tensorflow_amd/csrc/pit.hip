// PiT (pit.py:158-219): Unfold(patch, stride patch // 2) + Dense (:179-182) as unfolded rows (pit_ops.hip) times the kernel in image chunks, the
// class token and the position rows (:211-213), then per stage a Transformer (:91-108) of `depth` layers x + Attention(LN x), x + MLP(LN x) on
// one ordinary ViT engine per stage (none at depth 0; stages never share one), and LayerNorm + Dense on row 0 (:202-205,217).
// pit.py:194 reads `not_last = ind < (len(depth) < 1)`, which is never true: the reference's PiT holds Transformers only and never calls its Pool
// (:140-156).  pool_stages == 0 is that model.  pool_stages != 0 runs the body of :196-200 with not_last true: Pool(dim) behind every stage but
// the last, the width doubled there.  Pool is pit_ops.hip's depthwise kernels around two Dense products.
// The tokenizer, Pool and the head keep fp32 storage in every compute mode; in the bf16 / bf16x3 modes their GEMMs take the split-operand MFMA
// path.  The composite owns the public parameter / gradient arenas in its own table order and copies them to / from the engines.
// Only the deterministic path exists (dropout 0).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

struct PitStage {
  int d = 0, heads = 0, depth = 0;
  int h = 0, w = 0, n = 0;                                                          // the stage's token map and 1 + h w (0 without an image)
  bool pool = false;                                                                // a Pool follows
  int64_t dw_k = -1, dw_b = -1, pw_k = -1, pw_b = -1, cls_k = -1, cls_b = -1;       // its arena offsets
  vitx_engine* eng = nullptr;
  std::vector<ArenaMap> maps;
  float *in = nullptr, *out = nullptr, *dw = nullptr;                               // [B, n, d] twice, Pool's depthwise output [B, 1 + oh ow, 2 d]
};

}  // namespace

struct vitx_pit {
  vitx_pit_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<PitStage> st;
  vitx_engine* prof_eng = nullptr;   // the composite's own launches are booked on the first engine
  int64_t emb_w = -1, emb_b = -1, pos = -1, cls = -1, hn_g = -1, hn_b = -1, fc_w = -1, fc_b = -1;
  int p = 0, stride = 0, pos_rows = 0, oh = 0, ow = 0, K = 0, Kp = 0, chunk = 1;
  int nc = 0, B = 0, x3 = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *rows = nullptr, *drows = nullptr, *gw_part = nullptr, *gw_slices = nullptr, *ga = nullptr, *gb = nullptr, *scr = nullptr;
  float *yh = nullptr, *dyh = nullptr, *mean_h = nullptr, *rstd_h = nullptr, *ws = nullptr, *pool_ws = nullptr;
  bool have_fwd = false;
  int b = 0;
  int pool_stage = -1, pool_b = 0, pool_hw = 0;   // state of the last vitx_pit_pool_forward
};

namespace {

// stages and, when the configuration names an image, their maps; "" or what is wrong with the configuration
std::string pit_geometry(const vitx_pit_config& c, vitx_pit& m) {
  m.st.clear();
  if (c.num_classes <= 0) return "num_classes must be positive";
  if (c.patch_size <= 0 || c.image_size <= 0 || c.image_size % c.patch_size) return "Image dimensions must be divisible by the patch size.";   // pit.py:173
  if (c.patch_size / 2 <= 0) return "patch_size // 2 (the stride of the patch windows, pit.py:180) must be positive";
  if (c.n_stages <= 0 || c.n_stages > VITX_PIT_MAX_STAGES) return "depth must name between 1 and 8 stages";
  if (c.dim <= 0 || c.mlp_dim <= 0 || c.dim_head <= 0) return "dim, mlp_dim and dim_head must be positive";
  if (c.image_h < 0 || c.image_w < 0 || (c.image_h == 0) != (c.image_w == 0)) return "invalid image size";
  m.p = c.patch_size; m.stride = c.patch_size / 2;
  const int out = (c.image_size - m.p) / m.stride + 1;   // conv_output_size (pit.py:16-17,184)
  m.pos_rows = out * out + 1;
  m.K = m.p * m.p * 3; m.Kp = (int)round_up(m.K, 64);
  m.oh = m.ow = 0;
  int h = 0, w = 0;
  if (c.image_h > 0) {
    if (c.image_h < m.p || c.image_w < m.p) return "the image is smaller than a patch";
    h = m.oh = (c.image_h - m.p) / m.stride + 1; w = m.ow = (c.image_w - m.p) / m.stride + 1;
    if ((int64_t)h * w + 1 > m.pos_rows)
      return "the image makes " + std::to_string((int64_t)h * w + 1) + " tokens, pos_embedding has " + std::to_string(m.pos_rows) + " rows";
  }
  int64_t d = c.dim;
  for (int i = 0; i < c.n_stages; ++i) {
    PitStage S;
    if (c.depth[i] < 0) return "depth must be >= 0";
    if (c.heads[i] <= 0) return "heads must be positive";
    if (d > 16384) return "a stage's width must be <= 16384";
    S.d = (int)d; S.heads = c.heads[i]; S.depth = c.depth[i];
    S.h = h; S.w = w; S.n = h > 0 ? 1 + h * w : 0;
    S.pool = c.pool_stages && i + 1 < c.n_stages;
    if (S.pool) {
      if (h > 0 && h != w) return "pool_stages: the token map of stage " + std::to_string(i) + " is " + std::to_string(h) + " x " + std::to_string(w) + ", Pool (pit.py:150) takes a square one";
      h = (h + 1) / 2; w = (w + 1) / 2; d *= 2;
    }
    m.st.push_back(S);
  }
  return "";
}

}  // namespace

// Table of PiT's variables in the documented order: the reference's attribute order, shapes as the reference holds them
std::string pit_param_table(const vitx_pit_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_pit* m = nullptr) {
  out.clear();
  vitx_pit local;
  vitx_pit& g = m ? *m : local;
  const std::string e = pit_geometry(c, g);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  const int64_t mlp = c.mlp_dim;
  g.emb_w = tb.add("patch_embedding.kernel", {g.K, c.dim}); g.emb_b = tb.add("patch_embedding.bias", {c.dim});
  g.pos = tb.add("pos_embedding", {1, g.pos_rows, c.dim}); g.cls = tb.add("cls_token", {1, 1, c.dim});
  for (size_t i = 0; i < g.st.size(); ++i) {
    PitStage& S = g.st[i];
    const int64_t d = S.d, inner = (int64_t)S.heads * c.dim_head;
    const bool project_out = !(S.heads == 1 && c.dim_head == S.d);   // pit.py:59
    for (int l = 0; l < S.depth; ++l) {
      const std::string q = "stage." + std::to_string(i) + "." + std::to_string(l);
      tb.add(q + ".attn.norm.gamma", {d}); tb.add(q + ".attn.norm.beta", {d});
      tb.add(q + ".attn.to_qkv.kernel", {d, 3 * inner});
      if (project_out) { tb.add(q + ".attn.to_out.kernel", {inner, d}); tb.add(q + ".attn.to_out.bias", {d}); }
      tb.add(q + ".ff.norm.gamma", {d}); tb.add(q + ".ff.norm.beta", {d});
      tb.add(q + ".ff.fc1.kernel", {d, mlp}); tb.add(q + ".ff.fc1.bias", {mlp});
      tb.add(q + ".ff.fc2.kernel", {mlp, d}); tb.add(q + ".ff.fc2.bias", {d});
    }
    if (!S.pool) continue;
    const std::string q = "pool." + std::to_string(i);
    S.dw_k = tb.add(q + ".downsample.dw.kernel", {3, 3, 1, 2 * d}); S.dw_b = tb.add(q + ".downsample.dw.bias", {2 * d});
    S.pw_k = tb.add(q + ".downsample.pw.kernel", {1, 1, 2 * d, 2 * d}); S.pw_b = tb.add(q + ".downsample.pw.bias", {2 * d});
    S.cls_k = tb.add(q + ".cls_ff.kernel", {d, 2 * d}); S.cls_b = tb.add(q + ".cls_ff.bias", {2 * d});
  }
  const int64_t dl = g.st.back().d;
  g.hn_g = tb.add("mlp_head.norm.gamma", {dl}); g.hn_b = tb.add("mlp_head.norm.beta", {dl});
  g.fc_w = tb.add("mlp_head.kernel", {dl, c.num_classes}); g.fc_b = tb.add("mlp_head.bias", {c.num_classes});
  g.nc = c.num_classes;
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config pit_engine_config(const vitx_pit_config& c, const PitStage& S) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.image_h = 1; ec.image_w = S.n - 1; ec.max_batch = c.max_batch;   // 1 + h w tokens with the class row
  ec.num_classes = 1; ec.dim = S.d; ec.depth = S.depth; ec.heads = S.heads; ec.dim_head = c.dim_head;
  ec.mlp_dim = c.mlp_dim; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.device_id = c.device_id;
  return ec;
}

// everything a configuration can be refused for without a device
int pit_check(const vitx_pit_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_pit probe;
  const std::string e = pit_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.image_h <= 0) { err = "vitx_pit_create needs the image size"; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  const int64_t B = c.max_batch;
  if (!pit_ops_fits(B * c.image_h * c.image_w * 3)) { err = "max_batch images exceed 2^31 elements"; return VITX_ERR_UNSUPPORTED; }
  for (const PitStage& S : probe.st) {
    if (c.compute == VITX_COMPUTE_BF16 && S.depth && S.d % 64) {
      err = "BF16 compute needs every stage's width to be a multiple of 64 (use FP32_PARITY or BF16X3 otherwise)";
      return VITX_ERR_UNSUPPORTED;
    }
    if (!pit_ops_fits(B * S.n * S.d * (S.pool ? 2 : 1))) { err = "max_batch token maps exceed 2^31 elements"; return VITX_ERR_UNSUPPORTED; }
    if (!S.depth) continue;
    std::vector<ParamDesc> et;
    const std::string ee = build_param_table(pit_engine_config(c, S), et);
    if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
  }
  return VITX_OK;
}

#define PTALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void pit_destroy(vitx_pit* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (PitStage& S : m->st) if (S.eng) engine_destroy(S.eng);
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  delete m;
}

// parameter maps of one stage: the composite's tensors of its blocks -> the engine's, same order in both; adjacent runs are merged
int pit_maps(vitx_pit* m, size_t si, std::string& err) {
  PitStage& S = m->st[si];
  static const char* NAMES[][2] = {
      {"attn.norm.gamma", "attn.norm.gamma"}, {"attn.norm.beta", "attn.norm.beta"}, {"attn.to_qkv.kernel", "attn.to_qkv.kernel"},
      {"attn.to_out.kernel", "attn.to_out.kernel"}, {"attn.to_out.bias", "attn.to_out.bias"},
      {"ff.norm.gamma", "mlp.norm.gamma"}, {"ff.norm.beta", "mlp.norm.beta"}, {"ff.fc1.kernel", "mlp.fc1.kernel"}, {"ff.fc1.bias", "mlp.fc1.bias"},
      {"ff.fc2.kernel", "mlp.fc2.kernel"}, {"ff.fc2.bias", "mlp.fc2.bias"}};
  const bool project_out = !(S.heads == 1 && m->cfg.dim_head == S.d);
  int rc = VITX_OK;
  for (int l = 0; l < S.depth && rc == VITX_OK; ++l) {
    const std::string q = "stage." + std::to_string(si) + "." + std::to_string(l) + ".";
    const std::string eq = "transformer." + std::to_string(l) + ".";
    for (const auto& pr : NAMES) {
      if (!project_out && !std::strncmp(pr[0], "attn.to_out", 11)) continue;
      if ((rc = add_arena_map(S.maps, m->table, q + pr[0], S.eng->table, eq + pr[1], err)) != VITX_OK) break;
    }
  }
  return rc;
}

int pit_create(const vitx_pit_config& cin, vitx_pit** out, std::string& err) {
  vitx_pit_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-3f;   // Keras LayerNormalization (pit.py:23,203)
  int rc = pit_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_pit* m = new vitx_pit();
  m->cfg = c;
  auto fail = [&](int code) { pit_destroy(m); return code; };
  pit_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  // one engine per stage with blocks; all of them run on the first one's stream
  for (size_t i = 0; i < m->st.size(); ++i) {
    PitStage& S = m->st[i];
    if (!S.depth) continue;
    if ((rc = engine_create(pit_engine_config(c, S), &S.eng, err)) != VITX_OK) return fail(rc);
    if (!m->prof_eng) { m->prof_eng = S.eng; m->stream = S.eng->stream; }
    if ((rc = pit_maps(m, i, err)) != VITX_OK) return fail(rc);
  }
  if (!m->prof_eng) {   // a handle of pools alone
    if (hipSetDevice(c.device_id) != hipSuccess || hipStreamCreate(&m->own_stream) != hipSuccess) { err = "hipStreamCreate failed"; return fail(VITX_ERR_HIP); }
    m->stream = m->own_stream;
  }
  if (c.long_attn) {
    for (PitStage& S : m->st)
      if (S.eng && (rc = vitx_set_long_attn(S.eng, 1)) != VITX_OK) { err = vitx_last_error(); return fail(rc); }
  }
  const int64_t B = m->B;
  PTALLOC(m->params, m->n_arena);
  PTALLOC(m->grads, m->n_arena);
  const int n0 = m->st[0].n;
  const int64_t per_image = (int64_t)n0 * m->Kp;
  m->chunk = (int)std::min<int64_t>(B, std::max<int64_t>(1, IM2COL_BUDGET / per_image));
  if (!pit_ops_fits((int64_t)m->chunk * per_image)) { err = "one image's patch rows exceed 2^31 elements"; return fail(VITX_ERR_UNSUPPORTED); }
  int64_t map_max = 1, scr_max = 1;
  int dmax = 1;
  for (size_t i = 0; i < m->st.size(); ++i) {
    PitStage& S = m->st[i];
    const int64_t el = B * S.n * S.d;
    map_max = std::max(map_max, el);
    dmax = std::max(dmax, S.d * (S.pool ? 2 : 1));
    if (i == 0) PTALLOC(S.in, el);
    else if (m->st[i - 1].pool) PTALLOC(S.in, el);
    else S.in = m->st[i - 1].out;
    if (S.eng) PTALLOC(S.out, el); else S.out = S.in;
    if (S.pool) {
      const int64_t no = 1 + (int64_t)((S.h + 1) / 2) * ((S.w + 1) / 2);
      PTALLOC(S.dw, B * no * 2 * S.d);
      scr_max = std::max(scr_max, B * no * 2 * S.d);
    }
  }
  const int64_t img_elems = B * c.image_h * c.image_w * 3;
  PTALLOC(m->img, img_elems); PTALLOC(m->dimg, img_elems);
  PTALLOC(m->logits, B * m->nc); PTALLOC(m->dlogits, B * m->nc);
  PTALLOC(m->rows, (int64_t)m->chunk * per_image); PTALLOC(m->drows, (int64_t)m->chunk * per_image);
  PTALLOC(m->gw_part, (int64_t)m->Kp * c.dim); PTALLOC(m->gw_slices, (int64_t)CONV_WGRAD_SLICES * m->Kp * c.dim);
  map_max = round_up(map_max, 4);   // pit_backward zeroes ga in 16-byte units
  PTALLOC(m->ga, map_max); PTALLOC(m->gb, map_max); PTALLOC(m->scr, scr_max);
  const int dl = m->st.back().d;
  PTALLOC(m->yh, B * dl); PTALLOC(m->dyh, B * dl); PTALLOC(m->mean_h, B); PTALLOC(m->rstd_h, B);
  PTALLOC(m->ws, std::max<int64_t>({layernorm_bwd_ws_elems(dmax), colsum_ws_elems(std::max(dmax, m->nc)), pit_rowsum_ws_elems(dmax)}) + 64);
  PTALLOC(m->pool_ws, pit_pool_ws_elems(dmax));
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

int push_params(vitx_pit* m, std::string& err) {
  int rc;
  for (PitStage& S : m->st) {
    if (!S.eng) continue;
    if ((rc = copy_maps(m->params, S.eng->params, S.maps, true, m->stream, err)) != VITX_OK) return rc;
    S.eng->params_dirty = true;
  }
  return VITX_OK;
}

// Dense products on rows that lie `ld` floats apart (the class rows of a token buffer)
void dense_fwd_ld(const float* X, int64_t ldx, const float* W, const float* bias, float* Y, int64_t ldy, int M, int N, int K, hipStream_t s, int x3) {
  GenericGemmArgs g;
  g.A = X; g.B = W; g.M = M; g.N = N; g.K = K; g.sam = ldx; g.sak = 1; g.sbk = N; g.sbn = 1; g.x3 = x3;
  EpiParams ep;
  ep.out = Y; ep.ldo = ldy; ep.M = M; ep.N = N; ep.bias = bias; ep.vec_ok = (N % 4 == 0) && (ldy % 4 == 0) && aligned16({Y, bias});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}
void dense_dx_ld(const float* dY, int64_t lddy, const float* W, float* dX, int64_t lddx, int M, int N, int K, hipStream_t s, int x3) {
  GenericGemmArgs g;
  g.A = dY; g.B = W; g.M = M; g.N = K; g.K = N; g.sam = lddy; g.sak = 1; g.sbk = 1; g.sbn = N; g.x3 = x3;
  EpiParams ep;
  ep.out = dX; ep.ldo = lddx; ep.M = M; ep.N = K; ep.vec_ok = (K % 4 == 0) && (lddx % 4 == 0) && aligned16({dX});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}
void dense_dw_ld(const float* X, int64_t ldx, const float* dY, int64_t lddy, float* dW, int M, int N, int K, hipStream_t s, int x3) {
  GenericGemmArgs g;
  g.A = X; g.B = dY; g.M = K; g.N = N; g.K = M; g.sam = 1; g.sak = ldx; g.sbk = lddy; g.sbn = 1; g.x3 = x3;
  EpiParams ep;
  ep.out = dW; ep.ldo = N; ep.M = K; ep.N = N; ep.vec_ok = (N % 4 == 0) && aligned16({dW});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}

// Pool(d) of stage si (pit.py:146-156) on x [b, 1 + h w, d] -> out [b, 1 + oh ow, 2 d]; the depthwise output stays in S.dw for the VJP
void pool_forward(vitx_pit* m, size_t si, const float* x, float* out, int b, int h, int w) {
  PitStage& S = m->st[si];
  const float* P = m->params;
  hipStream_t s = m->stream;
  const int d = S.d, C2 = 2 * d, n = 1 + h * w, no = 1 + ((h + 1) / 2) * ((w + 1) / 2);
  CompositeProf pr(m->prof_eng, "pit_pool_fwd");
  launch_pit_pool_dw_fwd(x, P + S.dw_k, P + S.dw_b, S.dw, b, h, w, d, s);                                  // :130
  dense_fwd(S.dw, C2, P + S.pw_k, P + S.pw_b, out, b * no, C2, C2, s, m->x3);                             // :131 (row 0: overwritten below)
  dense_fwd_ld(x, (int64_t)n * d, P + S.cls_k, P + S.cls_b, out, (int64_t)no * C2, b, C2, d, s, m->x3);   // :148
}

// its VJP: dout [b, 1 + oh ow, 2 d] -> the pool's entries of the gradient arena and, when asked for, dx [b, 1 + h w, d] (every element written)
void pool_backward(vitx_pit* m, size_t si, const float* x, const float* dout, float* dx, int b, int h, int w) {
  PitStage& S = m->st[si];
  const float* P = m->params;
  float* G = m->grads;
  hipStream_t s = m->stream;
  const int d = S.d, C2 = 2 * d, n = 1 + h * w, no = 1 + ((h + 1) / 2) * ((w + 1) / 2);
  CompositeProf pr(m->prof_eng, "pit_pool_bwd");
  dense_dw(S.dw, C2, dout, G + S.pw_k, b * no, C2, C2, s, m->x3);   // (row 0 of S.dw is zero)
  launch_pit_rowsum(dout, m->ws, G + S.pw_b, b, no, C2, s);
  dense_dx(dout, P + S.pw_k, m->scr, b * no, C2, C2, s, m->x3);     // d(depthwise output); its row 0 is never read
  launch_pit_pool_dw_bwd_params(x, m->scr, m->pool_ws, G + S.dw_k, G + S.dw_b, b, h, w, d, s);
  dense_dw_ld(x, (int64_t)n * d, dout, (int64_t)no * C2, G + S.cls_k, b, C2, d, s, m->x3);
  launch_colsum(dout, 0, (int64_t)no * C2, b, C2, m->ws, G + S.cls_b, s);
  if (!dx) return;
  launch_pit_pool_dw_bwd_dx(m->scr, P + S.dw_k, dx, b, h, w, d, s);
  dense_dx_ld(dout, (int64_t)no * C2, P + S.cls_k, dx, (int64_t)n * d, b, C2, d, s, m->x3);
}

int pit_forward(vitx_pit* m, const float* img_dev, int b, std::string& err) {
  const vitx_pit_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  PitStage& S0 = m->st[0];
  const int n = S0.n, d = S0.d;
  const int64_t in_img = (int64_t)c.image_h * c.image_w * 3;
  for (int b0 = 0; b0 < b; b0 += m->chunk) {   // Unfold + Dense (pit.py:179-182) in image chunks
    const int nb = std::min(m->chunk, b - b0);
    { CompositeProf pr(m->prof_eng, "pit_unfold"); launch_pit_unfold(img_dev + b0 * in_img, m->rows, nb, c.image_h, c.image_w, 3, m->p, m->stride, m->oh, m->ow, m->Kp, s); }
    CompositeProf pr(m->prof_eng, "pit_embed");
    dense_fwd(m->rows, m->Kp, P + m->emb_w, P + m->emb_b, S0.in + (int64_t)b0 * n * d, nb * n, d, m->K, s, m->x3);
  }
  { CompositeProf pr(m->prof_eng, "pit_embed"); launch_pit_cls_pos(S0.in, P + m->cls, P + m->pos, b, n, d, s); }   // :211-213
  int rc;
  for (size_t i = 0; i < m->st.size(); ++i) {
    PitStage& S = m->st[i];
    if (S.eng) {
      S.eng->stream = s;
      if ((rc = engine_transformer_forward(S.eng, S.in, b, S.n, 0, 0, S.out, err)) != VITX_OK) return rc;   // :196
    }
    if (S.pool) pool_forward(m, i, S.out, m->st[i + 1].in, b, S.h, S.w);                                    // :199
  }
  // LayerNormalization + Dense on row 0 (:202-205,217)
  const PitStage& last = m->st.back();
  CompositeProf pr(m->prof_eng, "pit_head");
  launch_layernorm_fwd(last.out, (int64_t)last.n * last.d, P + m->hn_g, P + m->hn_b, m->yh, 0, last.d, m->mean_h, m->rstd_h, b, last.d, c.ln_eps, s);
  dense_fwd(m->yh, last.d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, last.d, s, m->x3);
  m->have_fwd = true;
  m->pool_stage = -1;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and, when dimg_dev is given, d(img)
int pit_backward(vitx_pit* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  const vitx_pit_config& c = m->cfg;
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b;
  launch_fill_zero(G, m->n_arena * 4, s);
  float *g = m->ga, *g2 = m->gb;   // g holds d(stage output)
  {
    const PitStage& last = m->st.back();
    const int d = last.d;
    CompositeProf pr(m->prof_eng, "pit_head");
    dense_dw(m->yh, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s, m->x3);
    launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
    dense_dx(dlogits_dev, P + m->fc_w, m->dyh, b, m->nc, d, s, m->x3);
    launch_fill_zero(g, round_up((int64_t)b * last.n * d, 4) * 4, s);   // only row 0 reaches the logits (ga holds round_up(map_max, 4) floats)
    launch_layernorm_bwd(m->dyh, 0, d, last.out, (int64_t)last.n * d, m->mean_h, m->rstd_h, P + m->hn_g, nullptr, 0, g, (int64_t)last.n * d, nullptr, 0, m->ws,
                         G + m->hn_g, G + m->hn_b, nullptr, b, d, s);
  }
  int rc;
  for (int i = (int)m->st.size() - 1; i >= 0; --i) {
    PitStage& S = m->st[(size_t)i];
    if (S.eng) {
      S.eng->stream = s;
      if ((rc = engine_transformer_backward(S.eng, g, g, err)) != VITX_OK) return rc;
      if ((rc = copy_maps(m->grads, S.eng->grads, S.maps, false, s, err)) != VITX_OK) return rc;
    }
    if (i > 0 && m->st[(size_t)i - 1].pool) {
      const PitStage& Q = m->st[(size_t)i - 1];
      pool_backward(m, (size_t)i - 1, Q.out, g, g2, b, Q.h, Q.w);
      std::swap(g, g2);
    }
  }
  // g = d(tokens) [b, n, dim]
  const PitStage& S0 = m->st[0];
  const int n = S0.n, d = S0.d;
  {
    CompositeProf pr(m->prof_eng, "pit_embed");
    launch_pit_pos_grad(g, G + m->pos, G + m->cls, b, n, m->pos_rows, d, s);
    launch_pit_rowsum(g, m->ws, G + m->emb_b, b, n, d, s);
  }
  const int64_t in_img = (int64_t)c.image_h * c.image_w * 3;
  for (int b0 = 0; b0 < b; b0 += m->chunk) {
    const int nb = std::min(m->chunk, b - b0);
    const int rows = nb * n;
    const float* dy = g + (int64_t)b0 * n * d;
    { CompositeProf pr(m->prof_eng, "pit_unfold"); launch_pit_unfold(m->img + b0 * in_img, m->rows, nb, c.image_h, c.image_w, 3, m->p, m->stride, m->oh, m->ow, m->Kp, s); }
    {
      CompositeProf pr(m->prof_eng, "pit_embed");
      conv_wgrad(m->rows, m->Kp, dy, m->gw_part, m->gw_slices, rows, d, m->x3, s);   // (the class rows of m->rows are zero)
      const int64_t nw = (int64_t)m->K * d;
      hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + m->emb_w, (const float*)m->gw_part, nw, b0 == 0 ? 1 : 0);
      if (dimg_dev) dense_dx(dy, P + m->emb_w, m->drows, rows, d, m->K, s, m->x3);
    }
    if (!dimg_dev) continue;
    CompositeProf pr(m->prof_eng, "pit_unfold");
    launch_pit_unfold_bwd(m->drows, dimg_dev + b0 * in_img, nb, c.image_h, c.image_w, 3, m->p, m->stride, m->oh, m->ow, m->K, s);
  }
  return VITX_OK;
}

std::vector<vitx_engine*> pit_engines(vitx_pit* m) {
  std::vector<vitx_engine*> v;
  for (PitStage& S : m->st) if (S.eng) v.push_back(S.eng);
  return v;
}

int isqrt_exact(int v) {
  const int r = (int)std::lround(std::sqrt((double)v));
  return r * r == v ? r : -1;
}

}  // namespace

extern "C" {

int32_t vitx_pit_param_table_size(const vitx_pit_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, pit_param_table);
}
int32_t vitx_pit_param_table_entry(const vitx_pit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, pit_param_table);
}
int32_t vitx_pit_create(const vitx_pit_config* cfg, vitx_pit_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, pit_create);
}
int32_t vitx_pit_destroy(vitx_pit_handle m) {
  CAPI_TRY
  pit_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_pit, "blob size does not match the PiT parameter table")
int32_t vitx_pit_set_long_attn(vitx_pit_handle m, int32_t on) {
  CAPI_TRY
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  const std::vector<vitx_engine*> engs = pit_engines(m);
  std::vector<bool> was;
  for (vitx_engine* e : engs) was.push_back(e->long_attn);
  for (size_t i = 0; i < engs.size(); ++i) {
    const int rc = vitx_set_long_attn(engs[i], on);
    if (rc == VITX_OK) continue;
    for (size_t j = 0; j < i; ++j) engs[j]->long_attn = was[j];   // a refusal leaves every stage as it was
    return rc;                                                    // (the engine's refusal is the last-error text)
  }
  m->cfg.long_attn = on != 0;
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_pit_forward_dev(vitx_pit_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  // (the embedding's weight gradient re-reads the image: the handle keeps its own copy)
  CAPI_HIP(hipMemcpyAsync(m->img, img_dev, (size_t)b * m->cfg.image_h * m->cfg.image_w * 3 * 4, hipMemcpyDeviceToDevice, m->stream));
  std::string err;
  int rc = pit_forward(m, m->img, b, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_pit_forward(vitx_pit_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.image_h * m->cfg.image_w * 3, b, logits_host,
                                [&](std::string& err) { return pit_forward(m, m->img, b, err); });
}
int32_t vitx_pit_backward_dev(vitx_pit_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = pit_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_pit_backward(vitx_pit_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.image_h * m->cfg.image_w * 3,
                                 [&](float* dimg_dev, std::string& err) { return pit_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_pit_pool_forward(vitx_pit_handle m, int32_t stage, const float* tokens_host, int32_t b, int32_t n, float* out_host) {
  CAPI_TRY
  if (!m || !tokens_host || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (stage < 0 || stage >= (int)m->st.size() || !m->st[(size_t)stage].pool) return capi_fail(VITX_ERR_INVALID, "pool_forward: no Pool follows that stage");
  PitStage& S = m->st[(size_t)stage];
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  const int hw = n > 1 ? isqrt_exact(n - 1) : -1;
  if (hw < 1 || n > S.n) return capi_fail(VITX_ERR_INVALID, "pool_forward: n must be 1 + h * h, at most the stage's own token count");
  m->have_fwd = false; m->pool_stage = -1;   // the stage buffers no longer describe a model forward
  const int no = 1 + ((hw + 1) / 2) * ((hw + 1) / 2);
  float* out = m->st[(size_t)stage + 1].in;
  CAPI_HIP(hipMemcpyAsync(S.out, tokens_host, (size_t)b * n * S.d * 4, hipMemcpyHostToDevice, m->stream));
  pool_forward(m, (size_t)stage, S.out, out, b, hw, hw);
  CAPI_HIP(hipMemcpyAsync(out_host, out, (size_t)b * no * 2 * S.d * 4, hipMemcpyDeviceToHost, m->stream));
  CAPI_HIP(hipStreamSynchronize(m->stream));
  m->pool_stage = stage; m->pool_b = b; m->pool_hw = hw;
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_pit_pool_backward(vitx_pit_handle m, int32_t stage, const float* dout_host, float* dtokens_host_or_null) {
  CAPI_TRY
  if (!m || !dout_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (stage < 0 || stage != m->pool_stage) return capi_fail(VITX_ERR_STATE, "pool_backward requires a preceding pool_forward of the same stage");
  PitStage& S = m->st[(size_t)stage];
  const int b = m->pool_b, hw = m->pool_hw, n = 1 + hw * hw, no = 1 + ((hw + 1) / 2) * ((hw + 1) / 2);
  CAPI_HIP(hipMemcpyAsync(m->ga, dout_host, (size_t)b * no * 2 * S.d * 4, hipMemcpyHostToDevice, m->stream));
  pool_backward(m, (size_t)stage, S.out, m->ga, dtokens_host_or_null ? m->gb : nullptr, b, hw, hw);
  if (dtokens_host_or_null) CAPI_HIP(hipMemcpyAsync(dtokens_host_or_null, m->gb, (size_t)b * n * S.d * 4, hipMemcpyDeviceToHost, m->stream));
  CAPI_HIP(hipStreamSynchronize(m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_pit_profile_begin(vitx_pit_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin(pit_engines(m));
}
int32_t vitx_pit_profile_end(vitx_pit_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end(pit_engines(m), out, cap, n_out);
}
int32_t vitx_pit_read(vitx_pit_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const int64_t b = m->b;
  auto stage_of = [&](const std::string& prefix) -> int {   // "<prefix><s>" with a one-digit s; -1 otherwise
    if (w.size() != prefix.size() + 1 || w.compare(0, prefix.size(), prefix) != 0) return -1;
    const int v = w.back() - '0';
    return v >= 0 && v < (int)m->st.size() ? v : -1;
  };
  const float* src = nullptr;
  int64_t n = 0;
  int i;
  if (w == "tokens") { const PitStage& S = m->st[0]; src = S.in; n = b * S.n * S.d; }
  else if ((i = stage_of("stage.")) >= 0) { const PitStage& S = m->st[(size_t)i]; src = S.out; n = b * S.n * S.d; }
  else if ((i = stage_of("pooled.")) >= 0 && m->st[(size_t)i].pool) { const PitStage& S = m->st[(size_t)i + 1]; src = S.in; n = b * S.n * S.d; }
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
