// CCT (cct.py:307-345): Tokenizer (n_conv_layers x [Conv2D 'SAME' without bias, ReLU, MaxPool2D 'SAME'], :176-215), optional positional embedding,
// num_layers TransformerEncoderLayers (:139-174), LayerNorm, sequence pooling (:293-299) and fc.  The blocks run on one ViT engine whose
// vitx_config.cct_block is set (the MLP residual leaves from the normalised stream, engine.hip); around it the composite runs the tokenizer --
// each convolution as im2col rows (cct_tok.hip) times the HWIO kernel viewed as [k*k*Cin, Cout], in image chunks so that the row
// workspace is bounded, then the fused ReLU + max-pool of cct_tok.hip -- the positional add, the final norm, the sequence-pooling kernels below and fc.
// Everything outside the engine keeps fp32 storage; in the bf16 / bf16x3 modes its large GEMMs take the split-operand (hi + lo bf16) MFMA path.
// The composite owns the public parameter / gradient arenas in its own table order and copies them to / from the engine.
// Only the deterministic path exists: attention dropout and stochastic depth (training=True in the reference) are not built.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "composite.h"
#include "conv_same.h"

namespace {

// ------------------------------------------------------------------------------------------------ sequence pooling (cct.py:293-299)
// One workgroup of 256 threads per image; the token logits / weights stay in LDS ([n] floats, twice in the backward).
constexpr int SP_THREADS = 256, SP_WAVES = SP_THREADS / 64, SP_N_MAX = 6144;

__device__ __forceinline__ float sp_block_reduce(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < SP_WAVES; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

// p[b, t] = softmax_t(x[b, t] . w + bias);  pooled[b, :] = sum_t p[b, t] x[b, t, :]
__global__ __launch_bounds__(SP_THREADS) void cct_seqpool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                     float* __restrict__ p, float* __restrict__ pooled, int n, int d) {
  extern __shared__ float sp_lds[];
  float* pl = sp_lds;                      // [n]
  float* red = pl + ((n + 3) & ~3);        // [SP_WAVES]
  const int tid = threadIdx.x, wave = tid / 64, lane = tid & 63;
  const float* xi = x + (int64_t)blockIdx.x * n * d;
  const float b0 = bias[0];
  for (int t = wave; t < n; t += SP_WAVES) {
    float a = 0.f;
    for (int c = lane; c < d; c += 64) a += xi[(int64_t)t * d + c] * w[c];
    a = wave_sum(a);
    if (lane == 0) pl[t] = a + b0;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = tid; t < n; t += SP_THREADS) m = fmaxf(m, pl[t]);
  m = sp_block_reduce(m, red, true);
  float s = 0.f;
  for (int t = tid; t < n; t += SP_THREADS) {
    const float e = expf(pl[t] - m);
    pl[t] = e;
    s += e;
  }
  s = sp_block_reduce(s, red, false);
  const float inv = 1.f / s;
  for (int t = tid; t < n; t += SP_THREADS) {
    const float q = pl[t] * inv;
    pl[t] = q;
    p[(int64_t)blockIdx.x * n + t] = q;
  }
  __syncthreads();
  for (int c = tid; c < d; c += SP_THREADS) {
    float r = 0.f;
    for (int t = 0; t < n; ++t) r += pl[t] * xi[(int64_t)t * d + c];
    pooled[(int64_t)blockIdx.x * d + c] = r;
  }
}

// dlogit_t = p_t (x_t . dout - sum_s p_s x_s . dout);  dx_t = p_t dout + dlogit_t w;  per image: dwp[b, :] = sum_t dlogit_t x_t, dbp[b] = sum_t dlogit_t
// (summed over the images in a fixed order by a second launch)
__global__ __launch_bounds__(SP_THREADS) void cct_seqpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ p,
                                                                     const float* __restrict__ dout, float* __restrict__ dx, float* __restrict__ dwp,
                                                                     float* __restrict__ dbp, int n, int d) {
  extern __shared__ float sp_lds[];
  const int n4 = (n + 3) & ~3;
  float* pl = sp_lds;             // [n]
  float* al = pl + n4;            // [n]
  float* red = al + n4;           // [SP_WAVES]
  const int tid = threadIdx.x, wave = tid / 64, lane = tid & 63;
  const float* xi = x + (int64_t)blockIdx.x * n * d;
  const float* doi = dout + (int64_t)blockIdx.x * d;
  for (int t = tid; t < n; t += SP_THREADS) pl[t] = p[(int64_t)blockIdx.x * n + t];
  for (int t = wave; t < n; t += SP_WAVES) {
    float a = 0.f;
    for (int c = lane; c < d; c += 64) a += xi[(int64_t)t * d + c] * doi[c];
    a = wave_sum(a);
    if (lane == 0) al[t] = a;
  }
  __syncthreads();
  float s = 0.f;
  for (int t = tid; t < n; t += SP_THREADS) s += pl[t] * al[t];
  s = sp_block_reduce(s, red, false);
  float sb = 0.f;
  for (int t = tid; t < n; t += SP_THREADS) {
    const float dl = pl[t] * (al[t] - s);
    al[t] = dl;
    sb += dl;
  }
  sb = sp_block_reduce(sb, red, false);   // (its barriers also publish al)
  if (tid == 0) dbp[blockIdx.x] = sb;
  float* dxi = dx + (int64_t)blockIdx.x * n * d;
  for (int64_t e = tid; e < (int64_t)n * d; e += SP_THREADS) {
    const int t = (int)(e / d), c = (int)(e - (int64_t)t * d);
    dxi[e] = pl[t] * doi[c] + al[t] * w[c];
  }
  for (int c = tid; c < d; c += SP_THREADS) {
    float r = 0.f;
    for (int t = 0; t < n; ++t) r += al[t] * xi[(int64_t)t * d + c];
    dwp[(int64_t)blockIdx.x * d + c] = r;
  }
}

size_t seqpool_lds_bytes(int n, bool bwd) { return (size_t)((bwd ? 2 : 1) * round_up(n, 4) + 8) * 4; }

// out[b, t, c] = x[b, t, c] + pos[t, c]
__global__ void cct_add_pos_kernel(const float* __restrict__ x, const float* __restrict__ pos, float* __restrict__ out, int64_t per_image, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) out[e] = x[e] + pos[e % per_image];
}
// one conv layer of the tokenizer and the geometry of its two 'SAME' stages
struct ConvLayer {
  int H = 0, W = 0, Cin = 0, Cout = 0;   // input extent / planes, filters
  int oh = 0, ow = 0;                    // conv output
  int ph = 0, pw = 0;                    // pooled output
  int K = 0, Kp = 0;                     // k * k * Cin, and the row stride of the im2col operand: K rounded up to 64
  int chunk = 1;                         // images per im2col + GEMM pass
  int64_t w = -1;                        // arena offset of the kernel [k, k, Cin, Cout]
  float *conv = nullptr, *pooled = nullptr;   // [B, oh, ow, Cout] pre-activation (kept for the VJP), [B, ph, pw, Cout]
};


}  // namespace

struct vitx_cct {
  vitx_cct_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  vitx_engine* eng = nullptr;
  std::vector<ArenaMap> maps;   // the block tensors -> the engine's
  std::vector<ConvLayer> conv;
  int64_t pool_w = -1, pool_b = -1, pos = -1, norm_g = -1, norm_b = -1, fc_w = -1, fc_b = -1;
  int n = 0, d = 0, nc = 0, B = 0, x3 = 0;
  hipStream_t stream = nullptr;
  DevicePool pool;
  float *img = nullptr, *dimg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *rows = nullptr, *drows = nullptr, *gw_part = nullptr, *gw_slices = nullptr, *dconv = nullptr, *dact[2] = {nullptr, nullptr};
  float *sine = nullptr, *tok_in = nullptr, *enc = nullptr, *xn = nullptr, *mean = nullptr, *rstd = nullptr, *p = nullptr, *pooled = nullptr;
  float *dpooled = nullptr, *dxn = nullptr, *denc = nullptr, *dtok = nullptr, *dwp = nullptr, *dbp = nullptr, *ws = nullptr;
  bool have_fwd = false;
  int b = 0;
};

namespace {

// conv layers with their 'SAME' geometry (cct.py:190-200); "" or what is wrong with the configuration
std::string cct_geometry(const vitx_cct_config& c, std::vector<ConvLayer>& out) {
  out.clear();
  if (c.img_height <= 0 || c.img_width <= 0 || c.n_input_channels <= 0 || c.embedding_dim <= 0 || c.n_conv_layers <= 0 || c.kernel_size <= 0 ||
      c.stride <= 0 || c.pooling_kernel_size <= 0 || c.pooling_stride <= 0 || c.num_layers < 0 || c.num_heads <= 0 || c.dim_feedforward <= 0 ||
      c.num_classes <= 0)
    return "invalid CCT configuration";
  if (c.n_conv_layers > 16) return "n_conv_layers must be <= 16";
  if (c.positional_embedding < VITX_CCT_POS_LEARNABLE || c.positional_embedding > VITX_CCT_POS_NONE) return "unknown positional_embedding";
  if (c.embedding_dim % c.num_heads) return "embedding_dim must be divisible by num_heads (cct.py:110,127)";
  const int planes = c.in_planes > 0 ? c.in_planes : 64;
  int H = c.img_height, W = c.img_width, C = c.n_input_channels;
  for (int i = 0; i < c.n_conv_layers; ++i) {
    ConvLayer L;
    L.H = H; L.W = W; L.Cin = C; L.Cout = i == c.n_conv_layers - 1 ? c.embedding_dim : planes;
    int pt, pl;
    extract_patches_geometry(H, W, c.kernel_size, c.stride, &L.oh, &L.ow, &pt, &pl);
    extract_patches_geometry(L.oh, L.ow, c.pooling_kernel_size, c.pooling_stride, &L.ph, &L.pw, &pt, &pl);
    if ((int64_t)c.kernel_size * c.kernel_size * C > (1 << 24)) return "kernel_size * kernel_size * planes too large";
    L.K = c.kernel_size * c.kernel_size * C;
    L.Kp = (int)round_up(L.K, 64);
    out.push_back(L);
    H = L.ph; W = L.pw; C = L.Cout;
  }
  if ((int64_t)H * W > SP_N_MAX) return "sequence pooling holds at most " + std::to_string(SP_N_MAX) + " tokens per image";
  return "";
}

}  // namespace

// Table of CCT's variables in the documented order: the reference's attribute order
std::string cct_param_table(const vitx_cct_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena, vitx_cct* m = nullptr) {
  out.clear();
  std::vector<ConvLayer> conv;
  const std::string e = cct_geometry(c, conv);
  if (!e.empty()) return e;
  TableBuilder tb{out};
  const int64_t d = c.embedding_dim, ff = c.dim_feedforward, k = c.kernel_size;
  const int64_t n = (int64_t)conv.back().ph * conv.back().pw;
  for (size_t i = 0; i < conv.size(); ++i)
    conv[i].w = tb.add("tokenizer.conv_layers." + std::to_string(i) + ".kernel", {k, k, conv[i].Cin, conv[i].Cout});
  const int64_t pw = tb.add("classifier.attention_pool.kernel", {d, 1}), pb = tb.add("classifier.attention_pool.bias", {1});
  const int64_t pos = c.positional_embedding == VITX_CCT_POS_LEARNABLE ? tb.add("classifier.positional_emb", {1, n, d}) : -1;
  for (int l = 0; l < c.num_layers; ++l) {
    const std::string p = "classifier.blocks." + std::to_string(l) + ".";
    tb.add(p + "pre_norm.gamma", {d}); tb.add(p + "pre_norm.beta", {d});
    tb.add(p + "self_attn.to_qkv.kernel", {d, 3 * d});
    tb.add(p + "self_attn.proj.kernel", {d, d}); tb.add(p + "self_attn.proj.bias", {d});
    tb.add(p + "linear1.kernel", {d, ff}); tb.add(p + "linear1.bias", {ff});
    tb.add(p + "norm1.gamma", {d}); tb.add(p + "norm1.beta", {d});
    tb.add(p + "linear2.kernel", {ff, d}); tb.add(p + "linear2.bias", {d});
  }
  const int64_t ng = tb.add("classifier.norm.gamma", {d}), nb = tb.add("classifier.norm.beta", {d});
  const int64_t fw = tb.add("classifier.fc.kernel", {d, c.num_classes}), fb = tb.add("classifier.fc.bias", {c.num_classes});
  if (m) {
    m->conv = conv;
    m->pool_w = pw; m->pool_b = pb; m->pos = pos; m->norm_g = ng; m->norm_b = nb; m->fc_w = fw; m->fc_b = fb;
    m->n = (int)n; m->d = (int)d; m->nc = c.num_classes;
  }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

vitx_config cct_engine_config(const vitx_cct_config& c, int n) {
  vitx_config ec{};
  ec.variant = VITX_VARIANT_VIT;
  ec.image_h = 1; ec.image_w = n; ec.patch_h = ec.patch_w = 1; ec.channels = 1;   // token rows only: the engine's own embedding / head are never run
  ec.num_classes = 1; ec.dim = c.embedding_dim; ec.depth = c.num_layers; ec.heads = c.num_heads; ec.dim_head = c.embedding_dim / c.num_heads;
  ec.mlp_dim = c.dim_feedforward; ec.pool = VITX_POOL_CLS; ec.ln_eps = c.ln_eps;
  ec.compute = c.compute; ec.max_batch = c.max_batch; ec.device_id = c.device_id;
  ec.cct_block = 1;
  return ec;
}

// everything a configuration can be refused for without a device
int cct_check(const vitx_cct_config& c, std::string& err) {
  std::vector<ParamDesc> t;
  vitx_cct probe;
  const std::string e = cct_param_table(c, t, nullptr, nullptr, &probe);
  if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  if (c.num_layers < 1) { err = "num_layers must be >= 1"; return VITX_ERR_UNSUPPORTED; }
  if (c.compute == VITX_COMPUTE_BF16 && (c.embedding_dim % 64 || c.dim_feedforward % 64)) {
    err = "BF16 compute needs embedding_dim and int(embedding_dim * mlp_ratio) to be multiples of 64 (use FP32_PARITY otherwise)";
    return VITX_ERR_UNSUPPORTED;
  }
  std::vector<ParamDesc> et;
  const std::string ee = build_param_table(cct_engine_config(c, probe.n), et);
  if (!ee.empty()) { err = ee; return VITX_ERR_INVALID; }
  return VITX_OK;
}

#define CALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, fail(rc_))

void cct_destroy(vitx_cct* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  if (m->eng) engine_destroy(m->eng);
  delete m;
}

int cct_create(const vitx_cct_config& cin, vitx_cct** out, std::string& err) {
  vitx_cct_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-3f;   // Keras LayerNormalization default
  int rc = cct_check(c, err);
  if (rc != VITX_OK) return rc;
  vitx_cct* m = new vitx_cct();
  m->cfg = c;
  auto fail = [&](int code) { cct_destroy(m); return code; };
  cct_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->B = c.max_batch;
  m->x3 = c.compute == VITX_COMPUTE_FP32_PARITY ? 0 : 1;
  if ((rc = engine_create(cct_engine_config(c, m->n), &m->eng, err)) != VITX_OK) return fail(rc);
  m->stream = m->eng->stream;
  // parameter maps: every block tensor is one contiguous run
  static const char* PAIRS[][2] = {{"pre_norm.gamma", "attn.norm.gamma"}, {"pre_norm.beta", "attn.norm.beta"}, {"self_attn.to_qkv.kernel", "attn.to_qkv.kernel"},
                                   {"self_attn.proj.kernel", "attn.to_out.kernel"}, {"self_attn.proj.bias", "attn.to_out.bias"},
                                   {"linear1.kernel", "mlp.fc1.kernel"}, {"linear1.bias", "mlp.fc1.bias"}, {"norm1.gamma", "mlp.norm.gamma"},
                                   {"norm1.beta", "mlp.norm.beta"}, {"linear2.kernel", "mlp.fc2.kernel"}, {"linear2.bias", "mlp.fc2.bias"}};
  for (int l = 0; l < c.num_layers; ++l)
    for (const auto& pr : PAIRS)
      if ((rc = add_arena_map(m->maps, m->table, "classifier.blocks." + std::to_string(l) + "." + pr[0], m->eng->table,
                              "transformer." + std::to_string(l) + "." + pr[1], err)) != VITX_OK) return fail(rc);
  // buffers
  const int64_t B = m->B, n = m->n, d = m->d;
  CALLOC(m->params, m->n_arena);
  CALLOC(m->grads, m->n_arena);
  int64_t rows_max = 0, gw_max = 0, conv_max = 0, act_max = 0;
  for (size_t i = 0; i < m->conv.size(); ++i) {
    ConvLayer& L = m->conv[i];
    const int64_t per_image = (int64_t)L.oh * L.ow * L.Kp;
    L.chunk = (int)std::min<int64_t>(B, c.conv_chunk > 0 ? c.conv_chunk : std::max<int64_t>(1, IM2COL_BUDGET / per_image));
    rows_max = std::max(rows_max, (int64_t)L.chunk * per_image);
    gw_max = std::max(gw_max, (int64_t)L.Kp * L.Cout);
    conv_max = std::max(conv_max, B * L.oh * L.ow * L.Cout);
    if (i > 0) act_max = std::max(act_max, B * L.H * L.W * L.Cin);   // gradients of the pooled outputs between conv layers
    CALLOC(L.conv, B * L.oh * L.ow * L.Cout);
    CALLOC(L.pooled, B * L.ph * L.pw * L.Cout);
  }
  CALLOC(m->rows, rows_max); CALLOC(m->drows, rows_max); CALLOC(m->gw_part, gw_max); CALLOC(m->gw_slices, CONV_WGRAD_SLICES * gw_max); CALLOC(m->dconv, conv_max);
  CALLOC(m->dact[0], act_max); CALLOC(m->dact[1], act_max);
  const int64_t img_elems = B * c.img_height * c.img_width * c.n_input_channels;
  CALLOC(m->img, img_elems); CALLOC(m->dimg, img_elems);
  CALLOC(m->logits, B * m->nc); CALLOC(m->dlogits, B * m->nc);
  const int64_t rows = B * n;
  CALLOC(m->tok_in, rows * d); CALLOC(m->enc, rows * d); CALLOC(m->xn, rows * d); CALLOC(m->mean, rows); CALLOC(m->rstd, rows);
  CALLOC(m->p, rows); CALLOC(m->pooled, B * d); CALLOC(m->dpooled, B * d); CALLOC(m->dxn, rows * d); CALLOC(m->denc, rows * d);
  CALLOC(m->dtok, rows * d); CALLOC(m->dwp, B * d); CALLOC(m->dbp, B);
  CALLOC(m->ws, std::max<int64_t>(layernorm_bwd_ws_elems((int)d), colsum_ws_elems((int)std::max<int64_t>(d, m->nc))) + 64);
  if (c.positional_embedding == VITX_CCT_POS_SINE) {
    // cct.py:269-275 as evidently meant (the reference assigns into a tensor there and raises): p / 10000^(2 (i // 2) / dim), sin on even, cos on odd columns
    std::vector<float> pe((size_t)(n * d));
    for (int64_t p = 0; p < n; ++p)
      for (int64_t i = 0; i < d; ++i) {
        const double a = (double)p / std::pow(10000.0, 2.0 * (double)(i / 2) / (double)d);
        pe[(size_t)(p * d + i)] = (float)(i % 2 == 0 ? std::sin(a) : std::cos(a));
      }
    CALLOC(m->sine, n * d);
    if (hipMemcpyAsync(m->sine, pe.data(), pe.size() * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess) { err = "copying the sine table failed"; return fail(VITX_ERR_HIP); }
  }
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

int push_params(vitx_cct* m, std::string& err) {
  const int rc = copy_maps(m->params, m->eng->params, m->maps, true, m->stream, err);
  if (rc == VITX_OK) m->eng->params_dirty = true;
  return rc;
}

int cct_forward(vitx_cct* m, const float* img_dev, int b, std::string& err) {
  const vitx_cct_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  m->eng->stream = m->stream;
  hipStream_t s = m->stream;
  const float* P = m->params;
  m->b = b;
  const int n = m->n, d = m->d;
  // Tokenizer (cct.py:211-215): per layer, im2col + GEMM in image chunks, then ReLU + max-pool over the whole batch
  const float* x = img_dev;
  for (ConvLayer& L : m->conv) {
    const int64_t in_img = (int64_t)L.H * L.W * L.Cin, out_img = (int64_t)L.oh * L.ow * L.Cout;
    for (int b0 = 0; b0 < b; b0 += L.chunk) {
      const int nb = std::min(L.chunk, b - b0);
      { CompositeProf pr(m->eng, "cct_im2col"); launch_cct_im2col(x + b0 * in_img, m->rows, nb, L.H, L.W, L.Cin, c.kernel_size, c.stride, L.Kp, s); }
      CompositeProf pr(m->eng, "cct_conv_gemm");
      dense_fwd(m->rows, L.Kp, P + L.w, nullptr, L.conv + b0 * out_img, nb * L.oh * L.ow, L.Cout, L.K, s, m->x3);
    }
    CompositeProf pr(m->eng, "cct_relu_maxpool_fwd");
    launch_cct_relu_maxpool_fwd(L.conv, L.pooled, b, L.oh, L.ow, L.Cout, c.pooling_kernel_size, c.pooling_stride, s);
    x = L.pooled;
  }
  // TransformerClassifier.call (cct.py:277-305), seq_pool = True
  const float* tok = x;   // [b, n, d]: the flattened pooled output of the last layer
  const float* pos = c.positional_embedding == VITX_CCT_POS_LEARNABLE ? P + m->pos : c.positional_embedding == VITX_CCT_POS_SINE ? m->sine : nullptr;
  if (pos) {
    const int64_t total = (int64_t)b * n * d;
    hipLaunchKernelGGL(cct_add_pos_kernel, dim3(grid256(total)), dim3(256), 0, s, tok, pos, m->tok_in, (int64_t)n * d, total);   // :285-286
    tok = m->tok_in;
  }
  int rc;
  if ((rc = engine_transformer_forward(m->eng, tok, b, n, 0, 0, m->enc, err)) != VITX_OK) return rc;                               // :290
  launch_layernorm_fwd(m->enc, d, P + m->norm_g, P + m->norm_b, m->xn, 0, d, m->mean, m->rstd, b * n, d, c.ln_eps, s);               // :291
  {
    CompositeProf pr(m->eng, "cct_seqpool_fwd");
    hipLaunchKernelGGL(cct_seqpool_fwd_kernel, dim3((unsigned)b), dim3(SP_THREADS), seqpool_lds_bytes(n, false), s, m->xn, P + m->pool_w, P + m->pool_b,
                       m->p, m->pooled, n, d);                                                                                       // :293-299
  }
  dense_fwd(m->pooled, d, P + m->fc_w, P + m->fc_b, m->logits, b, m->nc, d, s);                                                    // :303
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and, when dimg_dev is given, d(img)
int cct_backward(vitx_cct* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  const vitx_cct_config& c = m->cfg;
  m->eng->stream = m->stream;
  hipStream_t s = m->stream;
  const float* P = m->params;
  float* G = m->grads;
  const int b = m->b, n = m->n, d = m->d;
  launch_fill_zero(G, m->n_arena * 4, s);
  // fc
  dense_dw(m->pooled, d, dlogits_dev, G + m->fc_w, b, m->nc, d, s);
  launch_colsum(dlogits_dev, 0, m->nc, b, m->nc, m->ws, G + m->fc_b, s);
  dense_dx(dlogits_dev, P + m->fc_w, m->dpooled, b, m->nc, d, s);
  // sequence pooling: per-image partials, then a fixed-order sum over the images
  {
    CompositeProf pr(m->eng, "cct_seqpool_bwd");
    hipLaunchKernelGGL(cct_seqpool_bwd_kernel, dim3((unsigned)b), dim3(SP_THREADS), seqpool_lds_bytes(n, true), s, m->xn, P + m->pool_w, m->p, m->dpooled,
                       m->dxn, m->dwp, m->dbp, n, d);
    launch_sum_rows(m->dwp, b, d, G + m->pool_w, s);
    launch_sum_rows(m->dbp, b, 1, G + m->pool_b, s);
  }
  // final norm
  launch_layernorm_bwd(m->dxn, 0, d, m->enc, d, m->mean, m->rstd, P + m->norm_g, nullptr, 0, m->denc, d, nullptr, 0, m->ws, G + m->norm_g, G + m->norm_b,
                       nullptr, b * n, d, s);
  // blocks
  int rc;
  if ((rc = engine_transformer_backward(m->eng, m->denc, m->dtok, err)) != VITX_OK) return rc;
  if ((rc = copy_maps(m->grads, m->eng->grads, m->maps, false, m->stream, err)) != VITX_OK) return rc;
  if (c.positional_embedding == VITX_CCT_POS_LEARNABLE) launch_batch_reduce(m->dtok, b, n, d, 0, n, G + m->pos, s);
  // tokenizer, last layer first
  const float* dpool = m->dtok;
  for (int i = (int)m->conv.size() - 1; i >= 0; --i) {
    ConvLayer& L = m->conv[(size_t)i];
    const int64_t in_img = (int64_t)L.H * L.W * L.Cin, out_img = (int64_t)L.oh * L.ow * L.Cout;
    const float* xin = i == 0 ? (const float*)m->img : m->conv[(size_t)i - 1].pooled;
    float* dxin = i == 0 ? dimg_dev : m->dact[i & 1];
    {
      CompositeProf pr(m->eng, "cct_relu_maxpool_bwd");
      launch_cct_relu_maxpool_bwd(L.conv, dpool, m->dconv, b, L.oh, L.ow, L.Cout, c.pooling_kernel_size, c.pooling_stride, s);
    }
    for (int b0 = 0; b0 < b; b0 += L.chunk) {
      const int nb = std::min(L.chunk, b - b0);
      const int rows = nb * L.oh * L.ow;
      const float* dy = m->dconv + b0 * out_img;
      { CompositeProf pr(m->eng, "cct_im2col"); launch_cct_im2col(xin + b0 * in_img, m->rows, nb, L.H, L.W, L.Cin, c.kernel_size, c.stride, L.Kp, s); }
      {
        CompositeProf pr(m->eng, "cct_conv_gemm");
        conv_wgrad(m->rows, L.Kp, dy, m->gw_part, m->gw_slices, rows, L.Cout, m->x3, s);
        const int64_t nw = (int64_t)L.K * L.Cout;
        hipLaunchKernelGGL(conv_accum_kernel, dim3(grid256(nw)), dim3(256), 0, s, G + L.w, (const float*)m->gw_part, nw, b0 == 0 ? 1 : 0);
        if (dxin) dense_dx(dy, P + L.w, m->drows, rows, L.Cout, L.K, s, m->x3);
      }
      if (dxin) {
        CompositeProf pr(m->eng, "cct_col2im");
        launch_extract_patches_bwd(m->drows, dxin + b0 * in_img, nb, L.H, L.W, L.Cin, c.kernel_size, c.stride, s);
      }
    }
    dpool = dxin;
  }
  return VITX_OK;
}

}  // namespace

extern "C" {

int32_t vitx_cct_param_table_size(const vitx_cct_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, cct_param_table);
}
int32_t vitx_cct_param_table_entry(const vitx_cct_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, cct_param_table);
}
int32_t vitx_cct_sequence_length(const vitx_cct_config* cfg, int32_t* n_tokens) {
  CAPI_TRY
  if (!cfg || !n_tokens) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::vector<ConvLayer> conv;
  std::string e = cct_geometry(*cfg, conv);
  if (!e.empty()) return capi_fail(VITX_ERR_INVALID, e);
  *n_tokens = conv.back().ph * conv.back().pw;
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_cct_create(const vitx_cct_config* cfg, vitx_cct_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, cct_create);
}
int32_t vitx_cct_destroy(vitx_cct_handle m) {
  CAPI_TRY
  cct_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_cct, "blob size does not match the CCT parameter table")
int32_t vitx_cct_forward_dev(vitx_cct_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  // the tokenizer's VJP re-reads the image: the handle keeps its own copy
  if (img_dev != m->img)
    CAPI_HIP(hipMemcpyAsync(m->img, img_dev, (size_t)b * m->cfg.img_height * m->cfg.img_width * m->cfg.n_input_channels * 4, hipMemcpyDeviceToDevice, m->stream));
  std::string err;
  int rc = cct_forward(m, m->img, b, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_cct_forward(vitx_cct_handle m, const float* img_host, int32_t b, float* logits_host) {
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_forward_host(m, img_host, (int64_t)m->cfg.img_height * m->cfg.img_width * m->cfg.n_input_channels, b, logits_host,
                                [&](std::string& err) { return cct_forward(m, m->img, b, err); });
}
int32_t vitx_cct_backward_dev(vitx_cct_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = cct_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_cct_backward(vitx_cct_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->cfg.img_height * m->cfg.img_width * m->cfg.n_input_channels,
                                 [&](float* dimg_dev, std::string& err) { return cct_backward(m, m->dlogits, dimg_dev, err); });
}
int32_t vitx_cct_profile_begin(vitx_cct_handle m) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_begin({m->eng});
}
int32_t vitx_cct_profile_end(vitx_cct_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");
  return composite_profile_end({m->eng}, out, cap, n_out);
}
int32_t vitx_cct_read(vitx_cct_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const float* src = nullptr;
  int64_t n = 0;
  if (w == "tokens") { src = m->conv.back().pooled; n = (int64_t)m->b * m->n * m->d; }
  else if (w == "encoded") { src = m->xn; n = (int64_t)m->b * m->n * m->d; }
  else if (w == "pool_weights") { src = m->p; n = (int64_t)m->b * m->n; }
  else if (w == "pooled") { src = m->pooled; n = (int64_t)m->b * m->d; }
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
