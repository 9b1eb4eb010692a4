// CrossViT (cross_vit.py:232-301): two ImageEmbedders on the same image, `depth` multi-scale layers of [sm Transformer, lg Transformer,
// CrossTransformer] and two summed mlp_heads.  Each encoder (Transformer, cross_vit.py:95-115) is an ordinary ViT engine holding that
// encoder's blocks; the first encoder's engine of a branch also serves as its ImageEmbedder (engine_embed_*), the last one as its mlp_head
// (engine_head_*).  Around them the composite runs the encoders' final LayerNorms, the emb_dropout, and the cross-attention layers
// (cross_vit.py:117-164): fp32 Dense layers on the generic GEMM path and one HIP cross-attention kernel pair (one query row per image).
// The composite owns the public parameter / gradient arenas in its own table order and maps them to / from the engines' arenas on the device.
#include <algorithm>
#include <cstring>

#include "composite.h"

namespace {

// ------------------------------------------------------------------------------------------------ cross-attention kernels
// One workgroup of 256 threads per (image, head).  Key / value rows are read straight from the to_kv output [b, nk, 2 * inner]
// (k = columns [h * dh, (h + 1) * dh), v = the same columns + inner); 16 lanes share a row (one float4 each at dh = 64), so a
// row is one coalesced 256-B read and 16 rows are in flight per pass.  Scores / probabilities stay in LDS ([nk] floats).
constexpr int XA_THREADS = 256, XA_G = 16, XA_ROWS = XA_THREADS / XA_G, XA_MAX_CHUNKS = 4;   // dh <= 4 * 16 * 4 = 256

__device__ __forceinline__ float group_sum16(float v) {
  for (int off = XA_G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, XA_G);
  return v;
}
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x / 64;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < XA_THREADS / 64; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

// o[b, h*dh:(h+1)*dh] = softmax(scale * q k^T) v;  lse[b * h + hh] = log-sum-exp of the scaled scores
__global__ __launch_bounds__(XA_THREADS) void crossvit_xattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ o,
                                                                        float* __restrict__ lse, int nk, int h, int dh, float scale) {
  extern __shared__ float xa_lds[];
  const int bi = blockIdx.x / h, hh = blockIdx.x % h, inner = h * dh, nch = dh / 4;
  float* p = xa_lds;                                  // [nk]
  float* part = p + ((nk + 3) & ~3);                  // [XA_ROWS][dh]
  float* red = part + XA_ROWS * dh;                   // [4]
  const int tid = threadIdx.x, grp = tid / XA_G, ln = tid % XA_G;
  const float4* q4 = reinterpret_cast<const float4*>(q + (int64_t)bi * inner + hh * dh);
  float4 qr[XA_MAX_CHUNKS];
  for (int t = 0; t < XA_MAX_CHUNKS; ++t) qr[t] = (ln + t * XA_G < nch) ? q4[ln + t * XA_G] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t ldkv = 2 * (int64_t)inner;
  const float* kbase = kv + (int64_t)bi * nk * ldkv + hh * dh;
  for (int j = grp; j < nk; j += XA_ROWS) {
    const float4* k4 = reinterpret_cast<const float4*>(kbase + j * ldkv);
    float acc = 0.f;
    for (int t = 0; t < XA_MAX_CHUNKS; ++t)
      if (ln + t * XA_G < nch) {
        const float4 k = k4[ln + t * XA_G];
        acc += qr[t].x * k.x + qr[t].y * k.y + qr[t].z * k.z + qr[t].w * k.w;
      }
    acc = group_sum16(acc);
    if (ln == 0) p[j] = acc * scale;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = tid; j < nk; j += XA_THREADS) m = fmaxf(m, p[j]);
  m = block_reduce(m, red, true);
  float s = 0.f;
  for (int j = tid; j < nk; j += XA_THREADS) {
    const float e = __expf(p[j] - m);
    p[j] = e;
    s += e;
  }
  s = block_reduce(s, red, false);   // (its barriers also publish p)
  float4 acc[XA_MAX_CHUNKS];
  for (int t = 0; t < XA_MAX_CHUNKS; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = grp; j < nk; j += XA_ROWS) {
    const float4* v4 = reinterpret_cast<const float4*>(kbase + j * ldkv + inner);
    const float pj = p[j];
    for (int t = 0; t < XA_MAX_CHUNKS; ++t)
      if (ln + t * XA_G < nch) {
        const float4 v = v4[ln + t * XA_G];
        acc[t].x += pj * v.x; acc[t].y += pj * v.y; acc[t].z += pj * v.z; acc[t].w += pj * v.w;
      }
  }
  for (int t = 0; t < XA_MAX_CHUNKS; ++t)
    if (ln + t * XA_G < nch) reinterpret_cast<float4*>(part + grp * dh)[ln + t * XA_G] = acc[t];
  __syncthreads();
  const float inv = 1.f / s;
  for (int c = tid; c < dh; c += XA_THREADS) {
    float r = 0.f;
    for (int g = 0; g < XA_ROWS; ++g) r += part[g * dh + c];
    o[(int64_t)bi * inner + hh * dh + c] = r * inv;
  }
  if (tid == 0) lse[blockIdx.x] = m + __logf(s);
}

// VJP: P recomputed from the saved LSE.  dq [b, inner]; dkv [b, nk, 2 * inner] (dk | dv, the layout of the to_kv output)
__global__ __launch_bounds__(XA_THREADS) void crossvit_xattn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                        const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                        float* __restrict__ dq, float* __restrict__ dkv, int nk, int h, int dh,
                                                                        float scale) {
  extern __shared__ float xa_lds[];
  const int bi = blockIdx.x / h, hh = blockIdx.x % h, inner = h * dh, nch = dh / 4;
  float* p = xa_lds;                                  // [nk]
  float* dp = p + ((nk + 3) & ~3);                    // [nk]
  float* part = dp + ((nk + 3) & ~3);                 // [XA_ROWS][dh]
  float* red = part + XA_ROWS * dh;
  const int tid = threadIdx.x, grp = tid / XA_G, ln = tid % XA_G;
  const float4* q4 = reinterpret_cast<const float4*>(q + (int64_t)bi * inner + hh * dh);
  const float4* do4 = reinterpret_cast<const float4*>(d_o + (int64_t)bi * inner + hh * dh);
  float4 qr[XA_MAX_CHUNKS], dor[XA_MAX_CHUNKS];
  for (int t = 0; t < XA_MAX_CHUNKS; ++t) {
    const bool in = ln + t * XA_G < nch;
    qr[t] = in ? q4[ln + t * XA_G] : make_float4(0.f, 0.f, 0.f, 0.f);
    dor[t] = in ? do4[ln + t * XA_G] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float L = lse[blockIdx.x];
  const int64_t ldkv = 2 * (int64_t)inner;
  const float* kbase = kv + (int64_t)bi * nk * ldkv + hh * dh;
  float* dkbase = dkv + (int64_t)bi * nk * ldkv + hh * dh;
  for (int j = grp; j < nk; j += XA_ROWS) {
    const float4* k4 = reinterpret_cast<const float4*>(kbase + j * ldkv);
    const float4* v4 = reinterpret_cast<const float4*>(kbase + j * ldkv + inner);
    float a = 0.f, b = 0.f;
    for (int t = 0; t < XA_MAX_CHUNKS; ++t)
      if (ln + t * XA_G < nch) {
        const float4 k = k4[ln + t * XA_G], v = v4[ln + t * XA_G];
        a += qr[t].x * k.x + qr[t].y * k.y + qr[t].z * k.z + qr[t].w * k.w;
        b += dor[t].x * v.x + dor[t].y * v.y + dor[t].z * v.z + dor[t].w * v.w;
      }
    a = group_sum16(a);
    b = group_sum16(b);
    if (ln == 0) { p[j] = __expf(a * scale - L); dp[j] = b; }
  }
  __syncthreads();
  float D = 0.f;
  for (int j = tid; j < nk; j += XA_THREADS) D += p[j] * dp[j];
  D = block_reduce(D, red, false);
  float4 acc[XA_MAX_CHUNKS];
  for (int t = 0; t < XA_MAX_CHUNKS; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = grp; j < nk; j += XA_ROWS) {
    const float pj = p[j], ds = pj * (dp[j] - D), dss = ds * scale;
    const float4* k4 = reinterpret_cast<const float4*>(kbase + j * ldkv);
    float4* dk4 = reinterpret_cast<float4*>(dkbase + j * ldkv);
    float4* dv4 = reinterpret_cast<float4*>(dkbase + j * ldkv + inner);
    for (int t = 0; t < XA_MAX_CHUNKS; ++t)
      if (ln + t * XA_G < nch) {
        const int c = ln + t * XA_G;
        const float4 k = k4[c];
        acc[t].x += ds * k.x; acc[t].y += ds * k.y; acc[t].z += ds * k.z; acc[t].w += ds * k.w;
        dk4[c] = make_float4(dss * qr[t].x, dss * qr[t].y, dss * qr[t].z, dss * qr[t].w);
        dv4[c] = make_float4(pj * dor[t].x, pj * dor[t].y, pj * dor[t].z, pj * dor[t].w);
      }
  }
  for (int t = 0; t < XA_MAX_CHUNKS; ++t)
    if (ln + t * XA_G < nch) reinterpret_cast<float4*>(part + grp * dh)[ln + t * XA_G] = acc[t];
  __syncthreads();
  for (int c = tid; c < dh; c += XA_THREADS) {
    float r = 0.f;
    for (int g = 0; g < XA_ROWS; ++g) r += part[g * dh + c];
    dq[(int64_t)bi * inner + hh * dh + c] = r * scale;
  }
}

size_t xattn_lds_bytes(int nk, int dh, bool bwd) { return (size_t)((bwd ? 2 : 1) * round_up(nk, 4) + XA_ROWS * dh + 8) * 4; }
bool xattn_supported(int nk, int dh) { return dh % 4 == 0 && dh <= 4 * XA_G * XA_MAX_CHUNKS && xattn_lds_bytes(nk, dh, true) <= 64 * 1024; }

// ------------------------------------------------------------------------------------------------ row kernels of the cross layers
// out[i, :] = X[i, 0, :]   (the cls row of every image)
__global__ void crossvit_cls_gather_kernel(const float* __restrict__ X, int ntok, int d, int b, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)b * d) return;
  const int64_t i = e / d, c = e % d;
  out[e] = X[i * ntok * d + c];
}
// X[i, 0, :] = (add ? X[i, 0, :] : 0) + y[i, :]  (+ y2[i, :] when given)
__global__ void crossvit_cls_store_kernel(float* __restrict__ X, int ntok, int d, int b, const float* __restrict__ y, const float* __restrict__ y2, int add) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)b * d) return;
  const int64_t i = e / d, c = e % d;
  float* x = X + i * ntok * d + c;
  *x = (add ? *x : 0.f) + y[e] + (y2 ? y2[e] : 0.f);
}
// ctx[i] = [xn[i]; Y[i, 1:]]  (cross_vit.py:75-76: the normalised query row is key / value row 0)
__global__ void crossvit_ctx_assemble_kernel(const float* __restrict__ xn, const float* __restrict__ Y, int nk, int d, int b, float* __restrict__ ctx) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)b * nk * d) return;
  const int64_t c = e % d, r = (e / d) % nk, i = e / ((int64_t)nk * d);
  ctx[e] = r == 0 ? xn[i * d + c] : Y[e];
}
// dxn[i] += dctx[i, 0];  dY[i, 1:] += dctx[i, 1:]
__global__ void crossvit_ctx_split_bwd_kernel(const float* __restrict__ dctx, int nk, int d, int b, float* __restrict__ dxn, float* __restrict__ dY) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)b * nk * d) return;
  const int64_t c = e % d, r = (e / d) % nk, i = e / ((int64_t)nk * d);
  if (r == 0) dxn[i * d + c] += dctx[e];
  else dY[e] += dctx[e];
}
__global__ void crossvit_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = a[e] + b[e];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ composite
struct XDense { int64_t w = -1, b = -1; int in = 0, out = 0; };
// one direction of one cross round (sm_attend_lg or lg_attend_sm): ProjectInOut(dx -> D, PreNorm(Attention(D)))
struct XLayer {
  int br = 0;                       // 0: the sm cls attends over the lg patches, 1: the mirror image
  int dx = 0, D = 0;                // the cls row's width, the attention's width (the other branch's)
  bool proj = false;
  XDense pin, pout, q, kv, out;
  int64_t ln_g = -1, ln_b = -1;
  // activations of the last forward
  float *x0 = nullptr, *xin = nullptr, *xn = nullptr, *mean = nullptr, *rstd = nullptr, *q_act = nullptr, *kv_act = nullptr, *o = nullptr, *lse = nullptr,
        *fd = nullptr;
};
struct vitx_crossvit {
  vitx_crossvit_config cfg{};
  std::vector<ParamDesc> table;
  int64_t n_params = 0, n_arena = 0;
  float *params = nullptr, *grads = nullptr;
  std::vector<vitx_engine*> eng;      // [br * depth + i]: the encoder of branch br in multi-scale layer i
  std::vector<std::vector<ArenaMap>> eng_maps, head_maps;   // per engine: the maps of its encoder (+ embedder) / of its mlp_head
  std::vector<XLayer> xl;             // [(i * cross_depth + k) * 2 + dir]
  int64_t fn_g[2][64] = {}, fn_b[2][64] = {};   // per branch / layer: the encoder's final LayerNorm
  int dim[2] = {0, 0}, np_max[2] = {0, 0}, patch[2] = {0, 0};
  int ci = 0, ch = 0, cdh = 0, nc = 0, B = 0;
  hipStream_t stream = nullptr;
  DevicePool pool;
  // per branch
  float* tok0[2] = {};                // embedding output (after emb_dropout)
  std::vector<float*> E[2], T[2], fmean[2], frstd[2];   // per layer: encoder output, final-norm output (cls row updated in place by the cross layers)
  float *G[2] = {}, *dE[2] = {}, *logit_br[2] = {};
  float *img = nullptr, *dimg = nullptr, *dimg_lg = nullptr, *logits = nullptr, *dlogits = nullptr;
  float *ctx = nullptr, *dctx = nullptr, *dkv = nullptr, *s_dfd = nullptr, *s_df = nullptr, *s_do = nullptr, *s_dq = nullptr, *s_dxn = nullptr,
        *s_dxin = nullptr, *s_dx0 = nullptr, *s_f = nullptr, *s_out = nullptr, *ws = nullptr;
  bool have_fwd = false;
  int b = 0, H = 0, W = 0, ntok[2] = {0, 0}, training = 0;
  uint64_t seed = 0;
};

namespace {

constexpr uint32_t SITE_EMB = 0x43560001u, SITE_XOUT = 0x43560100u;
uint64_t mix_seed(uint64_t seed, uint64_t k) {   // splitmix64 step: independent mask streams for the encoders' engines
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace

// Table of CrossViT's variables in the documented order; "" or the reference's assertion text.
std::string crossvit_param_table(const vitx_crossvit_config& c, std::vector<ParamDesc>& out, int64_t* n_elems, int64_t* n_arena,
                                 vitx_crossvit* m = nullptr) {
  out.clear();
  const int ps[2] = {c.sm_patch_size, c.lg_patch_size}, dm[2] = {c.sm_dim, c.lg_dim};
  const int edepth[2] = {c.sm_enc_depth, c.lg_enc_depth}, eheads[2] = {c.sm_enc_heads, c.lg_enc_heads};
  const int emlp[2] = {c.sm_enc_mlp_dim, c.lg_enc_mlp_dim}, edh[2] = {c.sm_enc_dim_head, c.lg_enc_dim_head};
  if (c.image_size <= 0 || c.num_classes <= 0 || c.depth < 0 || c.cross_attn_depth < 0 || c.cross_attn_heads <= 0 || c.cross_attn_dim_head <= 0)
    return "invalid CrossViT configuration";
  for (int br = 0; br < 2; ++br) {
    if (dm[br] <= 0 || ps[br] <= 0 || edepth[br] < 0 || eheads[br] <= 0 || emlp[br] <= 0 || edh[br] <= 0) return "invalid CrossViT configuration";
    if (c.image_size % ps[br]) return "Image dimensions must be divisible by the patch size.";   // cross_vit.py:208
  }
  if (c.depth > 64) return "depth must be <= 64";
  TableBuilder tb{out};
  static const char* BR[2] = {"sm", "lg"};
  for (int br = 0; br < 2; ++br) {   // ImageEmbedder (cross_vit.py:199-218)
    const std::string p = std::string(BR[br]) + "_image_embedder.";
    const int64_t np = (int64_t)(c.image_size / ps[br]) * (c.image_size / ps[br]), d = dm[br];
    tb.add(p + "pos_embedding", {1, np + 1, d});
    tb.add(p + "cls_token", {1, 1, d});
    tb.add(p + "patch_embedding.kernel", {(int64_t)ps[br] * ps[br] * 3, d});
    tb.add(p + "patch_embedding.bias", {d});
  }
  const int64_t ci = (int64_t)c.cross_attn_heads * c.cross_attn_dim_head;
  for (int i = 0; i < c.depth; ++i) {
    const std::string L = "multi_scale_encoder." + std::to_string(i) + ".";
    for (int br = 0; br < 2; ++br) {   // Transformer (cross_vit.py:95-115)
      const int64_t d = dm[br], inner = (int64_t)eheads[br] * edh[br], mlp = emlp[br];
      for (int j = 0; j < edepth[br]; ++j) {
        const std::string p = L + BR[br] + "_enc." + std::to_string(j) + ".";
        tb.add(p + "attn.norm.gamma", {d}); tb.add(p + "attn.norm.beta", {d});
        tb.add(p + "attn.to_q.kernel", {d, inner}); tb.add(p + "attn.to_kv.kernel", {d, 2 * inner});
        tb.add(p + "attn.to_out.kernel", {inner, d}); tb.add(p + "attn.to_out.bias", {d});
        tb.add(p + "mlp.norm.gamma", {d}); tb.add(p + "mlp.norm.beta", {d});
        tb.add(p + "mlp.fc1.kernel", {d, mlp}); tb.add(p + "mlp.fc1.bias", {mlp});
        tb.add(p + "mlp.fc2.kernel", {mlp, d}); tb.add(p + "mlp.fc2.bias", {d});
      }
      const int64_t g = tb.add(L + BR[br] + "_enc.norm.gamma", {d}), b = tb.add(L + BR[br] + "_enc.norm.beta", {d});
      if (m) { m->fn_g[br][i] = g; m->fn_b[br][i] = b; }
    }
    for (int k = 0; k < c.cross_attn_depth; ++k) {   // CrossTransformer (cross_vit.py:141-164)
      for (int dir = 0; dir < 2; ++dir) {
        const std::string p = L + "cross." + std::to_string(k) + (dir == 0 ? ".sm_attend_lg." : ".lg_attend_sm.");
        const int64_t dx = dm[dir], D = dm[1 - dir];
        XLayer x;
        x.br = dir; x.dx = (int)dx; x.D = (int)D; x.proj = dx != D;
        if (x.proj) { x.pin = {tb.add(p + "project_in.kernel", {dx, D}), tb.add(p + "project_in.bias", {D}), (int)dx, (int)D}; }
        x.ln_g = tb.add(p + "norm.gamma", {D}); x.ln_b = tb.add(p + "norm.beta", {D});
        x.q = {tb.add(p + "to_q.kernel", {D, ci}), -1, (int)D, (int)ci};
        x.kv = {tb.add(p + "to_kv.kernel", {D, 2 * ci}), -1, (int)D, (int)(2 * ci)};
        x.out.w = tb.add(p + "to_out.kernel", {ci, D}); x.out.b = tb.add(p + "to_out.bias", {D}); x.out.in = (int)ci; x.out.out = (int)D;
        if (x.proj) { x.pout = {tb.add(p + "project_out.kernel", {D, dx}), tb.add(p + "project_out.bias", {dx}), (int)D, (int)dx}; }
        if (m) m->xl.push_back(x);
      }
    }
  }
  for (int br = 0; br < 2; ++br) {   // Sequential([LayerNormalization, Dense]) (cross_vit.py:280-288)
    const std::string p = std::string(BR[br]) + "_mlp_head.";
    tb.add(p + "norm.gamma", {dm[br]}); tb.add(p + "norm.beta", {dm[br]});
    tb.add(p + "kernel", {dm[br], c.num_classes}); tb.add(p + "bias", {c.num_classes});
  }
  if (n_elems) *n_elems = tb.n;
  if (n_arena) *n_arena = tb.n_arena;
  return "";
}

namespace {

#define XALLOC(ptr, elems) POOL_ALLOC(m->pool, ptr, (int64_t)(elems) * 4, m->stream, rc_)

void crossvit_destroy(vitx_crossvit* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->pool.free_all();
  for (auto* e : m->eng) engine_destroy(e);
  delete m;
}

int crossvit_create(const vitx_crossvit_config& cin, vitx_crossvit** out, std::string& err) {
  vitx_crossvit_config c = cin;
  if (c.ln_eps <= 0.f) c.ln_eps = 1e-3f;   // Keras LayerNormalization default
  if (c.max_batch <= 0) { err = "max_batch must be positive"; return VITX_ERR_INVALID; }
  if (c.compute != VITX_COMPUTE_FP32_PARITY && c.compute != VITX_COMPUTE_BF16 && c.compute != VITX_COMPUTE_BF16X3) { err = "unknown compute mode"; return VITX_ERR_INVALID; }
  {
    std::vector<ParamDesc> t;
    std::string e = crossvit_param_table(c, t, nullptr, nullptr);
    if (!e.empty()) { err = e; return VITX_ERR_INVALID; }
  }
  const int dm[2] = {c.sm_dim, c.lg_dim}, eheads[2] = {c.sm_enc_heads, c.lg_enc_heads}, edh[2] = {c.sm_enc_dim_head, c.lg_enc_dim_head};
  for (int br = 0; br < 2; ++br)
    if (eheads[br] == 1 && edh[br] == dm[br]) {   // the engine's ViT table drops to_out there (vit.py:53); cross_vit.py:64-69 always has it
      err = std::string(br ? "lg" : "sm") + "_enc_heads == 1 and " + (br ? "lg" : "sm") +
            "_enc_dim_head == dim is not supported (the encoder's to_out would be dropped)";
      return VITX_ERR_UNSUPPORTED;
    }
  if (c.depth < 1) { err = "depth must be >= 1"; return VITX_ERR_UNSUPPORTED; }
  const int ps[2] = {c.sm_patch_size, c.lg_patch_size};
  const int nk_max = std::max((c.image_size / ps[0]) * (c.image_size / ps[0]), (c.image_size / ps[1]) * (c.image_size / ps[1])) + 1;
  if (!xattn_supported(nk_max, c.cross_attn_dim_head)) {
    err = "cross attention: cross_attn_dim_head must be a multiple of 4 and <= 256, with at most ~12k tokens per branch";
    return VITX_ERR_UNSUPPORTED;
  }
  vitx_crossvit* m = new vitx_crossvit();
  m->cfg = c;
  int rc = VITX_OK;
  auto fail = [&](int code) { crossvit_destroy(m); return code; };
  crossvit_param_table(c, m->table, &m->n_params, &m->n_arena, m);
  m->ci = c.cross_attn_heads * c.cross_attn_dim_head; m->ch = c.cross_attn_heads; m->cdh = c.cross_attn_dim_head;
  m->nc = c.num_classes; m->B = c.max_batch;
  const int edepth[2] = {c.sm_enc_depth, c.lg_enc_depth}, emlp[2] = {c.sm_enc_mlp_dim, c.lg_enc_mlp_dim};
  for (int br = 0; br < 2; ++br) {
    m->dim[br] = dm[br]; m->patch[br] = ps[br];
    m->np_max[br] = (c.image_size / ps[br]) * (c.image_size / ps[br]);
    for (int i = 0; i < c.depth; ++i) {
      vitx_config ec{};
      ec.variant = VITX_VARIANT_VIT;
      ec.image_h = ec.image_w = c.image_size; ec.patch_h = ec.patch_w = ps[br]; ec.channels = 3;
      ec.num_classes = c.num_classes; ec.dim = dm[br]; ec.depth = edepth[br]; ec.heads = eheads[br]; ec.dim_head = edh[br];
      ec.mlp_dim = emlp[br]; ec.pool = VITX_POOL_CLS; ec.dropout = c.dropout; ec.ln_eps = c.ln_eps;
      ec.compute = c.compute; ec.max_batch = c.max_batch; ec.device_id = c.device_id;
      vitx_engine* e = nullptr;
      if ((rc = engine_create(ec, &e, err)) != VITX_OK) return fail(rc);
      m->eng.push_back(e);
    }
  }
  m->stream = m->eng[0]->stream;
  // parameter maps
  m->eng_maps.assign(m->eng.size(), {});
  m->head_maps.assign(m->eng.size(), {});
  auto add_map = [&](int ei, const std::string& cname, const std::string& ename, int64_t col0, int64_t width, bool head) -> bool {
    return add_arena_map((head ? m->head_maps : m->eng_maps)[(size_t)ei], m->table, cname, m->eng[(size_t)ei]->table, ename, err, col0, width) == VITX_OK;
  };
  static const char* BR[2] = {"sm", "lg"};
  for (int br = 0; br < 2; ++br) {
    const int inner = eheads[br] * edh[br];
    const int e0 = br * c.depth, eL = br * c.depth + c.depth - 1;
    const std::string ie = std::string(BR[br]) + "_image_embedder.";
    for (const char* n : {"pos_embedding", "cls_token", "patch_embedding.kernel", "patch_embedding.bias"})
      if (!add_map(e0, ie + n, n, 0, -1, false)) return fail(VITX_ERR_INVALID);
    for (int i = 0; i < c.depth; ++i)
      for (int j = 0; j < edepth[br]; ++j) {
        const std::string cp = "multi_scale_encoder." + std::to_string(i) + "." + BR[br] + "_enc." + std::to_string(j) + ".";
        const std::string ep = "transformer." + std::to_string(j) + ".";
        const int ei = e0 + i;
        bool ok = add_map(ei, cp + "attn.to_q.kernel", ep + "attn.to_qkv.kernel", 0, inner, false) &&
                  add_map(ei, cp + "attn.to_kv.kernel", ep + "attn.to_qkv.kernel", inner, 2 * inner, false);
        for (const char* n : {"attn.norm.gamma", "attn.norm.beta", "attn.to_out.kernel", "attn.to_out.bias", "mlp.norm.gamma", "mlp.norm.beta",
                              "mlp.fc1.kernel", "mlp.fc1.bias", "mlp.fc2.kernel", "mlp.fc2.bias"})
          ok = ok && add_map(ei, cp + n, ep + n, 0, -1, false);
        if (!ok) return fail(VITX_ERR_INVALID);
      }
    const std::string hp = std::string(BR[br]) + "_mlp_head.";
    for (const char* n : {"norm.gamma", "norm.beta", "kernel", "bias"})
      if (!add_map(eL, hp + n, std::string("mlp_head.") + n, 0, -1, true)) return fail(VITX_ERR_INVALID);
  }
  // buffers
  const int64_t B = m->B, ci = m->ci;
  XALLOC(m->params, m->n_arena);
  XALLOC(m->grads, m->n_arena);
  int64_t big = 0;
  for (int br = 0; br < 2; ++br) {
    const int64_t n = m->np_max[br] + 1, d = dm[br], rows = B * n;
    big = std::max(big, rows * d);
    XALLOC(m->tok0[br], rows * d); XALLOC(m->G[br], rows * d); XALLOC(m->dE[br], rows * d); XALLOC(m->logit_br[br], B * m->nc);
    for (int i = 0; i < c.depth; ++i) {
      float *e, *t, *mu, *rs;
      XALLOC(e, rows * d); XALLOC(t, rows * d); XALLOC(mu, rows); XALLOC(rs, rows);
      m->E[br].push_back(e); m->T[br].push_back(t); m->fmean[br].push_back(mu); m->frstd[br].push_back(rs);
    }
  }
  const int64_t nk_rows = B * nk_max, dmax = std::max(dm[0], dm[1]);
  for (auto& x : m->xl) {
    const int64_t nk = m->np_max[1 - x.br] + 1;
    XALLOC(x.x0, B * x.dx); XALLOC(x.xn, B * x.D); XALLOC(x.mean, B); XALLOC(x.rstd, B); XALLOC(x.q_act, B * ci);
    XALLOC(x.kv_act, B * nk * 2 * ci); XALLOC(x.o, B * ci); XALLOC(x.lse, B * m->ch); XALLOC(x.fd, B * x.D);
    if (x.proj) XALLOC(x.xin, B * x.D);
    else x.xin = x.x0;
  }
  XALLOC(m->img, B * c.image_size * c.image_size * 3); XALLOC(m->dimg, B * c.image_size * c.image_size * 3);
  XALLOC(m->dimg_lg, B * c.image_size * c.image_size * 3);
  XALLOC(m->logits, B * m->nc); XALLOC(m->dlogits, B * m->nc);
  XALLOC(m->ctx, std::max(big, nk_rows * dmax)); XALLOC(m->dctx, std::max(big, nk_rows * dmax)); XALLOC(m->dkv, nk_rows * 2 * ci);
  for (float** p : {&m->s_dfd, &m->s_df, &m->s_dxn, &m->s_dxin, &m->s_dx0, &m->s_f, &m->s_out}) XALLOC(*p, B * dmax);
  XALLOC(m->s_do, B * ci); XALLOC(m->s_dq, B * ci);
  XALLOC(m->ws, std::max<int64_t>(layernorm_bwd_ws_elems((int)dmax), colsum_ws_elems((int)std::max<int64_t>({dmax, 2 * ci, (int64_t)m->nc}))) + 64);
  if (hipStreamSynchronize(m->stream) != hipSuccess) { err = "hipStreamSynchronize failed"; return fail(VITX_ERR_HIP); }
  *out = m;
  return VITX_OK;
}

void bind_streams(vitx_crossvit* m) {
  for (auto* e : m->eng) e->stream = m->stream;
}

// composite arena -> every engine's arena (the encoders' to_q | to_kv become the column blocks of to_qkv)
int push_params(vitx_crossvit* m, std::string& err) {
  int rc;
  for (size_t ei = 0; ei < m->eng.size(); ++ei)
    for (const auto* maps : {&m->eng_maps[ei], &m->head_maps[ei]})
      if ((rc = copy_maps(m->params, m->eng[ei]->params, *maps, true, m->stream, err)) != VITX_OK) return rc;
  for (auto* e : m->eng) e->params_dirty = true;
  return VITX_OK;
}
// one engine's gradients of one of its two lists -> the composite's arena
int pull_grads(vitx_crossvit* m, int ei, const std::vector<std::vector<ArenaMap>>& lists, std::string& err) {
  return copy_maps(m->grads, m->eng[(size_t)ei]->grads, lists[(size_t)ei], false, m->stream, err);
}

void launch_xattn_fwd(const float* q, const float* kv, float* o, float* lse, int b, int nk, int h, int dh, hipStream_t s) {
  hipLaunchKernelGGL(crossvit_xattn_fwd_kernel, dim3((unsigned)(b * h)), dim3(XA_THREADS), xattn_lds_bytes(nk, dh, false), s, q, kv, o, lse, nk, h, dh,
                     1.0f / sqrtf((float)dh));
}
void launch_xattn_bwd(const float* q, const float* kv, const float* d_o, const float* lse, float* dq, float* dkv, int b, int nk, int h, int dh,
                      hipStream_t s) {
  hipLaunchKernelGGL(crossvit_xattn_bwd_kernel, dim3((unsigned)(b * h)), dim3(XA_THREADS), xattn_lds_bytes(nk, dh, true), s, q, kv, d_o, lse, dq, dkv, nk,
                     h, dh, 1.0f / sqrtf((float)dh));
}

// ProjectInOut(PreNorm(Attention)) on the cls rows of X (branch x.br) with the other branch's final-norm tokens Y as context;
// X[:, 0] += result (cross_vit.py:158-159)
void cross_forward(vitx_crossvit* m, XLayer& x, float* X, int nx, const float* Y, int ny, uint32_t site) {
  hipStream_t s = m->stream;
  const int b = m->b, ci = m->ci;
  const float* P = m->params;
  hipLaunchKernelGGL(crossvit_cls_gather_kernel, dim3(grid256((int64_t)b * x.dx)), dim3(256), 0, s, X, nx, x.dx, b, x.x0);
  if (x.proj) dense_fwd(x.x0, x.dx, P + x.pin.w, P + x.pin.b, x.xin, b, x.D, x.dx, s);                          // project_in  :133-134
  launch_layernorm_fwd(x.xin, x.D, P + x.ln_g, P + x.ln_b, x.xn, 0, x.D, x.mean, x.rstd, b, x.D, m->cfg.ln_eps, s);   // PreNorm :22
  dense_fwd(x.xn, x.D, P + x.q.w, nullptr, x.q_act, b, ci, x.D, s);                                             // to_q     :78
  const int64_t nrow = (int64_t)b * ny;
  hipLaunchKernelGGL(crossvit_ctx_assemble_kernel, dim3(grid256(nrow * x.D)), dim3(256), 0, s, x.xn, Y, ny, x.D, b, m->ctx);   // :75-76
  dense_fwd(m->ctx, x.D, P + x.kv.w, nullptr, x.kv_act, (int)nrow, 2 * ci, x.D, s);                             // to_kv    :79
  launch_xattn_fwd(x.q_act, x.kv_act, x.o, x.lse, b, ny, m->ch, m->cdh, s);                                   // :80-88
  dense_fwd(x.o, ci, P + x.out.w, P + x.out.b, x.fd, b, x.D, ci, s);                                            // to_out   :89
  if (m->training) launch_dropout(x.fd, 0, (int64_t)b * x.D, m->cfg.dropout, m->seed, site, s);
  const float* r = x.fd;
  if (x.proj) { dense_fwd(x.fd, x.D, P + x.pout.w, P + x.pout.b, m->s_out, b, x.dx, x.D, s); r = m->s_out; }   // project_out :139-140
  hipLaunchKernelGGL(crossvit_cls_store_kernel, dim3(grid256((int64_t)b * x.dx)), dim3(256), 0, s, X, nx, x.dx, b, r, (const float*)nullptr, 1);
}

// VJP of the above: dX[:, 0] (the gradient of the updated cls row) is replaced by that of the old one; dY[:, 1:] accumulates
void cross_backward(vitx_crossvit* m, XLayer& x, float* dX, int nx, const float* Y, float* dY, int ny, uint32_t site) {
  hipStream_t s = m->stream;
  const int b = m->b, ci = m->ci;
  const float* P = m->params;
  float* Gd = m->grads;
  float* dout = m->s_dx0;   // d(new cls) [b, dx]
  hipLaunchKernelGGL(crossvit_cls_gather_kernel, dim3(grid256((int64_t)b * x.dx)), dim3(256), 0, s, dX, nx, x.dx, b, dout);
  float* df = m->s_df;
  if (x.proj) {
    dense_dx(dout, P + x.pout.w, df, b, x.dx, x.D, s);
    dense_dw(x.fd, x.D, dout, Gd + x.pout.w, b, x.dx, x.D, s);
    launch_colsum(dout, 0, x.dx, b, x.dx, m->ws, Gd + x.pout.b, s);
  } else {
    (void)hipMemcpyAsync(df, dout, (size_t)b * x.D * 4, hipMemcpyDeviceToDevice, s);
  }
  if (m->training) launch_dropout(df, 0, (int64_t)b * x.D, m->cfg.dropout, m->seed, site, s);   // the forward's mask, replayed
  dense_dw(x.o, ci, df, Gd + x.out.w, b, x.D, ci, s);
  launch_colsum(df, 0, x.D, b, x.D, m->ws, Gd + x.out.b, s);
  dense_dx(df, P + x.out.w, m->s_do, b, x.D, ci, s);
  launch_xattn_bwd(x.q_act, x.kv_act, m->s_do, x.lse, m->s_dq, m->dkv, b, ny, m->ch, m->cdh, s);
  dense_dw(x.xn, x.D, m->s_dq, Gd + x.q.w, b, ci, x.D, s);
  dense_dx(m->s_dq, P + x.q.w, m->s_dxn, b, ci, x.D, s);
  const int64_t nrow = (int64_t)b * ny;
  hipLaunchKernelGGL(crossvit_ctx_assemble_kernel, dim3(grid256(nrow * x.D)), dim3(256), 0, s, x.xn, Y, ny, x.D, b, m->ctx);
  dense_dw(m->ctx, x.D, m->dkv, Gd + x.kv.w, (int)nrow, 2 * ci, x.D, s);
  dense_dx(m->dkv, P + x.kv.w, m->dctx, (int)nrow, 2 * ci, x.D, s);
  hipLaunchKernelGGL(crossvit_ctx_split_bwd_kernel, dim3(grid256(nrow * x.D)), dim3(256), 0, s, m->dctx, ny, x.D, b, m->s_dxn, dY);
  launch_layernorm_bwd(m->s_dxn, 0, x.D, x.xin, x.D, x.mean, x.rstd, P + x.ln_g, nullptr, 0, m->s_dxin, x.D, nullptr, 0, m->ws, Gd + x.ln_g,
                       Gd + x.ln_b, nullptr, b, x.D, s);
  const float* dx0 = m->s_dxin;
  if (x.proj) {
    dense_dw(x.x0, x.dx, m->s_dxin, Gd + x.pin.w, b, x.D, x.dx, s);
    launch_colsum(m->s_dxin, 0, x.D, b, x.D, m->ws, Gd + x.pin.b, s);
    dense_dx(m->s_dxin, P + x.pin.w, m->s_dfd, b, x.D, x.dx, s);
    dx0 = m->s_dfd;
  }
  // d(old cls) = residual + branch
  hipLaunchKernelGGL(crossvit_cls_store_kernel, dim3(grid256((int64_t)b * x.dx)), dim3(256), 0, s, dX, nx, x.dx, b, dx0, (const float*)dout, 0);
}

int crossvit_forward(vitx_crossvit* m, const float* img_dev, int b, int H, int W, int training, uint64_t seed, std::string& err) {
  const vitx_crossvit_config& c = m->cfg;
  m->have_fwd = false;
  if (b <= 0 || b > c.max_batch) { err = "batch must be in [1, max_batch]"; return VITX_ERR_INVALID; }
  if (H <= 0 || W <= 0 || H > c.image_size || W > c.image_size || H % c.sm_patch_size || W % c.sm_patch_size || H % c.lg_patch_size ||
      W % c.lg_patch_size) {
    err = "Image dimensions must be divisible by the patch size.";
    return VITX_ERR_INVALID;
  }
  bind_streams(m);
  hipStream_t s = m->stream;
  m->b = b; m->H = H; m->W = W; m->training = training ? 1 : 0; m->seed = seed;
  const int D = c.depth;
  int rc;
  for (int br = 0; br < 2; ++br) {
    m->ntok[br] = (H / m->patch[br]) * (W / m->patch[br]) + 1;
    vitx_engine* e0 = m->eng[(size_t)(br * D)];
    if ((rc = engine_embed_forward(e0, img_dev, b, H, W, m->tok0[br], err)) != VITX_OK) return rc;            // cross_vit.py:220-226
    if (m->training) launch_dropout(m->tok0[br], 0, (int64_t)b * m->ntok[br] * m->dim[br], c.emb_dropout, seed, SITE_EMB + br, s);   // :227
  }
  for (int i = 0; i < D; ++i) {
    for (int br = 0; br < 2; ++br) {   // Transformer: blocks on the engine, then its final norm (cross_vit.py:109-115)
      const int n = m->ntok[br], d = m->dim[br];
      const float* in = i == 0 ? m->tok0[br] : m->T[br][(size_t)i - 1];
      vitx_engine* e = m->eng[(size_t)(br * D + i)];
      if ((rc = engine_transformer_forward(e, in, b, n, training, mix_seed(seed, (uint64_t)(br * D + i)), m->E[br][(size_t)i], err)) != VITX_OK) return rc;
      launch_layernorm_fwd(m->E[br][(size_t)i], d, m->params + m->fn_g[br][i], m->params + m->fn_b[br][i], m->T[br][(size_t)i], 0, d,
                           m->fmean[br][(size_t)i], m->frstd[br][(size_t)i], b * n, d, c.ln_eps, s);
    }
    for (int k = 0; k < c.cross_attn_depth; ++k)
      for (int dir = 0; dir < 2; ++dir) {
        XLayer& x = m->xl[(size_t)((i * c.cross_attn_depth + k) * 2 + dir)];
        cross_forward(m, x, m->T[dir][(size_t)i], m->ntok[dir], m->T[1 - dir][(size_t)i], m->ntok[1 - dir],
                      SITE_XOUT + (uint32_t)((i * c.cross_attn_depth + k) * 2 + dir));
      }
  }
  for (int br = 0; br < 2; ++br) {   // sm_mlp_head(sm_tokens[:, 0]) (+) lg_mlp_head(lg_tokens[:, 0])  (cross_vit.py:295-301)
    vitx_engine* e = m->eng[(size_t)(br * D + D - 1)];
    if ((rc = engine_head_forward(e, m->T[br][(size_t)D - 1], b, m->ntok[br], m->logit_br[br], err)) != VITX_OK) return rc;
  }
  hipLaunchKernelGGL(crossvit_add_kernel, dim3(grid256((int64_t)b * m->nc)), dim3(256), 0, s, m->logit_br[0], m->logit_br[1], m->logits, (int64_t)b * m->nc);
  m->have_fwd = true;
  return VITX_OK;
}

// dlogits_dev [b, num_classes] -> the gradient arena (every entry overwritten) and optionally d(img) into dimg_dev
int crossvit_backward(vitx_crossvit* m, const float* dlogits_dev, float* dimg_dev, std::string& err) {
  if (!m->have_fwd) { err = "backward requires a preceding forward"; return VITX_ERR_STATE; }
  const vitx_crossvit_config& c = m->cfg;
  bind_streams(m);
  hipStream_t s = m->stream;
  const int b = m->b, D = c.depth;
  int rc;
  launch_fill_zero(m->grads, m->n_arena * 4, s);
  for (int br = 0; br < 2; ++br) {
    const int ei = br * D + D - 1;
    if ((rc = engine_head_backward(m->eng[(size_t)ei], dlogits_dev, m->G[br], err)) != VITX_OK) return rc;
    if ((rc = pull_grads(m, ei, m->head_maps, err)) != VITX_OK) return rc;   // before that engine's transformer backward clears its arena
  }
  for (int i = D - 1; i >= 0; --i) {
    for (int k = c.cross_attn_depth - 1; k >= 0; --k)
      for (int dir = 1; dir >= 0; --dir) {
        XLayer& x = m->xl[(size_t)((i * c.cross_attn_depth + k) * 2 + dir)];
        cross_backward(m, x, m->G[dir], m->ntok[dir], m->T[1 - dir][(size_t)i], m->G[1 - dir], m->ntok[1 - dir],
                       SITE_XOUT + (uint32_t)((i * c.cross_attn_depth + k) * 2 + dir));
      }
    for (int br = 0; br < 2; ++br) {
      const int n = m->ntok[br], d = m->dim[br], ei = br * D + i;
      launch_layernorm_bwd(m->G[br], 0, d, m->E[br][(size_t)i], d, m->fmean[br][(size_t)i], m->frstd[br][(size_t)i], m->params + m->fn_g[br][i],
                           nullptr, 0, m->dE[br], d, nullptr, 0, m->ws, m->grads + m->fn_g[br][i], m->grads + m->fn_b[br][i], nullptr, b * n, d, s);
      vitx_engine* e = m->eng[(size_t)ei];
      if ((rc = engine_transformer_backward(e, m->dE[br], m->G[br], err)) != VITX_OK) return rc;
      if (i == 0) {
        if (m->training) launch_dropout(m->G[br], 0, (int64_t)b * n * d, c.emb_dropout, m->seed, SITE_EMB + br, s);
        // the fold-back writes (not adds) every pixel: the lg branch's goes to a buffer of its own, summed below (both embedders read img)
        if ((rc = engine_embed_backward(e, m->G[br], dimg_dev ? (br ? m->dimg_lg : dimg_dev) : nullptr, err)) != VITX_OK) return rc;
      }
      if ((rc = pull_grads(m, ei, m->eng_maps, err)) != VITX_OK) return rc;
    }
  }
  if (dimg_dev) {
    const int64_t n = (int64_t)b * m->H * m->W * 3;
    hipLaunchKernelGGL(crossvit_add_kernel, dim3(grid256(n)), dim3(256), 0, s, dimg_dev, m->dimg_lg, dimg_dev, n);
  }
  return VITX_OK;
}

}  // namespace

extern "C" {

int32_t vitx_crossvit_param_table_size(const vitx_crossvit_config* cfg, int64_t* n_tensors, int64_t* n_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_size(*cfg, n_tensors, n_elems, crossvit_param_table);
}
int32_t vitx_crossvit_param_table_entry(const vitx_crossvit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                        int64_t* offset_elems) {
  if (!cfg) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_table_entry(*cfg, index, name, name_cap, shape, rank, offset_elems, crossvit_param_table);
}
int32_t vitx_crossvit_create(const vitx_crossvit_config* cfg, vitx_crossvit_handle* out) {
  if (!cfg || !out) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_create(*cfg, out, crossvit_create);
}
int32_t vitx_crossvit_destroy(vitx_crossvit_handle m) {
  CAPI_TRY
  crossvit_destroy(m);
  return VITX_OK;
  CAPI_CATCH
}
COMPOSITE_ARENA_EXPORTS(vitx_crossvit, "blob size does not match the CrossViT parameter table")
int32_t vitx_crossvit_forward_dev(vitx_crossvit_handle m, const float* img_dev, int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed,
                                  float* logits_dev_or_null) {
  CAPI_TRY
  if (!m || !img_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = crossvit_forward(m, img_dev, b, H, W, training, seed, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (logits_dev_or_null) CAPI_HIP(hipMemcpyAsync(logits_dev_or_null, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToDevice, m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossvit_forward(vitx_crossvit_handle m, const float* img_host, int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed,
                              float* logits_host) {
  CAPI_TRY
  if (!m || !img_host || !logits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  if (H <= 0 || W <= 0 || H > m->cfg.image_size || W > m->cfg.image_size) return capi_fail(VITX_ERR_INVALID, "image larger than the configured image_size");
  CAPI_HIP(hipMemcpyAsync(m->img, img_host, (size_t)b * H * W * 3 * 4, hipMemcpyHostToDevice, m->stream));
  std::string err;
  int rc = crossvit_forward(m, m->img, b, H, W, training, seed, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  CAPI_HIP(hipMemcpyAsync(logits_host, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToHost, m->stream));
  CAPI_HIP(hipStreamSynchronize(m->stream));
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossvit_backward_dev(vitx_crossvit_handle m, const float* dlogits_dev, float* dimg_dev_or_null) {
  CAPI_TRY
  if (!m || !dlogits_dev) return capi_fail(VITX_ERR_INVALID, "null argument");
  std::string err;
  int rc = crossvit_backward(m, dlogits_dev, dimg_dev_or_null, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  return VITX_OK;
  CAPI_CATCH
}
int32_t vitx_crossvit_backward(vitx_crossvit_handle m, const float* dlogits_host, float* dimg_host_or_null) {
  if (!m || !dlogits_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  return composite_backward_host(m, dlogits_host, dimg_host_or_null, (int64_t)m->H * m->W * 3,
                                 [&](float* dimg_dev, std::string& err) { return crossvit_backward(m, m->dlogits, dimg_dev, err); });
}
// "sm_tokens" / "lg_tokens": the final tokens [b, n, dim] (after the last cross layer); "sm_logits" / "lg_logits": the two heads
int32_t vitx_crossvit_read(vitx_crossvit_handle m, const char* which, float* out_host, int64_t cap, int64_t* n_elems) {
  CAPI_TRY
  if (!m || !which || !out_host) return capi_fail(VITX_ERR_INVALID, "null argument");
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "read requires a preceding forward");
  const std::string w = which;
  const float* src = nullptr;
  int64_t n = 0;
  const size_t L = (size_t)m->cfg.depth - 1;
  if (w == "sm_tokens") { src = m->T[0][L]; n = (int64_t)m->b * m->ntok[0] * m->dim[0]; }
  else if (w == "lg_tokens") { src = m->T[1][L]; n = (int64_t)m->b * m->ntok[1] * m->dim[1]; }
  else if (w == "sm_logits") { src = m->logit_br[0]; n = (int64_t)m->b * m->nc; }
  else if (w == "lg_logits") { src = m->logit_br[1]; n = (int64_t)m->b * m->nc; }
  else return capi_fail(VITX_ERR_INVALID, "unknown tensor name");
  return composite_read_tail(src, n, out_host, cap, n_elems, m->stream);
  CAPI_CATCH
}

}  // extern "C"
