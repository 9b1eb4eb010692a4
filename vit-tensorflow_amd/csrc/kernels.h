// Host-callable launchers of every HIP kernel in libvitx (one translation unit per kernel family).
#pragma once
#include "common.h"
#include "epilogue.h"

// ---------------------------------------------------------------- gemm_generic.hip
struct GenericGemmArgs {
  const void* A = nullptr;
  const void* B = nullptr;
  int M = 0, N = 0, K = 0;
  int64_t sam = 0, sak = 1, sbk = 0, sbn = 1;
  int nb = 1, nh = 1;
  int64_t sAb = 0, sAh = 0, sBb = 0, sBh = 0;
  int k_last = 0;   // > 0: K extent of the LAST batch slice (split-K over the batch index: slices of K rows, the last one shorter); gemm_bf16x3.hip only
  int x3 = 0;   // BF16X3 compute mode: all-fp32 problems run as three bf16 MFMA products of hi / lo split operands (gemm_bf16x3.hip)
};
void launch_gemm_generic(const GenericGemmArgs& g, const EpiParams& ep, int mode, int ta, int tb, int to, hipStream_t s);
// ---------------------------------------------------------------- gemm_f32_mfma.hip
// the same contract on v_mfma_f32_32x32x2_f32 for all-fp32 problems (bit-identical to the scalar kernel: a k-ordered fmaf chain);
// launch_gemm_generic routes to it when supported (VITX_F32_MFMA=0 keeps the scalar kernel)
bool gemm_f32_mfma_supported(const GenericGemmArgs& g, int ta, int tb, int to);
void launch_gemm_f32_mfma(const GenericGemmArgs& g, const EpiParams& ep, int mode, hipStream_t s);
void gemm_f32_mfma_read_env();   // VITX_F32_MFMA, read once per engine handle (not per launch)
// ---------------------------------------------------------------- gemm_bf16x3.hip
// the same contract with every fp32 operand split into bf16 hi + lo and three bf16 MFMA products per k-step (~2^-16 per product);
// launch_gemm_generic routes to it when GenericGemmArgs::x3 is set
bool gemm_bf16x3_supported(const GenericGemmArgs& g, int ta, int tb, int to);
void launch_gemm_bf16x3(const GenericGemmArgs& g, const EpiParams& ep, int mode, hipStream_t s);

// ---------------------------------------------------------------- attn_headchain.hip
// fused head-axis chains (one wave per (image, query) row): CaiT talking heads, DeepViT re-attention, and their VJPs
bool headchain_supported(int h, int nk);
int64_t headchain_ws_elems(int h);
void launch_cait_chain_fwd(const float* s0, const float* wpre, const float* wpost, float* a1_or_null, float* a2, int b, int h, int nq, int nk,
                           int64_t ld, hipStream_t s);
void launch_cait_chain_bwd(const float* s0, const float* a1, float* da_inout, const float* wpre, const float* wpost, float* ws, float* dwpre,
                           float* dwpost, int b, int h, int nq, int nk, int64_t ld, hipStream_t s, bf16_t* ds_lp = nullptr);
bool cait_chain_bwd_bf16_out_ok();
void launch_deepvit_chain_fwd(float* s0_inout, const float* wre, const float* gamma, const float* beta, float* mixed_or_null, float* a2, int keep,
                              int b, int h, int nq, int nk, int64_t ld, float eps, hipStream_t s);
void launch_deepvit_chain_bwd(const float* a0, const float* mixed, float* da_inout, const float* wre, const float* gamma, float* ws, float* dwre,
                              float* dgamma, float* dbeta, int b, int h, int nq, int nk, int64_t ld, float eps, hipStream_t s);

// ---------------------------------------------------------------- attn_bgemm_mfma.hip
// batched small GEMM (M, N, K <= 128 per (image, head)) on MFMA for the materialised attention path in bf16 mode
bool bgemm_mfma_supported(const GenericGemmArgs& g, int ta, int tb, int to, int mode);
void launch_bgemm_mfma(const GenericGemmArgs& g, const EpiParams& ep, int ta, int to, hipStream_t s);
void launch_bgemm_mfma_pair(const GenericGemmArgs& g1, const EpiParams& ep1, int ta1, int to1, const GenericGemmArgs& g2, const EpiParams& ep2, int ta2,
                            int to2, hipStream_t s);   // two products of the same (image, head) back to back in one launch (same nb, nh)

// ---------------------------------------------------------------- gemm_bf16.hip
// C[M,N] = A[M,K] * B[N,K]^T, bf16 operands (K contiguous), fp32 MFMA accumulation.
struct Bf16GemmArgs {
  const bf16_t* A = nullptr;
  const bf16_t* B = nullptr;
  int64_t lda = 0, ldb = 0;
  int M = 0, N = 0, K = 0;   // K multiple of 64; A has >= round_up(M,tile) rows, B >= round_up(N,tile) rows
  int split_k = 1;           // >1: EPI_PARTIAL slices of K/split_k (each a multiple of 64)
  int kernel = 0;            // tile variant: 0 auto, 1 = 128x128 (4 waves), 2 = 256x256 (8 waves), 3 = 256x128
  unsigned long long* stamps = nullptr;   // diagnostics (VITX_GEMM_STAMPS=1 in vitx_bench_gemm): cycle stamps of the tile phases, [256 WGs][16 tiles][4]
  int phase = 0;             // persistent pipelined kernels: workgroup i starts ((i >> 3) & 7) * phase * 4096 cycles late (de-phases the tile loops)
  int reverse_m = 0;         // 1: row tiles are walked from the last to the first (see decode_tile)
  int shared_gpu = 0;        // 1: a collective of this handle may hold CUs while this launch runs (comm_busy): one tile per workgroup instead of a persistent grid
  int walk = 0;              // set by the launcher of the pipelined kernel: 2 = XCD-owned row bands (see gemm_bf16_nt_pipe_kernel)
  int stagger = 0;           // >0: first-wave workgroups start (cu_slot & 3) * stagger * 2048 cycles late (de-phases store-heavy epilogues)
  int tail = 0;              // (round 6) tail balancing: > 0 = tile variant (1 = 128 x 128, 3 = 256 x 128, 10 = 192 x 128) for the rows of the last PARTIAL round of the
                             //   persistent grid, launched on their own behind the full rounds (gemm_bf16.hip: dispatch_gemm_bf16_tail); 0 = one launch
};
void launch_gemm_bf16(const Bf16GemmArgs& g, const EpiParams& ep, int mode, hipStream_t s);
int gemm_bf16_variant_for(int mode, int M, int N, int K, int has_scale, int shared_gpu);   // variant an automatic launch of this shape runs (measured if known, else the static rule)
bool gemm_bf16_gelu_table_active();   // EPI_BIAS_GELU: interior tiles of variant 13 read GELU from the LDS table (VITX_GELU_TABLE)
int gemm_bf16_tile_m(int kernel, int M, int N);
int gemm_bf16_tile_n(int kernel, int M, int N);
int gemm_bf16_num_slices(int K, int split_k);
void gemm_bf16_set_shared_gpu(int on);   // 1: other kernels (collectives) share the CUs -> no persistent variants
void gemm_bf16_allow_320(int on);   // the 320-row tile needs operand/output buffers with 320 spare rows
// weight-gradient form: C[M,N] partials = A[K,M]^T * B[K,N] (A, B row-major with leading dims lda, ldb; K = token rows, multiple of 64)
void launch_gemm_bf16_tn(const Bf16GemmArgs& g, const EpiParams& ep, hipStream_t s);
int gemm_bf16_tn_tile(int kernel, int M, int N);

// ---------------------------------------------------------------- attn_bf16.hip
// fused multi-head self-attention (vit.py:73-82) on packed qkv [b, n, 3, h, 64] bf16.
bool attn_bf16_supported(int n, int dim_head);
// nq_live (both launchers; 0 = n): live-query count.  Forward: only rows < nq_live of o / lse are computed and stored.  Backward: d_o rows >= nq_live
// are taken as zero (those of a live 16-row query block are read, with their o and lse rows, but cannot reach any stored value: they stay in their own
// query column, which is stored as zero and gets no D; the others are not read), the dq rows >= nq_live are written as zeros, dk / dv keep the bits of
// the full launch on such a d_o.
void launch_attn_bf16_fwd(const bf16_t* qkv, bf16_t* o, float* lse, int b, int n, int h, float scale, const bf16_t* zero_page, int reverse,
                          hipStream_t s, int nq_live = 0);   // zero_page: >= 128 B of zeros; reverse: 1 = (image, head) tasks from the last to the first
// attn_x3.hip: the same fused attention on fp32 storage with split-operand (hi + lo) bf16 MFMA products (BF16X3 mode)
bool attn_x3_supported(int n, int dim_head);
void launch_attn_x3_fwd(const float* qkv, float* o, float* lse, int b, int n, int h, float scale, hipStream_t s);
void launch_attn_x3_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, int b, int n, int h, float scale, hipStream_t s);
void launch_attn_bf16_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, float* dsum_ws,
                          bf16_t* dqkv, int b, int n, int h, float scale, const bf16_t* zero_page, hipStream_t s, int nq_live = 0);

// ---------------------------------------------------------------- attn_stream.hip
// the same attention for n > 288 tokens: K / V (backward: also Q / dO) chunks of 64 rows streamed through a double-buffered LDS ring, online softmax;
// same layouts and the same meaning of lse.  LDS per workgroup does not depend on n.  Upper bounds: n <= ATTN_STREAM_MAX_N (supported), and per launch
// b * h <= 65535 with n * 3 * h * 64 < 2^30 elements (31-bit byte offsets) per image (fits); lse and dsum_ws hold b * h * n floats.  No allocation, no host synchronisation.
constexpr int ATTN_STREAM_MAX_N = 1 << 20;
bool attn_stream_supported(int n, int dim_head);
bool attn_stream_fits(int b, int n, int h);
void launch_attn_stream_fwd(const bf16_t* qkv, bf16_t* o, float* lse, int b, int n, int h, float scale, hipStream_t s);
// d(q) (which also writes D = rowsum(dO * O) to dsum_ws), then d(k) / d(v); every row < n of dqkv [b, n, 3, h, 64] is written
void launch_attn_stream_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, float* dsum_ws, bf16_t* dqkv, int b, int n, int h,
                            float scale, hipStream_t s);

// ---------------------------------------------------------------- attn_lsa.hip
// locality self-attention (vit_for_small_dataset.py:88-121) on packed qkv [b, n, 3, h, dh] (fp32 storage: exact fp32 FMA; bf16 storage: every product
// on the bf16 matrix pipe with P / dS rounded to bf16 in front of the second products, fp32 softmax and accumulation): scores scaled by
// exp(*temperature) (a device scalar in the parameter arena), diagonal masked, softmax, P v.  dim_head in {16, 32, 64}, 2 <= n <= LSA_N_MAX.
constexpr int LSA_N_MAX = 288;
bool attn_lsa_supported(int n, int dim_head);
int64_t attn_lsa_ws_elems(int b, int n, int h);   // floats of part_ws (one temperature-gradient partial per workgroup)
void launch_attn_lsa_fwd(const void* qkv, void* o, float* lse, int is_bf16, int b, int n, int h, int dim_head, const float* temperature, hipStream_t s);
// dsum_ws: b * h * n floats; *dtemperature is overwritten (fixed-order two-pass sum)
void launch_attn_lsa_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* dsum_ws, void* dqkv, int is_bf16, int b, int n, int h,
                         int dim_head, const float* temperature, float* dtemperature, float* part_ws, hipStream_t s);
// plain small-head attention (nest.py:93-109): the same kernels compiled without the diagonal mask and the temperature, softmax scale by value;
// dim_head in {16, 32}, 1 <= n <= LSA_N_MAX
bool attn_small_supported(int n, int dim_head);
// bias: optional fp32 [n, n] added to the scaled scores (dim_head 32 only; crossformer.py:165)
// bias_hs: element stride between the heads' planes of a per-head bias [h, n, n] (regionvit.py:154); 0: one [n, n] plane for every head
void launch_attn_small_fwd(const void* qkv, void* o, float* lse, int is_bf16, int b, int n, int h, int dim_head, float scale, hipStream_t s,
                           const float* bias = nullptr, int64_t bias_hs = 0);
void launch_attn_small_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* dsum_ws, void* dqkv, int is_bf16, int b, int n, int h,
                           int dim_head, float scale, hipStream_t s, const float* bias = nullptr, int64_t bias_hs = 0);
// attn_window.hip -- biased attention of tiny windows (crossformer.py:149-172): bf16 storage, dim_head 32, 1 <= n <= 64; one wave per (sequence, head);
// s = scale q k^T + bias[n, n] (fp32), softmax, P v on the packed qkv [b, n, 3, h, 32] and its VJP (d(q, k, v) written by the same wave: no workspace)
bool attn_window_supported(int n, int dim_head);
// bias_hs != 0: a per-head bias [h, n, n]; a workgroup then stays on one head (its LDS holds one plane, as with the shared bias)
void launch_attn_window_fwd(const bf16_t* qkv, bf16_t* o, float* lse, const float* bias, int b, int n, int h, float scale, hipStream_t s, int64_t bias_hs = 0);
void launch_attn_window_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dqkv, const float* bias, int b, int n, int h,
                            float scale, hipStream_t s, int64_t bias_hs = 0);
// d(bias) of a learned bias (attn_lsa.hip; both families, fp32 or bf16 storage, dim_head 32, n <= LSA_N_MAX): dbias_acc [h, n, n] += the sum over the
// b sequences of dS = P o (dP - rowsum(dO o O)), P recomputed from lse; per-slice partials in ws (attn_dbias_ws_elems floats), summed in slice order
int64_t attn_dbias_ws_elems(int b, int n, int h);
void launch_attn_dbias(const void* qkv, const void* o, const void* d_o, const float* lse, int is_bf16, int b, int n, int h, float scale, const float* bias,
                       int64_t bias_hs, float* ws, float* dbias_acc, hipStream_t s);
// regionvit_ops.hip -- RegionViT (regionvit.py) outside its transformer blocks
// tokens[(b wy wx), 0, c] = region[b, wy, wx, c]; tokens[(b wy wx), 1 + p1 ww + p2, c] = local[b, wy wh + p1, wx ww + p2, c] (:163-168) and the split
// back (:175-177); each is the other's VJP
void launch_rv_join(const float* region, const float* local, float* tokens, int b, int rh, int rw, int wh, int ww, int c, hipStream_t s);
void launch_rv_split(const float* tokens, float* region, float* local, int b, int rh, int rw, int wh, int ww, int c, hipStream_t s);
// bias[h, 1 + i, 1 + j] = table[(dh + ws - 1) + (dw + ws - 1)(2 ws - 1), h] for tokens i, j of a wh x ww window, row 0 and column 0 zero (:144-155);
// dtable[idx, h] = the sum of dbias[h, 1 + i, 1 + j] over the pairs with that index, in (y, x) order; an index no pair has gets 0
void launch_rv_bias_build(const float* table, float* bias, int ws, int wh, int ww, int heads, hipStream_t s);
void launch_rv_table_grad(const float* dbias, float* dtable, int ws, int wh, int ww, int heads, hipStream_t s);
void launch_rv_add(float* dst, const float* src, int64_t n, hipStream_t s);   // dst += src
// exact GELU (:28) on fp32 and its VJP (dx = dy * gelu'(x))
void launch_rv_gelu_fwd(const float* x, float* y, int64_t n, hipStream_t s);
void launch_rv_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, hipStream_t s);
// crossformer_ops.hip -- CrossFormer (crossformer.py) outside its transformer blocks
// tokens[(b h w), (l1 l2), c] = x[b, l1 * (H / g) + h, l2 * (W / g) + w, c] ('b (l1 h) (l2 w) d -> (b h w) l1 l2 d', :146) and its inverse (:178);
// each is the other's VJP
void launch_cf_to_dilated(const float* x, float* tokens, int b, int H, int W, int g, int c, hipStream_t s);
void launch_cf_from_dilated(const float* tokens, float* x, int b, int H, int W, int g, int c, hipStream_t s);
// DynamicPositionBias (:51-71) of one attention on its (2 wsz + 1)^2 positions and the [n, n] gather through rel_pos_indices (:126-131,159-163),
// fp32 in every compute mode.  t: the 14 dpb tensors of the attention in table order -- (kernel, bias, gamma, beta) x 3, then kernel [d4, 1], bias [1].
// ws: cf_dpb_ws_elems floats (the network's output per position); bias: [wsz^2, wsz^2].
struct CfDpbParams { const float* t[14]; };
int64_t cf_dpb_ws_elems(int wsz);
void launch_cf_dpb_bias(const CfDpbParams& p, int d4, int wsz, float* ws, float* bias, hipStream_t s);
// dst[r, col0 : col0 + w] = src[r, 0 : w] (put) / dst[r, 0 : w] = src[r, col0 : col0 + w] (get): one scale's column block of the stage input
void launch_cf_cols_put(const float* src, float* dst, int64_t rows, int w, int ld, int col0, hipStream_t s);
void launch_cf_cols_get(const float* src, float* dst, int64_t rows, int w, int ld, int col0, hipStream_t s);

// ---------------------------------------------------------------- spt.hip
// shifted patch tokenization (vit_for_small_dataset.py:15-47,142-157): NHWC image -> LayerNorm'ed rows [b * np, 5 p p C] of the image concatenated
// with its four one-pixel shifts (zero fill), unfolded; the shifted copies are index arithmetic on the one image.  mean / rstd: fp32 per row.
void launch_spt_fwd(const float* img, void* rows, int rows_bf16, int64_t ldo, float* mean, float* rstd, const float* gamma, const float* beta, int b,
                    int H, int W, int C, int p, float eps, hipStream_t s);
int64_t spt_bwd_ws_elems(int feat);
// LayerNorm VJP of the rows: d_rows [b * np, feat] (fp32, row stride ld) is replaced IN PLACE by the gradient of the un-normalised rows when
// want_dx; dgamma / dbeta through partial rows in ws and a fixed-order second pass.
void launch_spt_bwd(const float* img, float* d_rows, int64_t ld, const float* mean, const float* rstd, const float* gamma, float* ws, float* dgamma,
                    float* dbeta, int want_dx, int b, int H, int W, int C, int p, hipStream_t s);
// dimg[b, y, x, c] = the at most five entries of dx that read that pixel (gather: deterministic)
void launch_spt_dimg(const float* dx, int64_t ld, float* dimg, int b, int H, int W, int C, int p, hipStream_t s);

// ---------------------------------------------------------------- cct_tok.hip
// CCT tokenizer behind the convolution (cct.py:196-200): out = MaxPool2D(k, st, 'SAME')(ReLU(conv)), conv [b, H, W, C] NHWC, out [b, ceil(H/st), ceil(W/st), C]
// im2col rows [b * oh * ow, Kp] of a 'SAME' convolution (row order (ky, kx, c)); Kp >= k * k * C, columns beyond it are written as zeros
void launch_cct_im2col(const float* x, float* rows, int b, int H, int W, int C, int k, int st, int Kp, hipStream_t s);
void launch_cct_relu_maxpool_fwd(const float* conv, float* out, int b, int H, int W, int C, int k, int st, hipStream_t s);
// its VJP in gather form (every element of dconv written; first maximum in row-major window order takes a window; no atomics)
void launch_cct_relu_maxpool_bwd(const float* conv, const float* dout, float* dconv, int b, int H, int W, int C, int k, int st, hipStream_t s);

// ---------------------------------------------------------------- nest_ops.hip
// NesT (nest.py:137-148,207-212): block partition fused with the positional add, its inverse, their VJPs, and the plain 'SAME' max-pool
// tokens[(b b1 b2), (h w), c] = x[b, (b1 h), (b2 w), c] + pos[h * w_ + w]   (x: [b, nb * hb, nb * wb, c]; pos == nullptr: the pure copy)
// nbx > 0: a rectangular grid of nb x nbx blocks (twins_svt.py:141,153: '(b x y) p1 p2 c' windows of a rectangular map); 0: nb x nb
void launch_nest_to_blocks(const float* x, const float* pos, float* tokens, int b, int nb, int hb, int wb, int c, hipStream_t s, int nbx = 0);
// x[b, (b1 h), (b2 w), c] = tokens[(b b1 b2), (h w), c]
void launch_nest_from_blocks(const float* tokens, float* x, int b, int nb, int hb, int wb, int c, hipStream_t s, int nbx = 0);
// d(pos)[j] = sum over sequences and channels of dtokens[seq, j, :]: one partial row per sequence (part: [nseq, n]), then launch_sum_rows
void launch_nest_dpos(const float* dtokens, float* part, float* dpos, int nseq, int n, int c, hipStream_t s);
// MaxPool2D(padding='SAME') on a signed input (the running maximum starts at -inf; taps outside the map never win) and its gather-form VJP
// (every element of dx written; the first maximum in row-major window order takes the window's gradient; no atomics)
void launch_nest_maxpool_fwd(const float* x, float* out, int b, int H, int W, int C, int k, int st, hipStream_t s);
void launch_nest_maxpool_bwd(const float* x, const float* dout, float* dx, int b, int H, int W, int C, int k, int st, hipStream_t s);

// ---------------------------------------------------------------- attn_fewkey.hip
// softmax(q k^T scale) v of nq queries against nk <= 64 keys per (image, head), dim_head 64, bf16 storage, MFMA products, no score tensor:
// q [b, nq, ldq], kv [b, nk, ldkv] = [k | v] (v at column heads * 64), o [b, nq, ldo], lse [b, heads, nq]; the VJP writes dq [b, nq, lddq] and
// dkv [b, nk, lddkv] = [dk | dv] (one workgroup per (image, head): no second pass)
bool attn_fewkey_supported(int nq, int nk, int dim_head);
void launch_attn_fewkey_fwd(const bf16_t* q, const bf16_t* kv, bf16_t* o, float* lse, int b, int nq, int nk, int heads, int64_t ldq, int64_t ldkv,
                            int64_t ldo, float scale, hipStream_t s);
void launch_attn_fewkey_bwd(const bf16_t* q, const bf16_t* kv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dq, bf16_t* dkv, int b, int nq,
                            int nk, int heads, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddkv, float scale, hipStream_t s);

// 64 < nk <= MANYKEY_MAX keys (cvt.py:120-123), same layouts and lse: the forward keeps all of K and V in LDS and walks 64-key chunks with an
// online softmax; the VJP is two launches -- d(k) / d(v) per 64-key chunk (the few-key kernel with a key offset), then d(q) with all keys in LDS.
// MANYKEY_MAX is what the d(q) kernel's K, V and K^T fit of the 160 KiB of LDS (attn_fewkey.hip asserts it).
constexpr int MANYKEY_MAX = 320;
bool attn_manykey_supported(int nq, int nk, int dim_head);
void launch_attn_manykey_fwd(const bf16_t* q, const bf16_t* kv, bf16_t* o, float* lse, int b, int nq, int nk, int heads, int64_t ldq, int64_t ldkv,
                             int64_t ldo, float scale, hipStream_t s);
void launch_attn_manykey_bwd(const bf16_t* q, const bf16_t* kv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dq, bf16_t* dkv, int b, int nq,
                             int nk, int heads, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddkv, float scale, hipStream_t s);

// ---------------------------------------------------------------- twins_ops.hip
// TwinsSVT PatchEmbedding's Rearrange (twins_svt.py:103): out[(b h w), (c p1 p2)] = x[b, h p + p1, w p + p2, c] (row stride ld), and its VJP,
// the inverse permutation (every element of dx written)
void launch_twins_patch_gather(const float* x, float* out, int b, int H, int W, int C, int p, int64_t ld, hipStream_t s);
void launch_twins_patch_scatter(const float* dpatches, int64_t ld, float* dx, int b, int H, int W, int C, int p, hipStream_t s);
// rows of the non-overlapping k x k windows of x [b, H, W, C] in (p1 p2 c) order, one row per window (row stride ldo >= k k C), on fp32 or
// bf16 storage; the VJP ADDS d(windows) into dx [b, H, W, C].  H and W are multiples of k.
void launch_twins_kunfold(const void* x, void* out, int is_bf16, int b, int H, int W, int C, int k, int64_t ldo, hipStream_t s);
void launch_twins_kfold_add(const void* dwin, int64_t ld, void* dx, int is_bf16, int b, int H, int W, int C, int k, hipStream_t s);
// PEG (twins_svt.py:108-115): out = x + bias + depthwise 'SAME' convolution of x with kern [kp, kp, 1, C] (kp odd), NHWC fp32; its VJPs:
// dx = dy + correlation of dy with the flipped kernel; dkern [kp, kp, 1, C] as partials over fixed pixel slices (ws: twins_peg_ws_elems
// floats) summed in order.  d(bias) is launch_colsum of dy.
void launch_twins_peg_fwd(const float* x, const float* kern, const float* bias, float* out, int b, int H, int W, int C, int kp, hipStream_t s);
void launch_twins_peg_bwd_dx(const float* dy, const float* kern, float* dx, int b, int H, int W, int C, int kp, hipStream_t s);
int64_t twins_peg_ws_elems(int C, int kp);
void launch_twins_peg_bwd_dkern(const float* x, const float* dy, float* ws, float* dkern, int b, int H, int W, int C, int kp, hipStream_t s);

// ---------------------------------------------------------------- cvt_ops.hip
// CvT's convolutional projection in front of its pointwise Dense (cvt.py:84-85): depthwise Conv2D(k, stride st, 'SAME', no bias) with kern
// [k, k, 1, C] on x [b, H, W, C] NHWC in the storage type, then BatchNormalization over all b * oh * ow positions.  conv [b, oh, ow, C] (fp32)
// and stats [2 C] = (mean | rstd) (double, as every sum behind them) are kept for the VJP; y [b * oh * ow, ldy] is the normalised result in the storage type.  training == 0
// normalises with mov_mean / mov_var.  ws: cvt_dwbn_ws_elems floats.  Every sum is fixed-slice partials added in order (no atomics).
int64_t cvt_dwbn_ws_elems(int C, int k);
void launch_cvt_dwbn_fwd(const void* x, int is_bf16, const float* kern, const float* gamma, const float* beta, const float* mov_mean, const float* mov_var,
                         int training, float eps, float* conv, double* stats, void* y, int64_t ldy, float* ws, int b, int H, int W, int C, int k, int st,
                         hipStream_t s);
// BatchNorm VJP on batch statistics: dgamma = sum dy xhat, dbeta = sum dy, dconv = gamma rstd (dy - dbeta / N - xhat dgamma / N) (fp32)
void launch_cvt_bn_bwd(const void* dy, int is_bf16, int64_t lddy, const float* conv, const double* stats, const float* gamma, float* dgamma, float* dbeta,
                       float* dconv, float* ws, int64_t rows, int C, hipStream_t s);
// d(kern) [k, k, 1, C] from the convolution's input and dconv
void launch_cvt_dw_bwd_dkern(const void* x, int is_bf16, const float* dconv, float* ws, float* dkern, int b, int H, int W, int C, int k, int st, hipStream_t s);
// d(x) [b, H, W, C] in the storage type, every element written once: the q projection's share (stride 1) plus the kv projection's (stride st_kv)
void launch_cvt_dw_bwd_dx(const float* dconv_q, const float* kern_q, const float* dconv_kv, const float* kern_kv, int st_kv, void* dx, int is_bf16, int b, int H,
                          int W, int C, int k, hipStream_t s);

// ---------------------------------------------------------------- pit_ops.hip
// PiT (pit.py) on fp32 token rows [b, 1 + h w, d], row 0 the class token; 32-bit index arithmetic: the caller checks pit_ops_fits(elements) of
// every tensor it passes.  Buffers that feed a GEMM over token rows keep a row 0 of zeros per image.
bool pit_ops_fits(int64_t elems);
// Unfold (pit.py:110-122): rows [b, 1 + oh ow, Kp] (Kp a multiple of 4, columns past p p C zeros, row 0 zeros) of the p x p patches every st pixels
// ('VALID') in (kh, kw, c) order; its VJP gathers for every pixel the patches that cover it (every element of dimg written once)
void launch_pit_unfold(const float* img, float* rows, int b, int H, int W, int C, int p, int st, int oh, int ow, int Kp, hipStream_t s);
void launch_pit_unfold_bwd(const float* drows, float* dimg, int b, int H, int W, int C, int p, int st, int oh, int ow, int Kp, hipStream_t s);
// x[bi, 0] = cls + pos[0], x[bi, r] += pos[r] (pit.py:211-213); dpos [pos_rows, d] = the sum over the images of g (rows >= n zeros), dcls = dpos[0]
void launch_pit_cls_pos(float* x, const float* cls, const float* pos, int b, int n, int d, hipStream_t s);
void launch_pit_pos_grad(const float* g, float* dpos, float* dcls, int b, int n, int pos_rows, int d, hipStream_t s);
// out[c] = sum over the images and the rows 1 .. ntok - 1 of v[bi, row, c], as fixed-slice partials (ws: pit_rowsum_ws_elems floats) added in order
int64_t pit_rowsum_ws_elems(int C);
void launch_pit_rowsum(const float* v, float* ws, float* out, int b, int ntok, int C, hipStream_t s);
// Pool's depthwise Conv2D(2 d, 3, strides 2, 'SAME', groups = d) with bias (pit.py:130,143) on rows 1.. of x read as the h x w map: dw
// [b, 1 + oh ow, 2 d] with row 0 zeros; d(kernel) [3, 3, 1, 2 d] and d(bias) from x and d(dw) (ws: pit_pool_ws_elems floats); rows 1.. of d(x)
int64_t pit_pool_ws_elems(int d);
void launch_pit_pool_dw_fwd(const float* x, const float* kern, const float* bias, float* dw, int b, int h, int w, int d, hipStream_t s);
void launch_pit_pool_dw_bwd_params(const float* x, const float* ddw, float* ws, float* dkern, float* dbias, int b, int h, int w, int d, hipStream_t s);
void launch_pit_pool_dw_bwd_dx(const float* ddw, const float* kern, float* dx, int b, int h, int w, int d, hipStream_t s);

// ---------------------------------------------------------------- elementwise.hip
void launch_unfold(const float* img, void* out, int out_bf16, int b, int H, int W, int C, int ph, int pw,
                   int64_t ldo, hipStream_t s);
void launch_fold_add(const float* dpatches, int64_t ld, float* dimg, int b, int H, int W, int C, int ph, int pw, hipStream_t s);
// tf.image.extract_patches(..., rates 1, padding 'SAME') (t2t.py:42) and its VJP; out [b, ceil(H/st), ceil(W/st), k*k*C]
void extract_patches_geometry(int H, int W, int k, int st, int* oh, int* ow, int* pad_top, int* pad_left);
void launch_extract_patches(const float* x, float* out, int b, int H, int W, int C, int k, int st, hipStream_t s);
void launch_extract_patches_bwd(const float* dout, float* dx, int b, int H, int W, int C, int k, int st, hipStream_t s);
void launch_cls_pos_row(float* x, const float* cls, const float* pos, int b, int ntok, int d, int64_t ldx, hipStream_t s);
void launch_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int y_bf16,
                          int64_t ldy, float* mean, float* rstd, int rows, int d, float eps, hipStream_t s);
// g_out = (g_in ? g_in : 0) + LN_bwd(dy); optional low-precision copy of g_out; dgamma/dbeta via partial_ws
void launch_layernorm_bwd(const void* dy, int dy_bf16, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                          const float* rstd, const float* gamma, const float* g_in, int64_t ldgi, float* g_out, int64_t ldgo,
                          void* g_lp, int64_t ldglp, float* partial_ws, float* dgamma, float* dbeta, float* gsum, int rows, int d,
                          hipStream_t s, int* deferred = nullptr);   // gsum (optional): column sums of g_in; deferred: see the definition
void launch_layernorm_bwd_reduce(float* partial_ws, int nparts, int d, float* dgamma, float* dbeta, float* gsum, hipStream_t s);
int64_t layernorm_bwd_ws_elems(int d);
// LayerNorm VJP that also runs the LayerScale VJP of the branch consuming its result (bf16 mode, CaiT): dbr = g_out * nscale, partial rows for
// d nscale = colsum(g_out * nf) and that branch's bias gradient nscale * colsum(g_out); the caller runs the reduction on a stream of its choice
bool layernorm_bwd_scale_ok(int d);   // (every operand 16-B aligned with row strides that are multiples of 4: true of the engine's own buffers)
void launch_layernorm_bwd_scale(const bf16_t* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                const float* g_in, int64_t ldgi, float* g_out, int64_t ldgo, bf16_t* dbr, int64_t lddbr, const bf16_t* nf, int64_t ldnf,
                                const float* nscale, float* partial_ws, int rows, int d, hipStream_t s, int* nparts);
void launch_layernorm_bwd_scale_reduce(float* partial_ws, int nparts, int d, float* dgamma, float* dbeta, float* dscale, float* dbias, const float* nscale,
                                       hipStream_t s);
void launch_colsum(const void* x, int is_bf16, int64_t ld, int rows, int cols, float* partial_ws, float* out, hipStream_t s);
int64_t colsum_ws_elems(int cols);
void launch_reduce_partials(const float* partial, int nparts, int64_t stride, int64_t n, float* out, float alpha, hipStream_t s);
void launch_reduce_partials3(const float* partial, int nparts, int64_t stride, int64_t seg, int nseg, float* out0, float* out1, float* out2,
                             float* ws2, float alpha, hipStream_t s);
void launch_convert_weight(const float* w, int in, int out, bf16_t* wn, int64_t ldwn, bf16_t* wt, int64_t ldwt, hipStream_t s);
// one table entry per Dense kernel; block0 = first block of this matrix in the batched launch (tiles of 64 x 64, tiles_x = ceil(out / 64))
struct ConvertDesc { const float* w; bf16_t* wn; bf16_t* wt; int64_t ldwn, ldwt; int in, out, tiles_x, block0; };
void launch_convert_weights_batched(const ConvertDesc* descs_dev, int n, int total_blocks, hipStream_t s);
void launch_transpose_bf16(const bf16_t* in, int64_t ldi, int rows, int cols, bf16_t* out, int64_t ldo, hipStream_t s);
void launch_convert(const float* in, int64_t ldi, void* out, int out_bf16, int64_t ldo, int rows, int cols, int64_t out_cols_zero_to,
                    hipStream_t s);
void launch_to_f32(const void* in, int in_bf16, int64_t ldi, float* out, int64_t ldo, int rows, int cols, hipStream_t s);
void launch_set_token_row(float* x, const float* tok, int b, int ntok, int row, int d, hipStream_t s);   // x[b, row, :] = tok[:]
// dst[r][0 : row_bytes) = src[r][0 : row_bytes) for r < rows, rows at independent strides (row_bytes, both strides and both pointers multiples of 16 B):
// the gather (class row of every image -> compact [b, *]) and the scatter (back) of the last block's class-row form
void launch_copy_rows(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes, int rows, int row_bytes, hipStream_t s);
void launch_mean_pool(const float* x, int b, int ntok, int d, float* out, hipStream_t s, int stride_tok = 0);   // stride_tok: rows per image in memory (0 = ntok)
void launch_mean_pool_bwd(const float* dp, int b, int ntok, int d, float* g, hipStream_t s, int stride_tok = 0);   // rows >= ntok of an image are left alone
void launch_batch_reduce(const float* g, int b, int ntok, int d, int j0, int nj, float* out, hipStream_t s);  // out[j][c] = sum_b g[b][j0+j][c]
void launch_extract_rows(const float* g, int b, int ntok, int tok_off, int np, int d, void* out, int out_bf16, int64_t ldo, hipStream_t s);
void launch_sum_rows(const float* in, int rows, int d, float* out, hipStream_t s);  // out[c] = sum_r in[r][c] (small)
void launch_ce_grad(const float* logits, int64_t ld, const int32_t* labels, int b, int nc, float inv_batch, float* dlogits,
                    float* loss, hipStream_t s);
void launch_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, int step, hipStream_t s);
void launch_sgd(float* p, const float* g, float* m, int64_t n, float lr, float mom, float wd, hipStream_t s);   // m may be null (plain SGD)
void launch_fill_zero(void* p, int64_t bytes, hipStream_t s);   // bytes multiple of 16
void launch_fill_random_bf16(bf16_t* p, int64_t n, uint32_t seed, float scale, hipStream_t s);
// *out_max (zero it first) = max(*out_max, max |a - b| / (1 + |b|)) over [rows, cols]; +inf when a NaN is met (GEMM self-checks at full size)
void launch_max_rel_diff(const void* a, const void* b, int is_bf16, int64_t rows, int cols, int64_t lda, int64_t ldb, float* out_max, hipStream_t s);
void launch_dropout(void* x, int is_bf16, int64_t n, float rate, uint64_t seed, uint32_t site, hipStream_t s);
void launch_axpy_resid(const float* resid, const float* f, const float* scale, float* out, void* keep, int keep_bf16, int64_t rows, int d,
                       hipStream_t s);   // out = resid + f*scale[col]; keep[T] = f
void launch_branch_grad(const float* g, const float* scale, void* out, int out_bf16, int64_t rows, int d, float rate, uint64_t seed,
                        uint32_t site, hipStream_t s);   // out[T] = dropout_mask(g*scale[col])
void launch_resid_add(const float* resid, const void* t, int t_bf16, float* out, int64_t n, hipStream_t s);  // out = resid + t

// ---------------------------------------------------------------- attn_generic.hip (materialised attention pieces)
void launch_softmax_rows(float* sc, int64_t rows, int n, int64_t ld, hipStream_t s);
void launch_softmax_bwd_rows(const float* p, float* dp_inout, int64_t rows, int n, int64_t ld, hipStream_t s);
// DeepViT forward chain (softmax -> re-attention mix -> LayerNorm over heads) as row statistics + one fused point kernel
int64_t deepvit_point_bwd_ws_elems(int h);
void launch_deepvit_point_bwd(const float* a0, float* da_inout, const float* w, const float* gamma, float* ws, float* dw,
                              float* dgamma, float* dbeta, int b, int h, int nq, int nk, int64_t ld, float eps, hipStream_t s);
// attn_deepvit_fused.hip: the whole Re-attention forward (deepvit.py:79-88) in one kernel, bf16 mode, nk <= 80
bool deepvit_attn_fused_supported(int h, int dim_head, int nq, int nk);
// cait.py:121-128 forward in one kernel (attn_cait_fused.hip): raw scaled scores / softmax / mixed softmax are written (fp32 [b][h][nq][ld]) only when keep
bool cait_attn_fused_supported(int h, int dim_head, int nq, int nk);
void launch_cait_attn_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ldq, int64_t ldk, int64_t ldv, int64_t qb, int64_t kb, int64_t vb,
                          bf16_t* o, int64_t ldo, int64_t ob, const float* wpre, const float* wpost, float* s0_keep, float* a1_keep, float* a2_keep,
                          int keep, int b, int h, int nq, int nk, int64_t ld, float scale, const bf16_t* zero_page, hipStream_t s);
// the VJP of the same chain up to d(q) in one kernel (d(dots) leaves as fp32 for the d(k) product; P = what the fused forward kept)
int64_t deepvit_attn_bwd_ws_elems(int b, int h, int nq);
void launch_deepvit_attn_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ldq, int64_t ldk, int64_t ldv, int64_t qb, int64_t kb, int64_t vb,
                             const bf16_t* d_o, int64_t ldo, int64_t ob, const float* p_keep, const float* w, const float* gamma, float* ds_out,
                             bf16_t* dq, int64_t lddq, int64_t dqb, float* ws, float* dw, float* dgamma, float* dbeta, int b, int h, int nq, int nk,
                             int64_t ld, float scale, float eps, const bf16_t* zero_page, hipStream_t s, int ds_bf16 = 0);
void launch_deepvit_attn_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ldq, int64_t ldk, int64_t ldv, int64_t qb,
                             int64_t kb, int64_t vb, bf16_t* o, int64_t ldo, int64_t ob, const float* w, const float* gamma,
                             const float* beta, float* p_keep, float* a2_keep, int keep, int b, int h, int nq,
                             int nk, int64_t ld, float scale, float eps, const bf16_t* zero_page, hipStream_t s);
bool deepvit_point_fwd_supported(int h, int nk);
int64_t deepvit_point_ws_elems(int b, int h, int nq);
void launch_deepvit_point_fwd(float* s0_inout, float* stats_ws, const float* w, const float* gamma, const float* beta, float* mixed, float* a2,
                              int keep, int b, int h, int nq, int nk, int64_t ld, float eps, hipStream_t s);
// talking-heads style mix over the head axis of [b, h, nq, ld]: out[b,g,i,j] = sum_h in[b,h,i,j] * W[h,g]
void launch_headmix_fwd(const float* in, const float* w, float* out, int b, int h, int nq, int nk, int64_t ld, hipStream_t s);
// din[b,h,i,j] = sum_g dout[b,g,i,j] W[h,g];  dW[h,g] = sum_{b,i,j} in[b,h,i,j] dout[b,g,i,j]
void launch_headmix_bwd(const float* in, const float* dout, const float* w, float* din, float* dw_partial_ws, float* dw,
                        int b, int h, int nq, int nk, int64_t ld, hipStream_t s);
int64_t headmix_ws_elems(int b, int h, int nq, int nk);
// LayerNorm over the head axis at every (b,i,j)  (deepvit.py:59-63)
void launch_headnorm_fwd(const float* in, const float* gamma, const float* beta, float* out, int b, int h, int nq, int nk,
                         int64_t ld, float eps, hipStream_t s);
void launch_headnorm_bwd(const float* in, const float* dout, const float* gamma, float* din, float* partial_ws, float* dgamma,
                         float* dbeta, int b, int h, int nq, int nk, int64_t ld, float eps, hipStream_t s);
// ctx[b, 0:nq] = y[b]; ctx[b, nq:nq+nc] = context[b]   (cait.py:109-112), T-typed output
void launch_concat_ctx(const void* y, int y_bf16, const float* context, void* ctx, int ctx_bf16, int b, int nq, int nc, int d,
                       hipStream_t s);
// split d(ctx) [b, nq+nc, d] (T) back: dy_add[b, 0:nq] (T, overwritten) and dcontext[b, 0:nc] += (fp32 accumulate)
void launch_split_ctx_bwd(const void* dctx, int is_bf16, void* dy, float* dcontext, int b, int nq, int nc, int d, hipStream_t s);
void launch_add_T(void* a_inout, const void* b_in, int is_bf16, int64_t n, hipStream_t s);
void launch_scale_grad(const void* fx, int is_bf16, int64_t ldf, const float* g, int64_t ldg, int rows, int d, float* partial_ws,
                       float* dscale, hipStream_t s, const float* scale_or_null = nullptr, void* out_or_null = nullptr, int64_t ldo = 0,
                       float* dbias_or_null = nullptr);   // dbias (with out): += nothing, = column sums of out (the bias gradient of the Dense in front of the LayerScale)  // dscale[c] = sum_r g[r][c]*fx[r][c]   (cait.py:47-48 VJP)
void launch_mul_scale(const float* g, int64_t ldg, const float* scale, void* out, int out_bf16, int64_t ldo, int rows, int d,
                      hipStream_t s);          // out[T] = g * scale[col]
void launch_broadcast_rows(const float* src, int d, float* dst, int rows, hipStream_t s);  // dst[r][:] = src[:]

// ---------------------------------------------------------------- mim_ops.hip (MAE / SimMIM index, masking and loss kernels)
// idx: int32 [b, ldi]; inv: int32 [b, n] with inv[b, idx[b, j]] = j for j in [j0, j1), -1 elsewhere
void launch_index_inverse(const int32_t* idx, int64_t ldi, int b, int j0, int j1, int n, int32_t* inv, hipStream_t s);
// out[b, j, :] = src[b * src_batch_stride + idx[b, j0 + j] * d + :], j < k   (src_batch_stride = 0: one table for every image)
void launch_gather_rows(const float* src, int64_t src_batch_stride, const int32_t* idx, int64_t ldi, int j0, int b, int k, int d, float* out,
                        hipStream_t s);
// dst[b, t, :] = inv[b, t] in [j0, j1) ? src[b, inv[b, t] - j0, :] : 0        (src: [b, k_src, d], dst: [b, n, d])
void launch_scatter_rows(const float* src, int k_src, const int32_t* inv, int j0, int j1, int b, int n, int d, float* dst, hipStream_t s);
// dtab[t, :] (= | +=) sum_b (inv[b, t] in [j0, j1) ? src[b, inv[b, t] - j0, :] : 0)
void launch_table_grad(const float* src, int k_src, const int32_t* inv, int j0, int j1, int b, int n, int d, int accumulate, float* dtab,
                       hipStream_t s);
void launch_mae_assemble(const float* proj, const float* mask_token, const float* dpos, const int32_t* idx, int b, int np, int nm, int d, float* out,
                         hipStream_t s);
void launch_select_rowsum(const float* x, const int32_t* inv_or_null, int j0, int j1, int b, int n, int d, float* partial_ws, float* out,
                          hipStream_t s);   // partial_ws: b * d floats
void launch_simmim_select(float* x, const int32_t* inv, const float* mask_token, const float* pos, int b, int n, int d, hipStream_t s);
void launch_zero_selected_rows(float* x, const int32_t* inv, int64_t rows, int d, hipStream_t s);
void launch_scatter_by_index(const float* src, const int32_t* idx, int b, int k, int d, float* dst, int64_t dst_batch_stride, int row0, hipStream_t s);
void launch_mpp_labels(const float* img, int b, int H, int W, int C, int p, int bits, float mpv, int has_norm, const float* mean, const float* std_,
                       const int32_t* idx, int k, int32_t* labels, hipStream_t s);
int64_t recon_loss_ws_elems(int64_t count);
// kind 0: squared, 1: absolute; loss_out = scale * sum f(pred - target), dpred = scale * f'(pred - target); target may be null (= 0)
void launch_recon_loss(const float* pred, const float* target_or_null, int64_t count, int kind, float scale, float* dpred, float* partial_ws,
                       float* loss_out, hipStream_t s);
