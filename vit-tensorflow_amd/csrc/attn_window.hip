// Biased window attention for tiny windows (crossformer.py:149-172): bf16 storage, dim_head 32, 1 <= n <= 64 tokens, on the engine's packed
// qkv [b, n, 3, h, 32] / o [b, n, h * 32] rows:
//   S = scale q k^T + bias,  P = softmax(S),  o = P v            dS = P o (dP - rowsum(dO o O)),  dq = scale dS k,  dk = scale dS^T q,  dv = P^T dO
// A CrossFormer step has tens of thousands of (window, head) problems, each far too small for a workgroup.  Here ONE WAVE owns a whole
// (window, head): dim_head 32 is exactly one K extent of v_mfma_f32_16x16x32_bf16, so a 16 x 16 score tile is one MFMA.  A workgroup of four
// waves walks a list of problems (p = (k * gridDim.x + blockIdx.x) * 4 + wave); the [n, n] fp32 bias is staged once per workgroup in LDS.
// v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + 0..7], B[k = 8 (l >> 4) + 0..7][col l & 15] and
// C[row 4 (l >> 4) + r][col l & 15].  Q, K (forward) and Q, K, V, dO, O (backward) fragments come straight from global memory, one row per
// lane; the second product's operands go through two per-wave LDS tiles: X [n32][n32 + 8] (P, dS, dS^T, P^T as the A operand) and
// Y [32][n32 + 8] (V, K, Q, dO transposed as the B operand), n32 = 32 or 64 (a template parameter: every tile loop unrolls).  The backward
// keeps P and dS in registers and runs its three output products one after the other through the same two tiles, so the wave writes dq, dk, dv
// of its window itself: no cross-wave reduction, no second pass, no partials, the same bits every run.
// Masking, not padding: rows and columns >= n are selected to zero / -inf, never read from memory, and every LDS tile is written in full before
// it is read; nothing depends on what a buffer holds beyond n.
// LDS per workgroup: n^2 * 4 B of bias + 4 waves x (n32 + 32) x (n32 + 8) x 2 B: 70 KiB at 33..64 tokens (two workgroups, 8 waves per CU), 24 KiB
// at most up to 32 tokens.  Per-wave tiles need no workgroup barrier inside the problem loop: the waves may run different trip counts.
#include <algorithm>

#include "kernels.h"

namespace {

constexpr int AW_WAVES = 4;

// orders this wave's LDS writes before its later reads of them (another lane's data): the LDS queue of a wave is in order, the compiler is told
__device__ __forceinline__ void aw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bf16x8 aw_zero8() {
  bf16x8 z;
#pragma unroll
  for (int t = 0; t < 8; ++t) z[t] = (bf16_t)0.f;
  return z;
}
// row `row` of a [n, 32] head slice (row stride ld), elements 8 g .. 8 g + 7; zeros for row >= n
__device__ __forceinline__ bf16x8 aw_row_frag(const bf16_t* __restrict__ base, int64_t ld, int row, int n, int g) {
  return row < n ? *(const bf16x8*)(base + (int64_t)row * ld + 8 * g) : aw_zero8();
}
// Y[d][row] = frag of row `row`: the transposed image of NTT row fragments, the B operand of a product that sums over rows
template <int NTT, int PP>
__device__ __forceinline__ void aw_put_transposed(bf16_t* Y, const bf16x8* f, int lr, int lg) {
#pragma unroll
  for (int t = 0; t < NTT; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) Y[(8 * lg + j) * PP + t * 16 + lr] = f[t][j];
}
// out[it][dt] = sum_k X[it * 16 + .][k] Y[dt * 16 + .][k] over k < NTT * 16
template <int NTT, int PP>
__device__ __forceinline__ void aw_second_product(const bf16_t* X, const bf16_t* Y, int lr, int lg, f32x4 (&out)[NTT][2]) {
#pragma unroll
  for (int it = 0; it < NTT; ++it)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NTT / 2; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(X + (it * 16 + lr) * PP + ks * 32 + 8 * lg),
                                                      *(const bf16x8*)(Y + (dt * 16 + lr) * PP + ks * 32 + 8 * lg), acc, 0, 0, 0);
      out[it][dt] = acc;
    }
}
// rows < n of out (C layout) * mul[it][r] -> dst[row * ld + dt * 16 + lr]
template <int NTT>
__device__ __forceinline__ void aw_store(bf16_t* __restrict__ dst, int64_t ld, const f32x4 (&out)[NTT][2], int n, int lr, int lg) {
#pragma unroll
  for (int it = 0; it < NTT; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = it * 16 + 4 * lg + r;
      if (row < n) {
        dst[(int64_t)row * ld + lr] = (bf16_t)out[it][0][r];
        dst[(int64_t)row * ld + 16 + lr] = (bf16_t)out[it][1][r];
      }
    }
}

template <int NTT>
__global__ __launch_bounds__(256) void attn_window_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o, float* __restrict__ lse,
                                                              const float* __restrict__ bias, float scale, int n, int h, int nprob, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int N32 = NTT * 16, PP = N32 + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int inner = h * 32;
  const int64_t ld = 3 * (int64_t)inner;
  float* bs = (float*)smem;
  bf16_t* X = (bf16_t*)(smem + (((size_t)n * n * 4 + 15) & ~(size_t)15)) + wave * ((N32 + 32) * PP);
  bf16_t* Y = X + N32 * PP;
  // a per-head bias (bias_hs != 0): the workgroup stays on head blockIdx.x % h and walks sequences, so that one [n, n] plane is all it stages
  const bool per_head = bias_hs != 0;
  const int hfix = per_head ? (int)(blockIdx.x % h) : 0;
  bias += (int64_t)hfix * bias_hs;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) bs[e] = bias[e];
  __syncthreads();
  const int pstep = (per_head ? gridDim.x / h : gridDim.x) * AW_WAVES, pend = per_head ? nprob / h : nprob;
  for (int p = (per_head ? blockIdx.x / h : blockIdx.x) * AW_WAVES + wave; p < pend; p += pstep) {   // (wave-uniform)
    const int bi = per_head ? p : p / h, hi = per_head ? hfix : p - bi * h;
    const bf16_t* base = qkv + (int64_t)bi * n * ld + hi * 32;
    bf16x8 qf[NTT], kf[NTT], vf[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
      qf[t] = aw_row_frag(base, ld, t * 16 + lr, n, lg);
      kf[t] = aw_row_frag(base + inner, ld, t * 16 + lr, n, lg);
      vf[t] = aw_row_frag(base + 2 * inner, ld, t * 16 + lr, n, lg);
    }
    aw_put_transposed<NTT, PP>(Y, vf, lr, lg);
    float inv[NTT][4];
#pragma unroll
    for (int it = 0; it < NTT; ++it) {
      f32x4 s[NTT];
#pragma unroll
      for (int jt = 0; jt < NTT; ++jt)
        s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[it], kf[jt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = it * 16 + 4 * lg + r;
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < NTT; ++jt) {
          const int col = jt * 16 + lr;
          const float v = (row < n && col < n) ? fmaf(s[jt][r], scale, bs[row * n + col]) : -INFINITY;
          s[jt][r] = v;
          m = fmaxf(m, v);
        }
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) m = fmaxf(m, __shfl_xor(m, x));
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NTT; ++jt) {
          const int col = jt * 16 + lr;
          const float pv = (row < n && col < n) ? expf(s[jt][r] - m) : 0.f;   // masked entries are exactly 0
          sum += pv;
          X[row * PP + col] = (bf16_t)pv;                                     // un-normalised: the fp32 row sum divides the output
        }
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) sum += __shfl_xor(sum, x);
        inv[it][r] = row < n ? 1.0f / sum : 0.f;
        if (lr == 0 && row < n) lse[((int64_t)bi * h + hi) * n + row] = m + logf(sum);
      }
    }
    aw_wave_sync();
    f32x4 out[NTT][2];
    aw_second_product<NTT, PP>(X, Y, lr, lg, out);
#pragma unroll
    for (int it = 0; it < NTT; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) { out[it][0][r] *= inv[it][r]; out[it][1][r] *= inv[it][r]; }
    aw_store<NTT>(o + (int64_t)bi * n * inner + hi * 32, inner, out, n, lr, lg);
    aw_wave_sync();   // the next problem rewrites the tiles
  }
}

template <int NTT>
__global__ __launch_bounds__(256) void attn_window_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o, const bf16_t* __restrict__ d_o,
                                                              const float* __restrict__ lse, bf16_t* __restrict__ dqkv, const float* __restrict__ bias,
                                                              float scale, int n, int h, int nprob, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int N32 = NTT * 16, PP = N32 + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int inner = h * 32;
  const int64_t ld = 3 * (int64_t)inner;
  float* bs = (float*)smem;
  bf16_t* X = (bf16_t*)(smem + (((size_t)n * n * 4 + 15) & ~(size_t)15)) + wave * ((N32 + 32) * PP);
  bf16_t* Y = X + N32 * PP;
  // a per-head bias (bias_hs != 0): the workgroup stays on head blockIdx.x % h and walks sequences, so that one [n, n] plane is all it stages
  const bool per_head = bias_hs != 0;
  const int hfix = per_head ? (int)(blockIdx.x % h) : 0;
  bias += (int64_t)hfix * bias_hs;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) bs[e] = bias[e];
  __syncthreads();
  const int pstep = (per_head ? gridDim.x / h : gridDim.x) * AW_WAVES, pend = per_head ? nprob / h : nprob;
  for (int p = (per_head ? blockIdx.x / h : blockIdx.x) * AW_WAVES + wave; p < pend; p += pstep) {   // (wave-uniform)
    const int bi = per_head ? p : p / h, hi = per_head ? hfix : p - bi * h;
    const bf16_t* base = qkv + (int64_t)bi * n * ld + hi * 32;
    const bf16_t* dob = d_o + (int64_t)bi * n * inner + hi * 32;
    const bf16_t* ob = o + (int64_t)bi * n * inner + hi * 32;
    const float* lse_h = lse + ((int64_t)bi * h + hi) * n;
    bf16_t* dbase = dqkv + (int64_t)bi * n * ld + hi * 32;
    bf16x8 qf[NTT], kf[NTT], vf[NTT], gf[NTT];
    float Dl[NTT];   // D = rowsum(dO o O) of row t * 16 + lr (the same value in the four lanes that share lr)
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
      const int row = t * 16 + lr;
      qf[t] = aw_row_frag(base, ld, row, n, lg);
      kf[t] = aw_row_frag(base + inner, ld, row, n, lg);
      vf[t] = aw_row_frag(base + 2 * inner, ld, row, n, lg);
      gf[t] = aw_row_frag(dob, inner, row, n, lg);
      const bf16x8 of = aw_row_frag(ob, inner, row, n, lg);
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) a = fmaf((float)gf[t][j], (float)of[j], a);
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      Dl[t] = a;
    }
    // P and dS (scaled) of the whole window, in registers (C layout)
    f32x4 pt[NTT][NTT], ds[NTT][NTT];
#pragma unroll
    for (int it = 0; it < NTT; ++it) {
      float lrow[4], Drow[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = it * 16 + 4 * lg + r;
        lrow[r] = row < n ? lse_h[row] : 0.f;
        Drow[r] = __shfl(Dl[it], 4 * lg + r);
      }
#pragma unroll
      for (int jt = 0; jt < NTT; ++jt) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[it], kf[jt], z, 0, 0, 0);
        const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[it], vf[jt], z, 0, 0, 0);   // dP = dO V^T
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = it * 16 + 4 * lg + r, col = jt * 16 + lr;
          const bool live = row < n && col < n;
          const float pv = live ? expf(fmaf(s[r], scale, bs[row * n + col]) - lrow[r]) : 0.f;
          pt[it][jt][r] = pv;
          ds[it][jt][r] = pv * (dp[r] - Drow[r]) * scale;
        }
      }
    }
    f32x4 out[NTT][2];
    // d(q) = scale dS K
#pragma unroll
    for (int it = 0; it < NTT; ++it)
#pragma unroll
      for (int jt = 0; jt < NTT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(it * 16 + 4 * lg + r) * PP + jt * 16 + lr] = (bf16_t)ds[it][jt][r];
    aw_put_transposed<NTT, PP>(Y, kf, lr, lg);
    aw_wave_sync();
    aw_second_product<NTT, PP>(X, Y, lr, lg, out);
    aw_store<NTT>(dbase, ld, out, n, lr, lg);
    aw_wave_sync();
    // d(k) = scale dS^T Q
#pragma unroll
    for (int it = 0; it < NTT; ++it)
#pragma unroll
      for (int jt = 0; jt < NTT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(jt * 16 + lr) * PP + it * 16 + 4 * lg + r] = (bf16_t)ds[it][jt][r];
    aw_put_transposed<NTT, PP>(Y, qf, lr, lg);
    aw_wave_sync();
    aw_second_product<NTT, PP>(X, Y, lr, lg, out);
    aw_store<NTT>(dbase + inner, ld, out, n, lr, lg);
    aw_wave_sync();
    // d(v) = P^T dO
#pragma unroll
    for (int it = 0; it < NTT; ++it)
#pragma unroll
      for (int jt = 0; jt < NTT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(jt * 16 + lr) * PP + it * 16 + 4 * lg + r] = (bf16_t)pt[it][jt][r];
    aw_put_transposed<NTT, PP>(Y, gf, lr, lg);
    aw_wave_sync();
    aw_second_product<NTT, PP>(X, Y, lr, lg, out);
    aw_store<NTT>(dbase + 2 * inner, ld, out, n, lr, lg);
    aw_wave_sync();   // the next problem rewrites the tiles
  }
}

template <int NTT> size_t aw_lds(int n) {
  return (((size_t)n * n * 4 + 15) & ~(size_t)15) + (size_t)AW_WAVES * (NTT * 16 + 32) * (NTT * 16 + 8) * 2;
}
// per_head: a multiple of h workgroups, each on one head
unsigned aw_grid(int nprob, int h, bool per_head) {
  if (per_head) return (unsigned)(h * std::min<int64_t>(ceil_div(nprob / h, AW_WAVES), std::max(1, 2048 / h)));
  return (unsigned)std::min<int64_t>(ceil_div(nprob, AW_WAVES), 2048);
}

}  // namespace

bool attn_window_supported(int n, int dim_head) { return dim_head == 32 && n >= 1 && n <= 64; }

void launch_attn_window_fwd(const bf16_t* qkv, bf16_t* o, float* lse, const float* bias, int b, int n, int h, float scale, hipStream_t s, int64_t bias_hs) {
  const int nprob = b * h;
  if (nprob <= 0) return;
  if (n <= 32) {
    auto kern = attn_window_fwd_kernel<2>;
    hipLaunchKernelGGL(kern, dim3(aw_grid(nprob, h, bias_hs != 0)), dim3(256), aw_lds<2>(n), s, qkv, o, lse, bias, scale, n, h, nprob, bias_hs);
  } else {
    auto kern = attn_window_fwd_kernel<4>;
    vitx_set_max_smem((const void*)kern, (int)aw_lds<4>(64));
    hipLaunchKernelGGL(kern, dim3(aw_grid(nprob, h, bias_hs != 0)), dim3(256), aw_lds<4>(n), s, qkv, o, lse, bias, scale, n, h, nprob, bias_hs);
  }
}

void launch_attn_window_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dqkv, const float* bias, int b, int n, int h,
                            float scale, hipStream_t s, int64_t bias_hs) {
  const int nprob = b * h;
  if (nprob <= 0) return;
  if (n <= 32) {
    auto kern = attn_window_bwd_kernel<2>;
    hipLaunchKernelGGL(kern, dim3(aw_grid(nprob, h, bias_hs != 0)), dim3(256), aw_lds<2>(n), s, qkv, o, d_o, lse, dqkv, bias, scale, n, h, nprob, bias_hs);
  } else {
    auto kern = attn_window_bwd_kernel<4>;
    vitx_set_max_smem((const void*)kern, (int)aw_lds<4>(64));
    hipLaunchKernelGGL(kern, dim3(aw_grid(nprob, h, bias_hs != 0)), dim3(256), aw_lds<4>(n), s, qkv, o, d_o, lse, dqkv, bias, scale, n, h, nprob, bias_hs);
  }
}
