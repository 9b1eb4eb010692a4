// Locality self-attention (vit_for_small_dataset.py:88-121) on the packed qkv [b, n, 3, h, dh] of the fused ViT kernels:
//   S = (q k^T) * exp(temperature),  S_ii = -FLT_MAX,  P = softmax(S),  o = P v
// with the temperature a learned per-layer scalar read from the parameter arena ON THE DEVICE (no host read: capturable), and its VJP
//   dS = P o (dP - rowsum(dP o P)),  dq = dS k e^t,  dk = dS^T q e^t,  dv = P^T dO,  d temperature = sum_{i != j} dS_ij S_ij   (dS/dt = S).
// One workgroup (4 waves) per (image, head, tile of 64 rows).  The two operands every row of the tile is multiplied with (forward and d(q):
// K and V; d(k) / d(v): Q and dO) are staged in LDS in the storage type, row pitch odd in 32-bit words (one row per lane is read conflict-free);
// a wave walks its 16 rows R at a time: one lane per key for the dot products (R rows share each LDS read of the staged operand), fp32 softmax
// with DPP reductions, the probabilities through a per-wave LDS row, then one lane per feature column for the second product.  That is the fp32
// FMA form: forward and backward on fp32 storage (fp32 and bf16x3 modes).  On bf16 storage the forward (attn_lsa_fwd_mfma_kernel) and the
// backward (attn_lsa_bwd_mfma_kernel) run every product on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16), softmax and accumulation in fp32.
// Reductions are fixed-order: the temperature gradient goes through one partial per workgroup and a single-workgroup second pass -- no
// atomics, two runs give the same bits.
#include "kernels.h"

#include <algorithm>
#include <cfloat>

namespace {

constexpr int LSA_TILE = 64, LSA_WAVES = 4, LSA_ROWS = LSA_TILE / LSA_WAVES;
constexpr int LSA_NCH = 5;            // key chunks of 64 lanes: n <= 320
constexpr int LSA_LDS_MAX = 160 * 1024 - 64;   // dynamic share of the 160 KiB a workgroup may hold (the bwd kernel keeps 16 B static)

template <typename T, int DH> __host__ __device__ constexpr int lsa_pitch() { return sizeof(T) == 4 ? DH + 1 : DH + 2; }
__host__ __device__ inline int lsa_npad(int n) { return (n + 15) & ~15; }

// two consecutive staged elements (even column)
template <typename T> __device__ __forceinline__ float2 lsa_ld2(const T* p);
template <> __device__ __forceinline__ float2 lsa_ld2<float>(const float* p) { return make_float2(p[0], p[1]); }
template <> __device__ __forceinline__ float2 lsa_ld2<bf16_t>(const bf16_t* p) {
  const uint32_t w = *(const uint32_t*)p;
  return make_float2(__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u));
}

// rows [0, n) of one head's [n, DH] slice (row stride ld) -> LDS rows of pitch lsa_pitch
template <typename T, int DH>
__device__ __forceinline__ void lsa_stage(const T* __restrict__ src, int64_t ld, int n, T* dst) {
  constexpr int L = lsa_pitch<T, DH>();
  for (int e = threadIdx.x; e < n * (DH / 4); e += blockDim.x) {
    const int j = e / (DH / 4), d4 = (e - j * (DH / 4)) * 4;
    const float4 v = ld4<T>(src + (int64_t)j * ld + d4);
    T* p = dst + j * L + d4;
    stf<T>(p, v.x); stf<T>(p + 1, v.y); stf<T>(p + 2, v.z); stf<T>(p + 3, v.w);
  }
}

// acc[r] = sum_j w[r][j] * M[j][d]: lane = (group, d), group g takes the j quads g, g + G, ...; the groups are added in a fixed order
template <typename T, int DH, int R>
__device__ __forceinline__ void lsa_row_times_staged(const float* wrow, int npad, const T* M, int n, int lane, float* acc) {
  constexpr int L = lsa_pitch<T, DH>(), G = 64 / DH;
  const int gi = lane / DH, d = lane - gi * DH;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  for (int j0 = gi * 4; j0 < npad; j0 += 4 * G) {
    float m4[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) m4[t] = ldf<T>(M + min(j0 + t, n - 1) * L + d);   // (weights beyond n are zero)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 w = *(const float4*)(wrow + r * npad + j0);
      acc[r] = fmaf(w.x, m4[0], acc[r]);
      acc[r] = fmaf(w.y, m4[1], acc[r]);
      acc[r] = fmaf(w.z, m4[2], acc[r]);
      acc[r] = fmaf(w.w, m4[3], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (G == 4) acc[r] += __shfl_xor(acc[r], 16);
    if (G >= 2) acc[r] += __shfl_xor(acc[r], 32);
  }
}

template <typename T, int DH, int R, bool PLAIN, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_lsa_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ o, float* __restrict__ lse,
                                                           const float* __restrict__ temperature, float scale, int n, int h, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int L = lsa_pitch<T, DH>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bi = blockIdx.z, hi = blockIdx.y, q0 = blockIdx.x * LSA_TILE;
  if (BIAS) temperature += (int64_t)hi * bias_hs;   // (BIAS: the head's [n, n] plane; stride 0 = one plane for every head)
  const int inner = h * DH, npad = lsa_npad(n);
  const int64_t ld = 3 * (int64_t)inner;
  T* Ks = (T*)smem;
  T* Vs = Ks + n * L;
  float* wbase = (float*)(smem + (((size_t)2 * n * L * sizeof(T) + 15) & ~(size_t)15)) + wave * (R * DH + R * npad);
  float* qs = wbase;
  float* ps = wbase + R * DH;
  const T* base = qkv + (int64_t)bi * n * ld + hi * DH;
  lsa_stage<T, DH>(base + inner, ld, n, Ks);
  lsa_stage<T, DH>(base + 2 * inner, ld, n, Vs);
  const float et = PLAIN ? scale : expf(temperature[0]);
  __syncthreads();
  for (int g = 0; g < LSA_ROWS / R; ++g) {
    const int r0 = q0 + wave * LSA_ROWS + g * R;
    for (int e = lane; e < R * DH; e += 64) {
      const int r = e / DH, d = e - r * DH;
      qs[e] = ldf<T>(base + (int64_t)min(r0 + r, n - 1) * ld + d);
    }
    __syncthreads();
    float s[R][LSA_NCH];
#pragma unroll
    for (int jc = 0; jc < LSA_NCH; ++jc) {
      const int j = jc * 64 + lane;
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
      if (jc * 64 < n) {
        const T* kr = Ks + min(j, n - 1) * L;
#pragma unroll 4
        for (int d = 0; d < DH; d += 4) {
          const float2 k01 = lsa_ld2<T>(kr + d), k23 = lsa_ld2<T>(kr + d + 2);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float4 qv = *(const float4*)(qs + r * DH + d);
            acc[r] = fmaf(qv.x, k01.x, acc[r]);
            acc[r] = fmaf(qv.y, k01.y, acc[r]);
            acc[r] = fmaf(qv.z, k23.x, acc[r]);
            acc[r] = fmaf(qv.w, k23.y, acc[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float sv = acc[r] * et;
        if (BIAS && j < n) sv += temperature[(int64_t)min(r0 + r, n - 1) * n + j];   // (BIAS: `temperature` is the [n, n] bias)
        s[r][jc] = j >= n ? -INFINITY : (!PLAIN && j == r0 + r ? -FLT_MAX : sv);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float m = s[r][0];
#pragma unroll
      for (int jc = 1; jc < LSA_NCH; ++jc) m = fmaxf(m, s[r][jc]);
      m = wave_max(m);
      float sum = 0.f;
#pragma unroll
      for (int jc = 0; jc < LSA_NCH; ++jc) {
        const int j = jc * 64 + lane;
        s[r][jc] = (j < n && (PLAIN || j != r0 + r)) ? expf(s[r][jc] - m) : 0.f;   // the masked entry is exactly 0
        sum += s[r][jc];
      }
      sum = wave_sum(sum);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int jc = 0; jc < LSA_NCH; ++jc) {
        const int j = jc * 64 + lane;
        if (j < npad) ps[r * npad + j] = s[r][jc] * inv;
      }
      if (lane == 0 && r0 + r < n) lse[((int64_t)bi * h + hi) * n + r0 + r] = m + logf(sum);
    }
    __syncthreads();
    float acc[R];
    lsa_row_times_staged<T, DH, R>(ps, npad, Vs, n, lane, acc);
    if (lane < DH) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r0 + r < n) stf<T>(o + ((int64_t)bi * n + r0 + r) * inner + hi * DH + lane, acc[r]);
    }
    __syncthreads();
  }
}

// Forward on bf16 storage, on the matrix pipe.  One workgroup per (image, head, 64 queries), one wave per 16 queries.  K [n16][DHP + 8] and
// V transposed [DH][n32 + 8] are staged in LDS as bf16 (zero beyond n / DH; rows 16-B aligned for ds_read_b128), the wave's Q fragments come
// straight from global memory.  v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + 0..7], B[k = 8 (l >> 4) + 0..7][col l & 15]
// and C[row 4 (l >> 4) + r][col l & 15].  S tile by tile stays in registers (18 tiles x 4 fp32 at n = 288); row maxima / sums are reduced over
// the 16 lanes of a row group; P goes through a per-wave LDS tile as bf16 (un-normalised, the fp32 row sum divides the output) to become the
// A operand of P v.
template <int DH, bool PLAIN, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_lsa_fwd_mfma_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o, float* __restrict__ lse,
                                                                const float* __restrict__ temperature, float scale, int n, int h, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DHP = DH < 32 ? 32 : DH, KP = DHP + 8, KS = DHP / 32, NT = (LSA_N_MAX + 15) / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int bi = blockIdx.z, hi = blockIdx.y, r0 = blockIdx.x * LSA_TILE + wave * 16;
  if (BIAS) temperature += (int64_t)hi * bias_hs;
  const int inner = h * DH, n16 = (n + 15) & ~15, n32 = (n + 31) & ~31, PP = n32 + 8;
  const int64_t ld = 3 * (int64_t)inner;
  bf16_t* Ks = (bf16_t*)smem;                 // [n16][KP]
  bf16_t* Vt = Ks + n16 * KP;                 // [DH][PP]
  bf16_t* Ps = Vt + DH * PP + wave * 16 * PP; // [16][PP] per wave
  const bf16_t* base = qkv + (int64_t)bi * n * ld + hi * DH;
  for (int e = threadIdx.x; e < n16 * (DHP / 4); e += blockDim.x) {
    const int j = e / (DHP / 4), d4 = (e - j * (DHP / 4)) * 4;
    bf16x4 v = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    if (j < n && d4 < DH) v = *(const bf16x4*)(base + inner + (int64_t)j * ld + d4);
    *(bf16x4*)(Ks + j * KP + d4) = v;
  }
  for (int e = threadIdx.x; e < n32 * (DH / 4); e += blockDim.x) {
    const int j = e / (DH / 4), d4 = (e - j * (DH / 4)) * 4;
    bf16x4 v = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    if (j < n) v = *(const bf16x4*)(base + 2 * inner + (int64_t)j * ld + d4);
#pragma unroll
    for (int t = 0; t < 4; ++t) Vt[(d4 + t) * PP + j] = v[t];
  }
  bf16x8 qf[KS];
  {
    const bf16_t* qrow = base + (int64_t)min(r0 + lr, n - 1) * ld;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int kk = ks * 32 + 8 * lg;
#pragma unroll
      for (int t = 0; t < 8; ++t) qf[ks][t] = (bf16_t)0.f;
      if (kk < DH) qf[ks] = *(const bf16x8*)(qrow + kk);
    }
  }
  const float et = PLAIN ? scale : expf(temperature[0]);
  __syncthreads();
  f32x4 s[NT];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt) {
    s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (jt * 16 < n16) {       // (wave-uniform)
      const bf16_t* kr = Ks + (jt * 16 + lr) * KP + 8 * lg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[ks], *(const bf16x8*)(kr + ks * 32), s[jt], 0, 0, 0);
    }
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * lg + r;
    float m = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
      const int j = jt * 16 + lr;
      float v = (j < n && (PLAIN || j != row)) ? s[jt][r] * et : -INFINITY;
      if (BIAS && j < n) v += temperature[(int64_t)min(row, n - 1) * n + j];   // (BIAS: `temperature` is the [n, n] bias)
      s[jt][r] = v;
      m = fmaxf(m, v);
    }
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) m = fmaxf(m, __shfl_xor(m, x));
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
      const int j = jt * 16 + lr;
      const float p = (j < n && (PLAIN || j != row)) ? expf(s[jt][r] - m) : 0.f;   // the masked entry is exactly 0
      sum += p;
      if (jt * 16 < n32) Ps[(4 * lg + r) * PP + j] = (bf16_t)p;        // (columns [n, n32) are written as zeros)
    }
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) sum += __shfl_xor(sum, x);
    inv[r] = 1.0f / sum;
    if (lr == 0 && row < n) lse[((int64_t)bi * h + hi) * n + row] = m + logf(sum);
  }
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < DH / 16; ++dt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const bf16_t* pr = Ps + lr * PP + 8 * lg;
    const bf16_t* vr = Vt + (dt * 16 + lr) * PP + 8 * lg;
    for (int k0 = 0; k0 < n32; k0 += 32) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(pr + k0), *(const bf16x8*)(vr + k0), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * lg + r;
      if (row < n) o[((int64_t)bi * n + row) * inner + hi * DH + dt * 16 + lr] = (bf16_t)(acc[r] * inv[r]);
    }
  }
}
template <int DH> size_t lsa_fwd_mfma_lds(int n) {
  const int DHP = DH < 32 ? 32 : DH, n16 = (n + 15) & ~15, PP = ((n + 31) & ~31) + 8;
  return ((size_t)n16 * (DHP + 8) + (size_t)DH * PP + (size_t)LSA_WAVES * 16 * PP) * 2;
}
template <int DH, bool PLAIN, bool BIAS = false>
void lsa_fwd_mfma_launch(const bf16_t* qkv, bf16_t* o, float* lse, int b, int n, int h, const float* t, float scale, hipStream_t s, int64_t bhs = 0) {
  auto kern = attn_lsa_fwd_mfma_kernel<DH, PLAIN, BIAS>;
  vitx_set_max_smem((const void*)kern, LSA_LDS_MAX);
  const size_t lds = lsa_fwd_mfma_lds<DH>(n);
  hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(n, LSA_TILE), h, b), dim3(256), lds, s, qkv, o, lse, t, scale, n, h, bhs);
}

// KEYS = false: the tile's rows are queries, K and V are staged: d(q), the row sums D = dO . o (kept in dsum for the other pass) and this workgroup's
//               partial of the temperature gradient.
// KEYS = true:  the tile's rows are keys, Q and dO are staged: d(k) and d(v).
template <typename T, int DH, int R, bool KEYS, bool PLAIN, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_lsa_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o,
                                                           const float* __restrict__ lse, float* __restrict__ dsum, T* __restrict__ dqkv,
                                                           const float* __restrict__ temperature, float scale, float* __restrict__ dt_part, int n,
                                                           int h, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float dt_wave[LSA_WAVES];
  constexpr int L = lsa_pitch<T, DH>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bi = blockIdx.z, hi = blockIdx.y, t0 = blockIdx.x * LSA_TILE;
  if (BIAS) temperature += (int64_t)hi * bias_hs;
  const int inner = h * DH, npad = lsa_npad(n);
  const int64_t ld = 3 * (int64_t)inner;
  T* As = (T*)smem;          // dotted with the row's first vector: the scores
  T* Bs = As + n * L;        // dotted with its second vector: dP
  float* wbase = (float*)(smem + (((size_t)2 * n * L * sizeof(T) + 15) & ~(size_t)15)) + wave * (2 * R * DH + (KEYS ? 2 : 1) * R * npad);
  float* ra = wbase;                     // [R][DH] q rows (KEYS: k rows)
  float* rb = wbase + R * DH;            // [R][DH] dO rows (KEYS: v rows)
  float* dw = wbase + 2 * R * DH;        // [R][npad] dS * e^t
  float* pw = dw + R * npad;             // [R][npad] P (KEYS only: d(v) needs it)
  const T* base = qkv + (int64_t)bi * n * ld + hi * DH;
  const T* dob = d_o + (int64_t)bi * n * inner + hi * DH;
  const T* ob = o + (int64_t)bi * n * inner + hi * DH;
  const float* lse_h = lse + ((int64_t)bi * h + hi) * n;
  float* dsum_h = dsum + ((int64_t)bi * h + hi) * n;
  if (KEYS) {
    lsa_stage<T, DH>(base, ld, n, As);
    lsa_stage<T, DH>(dob, inner, n, Bs);
  } else {
    lsa_stage<T, DH>(base + inner, ld, n, As);
    lsa_stage<T, DH>(base + 2 * inner, ld, n, Bs);
  }
  const float et = PLAIN ? scale : expf(temperature[0]);
  float dt_acc = 0.f;
  __syncthreads();
  for (int g = 0; g < LSA_ROWS / R; ++g) {
    const int r0 = t0 + wave * LSA_ROWS + g * R;
    float Drow[R], lrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { Drow[r] = 0.f; lrow[r] = 0.f; }
    for (int e = lane; e < R * DH; e += 64) {
      const int r = e / DH, d = e - r * DH;
      const int64_t row = min(r0 + r, n - 1);
      ra[e] = ldf<T>(base + row * ld + (KEYS ? inner : 0) + d);
      rb[e] = KEYS ? ldf<T>(base + row * ld + 2 * inner + d) : ldf<T>(dob + row * inner + d);
    }
    if (!KEYS) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = min(r0 + r, n - 1);
        const float v = lane < DH ? ldf<T>(dob + row * inner + lane) * ldf<T>(ob + row * inner + lane) : 0.f;
        Drow[r] = wave_sum(v);
        lrow[r] = lse_h[row];
        if (lane == 0 && r0 + r < n) dsum_h[r0 + r] = Drow[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int jc = 0; jc < LSA_NCH; ++jc) {
      const int j = jc * 64 + lane;
      if (jc * 64 < npad) {       // (wave-uniform)
        float sa[R], sb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { sa[r] = 0.f; sb[r] = 0.f; }
        const int jj = min(j, n - 1);
        const T* ar = As + jj * L;
        const T* br = Bs + jj * L;
#pragma unroll 2
        for (int d = 0; d < DH; d += 4) {
          const float2 a01 = lsa_ld2<T>(ar + d), a23 = lsa_ld2<T>(ar + d + 2);
          const float2 b01 = lsa_ld2<T>(br + d), b23 = lsa_ld2<T>(br + d + 2);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float4 av = *(const float4*)(ra + r * DH + d);
            const float4 bv = *(const float4*)(rb + r * DH + d);
            sa[r] = fmaf(av.x, a01.x, sa[r]); sa[r] = fmaf(av.y, a01.y, sa[r]); sa[r] = fmaf(av.z, a23.x, sa[r]); sa[r] = fmaf(av.w, a23.y, sa[r]);
            sb[r] = fmaf(bv.x, b01.x, sb[r]); sb[r] = fmaf(bv.y, b01.y, sb[r]); sb[r] = fmaf(bv.z, b23.x, sb[r]); sb[r] = fmaf(bv.w, b23.y, sb[r]);
          }
        }
        const float lj = KEYS ? lse_h[jj] : 0.f, Dj = KEYS ? dsum_h[jj] : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool live = j < n && (PLAIN || j != r0 + r) && r0 + r < n;
          float sc = sa[r] * et;
          if (BIAS && live) sc += KEYS ? temperature[(int64_t)j * n + r0 + r] : temperature[(int64_t)(r0 + r) * n + j];   // bias[query][key]
          const float p = live ? expf(sc - (KEYS ? lj : lrow[r])) : 0.f;
          const float ds = p * (sb[r] - (KEYS ? Dj : Drow[r]));
          if (!KEYS && !PLAIN && live) dt_acc = fmaf(ds, sc, dt_acc);
          if (j < npad) { dw[r * npad + j] = ds * et; if (KEYS) pw[r * npad + j] = p; }
        }
      }
    }
    __syncthreads();
    float acc[R];
    lsa_row_times_staged<T, DH, R>(dw, npad, As, n, lane, acc);      // d(q) = dS k e^t   /   d(k) = dS^T q e^t
    if (lane < DH) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r0 + r < n) stf<T>(dqkv + ((int64_t)bi * n + r0 + r) * ld + (KEYS ? inner : 0) + hi * DH + lane, acc[r]);
    }
    if (KEYS) {
      lsa_row_times_staged<T, DH, R>(pw, npad, Bs, n, lane, acc);    // d(v) = P^T dO
      if (lane < DH) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r0 + r < n) stf<T>(dqkv + ((int64_t)bi * n + r0 + r) * ld + 2 * inner + hi * DH + lane, acc[r]);
      }
    }
    __syncthreads();
  }
  if (!KEYS && !PLAIN) {
    dt_acc = wave_sum(dt_acc);
    if (lane == 0) dt_wave[wave] = dt_acc;
    __syncthreads();
    if (threadIdx.x == 0)
      dt_part[((int64_t)bi * h + hi) * gridDim.x + blockIdx.x] = ((dt_wave[0] + dt_wave[1]) + dt_wave[2]) + dt_wave[3];
  }
}

// Backward on bf16 storage, on the matrix pipe, in the manner of the forward: two launches over (image, head, 64 rows), one wave per 16 rows.
//   KEYS = false: rows are queries.  S = Q K^T and dP = dO V^T tile by tile (A fragments of the wave's Q / dO rows from global memory, B from K / V
//                 rows staged row-major), P = exp(S e^t - lse), dS = P (dP - D) in fp32, dS e^t through a per-wave LDS tile as the A operand of
//                 d(q) = dS K (B from K staged transposed); also D = dO . o (kept in dsum) and the workgroup's temperature partial.
//   KEYS = true:  rows are keys.  S^T = K Q^T and dP^T = V dO^T (A fragments of the wave's K / V rows, B from Q / dO rows staged row-major), then
//                 d(k) = dS^T Q and d(v) = P^T dO with B from Q / dO staged transposed.
// The other side is walked in chunks of LSA_NC rows (staged, used, replaced), the outputs accumulate in registers over the chunks.
constexpr int LSA_NC = 96;
template <int DH>
__device__ __forceinline__ void lsa_stage_chunk(const bf16_t* __restrict__ src, int64_t ld, int c0, int n, bf16_t* rows, bf16_t* tr) {
  constexpr int DHP = DH < 32 ? 32 : DH, KP = DHP + 8, TP = LSA_NC + 8;
  for (int e = threadIdx.x; e < LSA_NC * (DHP / 4); e += blockDim.x) {
    const int j = e / (DHP / 4), d4 = (e - j * (DHP / 4)) * 4;
    bf16x4 v = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    if (c0 + j < n && d4 < DH) v = *(const bf16x4*)(src + (int64_t)(c0 + j) * ld + d4);
    *(bf16x4*)(rows + j * KP + d4) = v;
    if (tr != nullptr && d4 < DH) {
#pragma unroll
      for (int t = 0; t < 4; ++t) tr[(d4 + t) * TP + j] = v[t];
    }
  }
}
template <int DH, bool KEYS, bool PLAIN, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_lsa_bwd_mfma_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                                const bf16_t* __restrict__ d_o, const float* __restrict__ lse,
                                                                float* __restrict__ dsum, bf16_t* __restrict__ dqkv,
                                                                const float* __restrict__ temperature, float scale, float* __restrict__ dt_part,
                                                                int n, int h, int64_t bias_hs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float dt_wave[LSA_WAVES];
  constexpr int DHP = DH < 32 ? 32 : DH, KP = DHP + 8, KS = DHP / 32, TP = LSA_NC + 8, NTC = LSA_NC / 16, ND = DH / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int bi = blockIdx.z, hi = blockIdx.y, r0 = blockIdx.x * LSA_TILE + wave * 16;
  if (BIAS) temperature += (int64_t)hi * bias_hs;
  const int inner = h * DH;
  const int64_t ld = 3 * (int64_t)inner;
  bf16_t* X0s = (bf16_t*)smem;              // [NC][KP] rows dotted with the first fragment: the scores
  bf16_t* X1s = X0s + LSA_NC * KP;          // [NC][KP] rows dotted with the second fragment: dP
  bf16_t* X0t = X1s + LSA_NC * KP;          // [DH][TP] X0 transposed: B of d(q) / d(k)
  bf16_t* X1t = X0t + DH * TP;              // [DH][TP] X1 transposed (KEYS only): B of d(v)
  bf16_t* Dt = X0t + (KEYS ? 2 : 1) * DH * TP + wave * (KEYS ? 2 : 1) * 16 * TP;   // [16][TP] dS e^t of this wave
  bf16_t* Pt = Dt + 16 * TP;                // [16][TP] P of this wave (KEYS only)
  const bf16_t* base = qkv + (int64_t)bi * n * ld + hi * DH;
  const bf16_t* dob = d_o + (int64_t)bi * n * inner + hi * DH;
  const bf16_t* ob = o + (int64_t)bi * n * inner + hi * DH;
  const float* lse_h = lse + ((int64_t)bi * h + hi) * n;
  float* dsum_h = dsum + ((int64_t)bi * h + hi) * n;
  bf16x8 f0[KS], f1[KS];
  {
    const int64_t row = min(r0 + lr, n - 1);
    const bf16_t* p0 = KEYS ? base + inner + row * ld : base + row * ld;
    const bf16_t* p1 = KEYS ? base + 2 * inner + row * ld : dob + row * inner;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int kk = ks * 32 + 8 * lg;
#pragma unroll
      for (int t = 0; t < 8; ++t) { f0[ks][t] = (bf16_t)0.f; f1[ks][t] = (bf16_t)0.f; }
      if (kk < DH) { f0[ks] = *(const bf16x8*)(p0 + kk); f1[ks] = *(const bf16x8*)(p1 + kk); }
    }
  }
  float lrow[4], Drow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lrow[r] = 0.f; Drow[r] = 0.f;
    if (!KEYS) {
      const int64_t row = min(r0 + 4 * lg + r, n - 1);
      float v = 0.f;
#pragma unroll
      for (int dd = 0; dd < ND; ++dd) v = fmaf((float)dob[row * inner + dd * 16 + lr], (float)ob[row * inner + dd * 16 + lr], v);
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) v += __shfl_xor(v, x);
      Drow[r] = v;
      lrow[r] = lse_h[row];
      if (lr == 0 && r0 + 4 * lg + r < n) dsum_h[r0 + 4 * lg + r] = v;
    }
  }
  const float et = PLAIN ? scale : expf(temperature[0]);
  float dt_acc = 0.f;
  f32x4 acc1[ND], acc2[ND];
#pragma unroll
  for (int dd = 0; dd < ND; ++dd) { acc1[dd] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[dd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int c0 = 0; c0 < n; c0 += LSA_NC) {
    __syncthreads();   // the previous chunk's readers are done
    if (KEYS) {
      lsa_stage_chunk<DH>(base, ld, c0, n, X0s, X0t);
      lsa_stage_chunk<DH>(dob, inner, c0, n, X1s, X1t);
    } else {
      lsa_stage_chunk<DH>(base + inner, ld, c0, n, X0s, X0t);
      lsa_stage_chunk<DH>(base + 2 * inner, ld, c0, n, X1s, nullptr);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NTC; ++t) {
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
      const bf16_t* x0 = X0s + (t * 16 + lr) * KP + 8 * lg;
      const bf16_t* x1 = X1s + (t * 16 + lr) * KP + 8 * lg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0[ks], *(const bf16x8*)(x0 + ks * 32), sa, 0, 0, 0);
        sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1[ks], *(const bf16x8*)(x1 + ks * 32), sb, 0, 0, 0);
      }
      const int c = c0 + t * 16 + lr;     // the column's index on the other side
      const float lc = (KEYS && c < n) ? lse_h[c] : 0.f, Dc = (KEYS && c < n) ? dsum_h[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * lg + r;
        const bool live = row < n && c < n && (PLAIN || row != c);
        float sc = sa[r] * et;
        if (BIAS && live) sc += KEYS ? temperature[(int64_t)c * n + row] : temperature[(int64_t)row * n + c];   // bias[query][key]
        const float p = live ? expf(sc - (KEYS ? lc : lrow[r])) : 0.f;
        const float ds = p * (sb[r] - (KEYS ? Dc : Drow[r]));
        if (!KEYS && !PLAIN && live) dt_acc = fmaf(ds, sc, dt_acc);
        Dt[(4 * lg + r) * TP + t * 16 + lr] = (bf16_t)(ds * et);
        if (KEYS) Pt[(4 * lg + r) * TP + t * 16 + lr] = (bf16_t)p;
      }
    }
    __syncthreads();
#pragma unroll
    for (int dd = 0; dd < ND; ++dd) {
      const bf16_t* ar = Dt + lr * TP + 8 * lg;
      const bf16_t* br = X0t + (dd * 16 + lr) * TP + 8 * lg;
#pragma unroll
      for (int k0 = 0; k0 < LSA_NC; k0 += 32)
        acc1[dd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ar + k0), *(const bf16x8*)(br + k0), acc1[dd], 0, 0, 0);
      if (KEYS) {
        const bf16_t* ap = Pt + lr * TP + 8 * lg;
        const bf16_t* bv = X1t + (dd * 16 + lr) * TP + 8 * lg;
#pragma unroll
        for (int k0 = 0; k0 < LSA_NC; k0 += 32)
          acc2[dd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ap + k0), *(const bf16x8*)(bv + k0), acc2[dd], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int dd = 0; dd < ND; ++dd) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * lg + r;
      if (row < n) {
        bf16_t* dst = dqkv + ((int64_t)bi * n + row) * ld + hi * DH + dd * 16 + lr;
        dst[KEYS ? inner : 0] = (bf16_t)acc1[dd][r];               // d(q)   /   d(k)
        if (KEYS) dst[2 * inner] = (bf16_t)acc2[dd][r];            // d(v)
      }
    }
  }
  if (!KEYS && !PLAIN) {
    dt_acc = wave_sum(dt_acc);
    if (lane == 0) dt_wave[wave] = dt_acc;
    __syncthreads();
    if (threadIdx.x == 0)
      dt_part[((int64_t)bi * h + hi) * gridDim.x + blockIdx.x] = ((dt_wave[0] + dt_wave[1]) + dt_wave[2]) + dt_wave[3];
  }
}
template <int DH, bool KEYS, bool PLAIN, bool BIAS = false>
void lsa_bwd_mfma_launch(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, float* dsum, bf16_t* dqkv, int b, int n, int h,
                         const float* t, float scale, float* part, hipStream_t s, int64_t bhs = 0) {
  constexpr int DHP = DH < 32 ? 32 : DH, KP = DHP + 8, TP = LSA_NC + 8;
  const size_t lds = ((size_t)2 * LSA_NC * KP + (size_t)(KEYS ? 2 : 1) * DH * TP + (size_t)LSA_WAVES * (KEYS ? 2 : 1) * 16 * TP) * 2;
  auto kern = attn_lsa_bwd_mfma_kernel<DH, KEYS, PLAIN, BIAS>;
  vitx_set_max_smem((const void*)kern, LSA_LDS_MAX);
  hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(n, LSA_TILE), h, b), dim3(256), lds, s, qkv, o, d_o, lse, dsum, dqkv, t, scale, part, n, h, bhs);
}
template <int DH, bool PLAIN, bool BIAS = false>
void lsa_bwd_mfma_dh(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, float* dsum, bf16_t* dqkv, int b, int n, int h,
                     const float* t, float scale, float* part, hipStream_t s, int64_t bhs = 0) {
  lsa_bwd_mfma_launch<DH, false, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);   // (first: it writes the row sums the key pass reads)
  lsa_bwd_mfma_launch<DH, true, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);
}

// second pass of the temperature gradient: one workgroup, every thread a fixed strided share, then a fixed tree
__global__ __launch_bounds__(256) void attn_lsa_dtemp_kernel(const float* __restrict__ part, int64_t n, float* __restrict__ out) {
  __shared__ float red[256];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

template <typename T, int DH> size_t lsa_fwd_lds(int n, int R) {
  return (((size_t)2 * n * lsa_pitch<T, DH>() * sizeof(T) + 15) & ~(size_t)15) + (size_t)LSA_WAVES * (R * DH + R * lsa_npad(n)) * 4;
}
template <typename T, int DH> size_t lsa_bwd_lds(int n, int R, bool keys) {
  return (((size_t)2 * n * lsa_pitch<T, DH>() * sizeof(T) + 15) & ~(size_t)15) + (size_t)LSA_WAVES * (2 * R * DH + (keys ? 2 : 1) * R * lsa_npad(n)) * 4;
}

template <typename T, int DH, int R, bool PLAIN, bool BIAS = false>
void lsa_fwd_launch(const T* qkv, T* o, float* lse, int b, int n, int h, const float* t, float scale, size_t lds, hipStream_t s, int64_t bhs = 0) {
  auto kern = attn_lsa_fwd_kernel<T, DH, R, PLAIN, BIAS>;
  vitx_set_max_smem((const void*)kern, LSA_LDS_MAX);
  hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(n, LSA_TILE), h, b), dim3(256), lds, s, qkv, o, lse, t, scale, n, h, bhs);
}
template <typename T, int DH, bool PLAIN, bool BIAS = false>
void lsa_fwd_dh(const T* qkv, T* o, float* lse, int b, int n, int h, const float* t, float scale, hipStream_t s, int64_t bhs = 0) {
  if (lsa_fwd_lds<T, DH>(n, 4) <= (size_t)LSA_LDS_MAX) lsa_fwd_launch<T, DH, 4, PLAIN, BIAS>(qkv, o, lse, b, n, h, t, scale, lsa_fwd_lds<T, DH>(n, 4), s, bhs);
  else if (lsa_fwd_lds<T, DH>(n, 2) <= (size_t)LSA_LDS_MAX) lsa_fwd_launch<T, DH, 2, PLAIN, BIAS>(qkv, o, lse, b, n, h, t, scale, lsa_fwd_lds<T, DH>(n, 2), s, bhs);
  else lsa_fwd_launch<T, DH, 1, PLAIN, BIAS>(qkv, o, lse, b, n, h, t, scale, lsa_fwd_lds<T, DH>(n, 1), s, bhs);
}
template <typename T>
void lsa_fwd_t(const T* qkv, T* o, float* lse, int b, int n, int h, int dh, const float* t, hipStream_t s) {
  if (dh == 64) lsa_fwd_dh<T, 64, false>(qkv, o, lse, b, n, h, t, 0.f, s);
  else if (dh == 32) lsa_fwd_dh<T, 32, false>(qkv, o, lse, b, n, h, t, 0.f, s);
  else lsa_fwd_dh<T, 16, false>(qkv, o, lse, b, n, h, t, 0.f, s);
}

template <typename T, int DH, int R, bool KEYS, bool PLAIN, bool BIAS = false>
void lsa_bwd_launch(const T* qkv, const T* o, const T* d_o, const float* lse, float* dsum, T* dqkv, int b, int n, int h, const float* t, float scale,
                    float* part, hipStream_t s, int64_t bhs = 0) {
  auto kern = attn_lsa_bwd_kernel<T, DH, R, KEYS, PLAIN, BIAS>;
  vitx_set_max_smem((const void*)kern, LSA_LDS_MAX);
  const size_t lds = lsa_bwd_lds<T, DH>(n, R, KEYS);
  hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(n, LSA_TILE), h, b), dim3(256), lds, s, qkv, o, d_o, lse, dsum, dqkv, t, scale, part, n, h, bhs);
}
// each pass with the most rows per wave whose LDS rows still fit beside the staged operands
template <typename T, int DH, bool KEYS, bool PLAIN, bool BIAS = false>
void lsa_bwd_pass(const T* qkv, const T* o, const T* d_o, const float* lse, float* dsum, T* dqkv, int b, int n, int h, const float* t, float scale,
                  float* part, hipStream_t s, int64_t bhs = 0) {
  if (lsa_bwd_lds<T, DH>(n, 4, KEYS) <= (size_t)LSA_LDS_MAX) lsa_bwd_launch<T, DH, 4, KEYS, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);
  else if (lsa_bwd_lds<T, DH>(n, 2, KEYS) <= (size_t)LSA_LDS_MAX) lsa_bwd_launch<T, DH, 2, KEYS, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);
  else lsa_bwd_launch<T, DH, 1, KEYS, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);
}
template <typename T, int DH, bool PLAIN, bool BIAS = false>
void lsa_bwd_dh(const T* qkv, const T* o, const T* d_o, const float* lse, float* dsum, T* dqkv, int b, int n, int h, const float* t, float scale,
                float* part, hipStream_t s, int64_t bhs = 0) {
  lsa_bwd_pass<T, DH, false, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);   // (first: it writes the row sums the key pass reads)
  lsa_bwd_pass<T, DH, true, PLAIN, BIAS>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, scale, part, s, bhs);
}
template <typename T>
void lsa_bwd_t(const T* qkv, const T* o, const T* d_o, const float* lse, float* dsum, T* dqkv, int b, int n, int h, int dh, const float* t, float* part,
               hipStream_t s) {
  if (dh == 64) lsa_bwd_dh<T, 64, false>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, 0.f, part, s);
  else if (dh == 32) lsa_bwd_dh<T, 32, false>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, 0.f, part, s);
  else lsa_bwd_dh<T, 16, false>(qkv, o, d_o, lse, dsum, dqkv, b, n, h, t, 0.f, part, s);
}

}  // namespace

bool attn_lsa_supported(int n, int dim_head) {
  return (dim_head == 16 || dim_head == 32 || dim_head == 64) && n >= 2 && n <= LSA_N_MAX;
}
int64_t attn_lsa_ws_elems(int b, int n, int h) { return (int64_t)b * h * ceil_div(n, LSA_TILE); }

void launch_attn_lsa_fwd(const void* qkv, void* o, float* lse, int is_bf16, int b, int n, int h, int dim_head, const float* temperature, hipStream_t s) {
  if (is_bf16) {
    if (dim_head == 64) lsa_fwd_mfma_launch<64, false>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, temperature, 0.f, s);
    else if (dim_head == 32) lsa_fwd_mfma_launch<32, false>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, temperature, 0.f, s);
    else lsa_fwd_mfma_launch<16, false>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, temperature, 0.f, s);
  } else lsa_fwd_t<float>((const float*)qkv, (float*)o, lse, b, n, h, dim_head, temperature, s);
}

void launch_attn_lsa_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* dsum_ws, void* dqkv, int is_bf16, int b, int n, int h,
                         int dim_head, const float* temperature, float* dtemperature, float* part_ws, hipStream_t s) {
  if (is_bf16) {
    const bf16_t *q_ = (const bf16_t*)qkv, *o_ = (const bf16_t*)o, *do_ = (const bf16_t*)d_o;
    if (dim_head == 64) lsa_bwd_mfma_dh<64, false>(q_, o_, do_, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, temperature, 0.f, part_ws, s);
    else if (dim_head == 32) lsa_bwd_mfma_dh<32, false>(q_, o_, do_, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, temperature, 0.f, part_ws, s);
    else lsa_bwd_mfma_dh<16, false>(q_, o_, do_, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, temperature, 0.f, part_ws, s);
  } else lsa_bwd_t<float>((const float*)qkv, (const float*)o, (const float*)d_o, lse, dsum_ws, (float*)dqkv, b, n, h, dim_head, temperature, part_ws, s);
  hipLaunchKernelGGL(attn_lsa_dtemp_kernel, dim3(1), dim3(256), 0, s, part_ws, attn_lsa_ws_elems(b, n, h), dtemperature);
}

// Plain small-head attention (nest.py:93-109, on a vitx_config.nest_block engine): the kernels above in their PLAIN mode -- no diagonal mask, the scale
// dim_head^-0.5 passed by value, no temperature partials and no second pass, n >= 1.  dim_head 64 keeps attn_bf16 / attn_x3.
// BIAS (a third compile-time mode on top of PLAIN, dim_head 32): an additive fp32 [n, n] bias on the scaled scores, forward and where both
// backward passes recompute P.  The pointer rides in the kernels' `temperature` argument, which PLAIN never reads, so that the argument lists --
// and the code of the PLAIN and LSA instantiations -- stay what they were.
bool attn_small_supported(int n, int dim_head) { return (dim_head == 16 || dim_head == 32) && n >= 1 && n <= LSA_N_MAX; }

void launch_attn_small_fwd(const void* qkv, void* o, float* lse, int is_bf16, int b, int n, int h, int dim_head, float scale, hipStream_t s,
                           const float* bias, int64_t bias_hs) {
  if (bias) {   // BIAS mode (crossformer.py:156-168): s = scale q k^T + bias[i][j]; dim_head 32 only; the bias travels in the temperature slot
    if (is_bf16) lsa_fwd_mfma_launch<32, true, true>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, bias, scale, s, bias_hs);
    else lsa_fwd_dh<float, 32, true, true>((const float*)qkv, (float*)o, lse, b, n, h, bias, scale, s, bias_hs);
    return;
  }
  if (is_bf16) {
    if (dim_head == 32) lsa_fwd_mfma_launch<32, true>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, nullptr, scale, s);
    else lsa_fwd_mfma_launch<16, true>((const bf16_t*)qkv, (bf16_t*)o, lse, b, n, h, nullptr, scale, s);
  } else if (dim_head == 32) lsa_fwd_dh<float, 32, true>((const float*)qkv, (float*)o, lse, b, n, h, nullptr, scale, s);
  else lsa_fwd_dh<float, 16, true>((const float*)qkv, (float*)o, lse, b, n, h, nullptr, scale, s);
}

void launch_attn_small_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* dsum_ws, void* dqkv, int is_bf16, int b, int n, int h,
                           int dim_head, float scale, hipStream_t s, const float* bias, int64_t bias_hs) {
  if (bias) {   // d(q, k, v) need the bias only to recompute P (its own gradient: launch_attn_dbias)
    if (is_bf16) lsa_bwd_mfma_dh<32, true, true>((const bf16_t*)qkv, (const bf16_t*)o, (const bf16_t*)d_o, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, bias, scale, nullptr, s, bias_hs);
    else lsa_bwd_dh<float, 32, true, true>((const float*)qkv, (const float*)o, (const float*)d_o, lse, dsum_ws, (float*)dqkv, b, n, h, bias, scale, nullptr, s, bias_hs);
    return;
  }
  if (is_bf16) {
    const bf16_t *q_ = (const bf16_t*)qkv, *o_ = (const bf16_t*)o, *do_ = (const bf16_t*)d_o;
    if (dim_head == 32) lsa_bwd_mfma_dh<32, true>(q_, o_, do_, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, nullptr, scale, nullptr, s);
    else lsa_bwd_mfma_dh<16, true>(q_, o_, do_, lse, dsum_ws, (bf16_t*)dqkv, b, n, h, nullptr, scale, nullptr, s);
  } else if (dim_head == 32)
    lsa_bwd_dh<float, 32, true>((const float*)qkv, (const float*)o, (const float*)d_o, lse, dsum_ws, (float*)dqkv, b, n, h, nullptr, scale, nullptr, s);
  else
    lsa_bwd_dh<float, 16, true>((const float*)qkv, (const float*)o, (const float*)d_o, lse, dsum_ws, (float*)dqkv, b, n, h, nullptr, scale, nullptr, s);
}

// ---------------------------------------------------------------------------------------------- d(bias) of a learned bias (regionvit.py:107,126)
// d(bias)[h, i, j] = sum over the sequences of dS[h, i, j], dS = P o (dP - rowsum(dO o O)) = P o (dO_i . (v_j - o_i)): unscaled, the bias is added
// behind the scale.  A kernel of its own that recomputes P from lse, so that it serves both biased attention families and every storage type:
// one thread per DB_EPT entries (i, j) of one head, a workgroup walks a fixed slice of the sequences and keeps its sums in registers; one partial
// [h, n, n] per slice, added in slice order by the second pass INTO the accumulator (a bias shared by the layers of a stage collects them all).
// No atomics: the same bits every run.  Operands come straight from global memory (rows of 32 elements, the q / dO / o row shared by the
// threads of a row of entries); not tuned.
namespace {
constexpr int DB_EPT = 8, DB_SLICES = 64;

template <typename T>
__global__ __launch_bounds__(256) void attn_dbias_part_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o,
                                                              const float* __restrict__ lse, const float* __restrict__ bias, int64_t bias_hs, float scale,
                                                              int b, int n, int h, int per, float* __restrict__ part) {
  const int hi = blockIdx.y, sl = blockIdx.z, nn = n * n, inner = h * 32;
  const int e0 = blockIdx.x * (256 * DB_EPT) + threadIdx.x;
  const int64_t ld = 3 * (int64_t)inner;
  const float* bh = bias + (int64_t)hi * bias_hs;
  float acc[DB_EPT];
#pragma unroll
  for (int t = 0; t < DB_EPT; ++t) acc[t] = 0.f;
  const int b1 = min(b, (sl + 1) * per);
  for (int bi = sl * per; bi < b1; ++bi) {
    const T* base = qkv + (int64_t)bi * n * ld + hi * 32;
    const T* dob = d_o + (int64_t)bi * n * inner + hi * 32;
    const T* ob = o + (int64_t)bi * n * inner + hi * 32;
    const float* lse_h = lse + ((int64_t)bi * h + hi) * n;
#pragma unroll
    for (int t = 0; t < DB_EPT; ++t) {
      const int e = e0 + t * 256;
      if (e >= nn) continue;
      const int i = e / n, j = e - i * n;
      const T* qr = base + (int64_t)i * ld;
      const T* kr = base + inner + (int64_t)j * ld;
      const T* vr = kr + inner;
      const T* gr = dob + (int64_t)i * inner;
      const T* orow = ob + (int64_t)i * inner;
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < 32; d += 4) {
        const float4 q4 = ld4<T>(qr + d), k4 = ld4<T>(kr + d), v4 = ld4<T>(vr + d), g4 = ld4<T>(gr + d), o4 = ld4<T>(orow + d);
        sc = fmaf(q4.x, k4.x, sc); sc = fmaf(q4.y, k4.y, sc); sc = fmaf(q4.z, k4.z, sc); sc = fmaf(q4.w, k4.w, sc);
        dp = fmaf(g4.x, v4.x - o4.x, dp); dp = fmaf(g4.y, v4.y - o4.y, dp); dp = fmaf(g4.z, v4.z - o4.z, dp); dp = fmaf(g4.w, v4.w - o4.w, dp);
      }
      acc[t] += expf(fmaf(sc, scale, bh[e]) - lse_h[i]) * dp;
    }
  }
#pragma unroll
  for (int t = 0; t < DB_EPT; ++t) {
    const int e = e0 + t * 256;
    if (e < nn) part[((int64_t)sl * h + hi) * nn + e] = acc[t];
  }
}

// acc[e] += part[0][e] + part[1][e] + ... in slice order
__global__ __launch_bounds__(256) void attn_dbias_reduce_kernel(const float* __restrict__ part, int slices, int64_t total, float* __restrict__ acc) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  float a = part[e];
  for (int sl = 1; sl < slices; ++sl) a += part[(int64_t)sl * total + e];
  acc[e] += a;
}
}  // namespace

int64_t attn_dbias_ws_elems(int b, int n, int h) { return (int64_t)std::min(std::max(b, 1), DB_SLICES) * h * n * n; }

void launch_attn_dbias(const void* qkv, const void* o, const void* d_o, const float* lse, int is_bf16, int b, int n, int h, float scale, const float* bias,
                       int64_t bias_hs, float* ws, float* dbias_acc, hipStream_t s) {
  if (b <= 0) return;
  const int per = (int)ceil_div(b, DB_SLICES), slices = (int)ceil_div(b, per);
  const int64_t total = (int64_t)h * n * n;
  const dim3 grid((unsigned)ceil_div(n * n, 256 * DB_EPT), h, slices);
  if (is_bf16)
    hipLaunchKernelGGL(attn_dbias_part_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)o, (const bf16_t*)d_o, lse, bias, bias_hs, scale, b, n,
                       h, per, ws);
  else
    hipLaunchKernelGGL(attn_dbias_part_kernel<float>, grid, dim3(256), 0, s, (const float*)qkv, (const float*)o, (const float*)d_o, lse, bias, bias_hs, scale, b, n, h,
                       per, ws);
  hipLaunchKernelGGL(attn_dbias_reduce_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, (const float*)ws, slices, total, dbias_acc);
}
