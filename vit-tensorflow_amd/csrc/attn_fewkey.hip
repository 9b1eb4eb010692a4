// Few-key attention (twins_svt.py:184-187 of GlobalAttention): n queries of an (image, head) against m <= 64 keys, dim_head 64, bf16 storage,
// every product on the matrix pipe (v_mfma_f32_16x16x32_bf16), softmax statistics in fp32, the scores never written to HBM.
//   q [b, n, ldq] (head h at columns 64 h), k / v [b, m, ldkv] (the two halves of kv), o [b, n, ldo], lse [b, heads, n] = max + log(sum) of the
//   scaled scores.
// Forward: grid (query chunks, b * heads), 4 waves; K (key-major) and V (transposed: d-major) of the (image, head) are staged once in LDS, each
// wave streams tiles of 32 queries: S = Q K^T from global Q fragments, softmax across the 16 lanes that share a query row, P through a per-wave
// LDS tile into the A layout, O = P V.
// Backward: ONE workgroup per (image, head), so d(k) / d(v) need no second pass: per tile of 32 queries a wave recomputes P from q, k and lse,
// dP = dO V^T, D = rowsum(dO * O), dS = P (dP - D), dq = scale dS K (written at once), and accumulates dv += P^T dO and dk += dS^T Q in
// registers over all its tiles; the four waves' accumulators are added in wave order through LDS and written once.
// Masking, never padding: keys >= m get a score of -inf (P = 0) and their LDS rows are written as zeros when K / V are staged; query rows >= n
// are loaded from row n - 1, contribute P = dS = 0 and zero Q / dO rows to dk / dv, and are never stored.
// Many keys (cvt.py:120-123 of CvT's Attention: 64 < m <= MANYKEY_MAX keys, e.g. 784 queries against 196): the same operand layouts and lse.
//   Forward: all of K and V^T of the (image, head) stay in LDS; a wave walks its 32-query tile over chunks of 64 keys with an online softmax
//   (running max and sum per query row, the O accumulators rescaled in registers) and writes o and lse once.
//   Backward, two kernels, because d(k) / d(v) of that many keys do not fit one workgroup's registers: d(k) / d(v) on a grid of (key chunks,
//   b * heads) -- the few-key backward kernel with a key offset (CHUNK): it stages its 64 keys, sweeps all queries, recomputes P from the saved
//   lse (global, so chunks are independent) and does not store d(q) -- and d(q) on a grid of (query chunks, b * heads) with all of K, V and K^T
//   in LDS: per query tile dq = scale sum over the key chunks of dS K, accumulated in registers and written once.
// MFMA layouts: lane l holds A[row l & 15][k = 8 (l >> 4) + 0..7] and B[k = 8 (l >> 4) + 0..7][col l & 15]; result reg r is
// C[row 4 (l >> 4) + r][col l & 15].  Every operand here is read k-contiguous (16 bytes): A from X[row][k], B from Bt[col][k].
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace {

constexpr int DH = 64, QT = 32, LDK = DH + 8, LDQ = QT + 8;

__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x8 frag(const bf16_t* x, int row0, int ld, int k0, int c, int g) {
  return *(const bf16x8*)(x + (row0 + c) * ld + k0 + 8 * g);
}
// reduction over the 16 lanes that share l >> 4
__device__ __forceinline__ float row_max16(float v) {
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float row_sum16(float v) {
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// s[mt][jt] = Q[q0 + 16 mt ..][:] K^T[:, 16 jt ..] (unscaled); rows beyond n - 1 read row n - 1
template <int MP>
__device__ __forceinline__ void scores(const bf16_t* __restrict__ xrows, int64_t ld, int q0, int n, const bf16_t* Bt, int ldb, f32x4 (&s)[2][MP / 16], int c, int g) {
  for (int mt = 0; mt < 2; ++mt) {
    const int row = min(q0 + mt * 16 + c, n - 1);
    const bf16_t* xr = xrows + (int64_t)row * ld;
    for (int jt = 0; jt < MP / 16; ++jt) s[mt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 a = *(const bf16x8*)(xr + ks * 32 + 8 * g);
      for (int jt = 0; jt < MP / 16; ++jt) s[mt][jt] = mma(a, frag(Bt, jt * 16, ldb, ks * 32, c, g), s[mt][jt]);
    }
  }
}

template <int MP>
__global__ __launch_bounds__(256) void attn_fewkey_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, bf16_t* __restrict__ o,
                                                              float* __restrict__ lse, int n, int m, int heads, int64_t ldq, int64_t ldkv, int64_t ldo,
                                                              float scale) {
  constexpr int LDM = MP + 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = (bf16_t*)smem;          // [MP][LDK]   key-major
  bf16_t* Vt = Ks + MP * LDK;          // [DH][LDM]   d-major
  bf16_t* Ps = Vt + DH * LDM;          // [4][QT][LDM]
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int bh = blockIdx.y, bi = bh / heads, h = bh % heads, inner = heads * DH;
  const bf16_t* kb = kv + (int64_t)bi * m * ldkv + h * DH;
  const bf16_t* vb = kb + inner;
  for (int i = tid; i < MP * DH; i += 256) {
    const int key = i / DH, d = i % DH;
    const bool in = key < m;
    Ks[key * LDK + d] = in ? kb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
    Vt[d * LDM + key] = in ? vb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
  }
  __syncthreads();
  bf16_t* P = Ps + wave * QT * LDM;
  const bf16_t* qb = q + (int64_t)bi * n * ldq + h * DH;
  bf16_t* ob = o + (int64_t)bi * n * ldo + h * DH;
  const int ntiles = (n + QT - 1) / QT;
  for (int t0 = blockIdx.x * 4; t0 < ntiles; t0 += gridDim.x * 4) {   // (the same trip count for every wave: the barriers below are uniform)
    const int q0 = (t0 + wave) * QT;
    f32x4 s[2][MP / 16];
    scores<MP>(qb, ldq, q0, n, Ks, LDK, s, c, g);
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) {
        const int ql = mt * 16 + 4 * g + r, row = q0 + ql;
        float mx = -INFINITY;
        for (int jt = 0; jt < MP / 16; ++jt) {
          const float v = (jt * 16 + c) < m ? s[mt][jt][r] * scale : -INFINITY;
          s[mt][jt][r] = v;
          mx = fmaxf(mx, v);
        }
        mx = row_max16(mx);   // (key 0 is always live: finite)
        float sum = 0.f;
        for (int jt = 0; jt < MP / 16; ++jt) {
          const float p = __expf(s[mt][jt][r] - mx);
          s[mt][jt][r] = p;
          sum += p;
        }
        sum = row_sum16(sum);
        const float inv = 1.0f / sum;
        for (int jt = 0; jt < MP / 16; ++jt) P[ql * LDM + jt * 16 + c] = (bf16_t)(s[mt][jt][r] * inv);
        if (c == 0 && row < n) lse[(int64_t)bh * n + row] = mx + __logf(sum);
      }
    __syncthreads();
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 acc[4];
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < MP / 32; ++ks) {
        const bf16x8 a = frag(P, mt * 16, LDM, ks * 32, c, g);
        for (int nt = 0; nt < 4; ++nt) acc[nt] = mma(a, frag(Vt, nt * 16, LDM, ks * 32, c, g), acc[nt]);
      }
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + mt * 16 + 4 * g + r;
        if (row < n)
          for (int nt = 0; nt < 4; ++nt) ob[(int64_t)row * ldo + nt * 16 + c] = (bf16_t)acc[nt][r];
      }
    }
    __syncthreads();
  }
}

// CHUNK: workgroup (x, y) owns keys [64 x, 64 x + 64) of (image, head) y and leaves d(q) to attn_manykey_dq_kernel (MP == 64)
template <int MP, bool CHUNK = false>
__global__ __launch_bounds__(256) void attn_fewkey_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, const bf16_t* __restrict__ o,
                                                              const bf16_t* __restrict__ d_o, const float* __restrict__ lse, bf16_t* __restrict__ dq,
                                                              bf16_t* __restrict__ dkv, int n, int m, int heads, int64_t ldq, int64_t ldkv, int64_t ldo,
                                                              int64_t lddo, int64_t lddq, int64_t lddkv, float scale) {
  constexpr int LDM = MP + 8, JT = MP / 16;
  constexpr int WAVE_ELEMS = QT * LDM + 2 * MP * LDQ + 2 * DH * LDQ + 64;   // bf16 elements of one wave's scratch (the last 64: 32 floats of D)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = (bf16_t*)smem;          // [MP][LDK]
  bf16_t* Vs = Ks + MP * LDK;          // [MP][LDK]
  bf16_t* Kt = Vs + MP * LDK;          // [DH][LDM]
  bf16_t* W0 = Kt + DH * LDM;          // 4 x WAVE_ELEMS
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int bh = CHUNK ? blockIdx.y : blockIdx.x, bi = bh / heads, h = bh % heads, inner = heads * DH;
  const int key0 = CHUNK ? (int)blockIdx.x * MP : 0;   // first key of this workgroup
  const bf16_t* kb = kv + ((int64_t)bi * m + key0) * ldkv + h * DH;
  const bf16_t* vb = kb + inner;
  const int m_all = m;
  m = min(MP, m_all - key0);                           // live keys of this workgroup (all of them without CHUNK)
  for (int i = tid; i < MP * DH; i += 256) {
    const int key = i / DH, d = i % DH;
    const bool in = key < m;
    const bf16_t kk = in ? kb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
    Ks[key * LDK + d] = kk;
    Kt[d * LDM + key] = kk;
    Vs[key * LDK + d] = in ? vb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
  }
  __syncthreads();
  bf16_t* dSs = W0 + wave * WAVE_ELEMS;   // [QT][LDM]  dS, query-major
  bf16_t* PsT = dSs + QT * LDM;           // [MP][LDQ]  P^T, key-major
  bf16_t* dSsT = PsT + MP * LDQ;          // [MP][LDQ]
  bf16_t* Qt = dSsT + MP * LDQ;           // [DH][LDQ]  Q^T of the tile
  bf16_t* dOt = Qt + DH * LDQ;            // [DH][LDQ]
  float* Dl = (float*)(dOt + DH * LDQ);   // [QT]
  const bf16_t* qb = q + (int64_t)bi * n * ldq + h * DH;
  const bf16_t* ob = o + (int64_t)bi * n * ldo + h * DH;
  const bf16_t* dob = d_o + (int64_t)bi * n * lddo + h * DH;
  bf16_t* dqb = dq + (int64_t)bi * n * lddq + h * DH;
  f32x4 dk[JT][4], dv[JT][4];
  for (int jt = 0; jt < JT; ++jt)
    for (int nt = 0; nt < 4; ++nt) dk[jt][nt] = dv[jt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntiles = (n + QT - 1) / QT;
  for (int t0 = 0; t0 < ntiles; t0 += 4) {
    const int q0 = (t0 + wave) * QT;
    // Q^T and dO^T of the tile (zero rows beyond n), D = rowsum(dO * O)
    for (int i = l; i < QT * 8; i += 64) {
      const int ql = i >> 3, ch = i & 7, row = q0 + ql;
      const bool in = row < n;
      const int rr = min(row, n - 1);
      const bf16x8 qv = *(const bf16x8*)(qb + (int64_t)rr * ldq + ch * 8);
      const bf16x8 gv = *(const bf16x8*)(dob + (int64_t)rr * lddo + ch * 8);
      for (int j = 0; j < 8; ++j) {
        Qt[(ch * 8 + j) * LDQ + ql] = in ? qv[j] : (bf16_t)0.f;
        dOt[(ch * 8 + j) * LDQ + ql] = in ? gv[j] : (bf16_t)0.f;
      }
    }
    for (int mt = 0; mt < 2; ++mt) {
      const int rr = min(q0 + mt * 16 + c, n - 1);
      float a = 0.f;
      for (int ch = 0; ch < 2; ++ch) {
        const bf16x8 ov = *(const bf16x8*)(ob + (int64_t)rr * ldo + g * 16 + ch * 8);
        const bf16x8 gv = *(const bf16x8*)(dob + (int64_t)rr * lddo + g * 16 + ch * 8);
        for (int j = 0; j < 8; ++j) a += (float)ov[j] * (float)gv[j];
      }
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (g == 0) Dl[mt * 16 + c] = a;
    }
    f32x4 s[2][JT], dp[2][JT];
    scores<MP>(qb, ldq, q0, n, Ks, LDK, s, c, g);
    scores<MP>(dob, lddo, q0, n, Vs, LDK, dp, c, g);
    __syncthreads();   // D of this tile is visible
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) {
        const int ql = mt * 16 + 4 * g + r, row = q0 + ql;
        const bool in = row < n;
        const float ls = lse[(int64_t)bh * n + min(row, n - 1)], dd = Dl[ql];
        for (int jt = 0; jt < JT; ++jt) {
          const int key = jt * 16 + c;
          const float p = (in && key < m) ? __expf(s[mt][jt][r] * scale - ls) : 0.f;
          const float ds = p * (dp[mt][jt][r] - dd);
          PsT[key * LDQ + ql] = (bf16_t)p;
          dSsT[key * LDQ + ql] = (bf16_t)ds;
          dSs[ql * LDM + key] = (bf16_t)ds;
        }
      }
    __syncthreads();
    // dq = scale dS K
    if (!CHUNK)
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 acc[4];
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < MP / 32; ++ks) {
        const bf16x8 a = frag(dSs, mt * 16, LDM, ks * 32, c, g);
        for (int nt = 0; nt < 4; ++nt) acc[nt] = mma(a, frag(Kt, nt * 16, LDM, ks * 32, c, g), acc[nt]);
      }
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + mt * 16 + 4 * g + r;
        if (row < n)
          for (int nt = 0; nt < 4; ++nt) dqb[(int64_t)row * lddq + nt * 16 + c] = (bf16_t)(acc[nt][r] * scale);
      }
    }
    // dv += P^T dO, dk += dS^T Q (the 32 queries of the tile are the K extent)
    for (int jt = 0; jt < JT; ++jt) {
      const bf16x8 ap = frag(PsT, jt * 16, LDQ, 0, c, g), as = frag(dSsT, jt * 16, LDQ, 0, c, g);
      for (int nt = 0; nt < 4; ++nt) {
        dv[jt][nt] = mma(ap, frag(dOt, nt * 16, LDQ, 0, c, g), dv[jt][nt]);
        dk[jt][nt] = mma(as, frag(Qt, nt * 16, LDQ, 0, c, g), dk[jt][nt]);
      }
    }
    __syncthreads();
  }
  // the four waves' accumulators in wave order, through LDS (the per-wave scratch is free now)
  float* R = (float*)W0;   // [MP][DH]
  bf16_t* dkb = dkv + ((int64_t)bi * m_all + key0) * lddkv + h * DH;
  for (int which = 0; which < 2; ++which) {
    for (int w = 1; w < 4; ++w) {
      if (wave == w)
        for (int jt = 0; jt < JT; ++jt)
          for (int nt = 0; nt < 4; ++nt)
            for (int r = 0; r < 4; ++r) R[(jt * 16 + 4 * g + r) * DH + nt * 16 + c] = which ? dv[jt][nt][r] : dk[jt][nt][r];
      __syncthreads();
      if (wave == 0)
        for (int jt = 0; jt < JT; ++jt)
          for (int nt = 0; nt < 4; ++nt)
            for (int r = 0; r < 4; ++r) {
              const float v = R[(jt * 16 + 4 * g + r) * DH + nt * 16 + c];
              if (which) dv[jt][nt][r] += v; else dk[jt][nt][r] += v;
            }
      __syncthreads();
    }
    if (wave == 0)
      for (int jt = 0; jt < JT; ++jt)
        for (int r = 0; r < 4; ++r) {
          const int key = jt * 16 + 4 * g + r;
          if (key < m)
            for (int nt = 0; nt < 4; ++nt)
              dkb[(int64_t)key * lddkv + (which ? inner : 0) + nt * 16 + c] = (bf16_t)(which ? dv[jt][nt][r] : dk[jt][nt][r] * scale);
        }
  }
}

template <int MP> constexpr int fwd_smem() { return (MP * LDK + DH * (MP + 8) + 4 * QT * (MP + 8)) * 2; }
template <int MP> constexpr int bwd_smem() { return (2 * MP * LDK + DH * (MP + 8) + 4 * (QT * (MP + 8) + 2 * MP * LDQ + 2 * DH * LDQ + 64)) * 2; }
static_assert(bwd_smem<64>() <= 160 * 1024 && 4 * (QT * 72 + 2 * 64 * LDQ + 2 * DH * LDQ + 64) * 2 >= 64 * DH * 4, "LDS budget; the reduction tile fits the scratch");
static_assert(4 * (QT * 40 + 2 * 32 * LDQ + 2 * DH * LDQ + 64) * 2 >= 32 * DH * 4, "the reduction tile fits the scratch (32 keys)");

// ------------------------------------------------------------------------------------------------ many keys
constexpr int KC = 64, LDC = KC + 8;   // keys per chunk; row stride of a wave's [QT][KC] tile of P or dS

// mp = m rounded up to KC: every chunk has at least one live key
__global__ __launch_bounds__(256) void attn_manykey_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, bf16_t* __restrict__ o,
                                                               float* __restrict__ lse, int n, int m, int mp, int heads, int64_t ldq, int64_t ldkv, int64_t ldo,
                                                               float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldv = mp + 8;
  bf16_t* Ks = (bf16_t*)smem;          // [mp][LDK]   key-major
  bf16_t* Vt = Ks + mp * LDK;          // [DH][ldv]   d-major
  bf16_t* Ps = Vt + DH * ldv;          // [4][QT][LDC]
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int bh = blockIdx.y, bi = bh / heads, h = bh % heads, inner = heads * DH;
  const bf16_t* kb = kv + (int64_t)bi * m * ldkv + h * DH;
  const bf16_t* vb = kb + inner;
  for (int i = tid; i < mp * DH; i += 256) {
    const int key = i / DH, d = i % DH;
    const bool in = key < m;
    Ks[key * LDK + d] = in ? kb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
    Vt[d * ldv + key] = in ? vb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
  }
  __syncthreads();
  bf16_t* P = Ps + wave * QT * LDC;
  const bf16_t* qb = q + (int64_t)bi * n * ldq + h * DH;
  bf16_t* ob = o + (int64_t)bi * n * ldo + h * DH;
  const int ntiles = (n + QT - 1) / QT;
  for (int t0 = blockIdx.x * 4; t0 < ntiles; t0 += gridDim.x * 4) {   // (the same trip count for every wave: the barriers below are uniform)
    const int q0 = (t0 + wave) * QT;
    float mx[2][4], sm[2][4];
    f32x4 acc[2][4];
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) { mx[mt][r] = -INFINITY; sm[mt][r] = 0.f; acc[mt][r] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kc = 0; kc < mp; kc += KC) {
      f32x4 s[2][KC / 16];
      scores<KC>(qb, ldq, q0, n, Ks + kc * LDK, LDK, s, c, g);
      for (int mt = 0; mt < 2; ++mt)
        for (int r = 0; r < 4; ++r) {
          const int ql = mt * 16 + 4 * g + r;
          float cm = -INFINITY;
          for (int jt = 0; jt < KC / 16; ++jt) {
            const float v = (kc + jt * 16 + c) < m ? s[mt][jt][r] * scale : -INFINITY;
            s[mt][jt][r] = v;
            cm = fmaxf(cm, v);
          }
          const float nm = fmaxf(mx[mt][r], row_max16(cm));   // (key kc is always live: finite from the first chunk on)
          const float corr = __expf(mx[mt][r] - nm);          // (first chunk: exp(-inf) = 0 on a zero accumulator)
          float ps = 0.f;
          for (int jt = 0; jt < KC / 16; ++jt) {
            const float p = __expf(s[mt][jt][r] - nm);
            ps += p;
            P[ql * LDC + jt * 16 + c] = (bf16_t)p;
          }
          sm[mt][r] = sm[mt][r] * corr + row_sum16(ps);
          mx[mt][r] = nm;
          for (int nt = 0; nt < 4; ++nt) acc[mt][nt][r] *= corr;
        }
      __syncthreads();
      for (int mt = 0; mt < 2; ++mt)
        for (int ks = 0; ks < KC / 32; ++ks) {
          const bf16x8 a = frag(P, mt * 16, LDC, ks * 32, c, g);
          for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mma(a, frag(Vt, nt * 16, ldv, kc + ks * 32, c, g), acc[mt][nt]);
        }
      __syncthreads();
    }
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + mt * 16 + 4 * g + r;
        if (row >= n) continue;
        const float inv = 1.0f / sm[mt][r];
        for (int nt = 0; nt < 4; ++nt) ob[(int64_t)row * ldo + nt * 16 + c] = (bf16_t)(acc[mt][nt][r] * inv);
        if (c == 0) lse[(int64_t)bh * n + row] = mx[mt][r] + __logf(sm[mt][r]);
      }
  }
}

__global__ __launch_bounds__(256) void attn_manykey_dq_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, const bf16_t* __restrict__ o,
                                                              const bf16_t* __restrict__ d_o, const float* __restrict__ lse, bf16_t* __restrict__ dq, int n, int m,
                                                              int mp, int heads, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddo, int64_t lddq, float scale) {
  constexpr int WAVE_ELEMS = QT * LDC + 64;   // bf16 elements of one wave's scratch (the last 64: 32 floats of D)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldt = mp + 8;
  bf16_t* Ks = (bf16_t*)smem;          // [mp][LDK]
  bf16_t* Vs = Ks + mp * LDK;          // [mp][LDK]
  bf16_t* Kt = Vs + mp * LDK;          // [DH][ldt]
  bf16_t* W0 = Kt + DH * ldt;          // 4 x WAVE_ELEMS
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int bh = blockIdx.y, bi = bh / heads, h = bh % heads, inner = heads * DH;
  const bf16_t* kb = kv + (int64_t)bi * m * ldkv + h * DH;
  const bf16_t* vb = kb + inner;
  for (int i = tid; i < mp * DH; i += 256) {
    const int key = i / DH, d = i % DH;
    const bool in = key < m;
    const bf16_t kk = in ? kb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
    Ks[key * LDK + d] = kk;
    Kt[d * ldt + key] = kk;
    Vs[key * LDK + d] = in ? vb[(int64_t)key * ldkv + d] : (bf16_t)0.f;
  }
  __syncthreads();
  bf16_t* dSs = W0 + wave * WAVE_ELEMS;   // [QT][LDC]  dS of one key chunk, query-major
  float* Dl = (float*)(dSs + QT * LDC);   // [QT]
  const bf16_t* qb = q + (int64_t)bi * n * ldq + h * DH;
  const bf16_t* ob = o + (int64_t)bi * n * ldo + h * DH;
  const bf16_t* dob = d_o + (int64_t)bi * n * lddo + h * DH;
  bf16_t* dqb = dq + (int64_t)bi * n * lddq + h * DH;
  const int ntiles = (n + QT - 1) / QT;
  for (int t0 = blockIdx.x * 4; t0 < ntiles; t0 += gridDim.x * 4) {   // (the same trip count for every wave: the barriers below are uniform)
    const int q0 = (t0 + wave) * QT;
    for (int mt = 0; mt < 2; ++mt) {   // D = rowsum(dO * O)
      const int rr = min(q0 + mt * 16 + c, n - 1);
      float a = 0.f;
      for (int ch = 0; ch < 2; ++ch) {
        const bf16x8 ov = *(const bf16x8*)(ob + (int64_t)rr * ldo + g * 16 + ch * 8);
        const bf16x8 gv = *(const bf16x8*)(dob + (int64_t)rr * lddo + g * 16 + ch * 8);
        for (int j = 0; j < 8; ++j) a += (float)ov[j] * (float)gv[j];
      }
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (g == 0) Dl[mt * 16 + c] = a;
    }
    __syncthreads();   // D of this tile is visible
    float ls[2][4], dd[2][4];
    f32x4 acc[2][4];
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) {
        const int ql = mt * 16 + 4 * g + r;
        ls[mt][r] = lse[(int64_t)bh * n + min(q0 + ql, n - 1)];
        dd[mt][r] = Dl[ql];
        acc[mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    for (int kc = 0; kc < mp; kc += KC) {
      f32x4 s[2][KC / 16], dp[2][KC / 16];
      scores<KC>(qb, ldq, q0, n, Ks + kc * LDK, LDK, s, c, g);
      scores<KC>(dob, lddo, q0, n, Vs + kc * LDK, LDK, dp, c, g);
      for (int mt = 0; mt < 2; ++mt)
        for (int r = 0; r < 4; ++r) {
          const int ql = mt * 16 + 4 * g + r;
          const bool in = q0 + ql < n;
          for (int jt = 0; jt < KC / 16; ++jt) {
            const float p = (in && kc + jt * 16 + c < m) ? __expf(s[mt][jt][r] * scale - ls[mt][r]) : 0.f;
            dSs[ql * LDC + jt * 16 + c] = (bf16_t)(p * (dp[mt][jt][r] - dd[mt][r]));
          }
        }
      __syncthreads();
      for (int mt = 0; mt < 2; ++mt)
        for (int ks = 0; ks < KC / 32; ++ks) {
          const bf16x8 a = frag(dSs, mt * 16, LDC, ks * 32, c, g);
          for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mma(a, frag(Kt, nt * 16, ldt, kc + ks * 32, c, g), acc[mt][nt]);
        }
      __syncthreads();
    }
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) {
        const int row = q0 + mt * 16 + 4 * g + r;
        if (row < n)
          for (int nt = 0; nt < 4; ++nt) dqb[(int64_t)row * lddq + nt * 16 + c] = (bf16_t)(acc[mt][nt][r] * scale);
      }
  }
}

constexpr int manykey_fwd_smem(int mp) { return (mp * LDK + DH * (mp + 8) + 4 * QT * LDC) * 2; }
constexpr int manykey_dq_smem(int mp) { return (2 * mp * LDK + DH * (mp + 8) + 4 * (QT * LDC + 64)) * 2; }
// The key count all three kernels hold: the d(q) kernel is the largest (K, V and K^T of every key: 416 bytes a key, and 19968 of per-wave
// scratch and padding), the d(k) / d(v) kernel is the 64-key few-key one whatever m is.  The largest multiple of the 64-key chunk under 160 KiB:
constexpr int LDS_BUDGET = 160 * 1024;
static_assert(manykey_dq_smem(MANYKEY_MAX) <= LDS_BUDGET && manykey_dq_smem(MANYKEY_MAX + KC) > LDS_BUDGET, "MANYKEY_MAX is what the d(q) kernel's LDS holds");
static_assert(manykey_fwd_smem(MANYKEY_MAX) <= manykey_dq_smem(MANYKEY_MAX) && MANYKEY_MAX % KC == 0 && MANYKEY_MAX >= 196, "forward fits too; CvT's 196 keys fuse");

}  // namespace

bool attn_fewkey_supported(int nq, int nk, int dim_head) { return dim_head == DH && nq >= 1 && nk >= 1 && nk <= 64; }

void launch_attn_fewkey_fwd(const bf16_t* q, const bf16_t* kv, bf16_t* o, float* lse, int b, int nq, int nk, int heads, int64_t ldq, int64_t ldkv,
                            int64_t ldo, float scale, hipStream_t s) {
  const int ntiles = (nq + QT - 1) / QT;
  // enough workgroups to fill the chip when there are few (image, head) pairs; each restages K and V, so no more than that
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + 3) / 4, 1024 / std::max(1, b * heads)));
  const dim3 grid((unsigned)chunks, (unsigned)(b * heads));
  if (nk <= 32) {
    vitx_set_max_smem((const void*)attn_fewkey_fwd_kernel<32>, fwd_smem<32>());
    hipLaunchKernelGGL(attn_fewkey_fwd_kernel<32>, grid, dim3(256), fwd_smem<32>(), s, q, kv, o, lse, nq, nk, heads, ldq, ldkv, ldo, scale);
  } else {
    vitx_set_max_smem((const void*)attn_fewkey_fwd_kernel<64>, fwd_smem<64>());
    hipLaunchKernelGGL(attn_fewkey_fwd_kernel<64>, grid, dim3(256), fwd_smem<64>(), s, q, kv, o, lse, nq, nk, heads, ldq, ldkv, ldo, scale);
  }
}

bool attn_manykey_supported(int nq, int nk, int dim_head) { return dim_head == DH && nq >= 1 && nk > 64 && nk <= MANYKEY_MAX; }

// workgroups along the query axis: enough to fill the chip when there are few (image, head) pairs; each restages K and V, so no more than that
static int manykey_query_chunks(int nq, int bh) {
  const int ntiles = (nq + QT - 1) / QT;
  return (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + 3) / 4, 1024 / std::max(1, bh)));
}

void launch_attn_manykey_fwd(const bf16_t* q, const bf16_t* kv, bf16_t* o, float* lse, int b, int nq, int nk, int heads, int64_t ldq, int64_t ldkv,
                             int64_t ldo, float scale, hipStream_t s) {
  const int mp = (nk + KC - 1) / KC * KC;
  const dim3 grid((unsigned)manykey_query_chunks(nq, b * heads), (unsigned)(b * heads));
  vitx_set_max_smem((const void*)attn_manykey_fwd_kernel, manykey_fwd_smem(MANYKEY_MAX));
  hipLaunchKernelGGL(attn_manykey_fwd_kernel, grid, dim3(256), manykey_fwd_smem(mp), s, q, kv, o, lse, nq, nk, mp, heads, ldq, ldkv, ldo, scale);
}

void launch_attn_manykey_bwd(const bf16_t* q, const bf16_t* kv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dq, bf16_t* dkv, int b, int nq,
                             int nk, int heads, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddkv, float scale, hipStream_t s) {
  const int mp = (nk + KC - 1) / KC * KC;
  // d(k) / d(v): one workgroup per 64-key chunk of an (image, head)
  vitx_set_max_smem((const void*)attn_fewkey_bwd_kernel<KC, true>, bwd_smem<KC>());
  hipLaunchKernelGGL((attn_fewkey_bwd_kernel<KC, true>), dim3((unsigned)(mp / KC), (unsigned)(b * heads)), dim3(256), bwd_smem<KC>(), s, q, kv, o, d_o, lse, dq, dkv,
                     nq, nk, heads, ldq, ldkv, ldo, lddo, lddq, lddkv, scale);
  // d(q)
  const dim3 grid((unsigned)manykey_query_chunks(nq, b * heads), (unsigned)(b * heads));
  vitx_set_max_smem((const void*)attn_manykey_dq_kernel, manykey_dq_smem(MANYKEY_MAX));
  hipLaunchKernelGGL(attn_manykey_dq_kernel, grid, dim3(256), manykey_dq_smem(mp), s, q, kv, o, d_o, lse, dq, nq, nk, mp, heads, ldq, ldkv, ldo, lddo, lddq, scale);
}

void launch_attn_fewkey_bwd(const bf16_t* q, const bf16_t* kv, const bf16_t* o, const bf16_t* d_o, const float* lse, bf16_t* dq, bf16_t* dkv, int b, int nq,
                            int nk, int heads, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddkv, float scale, hipStream_t s) {
  const dim3 grid((unsigned)(b * heads));
  if (nk <= 32) {
    vitx_set_max_smem((const void*)attn_fewkey_bwd_kernel<32>, bwd_smem<32>());
    hipLaunchKernelGGL(attn_fewkey_bwd_kernel<32>, grid, dim3(256), bwd_smem<32>(), s, q, kv, o, d_o, lse, dq, dkv, nq, nk, heads, ldq, ldkv, ldo, lddo, lddq,
                       lddkv, scale);
  } else {
    vitx_set_max_smem((const void*)attn_fewkey_bwd_kernel<64>, bwd_smem<64>());
    hipLaunchKernelGGL(attn_fewkey_bwd_kernel<64>, grid, dim3(256), bwd_smem<64>(), s, q, kv, o, d_o, lse, dq, dkv, nq, nk, heads, ldq, ldkv, ldo, lddo, lddq,
                       lddkv, scale);
  }
}
