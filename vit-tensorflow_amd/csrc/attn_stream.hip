// Streamed-key fused attention (vit.py:73-82) for sequences past the 288 tokens the kernels of attn_bf16.hip hold in LDS: bf16 storage,
// dim_head 64, packed qkv [b, n, 3, h, 64] as the to_qkv Dense emits it, o [b, n, h * 64], lse [b, h, n] = max + log(sum) of the scaled scores
// (natural log, as attn_bf16.hip writes it).  The [b, h, n, n] score matrix is never written to HBM and no kernel's LDS depends on n.
//
// All three kernels walk the OTHER axis of the score matrix in chunks of 64 rows that pass through a double-buffered LDS ring: two stages of two
// swizzled row-major [64][128 B] images (attn_lds.h), filled with direct-to-LDS loads (inline asm, see stage_img).  The loads of chunk c + 1 are issued before chunk c is
// multiplied and are waited for (s_waitcnt vmcnt(0) + barrier) only behind it; that one barrier per chunk also retires the stage the chunk after
// next overwrites.  Operand layouts and the arithmetic of a tile pair are those of attn_bf16.hip: scores transposed (S^T = K Q^T) so that a lane
// owns one query column, P / dS straight from registers into the second product, the transposed operand through ds_read_b64_tr_b16.
//   forward   grid (query chunks of 128, b * h), 4 waves x 32 queries.  K and V chunks are streamed; online softmax per query column: running
//             maximum and sum, the O^T accumulators rescaled in registers; o and lse are written once.
//   d(q)      grid (query chunks of 128, b * h), 8 waves x 16 queries.  K and V chunks are streamed; P = exp(s - lse) from the saved lse,
//             D = rowsum(dO * O) from the wave's own rows (also written to the dsum workspace for the next kernel), dS = P (dP - D) scale,
//             dq^T += K^T dS^T in registers, written once.
//   d(k, v)   grid (key chunks of 128, b * h), 8 waves x 16 keys.  Q and dO chunks (with their lse and D) are streamed; dv^T += dO^T P,
//             dk^T += Q^T dS in registers, written once.  A wave owns its keys alone, so no cross-wave reduction exists.
// Every sum runs in a fixed order (chunks ascending, the MFMA's own order inside a tile): same input, same bits.
// Masking, never padding: rows of the last chunk past n are staged from the clamped row n - 1 (finite) and masked where they are used.  Forward:
// keys >= n get a score of -inf (P = 0); d(q): P = 0; d(k, v): P = 0 for query rows >= n (lse = D = 0 there), so dS = 0 as well.  Query (key)
// lanes >= n compute on the clamped row n - 1 and are never stored.
#include <cmath>

#include "kernels.h"
#include "attn_lds.h"

namespace {

using namespace attn_lds;

constexpr int KC = 64;                    // rows of a streamed chunk
constexpr int IMG_B = KC * ROWB;          // one [64][128 B] image
constexpr int STAGE_B = 2 * IMG_B;        // K | V (or Q | dO) of one chunk
constexpr int RING_B = 2 * STAGE_B;       // two stages
constexpr int FWD_WAVES = 4, FWD_QB = 2, FWD_QROWS = FWD_WAVES * FWD_QB * 16;   // 128 queries per workgroup
constexpr int BWD_WAVES = 8, BWD_ROWS = BWD_WAVES * 16;                          // 128 queries (keys) per workgroup
constexpr int DKV_LDS_B = RING_B + 2 * 2 * KC * 4;                               // + two stages of (lse | D) of a query chunk
// LDS per workgroup, whatever n is: 32 KiB (forward, d(q)) and 33 KiB (d(k, v)) of the 160 KiB -- four workgroups per CU by LDS
static_assert(RING_B == 32 * 1024 && DKV_LDS_B == 33 * 1024 && 4 * DKV_LDS_B <= 160 * 1024, "LDS budget of the streamed attention kernels");
constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;

// One [64][64] bf16 chunk image (rows row0 .. row0 + 63 of a matrix whose rows lie `stride_b` bytes apart behind `rsrc`) into the swizzled row-major
// LDS image at `img`: 8 direct-to-LDS pieces of 1 KiB (8 rows) shared among the waves.  The image is lane-linear, so the swizzle of attn_lds.h goes
// on the per-lane SOURCE chunk.  Rows >= n read the clamped row n - 1 (finite data that every consumer masks).  The loads are issued through
// vitx_dma16 (common.h), not the builtin of attn_lds::stage_head_dma: the compiler's wait-count pass answers the builtin with a full
// s_waitcnt vmcnt(0) in front of the next LDS read, which drains the chunk in flight and un-streams the loop; the asm form is invisible to that
// pass, and the only wait on these loads is ring_wait's own.
__device__ __forceinline__ void stage_img(i32x4 rsrc, uint32_t stride_b, int row0, int n, const char* img, int wave, int lane, int nwaves) {
  const uint32_t dst = vitx_lds_addr(img);
#pragma unroll
  for (int i = wave; i < KC / 8; i += nwaves) {
    const int r = i * 8 + (lane >> 3);
    const int c = (lane & 7) ^ swz_key(r);
    vitx_dma16(rsrc, dst + i * 1024, (uint32_t)min(row0 + r, n - 1) * stride_b + c * 16, 0);
  }
}
// chunk `ch` of two matrices into stage `ch & 1` of the ring
__device__ __forceinline__ void stage_chunk(i32x4 ra, uint32_t stride_a, i32x4 rb, uint32_t stride_b, int ch, int n, const char* ring, int wave, int lane,
                                            int nwaves) {
  const char* st = ring + (ch & 1) * STAGE_B;
  stage_img(ra, stride_a, ch * KC, n, st, wave, lane, nwaves);
  stage_img(rb, stride_b, ch * KC, n, st + IMG_B, wave, lane, nwaves);
}
// A register use the compiler cannot move: the wait for the global load behind `v` is placed HERE, in front of the chunk loop.  Left to its first
// real use the wait lands inside the loop, where a vmcnt(0) also drains the chunk just put in flight (hardware counts the asm loads too).
template <typename T>
__device__ __forceinline__ void land(T& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void ring_wait() {   // every load of this wave has landed; every wave is done with the stage read last
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// ------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(FWD_WAVES * 64) void attn_stream_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o, float* __restrict__ lse,
                                                                         int n, int h, float scale) {
  constexpr int QB = FWD_QB;
  __shared__ __attribute__((aligned(1024))) char ring[RING_B];
  const int bh = blockIdx.y, bi = bh / h, hi = bh - bi * h;
  const int64_t inner = (int64_t)h * DH, tok_stride = 3 * inner;
  const bf16_t* qbase = qkv + (int64_t)bi * n * tok_stride + hi * DH;
  const int tid = threadIdx.x, lane = tid & 63, qi = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (n + KC - 1) / KC;
  const i32x4 rk = vitx_make_rsrc(qbase + inner), rv = vitx_make_rsrc(qbase + 2 * inner);   // this (image, head)'s k and v rows
  const uint32_t sb = (uint32_t)tok_stride * 2;
  stage_chunk(rk, sb, rv, sb, 0, n, ring, wave, lane, FWD_WAVES);
  const int q0 = blockIdx.x * FWD_QROWS + wave * (16 * QB);
  bf16x8 qf[QB][2];
#pragma unroll
  for (int s = 0; s < QB; ++s) {
    const int qc = min(q0 + s * 16 + qi, n - 1);   // rows >= n compute on the clamped row n - 1 and are never stored
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[s][ks] = *(const bf16x8*)(qbase + (int64_t)qc * tok_stride + (g + 4 * ks) * 8);
  }
#pragma unroll
  for (int s = 0; s < QB; ++s) { land(qf[s][0]); land(qf[s][1]); }
  const float sl2 = scale * LOG2E;
  float m[QB], lv[QB];   // running maximum (log2 domain, the same in the four lanes of a query) and this lane's share of the running sum
  f32x4 oacc[QB][4];
#pragma unroll
  for (int s = 0; s < QB; ++s) {
    m[s] = -INFINITY; lv[s] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) oacc[s][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ring_wait();
#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    if (ch + 1 < nch) stage_chunk(rk, sb, rv, sb, ch + 1, n, ring, wave, lane, FWD_WAVES);
    const char* k_rm = ring + (ch & 1) * STAGE_B;
    const char* v_rm = k_rm + IMG_B;
    const int live = n - ch * KC;   // keys of this chunk below n (>= 1)
    // S^T of the chunk: a[t][s][r] = S[query qi of block s][key 16 t + 4 g + r]
    f32x4 a[4][QB];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 k0 = frag_rm(k_rm, t * 16 + qi, g), k1 = frag_rm(k_rm, t * 16 + qi, g + 4);
#pragma unroll
      for (int s = 0; s < QB; ++s) a[t][s] = mfma16(k0, qf[s][0], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int s = 0; s < QB; ++s) a[t][s] = mfma16(k1, qf[s][1], a[t][s]);
    }
    if (live < KC) {   // (the last chunk only)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < QB; ++s)
#pragma unroll
          for (int r = 0; r < 4; ++r) a[t][s][r] = (t * 16 + 4 * g + r) < live ? a[t][s][r] : -INFINITY;
    }
    bf16x8 pf[QB][2];
#pragma unroll
    for (int s = 0; s < QB; ++s) {
      float cm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) cm = fmaxf(fmaxf(cm, fmaxf(a[t][s][0], a[t][s][1])), fmaxf(a[t][s][2], a[t][s][3]));
      cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      const float nm = fmaxf(m[s], cm * sl2);     // (key 64 ch is always live: finite from the first chunk on)
      const float corr = fast_exp2(m[s] - nm);    // (first chunk: 2^-inf = 0 on zero accumulators)
      m[s] = nm;
      float ps = 0.f;
      f32x4 p[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[t][r] = fast_exp2(a[t][s][r] * sl2 - nm);   // masked keys: 2^-inf = 0
        ps += (p[t][0] + p[t][1]) + (p[t][2] + p[t][3]);
      }
      lv[s] = lv[s] * corr + ps;
#pragma unroll
      for (int c = 0; c < 4; ++c) oacc[s][c] *= corr;
      pf[s][0] = pack8(p[0], p[1]);
      pf[s][1] = pack8(p[2], p[3]);
    }
    // O^T += V^T P^T: k-slot (g, e) of pair u <-> key 32 u + 4 g + e | 32 u + 16 + 4 g + (e - 4), the same permutation on both operands
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 vf = frag_trr(v_rm, c, u, lane);
#pragma unroll
        for (int s = 0; s < QB; ++s) oacc[s][c] = mfma16(vf, pf[s][u], oacc[s][c]);
      }
    ring_wait();
  }
#pragma unroll
  for (int s = 0; s < QB; ++s) {
    const int q = q0 + s * 16 + qi;
    float ls = lv[s];
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    const float inv_l = 1.0f / ls;
    if (q < n) {
      if (g == 0) lse[(int64_t)bh * n + q] = (m[s] + log2f(ls)) * LN2;
      bf16_t* op = o + ((int64_t)bi * n + q) * inner + hi * DH;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (bf16_t)(oacc[s][c][r] * inv_l);
        *(bf16x4*)(op + 16 * c + 4 * g) = ov;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ d(q)
__global__ __launch_bounds__(BWD_WAVES * 64) void attn_stream_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                                        const bf16_t* __restrict__ d_o, const float* __restrict__ lse,
                                                                        float* __restrict__ dsum, bf16_t* __restrict__ dqkv, int n, int h, float scale) {
  __shared__ __attribute__((aligned(1024))) char ring[RING_B];
  const int bh = blockIdx.y, bi = bh / h, hi = bh - bi * h;
  const int64_t inner = (int64_t)h * DH, tok_stride = 3 * inner;
  const bf16_t* qbase = qkv + (int64_t)bi * n * tok_stride + hi * DH;
  const int tid = threadIdx.x, lane = tid & 63, qi = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (n + KC - 1) / KC;
  const i32x4 rk = vitx_make_rsrc(qbase + inner), rv = vitx_make_rsrc(qbase + 2 * inner);   // this (image, head)'s k and v rows
  const uint32_t sb = (uint32_t)tok_stride * 2;
  stage_chunk(rk, sb, rv, sb, 0, n, ring, wave, lane, BWD_WAVES);
  const int q = blockIdx.x * BWD_ROWS + wave * 16 + qi, qc = min(q, n - 1);
  const int64_t orow = ((int64_t)bi * n + qc) * inner + hi * DH;
  bf16x8 qf[2], dof[2];
  float d = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    qf[ks] = *(const bf16x8*)(qbase + (int64_t)qc * tok_stride + (g + 4 * ks) * 8);
    dof[ks] = *(const bf16x8*)(d_o + orow + (g + 4 * ks) * 8);
    const bf16x8 of = *(const bf16x8*)(o + orow + (g + 4 * ks) * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) d += (float)dof[ks][e] * (float)of[e];
  }
  d += __shfl_xor(d, 16, 64);
  d += __shfl_xor(d, 32, 64);   // D[q] = sum_d dO * O
  if (g == 0 && q < n) dsum[(int64_t)bh * n + q] = d;
  float lse2 = lse[(int64_t)bh * n + qc] * LOG2E;
  land(qf[0]); land(qf[1]); land(dof[0]); land(dof[1]); land(lse2);
  const float sl2 = scale * LOG2E, nds = -d * scale;
  f32x4 dq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dq[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  ring_wait();
#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    if (ch + 1 < nch) stage_chunk(rk, sb, rv, sb, ch + 1, n, ring, wave, lane, BWD_WAVES);
    const char* k_rm = ring + (ch & 1) * STAGE_B;
    const char* v_rm = k_rm + IMG_B;
    const int live = n - ch * KC;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x4 ds[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int row = (2 * u + tt) * 16 + qi;
        f32x4 sa = mfma16(frag_rm(k_rm, row, g), qf[0], f32x4{0.f, 0.f, 0.f, 0.f});
        f32x4 dp = mfma16(frag_rm(v_rm, row, g), dof[0], f32x4{0.f, 0.f, 0.f, 0.f});
        sa = mfma16(frag_rm(k_rm, row, g + 4), qf[1], sa);
        dp = mfma16(frag_rm(v_rm, row, g + 4), dof[1], dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = fast_exp2(sa[r] * sl2 - lse2);
          p = ((2 * u + tt) * 16 + 4 * g + r) < live ? p : 0.f;
          ds[tt][r] = p * (dp[r] * scale + nds);
        }
      }
      const bf16x8 dsf = pack8(ds[0], ds[1]);
#pragma unroll
      for (int c = 0; c < 4; ++c) dq[c] = mfma16(frag_trr(k_rm, c, u, lane), dsf, dq[c]);   // dQ^T += K^T dS^T
    }
    ring_wait();
  }
  if (q < n) {
    bf16_t* out = dqkv + ((int64_t)bi * n + q) * tok_stride + hi * DH;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = (bf16_t)dq[c][r];
      *(bf16x4*)(out + 16 * c + 4 * g) = ov;
    }
  }
}

// ------------------------------------------------------------------------------------------ d(k), d(v)
__global__ __launch_bounds__(BWD_WAVES * 64) void attn_stream_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_o,
                                                                         const float* __restrict__ lse, const float* __restrict__ dsum,
                                                                         bf16_t* __restrict__ dqkv, int n, int h, float scale) {
  __shared__ __attribute__((aligned(1024))) char ring[DKV_LDS_B];
  float* stats = (float*)(ring + RING_B);   // [2 stages][lse (log2 domain) | D][64 queries], rows >= n: 0 (a finite exponent for the masked P)
  const int bh = blockIdx.y, bi = bh / h, hi = bh - bi * h;
  const int64_t inner = (int64_t)h * DH, tok_stride = 3 * inner;
  const bf16_t* qbase = qkv + (int64_t)bi * n * tok_stride + hi * DH;
  const bf16_t* dobase = d_o + (int64_t)bi * n * inner + hi * DH;
  const int tid = threadIdx.x, lane = tid & 63, ki = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (n + KC - 1) / KC;
  const i32x4 rq = vitx_make_rsrc(qbase), rdo = vitx_make_rsrc(dobase);
  stage_chunk(rq, (uint32_t)tok_stride * 2, rdo, (uint32_t)inner * 2, 0, n, ring, wave, lane, BWD_WAVES);
  // threads with (tid & 64) == 0: lse of the chunk's queries, the others: D.  Every thread loads and writes (four threads per slot, the same value):
  // a load whose only use is conditional is sunk into that branch by the compiler, behind the products, with its whole latency exposed there.
  const int slot = tid & 127;
  const float* stat_src = (slot < 64 ? lse : dsum) + (int64_t)bh * n;
  const float stat_mul = slot < 64 ? LOG2E : 1.f;
  // The load and its finishing are two steps: the raw float stays in its register through a chunk's products and is scaled / masked only where it
  // is written to LDS, behind the last MFMA.  Any arithmetic on it at the load would put the compiler's wait for it -- a vmcnt(0) that also drains
  // the chunk just put in flight -- at the head of the loop.  One unconditional load from a clamped row: no branch, no merge in front of the products.
  auto load_stat = [&](int ch) { return stat_src[min(ch * KC + (tid & 63), n - 1)]; };
  auto finish_stat = [&](float raw, int ch) { return ch * KC + (tid & 63) < n ? raw * stat_mul : 0.f; };
  stats[slot] = finish_stat(load_stat(0), 0);
  const int key = blockIdx.x * BWD_ROWS + wave * 16 + ki, kc = min(key, n - 1);
  bf16x8 kf[2], vf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    kf[ks] = *(const bf16x8*)(qbase + inner + (int64_t)kc * tok_stride + (g + 4 * ks) * 8);
    vf[ks] = *(const bf16x8*)(qbase + 2 * inner + (int64_t)kc * tok_stride + (g + 4 * ks) * 8);
  }
  land(kf[0]); land(kf[1]); land(vf[0]); land(vf[1]);
  const float sl2 = scale * LOG2E;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { dk[c] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  ring_wait();
#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    const bool more = ch + 1 < nch;
    if (more) stage_chunk(rq, (uint32_t)tok_stride * 2, rdo, (uint32_t)inner * 2, ch + 1, n, ring, wave, lane, BWD_WAVES);
    const float next_raw = load_stat(ch + 1);   // (every thread, every chunk: a clamped row past the last one) raw, in flight under the products below
    asm volatile("" ::: "memory");               // (the load is issued above this line, not sunk to its use; nothing waits for it here)
    const char* q_rm = ring + (ch & 1) * STAGE_B;
    const char* do_rm = q_rm + IMG_B;
    const float* lse_s = stats + (ch & 1) * 2 * KC;
    const float* d_s = lse_s + KC;
    const int live = n - ch * KC;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x4 pp[2], ds[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * u + tt;
        f32x4 sa = mfma16(frag_rm(q_rm, t * 16 + ki, g), kf[0], f32x4{0.f, 0.f, 0.f, 0.f});     // S[query 16 t + 4 g + r][key ki]
        f32x4 dp = mfma16(frag_rm(do_rm, t * 16 + ki, g), vf[0], f32x4{0.f, 0.f, 0.f, 0.f});    // dP, same layout
        sa = mfma16(frag_rm(q_rm, t * 16 + ki, g + 4), kf[1], sa);
        dp = mfma16(frag_rm(do_rm, t * 16 + ki, g + 4), vf[1], dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = fast_exp2(fmaf(sa[r], sl2, -lse_s[t * 16 + 4 * g + r]));
          p = (t * 16 + 4 * g + r) < live ? p : 0.f;   // query rows >= n (the last chunk): no share in dv or dk
          pp[tt][r] = p;
          ds[tt][r] = p * ((dp[r] - d_s[t * 16 + 4 * g + r]) * scale);
        }
      }
      const bf16x8 pf = pack8(pp[0], pp[1]), dsf = pack8(ds[0], ds[1]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dv[c] = mfma16(frag_trr(do_rm, c, u, lane), pf, dv[c]);    // dV^T += dO^T P
        dk[c] = mfma16(frag_trr(q_rm, c, u, lane), dsf, dk[c]);    // dK^T += Q^T dS
      }
    }
    stats[((ch + 1) & 1) * 2 * KC + slot] = finish_stat(next_raw, ch + 1);   // (behind the last chunk: a stage nobody reads again)   // (that stage was read last in chunk ch - 1, a barrier ago)
    ring_wait();
  }
  if (key < n) {
    bf16_t* dkp = dqkv + ((int64_t)bi * n + key) * tok_stride + inner + hi * DH;
    bf16_t* dvp = dkp + inner;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x4 a, b2;
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = (bf16_t)dk[c][r]; b2[r] = (bf16_t)dv[c][r]; }
      *(bf16x4*)(dkp + 16 * c + 4 * g) = a;
      *(bf16x4*)(dvp + 16 * c + 4 * g) = b2;
    }
  }
}

}  // namespace

bool attn_stream_supported(int n, int dim_head) { return dim_head == attn_lds::DH && n > 288 && n <= ATTN_STREAM_MAX_N; }

// What a launch can address: (image, head) pairs on the grid's y axis, and 31-bit byte offsets (the buffer loads' per-lane offset) inside one
// image's packed qkv rows.  The lse and
// dsum buffers hold b * h * n floats each, whatever n is.
bool attn_stream_fits(int b, int n, int h) { return (int64_t)b * h <= 65535 && (int64_t)n * 3 * h * attn_lds::DH * 2 < (1LL << 31); }

void launch_attn_stream_fwd(const bf16_t* qkv, bf16_t* o, float* lse, int b, int n, int h, float scale, hipStream_t s) {
  const dim3 grid((unsigned)((n + FWD_QROWS - 1) / FWD_QROWS), (unsigned)(b * h));
  hipLaunchKernelGGL(attn_stream_fwd_kernel, grid, dim3(FWD_WAVES * 64), 0, s, qkv, o, lse, n, h, scale);
}

void launch_attn_stream_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse, float* dsum_ws, bf16_t* dqkv, int b, int n, int h,
                            float scale, hipStream_t s) {
  const dim3 grid((unsigned)((n + BWD_ROWS - 1) / BWD_ROWS), (unsigned)(b * h));
  hipLaunchKernelGGL(attn_stream_dq_kernel, grid, dim3(BWD_WAVES * 64), 0, s, qkv, o, d_o, lse, dsum_ws, dqkv, n, h, scale);
  hipLaunchKernelGGL(attn_stream_dkv_kernel, grid, dim3(BWD_WAVES * 64), 0, s, qkv, d_o, lse, (const float*)dsum_ws, dqkv, n, h, scale);
}
