// Kernels of NesT (nest.py) outside its transformer blocks: the block partition 'b (b1 h) (b2 w) c -> (b b1 b2) h w c' (:209) fused with the
// positional add of Transformer.call (:140-142), its inverse (:211), the positional gradient, and Aggregate's MaxPool2D(3, 2, 'SAME') (:118) on
// the signed LayerNorm output, forward and VJP.  The VJP of the partition is the inverse map and the other way round (both are permutations), so
// the two copy kernels serve the backward as well.
//
// 'SAME' pooling geometry is extract_patches_geometry's, as in cct_tok.hip; taps outside the map never win (TF pads with -inf) and every window
// holds at least one tap inside it.
#include <algorithm>

#include "composite.h"

namespace {

template <int V> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<4> { using type = float4; };

__device__ __forceinline__ float lane_of(const float& v, int) { return v; }
__device__ __forceinline__ float lane_of(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ void set_lane(float& v, int, float a) { v = a; }
__device__ __forceinline__ void set_lane(float4& v, int i, float a) {
  if (i == 0) v.x = a; else if (i == 1) v.y = a; else if (i == 2) v.z = a; else v.w = a;
}

bool vec4_ok(int C, const void* a, const void* b, const void* c) {
  return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// One thread per V channels of one token.  e walks the TOKEN layout [(b b1 b2), (h w), c]; the map element is x[b, b1 * hb + h, b2 * wb + w, c];
// the grid has nb x nbx blocks.
// TO_BLOCKS: tokens[e] = x[...] (+ pos[h * wb + w]); else x[...] = tokens[e].
template <int V, bool TO_BLOCKS>
__global__ __launch_bounds__(256) void nest_blocks_kernel(const float* __restrict__ src, const float* __restrict__ pos, float* __restrict__ dst, int64_t total,
                                                          int nb, int nbx, int hb, int wb, int CV) {
  using T = typename VecT<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int w = (int)(r % wb); r /= wb;
  const int h = (int)(r % hb); r /= hb;
  const int b2 = (int)(r % nbx); r /= nbx;
  const int b1 = (int)(r % nb);
  const int64_t bi = r / nb;
  const int64_t m = (((bi * nb + b1) * hb + h) * ((int64_t)nbx * wb) + (int64_t)b2 * wb + w) * CV + cv;
  if (TO_BLOCKS) {
    T v = reinterpret_cast<const T*>(src)[m];
    if (pos != nullptr) {
      const float p = pos[h * wb + w];
      for (int i = 0; i < V; ++i) set_lane(v, i, lane_of(v, i) + p);
    }
    reinterpret_cast<T*>(dst)[e] = v;
  } else {
    reinterpret_cast<T*>(dst)[m] = reinterpret_cast<const T*>(src)[e];
  }
}

// part[seq, j] = sum_c dtokens[seq, j, c]: one wave per token row, a fixed lane-strided order followed by the wave reduction
__global__ __launch_bounds__(256) void nest_dpos_part_kernel(const float* __restrict__ dtokens, float* __restrict__ part, int64_t rows, int c) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = dtokens + row * c;
  float a = 0.f;
  for (int i = lane; i < c; i += 64) a += p[i];
  a = wave_sum(a);
  if (lane == 0) part[row] = a;
}

// out[b, oy, ox, c] = max over the in-map taps of x[b, oy*st - pt + ky, ox*st - pl + kx, c]; one thread per V channels of one output
template <int V>
__global__ __launch_bounds__(256) void nest_maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t total, int H, int W, int CV,
                                                               int oh, int ow, int k, int st, int pt, int pl) {
  using T = typename VecT<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int ox = (int)(r % ow); r /= ow;
  const int oy = (int)(r % oh);
  const int64_t bi = r / oh;
  const T* src = reinterpret_cast<const T*>(x) + bi * H * W * CV + cv;
  T m;
  for (int i = 0; i < V; ++i) set_lane(m, i, -INFINITY);   // signed input: the running maximum starts at -inf
  const int y0 = oy * st - pt, x0 = ox * st - pl;
  for (int ky = 0; ky < k; ++ky) {
    const int y = y0 + ky;
    if (y < 0 || y >= H) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int xx = x0 + kx;
      if (xx < 0 || xx >= W) continue;
      const T v = src[((int64_t)y * W + xx) * CV];
      for (int i = 0; i < V; ++i) set_lane(m, i, fmaxf(lane_of(m, i), lane_of(v, i)));
    }
  }
  reinterpret_cast<T*>(out)[e] = m;
}

// Gather form of the VJP (no atomics: the same bits every run).  One thread per V channels of one input pixel: it sums d(out) of the windows that
// contain the pixel and in which it is the FIRST maximum in row-major window order (an earlier tap >= it, or a later tap > it, takes the window).
template <int V>
__global__ __launch_bounds__(256) void nest_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout, float* __restrict__ dx,
                                                               int64_t total, int H, int W, int CV, int oh, int ow, int k, int st, int pt, int pl) {
  using T = typename VecT<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int xq = (int)(r % W); r /= W;
  const int y = (int)(r % H);
  const int64_t bi = r / H;
  const T* src = reinterpret_cast<const T*>(x) + bi * H * W * CV + cv;
  const T* dsrc = reinterpret_cast<const T*>(dout) + bi * oh * ow * CV + cv;
  const T v = reinterpret_cast<const T*>(x)[e];
  T acc;
  for (int i = 0; i < V; ++i) set_lane(acc, i, 0.f);
  // windows oy with oy*st - pt <= y <= oy*st - pt + k - 1, i.e. ceil((y + pt - k + 1) / st) <= oy <= floor((y + pt) / st)
  const int ay = y + pt - k + 1, ax = xq + pl - k + 1;
  const int oy_lo = ay <= 0 ? 0 : (ay + st - 1) / st, oy_hi = min(oh - 1, (y + pt) / st);
  const int ox_lo = ax <= 0 ? 0 : (ax + st - 1) / st, ox_hi = min(ow - 1, (xq + pl) / st);
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const int y0 = oy * st - pt;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const int x0 = ox * st - pl;
      bool win[V];
      for (int i = 0; i < V; ++i) win[i] = true;
      for (int ky = 0; ky < k; ++ky) {
        const int yy = y0 + ky;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < k; ++kx) {
          const int xx = x0 + kx;
          if (xx < 0 || xx >= W || (yy == y && xx == xq)) continue;
          const T o = src[((int64_t)yy * W + xx) * CV];
          const bool before = yy < y || (yy == y && xx < xq);
          for (int i = 0; i < V; ++i) win[i] = win[i] && (before ? lane_of(o, i) < lane_of(v, i) : lane_of(o, i) <= lane_of(v, i));
        }
      }
      const T g = dsrc[((int64_t)oy * ow + ox) * CV];
      for (int i = 0; i < V; ++i)
        if (win[i]) set_lane(acc, i, lane_of(acc, i) + lane_of(g, i));
    }
  }
  reinterpret_cast<T*>(dx)[e] = acc;
}

}  // namespace

void launch_nest_to_blocks(const float* x, const float* pos, float* tokens, int b, int nb, int hb, int wb, int c, hipStream_t s, int nbx) {
  if (nbx <= 0) nbx = nb;
  if (vec4_ok(c, x, tokens, nullptr)) {
    const int64_t total = (int64_t)b * nb * nbx * hb * wb * (c / 4);
    if (total) hipLaunchKernelGGL((nest_blocks_kernel<4, true>), dim3(grid256(total)), dim3(256), 0, s, x, pos, tokens, total, nb, nbx, hb, wb, c / 4);
  } else {
    const int64_t total = (int64_t)b * nb * nbx * hb * wb * c;
    if (total) hipLaunchKernelGGL((nest_blocks_kernel<1, true>), dim3(grid256(total)), dim3(256), 0, s, x, pos, tokens, total, nb, nbx, hb, wb, c);
  }
}

void launch_nest_from_blocks(const float* tokens, float* x, int b, int nb, int hb, int wb, int c, hipStream_t s, int nbx) {
  if (nbx <= 0) nbx = nb;
  if (vec4_ok(c, x, tokens, nullptr)) {
    const int64_t total = (int64_t)b * nb * nbx * hb * wb * (c / 4);
    if (total) hipLaunchKernelGGL((nest_blocks_kernel<4, false>), dim3(grid256(total)), dim3(256), 0, s, tokens, (const float*)nullptr, x, total, nb, nbx, hb, wb, c / 4);
  } else {
    const int64_t total = (int64_t)b * nb * nbx * hb * wb * c;
    if (total) hipLaunchKernelGGL((nest_blocks_kernel<1, false>), dim3(grid256(total)), dim3(256), 0, s, tokens, (const float*)nullptr, x, total, nb, nbx, hb, wb, c);
  }
}

void launch_nest_dpos(const float* dtokens, float* part, float* dpos, int nseq, int n, int c, hipStream_t s) {
  const int64_t rows = (int64_t)nseq * n;
  if (!rows) return;
  hipLaunchKernelGGL(nest_dpos_part_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, dtokens, part, rows, c);
  launch_sum_rows(part, nseq, n, dpos, s);
}

void launch_nest_maxpool_fwd(const float* x, float* out, int b, int H, int W, int C, int k, int st, hipStream_t s) {
  int oh, ow, pt, pl;
  extract_patches_geometry(H, W, k, st, &oh, &ow, &pt, &pl);
  if (vec4_ok(C, x, out, nullptr)) {
    const int64_t total = (int64_t)b * oh * ow * (C / 4);
    if (total) hipLaunchKernelGGL(nest_maxpool_fwd_kernel<4>, dim3(grid256(total)), dim3(256), 0, s, x, out, total, H, W, C / 4, oh, ow, k, st, pt, pl);
  } else {
    const int64_t total = (int64_t)b * oh * ow * C;
    if (total) hipLaunchKernelGGL(nest_maxpool_fwd_kernel<1>, dim3(grid256(total)), dim3(256), 0, s, x, out, total, H, W, C, oh, ow, k, st, pt, pl);
  }
}

void launch_nest_maxpool_bwd(const float* x, const float* dout, float* dx, int b, int H, int W, int C, int k, int st, hipStream_t s) {
  int oh, ow, pt, pl;
  extract_patches_geometry(H, W, k, st, &oh, &ow, &pt, &pl);
  if (vec4_ok(C, x, dout, dx)) {
    const int64_t total = (int64_t)b * H * W * (C / 4);
    if (total) hipLaunchKernelGGL(nest_maxpool_bwd_kernel<4>, dim3(grid256(total)), dim3(256), 0, s, x, dout, dx, total, H, W, C / 4, oh, ow, k, st, pt, pl);
  } else {
    const int64_t total = (int64_t)b * H * W * C;
    if (total) hipLaunchKernelGGL(nest_maxpool_bwd_kernel<1>, dim3(grid256(total)), dim3(256), 0, s, x, dout, dx, total, H, W, C, oh, ow, k, st, pt, pl);
  }
}
