// Kernels of the CCT tokenizer (cct.py:176-215) behind its convolution: ReLU + MaxPool2D(padding='SAME') fused, forward and VJP.
// The convolution itself is im2col rows (cct_im2col_kernel below: the (ky, kx, c) row order of extract_patches, which is the HWIO kernel reshaped
// to [k*k*Cin, Cout]) times that matrix on the GEMM launchers (cct.hip).
//
// 'SAME' pooling geometry is extract_patches_geometry's: out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before =
// pad_total / 2 -- a 3/2 pool on an even extent pads 0 before and 1 after.  Taps outside the image never win (TF pads with -inf); every window
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

// out[b, oy, ox, c] = max(0, max over the in-image taps of conv[b, oy*st - pt + ky, ox*st - pl + kx, c]); one thread per V channels of one output
template <int V>
__global__ __launch_bounds__(256) void cct_relu_maxpool_fwd_kernel(const float* __restrict__ conv, float* __restrict__ out, int64_t total, int H, int W,
                                                                   int CV, int oh, int ow, int k, int st, int pt, int pl) {
  using T = typename VecT<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int ox = (int)(r % ow); r /= ow;
  const int oy = (int)(r % oh);
  const int64_t bi = r / oh;
  const T* src = reinterpret_cast<const T*>(conv) + bi * H * W * CV + cv;
  T m;
  for (int i = 0; i < V; ++i) set_lane(m, i, 0.f);   // ReLU: the running maximum starts at 0
  const int y0 = oy * st - pt, x0 = ox * st - pl;
  for (int ky = 0; ky < k; ++ky) {
    const int y = y0 + ky;
    if (y < 0 || y >= H) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int x = x0 + kx;
      if (x < 0 || x >= W) continue;
      const T v = src[((int64_t)y * W + x) * CV];
      for (int i = 0; i < V; ++i) set_lane(m, i, fmaxf(lane_of(m, i), lane_of(v, i)));
    }
  }
  reinterpret_cast<T*>(out)[e] = m;
}

// Gather form of the VJP (no atomics: the same bits every run).  One thread per V channels of one conv-output pixel: it sums d(out) of the windows
// that contain the pixel and in which it is the FIRST maximum in row-major window order (an earlier tap >= it, or a later tap > it, takes the
// window), and only if its pre-activation is > 0 (ReLU; ties at 0 carry no gradient either way).
template <int V>
__global__ __launch_bounds__(256) void cct_relu_maxpool_bwd_kernel(const float* __restrict__ conv, const float* __restrict__ dout,
                                                                   float* __restrict__ dconv, int64_t total, int H, int W, int CV, int oh, int ow, int k,
                                                                   int st, int pt, int pl) {
  using T = typename VecT<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int x = (int)(r % W); r /= W;
  const int y = (int)(r % H);
  const int64_t bi = r / H;
  const T* src = reinterpret_cast<const T*>(conv) + bi * H * W * CV + cv;
  const T* dsrc = reinterpret_cast<const T*>(dout) + bi * oh * ow * CV + cv;
  const T v = reinterpret_cast<const T*>(conv)[e];
  T acc;
  bool any = false;
  for (int i = 0; i < V; ++i) { set_lane(acc, i, 0.f); any = any || lane_of(v, i) > 0.f; }
  if (any) {
    // windows oy with oy*st - pt <= y <= oy*st - pt + k - 1, i.e. ceil((y + pt - k + 1) / st) <= oy <= floor((y + pt) / st)
    const int ay = y + pt - k + 1, ax = x + pl - k + 1;
    const int oy_lo = ay <= 0 ? 0 : (ay + st - 1) / st, oy_hi = min(oh - 1, (y + pt) / st);
    const int ox_lo = ax <= 0 ? 0 : (ax + st - 1) / st, ox_hi = min(ow - 1, (x + pl) / st);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      const int y0 = oy * st - pt;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const int x0 = ox * st - pl;
        bool win[V];
        for (int i = 0; i < V; ++i) win[i] = lane_of(v, i) > 0.f;
        for (int ky = 0; ky < k; ++ky) {
          const int yy = y0 + ky;
          if (yy < 0 || yy >= H) continue;
          for (int kx = 0; kx < k; ++kx) {
            const int xx = x0 + kx;
            if (xx < 0 || xx >= W || (yy == y && xx == x)) continue;
            const T o = src[((int64_t)yy * W + xx) * CV];
            const bool before = yy < y || (yy == y && xx < x);
            for (int i = 0; i < V; ++i) win[i] = win[i] && (before ? lane_of(o, i) < lane_of(v, i) : lane_of(o, i) <= lane_of(v, i));
          }
        }
        const T g = dsrc[((int64_t)oy * ow + ox) * CV];
        for (int i = 0; i < V; ++i)
          if (win[i]) set_lane(acc, i, lane_of(acc, i) + lane_of(g, i));
      }
    }
  }
  reinterpret_cast<T*>(dconv)[e] = acc;
}

// im2col rows as the GEMM operand: rows[r, (ky, kx, c)] = x[b, oy*st - pt + ky, ox*st - pl + kx, c] (zero outside the image), r = (b, oy, ox), with
// the row stride Kp = K rounded up to 64 and the columns [K, Kp) written as zeros on EVERY call -- the weight-gradient product runs over all Kp
// columns (an M extent the matrix-pipe kernels accept even at K = 27).  One thread per element; consecutive threads walk a row.
__global__ __launch_bounds__(256) void cct_im2col_kernel(const float* __restrict__ x, float* __restrict__ rows, int64_t total, int H, int W, int C, int oh,
                                                         int ow, int k, int st, int pt, int pl, int K, int Kp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int col = (int)(e % Kp);
  int64_t r = e / Kp;
  float v = 0.f;
  if (col < K) {
    const int c = col % C, kx = (col / C) % k, ky = col / (C * k);
    const int ox = (int)(r % ow);
    const int64_t r2 = r / ow;
    const int oy = (int)(r2 % oh);
    const int64_t bi = r2 / oh;
    const int y = oy * st - pt + ky, xx = ox * st - pl + kx;
    if (y >= 0 && y < H && xx >= 0 && xx < W) v = x[((bi * H + y) * W + xx) * C + c];
  }
  rows[e] = v;
}

bool vec4_ok(int C, const void* a, const void* b, const void* c) {
  return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

void launch_cct_im2col(const float* x, float* rows, int b, int H, int W, int C, int k, int st, int Kp, hipStream_t s) {
  int oh, ow, pt, pl;
  extract_patches_geometry(H, W, k, st, &oh, &ow, &pt, &pl);
  const int64_t total = (int64_t)b * oh * ow * Kp;
  if (total) hipLaunchKernelGGL(cct_im2col_kernel, dim3(grid256(total)), dim3(256), 0, s, x, rows, total, H, W, C, oh, ow, k, st, pt, pl, k * k * C, Kp);
}

void launch_cct_relu_maxpool_fwd(const float* conv, float* out, int b, int H, int W, int C, int k, int st, hipStream_t s) {
  int oh, ow, pt, pl;
  extract_patches_geometry(H, W, k, st, &oh, &ow, &pt, &pl);
  if (vec4_ok(C, conv, out, nullptr)) {
    const int64_t total = (int64_t)b * oh * ow * (C / 4);
    if (total) hipLaunchKernelGGL(cct_relu_maxpool_fwd_kernel<4>, dim3(grid256(total)), dim3(256), 0, s, conv, out, total, H, W, C / 4, oh, ow, k, st, pt, pl);
  } else {
    const int64_t total = (int64_t)b * oh * ow * C;
    if (total) hipLaunchKernelGGL(cct_relu_maxpool_fwd_kernel<1>, dim3(grid256(total)), dim3(256), 0, s, conv, out, total, H, W, C, oh, ow, k, st, pt, pl);
  }
}

void launch_cct_relu_maxpool_bwd(const float* conv, const float* dout, float* dconv, int b, int H, int W, int C, int k, int st, hipStream_t s) {
  int oh, ow, pt, pl;
  extract_patches_geometry(H, W, k, st, &oh, &ow, &pt, &pl);
  if (vec4_ok(C, conv, dout, dconv)) {
    const int64_t total = (int64_t)b * H * W * (C / 4);
    if (total) hipLaunchKernelGGL(cct_relu_maxpool_bwd_kernel<4>, dim3(grid256(total)), dim3(256), 0, s, conv, dout, dconv, total, H, W, C / 4, oh, ow, k, st, pt, pl);
  } else {
    const int64_t total = (int64_t)b * H * W * C;
    if (total) hipLaunchKernelGGL(cct_relu_maxpool_bwd_kernel<1>, dim3(grid256(total)), dim3(256), 0, s, conv, dout, dconv, total, H, W, C, oh, ow, k, st, pt, pl);
  }
}
