// Kernels of RegionViT (regionvit.py) outside its transformer blocks: the window partition of the local map with every window's region token
// prepended (:163-168) and the split back (:175-177) -- pure copies, each the VJP of the other --, the relative position bias gathered from the
// stage's embedding table with the zero row and column of the region token (:144-155, run when the parameters change), the gather of d(bias)
// back onto the table, the sum of two gradients of a weight that is used twice, and the exact GELU of the 3-convolution local encoder.
#include "composite.h"

namespace {

template <int V> struct RvVec;
template <> struct RvVec<1> { using type = float; };
template <> struct RvVec<4> { using type = float4; };

// One thread per V channels of one token.  e walks the TOKEN layout [(b wy wx), 1 + wh ww, c]; token 0 is region[b, wy, wx], token 1 + p1 ww + p2
// is local[b, wy wh + p1, wx ww + p2].
template <int V, bool JOIN>
__global__ __launch_bounds__(256) void rv_window_kernel(const float* __restrict__ tok_in, float* __restrict__ tok_out, const float* __restrict__ reg_in,
                                                        float* __restrict__ reg_out, const float* __restrict__ loc_in, float* __restrict__ loc_out,
                                                        int64_t total, int rh, int rw, int wh, int ww, int CV) {
  using T = typename RvVec<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int n = 1 + wh * ww;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int t = (int)(r % n);
  const int64_t win = r / n;   // (b wy wx)
  if (t == 0) {
    const int64_t m = win * CV + cv;
    if (JOIN) reinterpret_cast<T*>(tok_out)[e] = reinterpret_cast<const T*>(reg_in)[m];
    else reinterpret_cast<T*>(reg_out)[m] = reinterpret_cast<const T*>(tok_in)[e];
    return;
  }
  const int p2 = (t - 1) % ww, p1 = (t - 1) / ww;
  const int wx = (int)(win % rw);
  const int64_t q = win / rw;
  const int wy = (int)(q % rh);
  const int64_t bi = q / rh;
  const int64_t m = ((bi * ((int64_t)rh * wh) + (int64_t)wy * wh + p1) * ((int64_t)rw * ww) + (int64_t)wx * ww + p2) * CV + cv;
  if (JOIN) reinterpret_cast<T*>(tok_out)[e] = reinterpret_cast<const T*>(loc_in)[m];
  else reinterpret_cast<T*>(loc_out)[m] = reinterpret_cast<const T*>(tok_in)[e];
}

template <bool JOIN>
void rv_window(const float* tok_in, float* tok_out, const float* reg_in, float* reg_out, const float* loc_in, float* loc_out, int b, int rh, int rw, int wh,
               int ww, int c, hipStream_t s) {
  const bool v4 = c % 4 == 0 && aligned16({tok_in, tok_out, reg_in, reg_out, loc_in, loc_out});
  const int CV = v4 ? c / 4 : c;
  const int64_t total = (int64_t)b * rh * rw * (1 + wh * ww) * CV;
  if (total <= 0) return;
  if (v4) hipLaunchKernelGGL((rv_window_kernel<4, JOIN>), dim3(grid256(total)), dim3(256), 0, s, tok_in, tok_out, reg_in, reg_out, loc_in, loc_out, total, rh, rw, wh, ww, CV);
  else hipLaunchKernelGGL((rv_window_kernel<1, JOIN>), dim3(grid256(total)), dim3(256), 0, s, tok_in, tok_out, reg_in, reg_out, loc_in, loc_out, total, rh, rw, wh, ww, CV);
}

// one thread per element of bias [heads, n, n], n = 1 + wh ww
__global__ __launch_bounds__(256) void rv_bias_build_kernel(const float* __restrict__ table, float* __restrict__ bias, int ws, int wh, int ww, int heads) {
  const int n = 1 + wh * ww;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= heads * n * n) return;
  const int j = e % n, i = (e / n) % n, h = e / (n * n);
  float v = 0.f;
  if (i > 0 && j > 0) {
    const int dh = (i - 1) / ww - (j - 1) / ww, dw = (i - 1) % ww - (j - 1) % ww;
    v = table[(int64_t)((dh + ws - 1) + (dw + ws - 1) * (2 * ws - 1)) * heads + h];
  }
  bias[e] = v;
}

// one thread per element of dtable [(2 ws - 1)^2, heads]: the pairs (i, j) with i - j = (dh, dw), i in (y, x) order
__global__ __launch_bounds__(256) void rv_table_grad_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int ws, int wh, int ww, int heads) {
  const int side = 2 * ws - 1, n = 1 + wh * ww;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= side * side * heads) return;
  const int h = e % heads, idx = e / heads;
  const int dh = idx % side - (ws - 1), dw = idx / side - (ws - 1);
  float a = 0.f;
  for (int y1 = 0; y1 < wh; ++y1) {
    const int y2 = y1 - dh;
    if (y2 < 0 || y2 >= wh) continue;
    for (int x1 = 0; x1 < ww; ++x1) {
      const int x2 = x1 - dw;
      if (x2 < 0 || x2 >= ww) continue;
      a += dbias[((int64_t)h * n + 1 + y1 * ww + x1) * n + 1 + y2 * ww + x2];
    }
  }
  dtable[e] = a;
}

__global__ __launch_bounds__(256) void rv_add_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dst[e] += src[e];
}

__global__ __launch_bounds__(256) void rv_gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) { const float v = x[e]; y[e] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
}
// gelu'(x) = Phi(x) + x phi(x)
__global__ __launch_bounds__(256) void rv_gelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float v = x[e];
  dx[e] = dy[e] * (0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v));
}

}  // namespace

void launch_rv_join(const float* region, const float* local, float* tokens, int b, int rh, int rw, int wh, int ww, int c, hipStream_t s) {
  rv_window<true>(nullptr, tokens, region, nullptr, local, nullptr, b, rh, rw, wh, ww, c, s);
}
void launch_rv_split(const float* tokens, float* region, float* local, int b, int rh, int rw, int wh, int ww, int c, hipStream_t s) {
  rv_window<false>(tokens, nullptr, nullptr, region, nullptr, local, b, rh, rw, wh, ww, c, s);
}
void launch_rv_bias_build(const float* table, float* bias, int ws, int wh, int ww, int heads, hipStream_t s) {
  const int n = 1 + wh * ww;
  hipLaunchKernelGGL(rv_bias_build_kernel, dim3(grid256((int64_t)heads * n * n)), dim3(256), 0, s, table, bias, ws, wh, ww, heads);
}
void launch_rv_table_grad(const float* dbias, float* dtable, int ws, int wh, int ww, int heads, hipStream_t s) {
  const int side = 2 * ws - 1;
  hipLaunchKernelGGL(rv_table_grad_kernel, dim3(grid256((int64_t)side * side * heads)), dim3(256), 0, s, dbias, dtable, ws, wh, ww, heads);
}
void launch_rv_add(float* dst, const float* src, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(rv_add_kernel, dim3(grid256(n)), dim3(256), 0, s, dst, src, n);
}
void launch_rv_gelu_fwd(const float* x, float* y, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(rv_gelu_fwd_kernel, dim3(grid256(n)), dim3(256), 0, s, x, y, n);
}
void launch_rv_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(rv_gelu_bwd_kernel, dim3(grid256(n)), dim3(256), 0, s, x, dy, dx, n);
}
