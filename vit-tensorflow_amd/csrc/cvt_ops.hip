// Kernels of CvT's convolutional projection (cvt.py:79-92) in front of its pointwise Dense: a depthwise 'SAME' convolution without bias, of any
// kernel size and stride, followed by BatchNormalization over all b * oh * ow positions of the call's batch -- and their VJPs.
//   * Geometry is extract_patches_geometry's (TensorFlow's 'SAME'): out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before =
//     pad_total / 2, the rest behind.  A 3/2 convolution on an even map pads 0 in front and 1 behind; taps outside the map contribute nothing, so
//     a kernel larger than the map is mostly padding.
//   * The input is the LayerNorm output in the engine's storage type (bf16 or fp32), NHWC.  The convolution output and every statistic are
//     fp32 in every compute mode; only the normalised result is written in the storage type, for the Dense that reads it.
//   * Statistics are two passes over the fp32 convolution output: the mean, then the mean of the squared deviations from it (no E[x^2] - E[x]^2).
//     Every per-channel sum is taken as partials over fixed slices of the positions, added in slice order: the same bits every run, and the
//     slices depend on the position count alone, never on how the caller chunks images.
//   * The sums, the statistics (mean | rstd) and the normalised value xhat are DOUBLE.  With a float mean the centred values do not add up to
//     zero, and the VJP's dy - mean(dy) - xhat mean(dy xhat) -- which cancels to eps / (var + eps) of its terms when a channel is normalised
//     over few positions (two samples of a 1 x 1 map: xhat = +-1) -- turns that residue into a gradient error of 1e-3 of the tensor, and into
//     a non-zero sum of d(conv) over the batch where the true one is exactly zero.
//   * Not tuned: at the usage shape these launches are half of the bf16 step (DESIGN.md section 22 has the figures), some ten times what their
//     traffic alone would cost.  One thread per element or per (slice, channel), 64-bit index arithmetic per position, no vector loads.
//   * The VJPs are gathers: d(gamma) / d(beta) and d(kernel) as fixed-slice partials summed in order, d(input) collects for every input position
//     the outputs whose windows cover it -- of the q projection (stride 1) and of the kv projection (stride s) in one pass, written once.  No
//     atomics anywhere.
#include <algorithm>

#include "composite.h"

namespace {

// slices of the positions a per-channel sum is cut into: at the usage's stage 1 (802816 positions, 64 channels) 2048 slices are 131072 threads
// of 392 positions each
constexpr int CVT_SLICES_MAX = 2048;

struct DwGeom { int H, W, C, k, st, oh, ow, pt, pl; };

DwGeom dw_geom(int H, int W, int C, int k, int st) {
  DwGeom g{H, W, C, k, st, 0, 0, 0, 0};
  extract_patches_geometry(H, W, k, st, &g.oh, &g.ow, &g.pt, &g.pl);
  return g;
}

// conv[b, oy, ox, c] = sum over the taps inside the map of kern[ty, tx, c] x[b, oy st + ty - pt, ox st + tx - pl, c]
template <typename T>
__global__ __launch_bounds__(256) void cvt_dw_conv_kernel(const T* __restrict__ x, const float* __restrict__ kern, float* __restrict__ conv, int64_t total,
                                                          DwGeom g) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % g.C);
  const int64_t r = e / g.C;
  const int ox = (int)(r % g.ow), oy = (int)((r / g.ow) % g.oh);
  const int64_t bi = r / ((int64_t)g.ow * g.oh);
  const T* img = x + bi * g.H * g.W * g.C + c;
  float acc = 0.f;
  for (int ty = 0; ty < g.k; ++ty) {
    const int yy = oy * g.st + ty - g.pt;
    if (yy < 0 || yy >= g.H) continue;
    for (int tx = 0; tx < g.k; ++tx) {
      const int xx = ox * g.st + tx - g.pl;
      if (xx < 0 || xx >= g.W) continue;
      acc = fmaf(kern[(ty * g.k + tx) * g.C + c], ldf<T>(img + ((int64_t)yy * g.W + xx) * g.C), acc);
    }
  }
  conv[e] = acc;
}

// part[slice, c] = sum over the slice's rows of v[row, c] (CENTRED: of (v[row, c] - stats[c])^2); one thread per (slice, c)
template <bool CENTRED>
__global__ __launch_bounds__(256) void cvt_stat_part_kernel(const float* __restrict__ v, const double* __restrict__ stats, double* __restrict__ part, int64_t rows,
                                                            int64_t per_slice, int slices, int C) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= slices * C) return;
  const int c = t % C, sl = t / C;
  const int64_t r0 = (int64_t)sl * per_slice, r1 = min(rows, r0 + per_slice);
  const double mean = CENTRED ? stats[c] : 0.0;
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const double d = (double)v[r * C + c] - mean;
    acc += CENTRED ? d * d : d;
  }
  part[t] = acc;
}
// RSTD: stats[C + c] = rsqrt(sum / rows + eps), else stats[c] = sum / rows; the slices in order
template <bool RSTD>
__global__ __launch_bounds__(256) void cvt_stat_sum_kernel(const double* __restrict__ part, double* __restrict__ stats, int slices, int C, double inv_rows, double eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double acc = 0.0;
  for (int s = 0; s < slices; ++s) acc += part[(int64_t)s * C + c];
  if (RSTD) stats[C + c] = 1.0 / sqrt(acc * inv_rows + eps); else stats[c] = acc * inv_rows;
}
// training=False: the moving statistics of the table
__global__ __launch_bounds__(256) void cvt_stat_moving_kernel(const float* __restrict__ mean, const float* __restrict__ var, double* __restrict__ stats, int C, double eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  stats[c] = (double)mean[c];
  stats[C + c] = 1.0 / sqrt((double)var[c] + eps);
}

// y[row, c] = (conv[row, c] - mean[c]) rstd[c] gamma[c] + beta[c], in the storage type (row stride ldy)
template <typename T>
__global__ __launch_bounds__(256) void cvt_bn_apply_kernel(const float* __restrict__ conv, const double* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, T* __restrict__ y, int64_t ldy, int64_t total, int C) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t r = e / C;
  stf<T>(y + r * ldy + c, (float)(((double)conv[e] - stats[c]) * stats[C + c] * (double)gamma[c] + (double)beta[c]));
}

// part[slice, 0, c] = sum dy, part[slice, 1, c] = sum dy xhat over the slice's rows
template <typename T>
__global__ __launch_bounds__(256) void cvt_bn_bwd_part_kernel(const T* __restrict__ dy, int64_t lddy, const float* __restrict__ conv, const double* __restrict__ stats,
                                                              double* __restrict__ part, int64_t rows, int64_t per_slice, int slices, int C) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= slices * C) return;
  const int c = t % C, sl = t / C;
  const int64_t r0 = (int64_t)sl * per_slice, r1 = min(rows, r0 + per_slice);
  const double mean = stats[c], rstd = stats[C + c];
  double sb = 0.0, sg = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const double g = (double)ldf<T>(dy + r * lddy + c);
    sb += g;
    sg = fma(g, ((double)conv[r * C + c] - mean) * rstd, sg);
  }
  part[((int64_t)sl * 2) * C + c] = sb;
  part[((int64_t)sl * 2 + 1) * C + c] = sg;
}
// sums[c] = d(beta), sums[C + c] = d(gamma) (double, for the d(conv) pass) and their float values into the gradient arena
__global__ __launch_bounds__(256) void cvt_bn_bwd_sum_kernel(const double* __restrict__ part, double* __restrict__ sums, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, int slices, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double sb = 0.0, sg = 0.0;
  for (int s = 0; s < slices; ++s) {
    sb += part[((int64_t)s * 2) * C + c];
    sg += part[((int64_t)s * 2 + 1) * C + c];
  }
  sums[c] = sb;
  sums[C + c] = sg;
  dbeta[c] = (float)sb;
  dgamma[c] = (float)sg;
}
// dconv = gamma rstd (dy - d(beta) / N - xhat d(gamma) / N)
template <typename T>
__global__ __launch_bounds__(256) void cvt_bn_bwd_dx_kernel(const T* __restrict__ dy, int64_t lddy, const float* __restrict__ conv, const double* __restrict__ stats,
                                                            const float* __restrict__ gamma, const double* __restrict__ sums, float* __restrict__ dconv,
                                                            int64_t total, int C, double inv_rows) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t r = e / C;
  const double rstd = stats[C + c], xhat = ((double)conv[e] - stats[c]) * rstd;
  dconv[e] = (float)((double)gamma[c] * rstd * ((double)ldf<T>(dy + r * lddy + c) - sums[c] * inv_rows - xhat * sums[C + c] * inv_rows));
}

// part[slice, tap, c] = sum over the slice's OUTPUT positions (b, oy, ox) of dconv[b, oy, ox, c] x[b, oy st + ty - pt, ox st + tx - pl, c]
template <typename T>
__global__ __launch_bounds__(256) void cvt_dw_dkern_part_kernel(const T* __restrict__ x, const float* __restrict__ dconv, float* __restrict__ part, int64_t rows,
                                                                int64_t per_slice, int slices, DwGeom g) {
  const int n = g.k * g.k * g.C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)slices * n) return;
  const int tc = (int)(t % n), sl = (int)(t / n);
  const int c = tc % g.C, tap = tc / g.C, ty = tap / g.k, tx = tap % g.k;
  const int64_t r0 = (int64_t)sl * per_slice, r1 = min(rows, r0 + per_slice);
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const int ox = (int)(r % g.ow), oy = (int)((r / g.ow) % g.oh);
    const int64_t bi = r / ((int64_t)g.ow * g.oh);
    const int yy = oy * g.st + ty - g.pt, xx = ox * g.st + tx - g.pl;
    if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) continue;
    acc = fmaf(dconv[r * g.C + c], ldf<T>(x + ((bi * g.H + yy) * g.W + xx) * g.C + c), acc);
  }
  part[t] = acc;
}
__global__ __launch_bounds__(256) void cvt_sum_slices_kernel(const float* __restrict__ part, float* __restrict__ out, int slices, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int s = 0; s < slices; ++s) acc += part[(int64_t)s * n + i];
  out[i] = acc;
}

// the outputs of one projection whose windows cover input position (y, x): oy st + ty - pt == y for a tap ty in [0, k)
__device__ __forceinline__ float dw_dx_gather(const float* __restrict__ dconv, const float* __restrict__ kern, const DwGeom& g, int64_t bi, int y, int x, int c) {
  float acc = 0.f;
  const float* img = dconv + bi * g.oh * g.ow * g.C + c;
  for (int ty = 0; ty < g.k; ++ty) {
    const int ny = y + g.pt - ty;
    if (ny < 0 || ny % g.st) continue;
    const int oy = ny / g.st;
    if (oy >= g.oh) continue;
    for (int tx = 0; tx < g.k; ++tx) {
      const int nx = x + g.pl - tx;
      if (nx < 0 || nx % g.st) continue;
      const int ox = nx / g.st;
      if (ox >= g.ow) continue;
      acc = fmaf(kern[(ty * g.k + tx) * g.C + c], img[((int64_t)oy * g.ow + ox) * g.C], acc);
    }
  }
  return acc;
}
// dx[b, y, x, c] = the q projection's share + the kv projection's, in the storage type
template <typename T>
__global__ __launch_bounds__(256) void cvt_dw_dx_kernel(const float* __restrict__ dconv_q, const float* __restrict__ kern_q, DwGeom gq,
                                                        const float* __restrict__ dconv_kv, const float* __restrict__ kern_kv, DwGeom gkv, T* __restrict__ dx,
                                                        int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % gq.C);
  const int64_t r = e / gq.C;
  const int x = (int)(r % gq.W), y = (int)((r / gq.W) % gq.H);
  const int64_t bi = r / ((int64_t)gq.W * gq.H);
  stf<T>(dx + e, dw_dx_gather(dconv_q, kern_q, gq, bi, y, x, c) + dw_dx_gather(dconv_kv, kern_kv, gkv, bi, y, x, c));
}

int slices_of(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(CVT_SLICES_MAX, ceil_div(rows, 32))); }

}  // namespace

// floats: the d(kernel) partials (slices x taps x C floats), or the BatchNorm partials and sums ((slices + 1) x 2 x C doubles)
int64_t cvt_dwbn_ws_elems(int C, int k) { return std::max<int64_t>((int64_t)CVT_SLICES_MAX * k * k * C, (int64_t)(CVT_SLICES_MAX + 1) * 4 * C); }

template <typename T>
static void dwbn_fwd(const T* x, const float* kern, const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, int training, float eps_f,
                     float* conv, double* stats, T* y, int64_t ldy, float* ws_f, int b, const DwGeom& g, hipStream_t s) {
  double* ws = (double*)ws_f;
  const double eps = (double)eps_f;
  const int64_t rows = (int64_t)b * g.oh * g.ow, total = rows * g.C;
  if (!total) return;
  hipLaunchKernelGGL((cvt_dw_conv_kernel<T>), dim3(grid256(total)), dim3(256), 0, s, x, kern, conv, total, g);
  if (training) {
    const int slices = slices_of(rows);
    const int64_t per_slice = ceil_div(rows, slices);
    const double inv = 1.0 / (double)rows;
    hipLaunchKernelGGL(cvt_stat_part_kernel<false>, dim3(grid256((int64_t)slices * g.C)), dim3(256), 0, s, (const float*)conv, (const double*)stats, ws, rows, per_slice, slices, g.C);
    hipLaunchKernelGGL(cvt_stat_sum_kernel<false>, dim3(grid256(g.C)), dim3(256), 0, s, (const double*)ws, stats, slices, g.C, inv, eps);
    hipLaunchKernelGGL(cvt_stat_part_kernel<true>, dim3(grid256((int64_t)slices * g.C)), dim3(256), 0, s, (const float*)conv, (const double*)stats, ws, rows, per_slice, slices, g.C);
    hipLaunchKernelGGL(cvt_stat_sum_kernel<true>, dim3(grid256(g.C)), dim3(256), 0, s, (const double*)ws, stats, slices, g.C, inv, eps);
  } else {
    hipLaunchKernelGGL(cvt_stat_moving_kernel, dim3(grid256(g.C)), dim3(256), 0, s, mov_mean, mov_var, stats, g.C, eps);
  }
  hipLaunchKernelGGL((cvt_bn_apply_kernel<T>), dim3(grid256(total)), dim3(256), 0, s, (const float*)conv, (const double*)stats, gamma, beta, y, ldy, total, g.C);
}

void launch_cvt_dwbn_fwd(const void* x, int is_bf16, const float* kern, const float* gamma, const float* beta, const float* mov_mean, const float* mov_var,
                         int training, float eps, float* conv, double* stats, void* y, int64_t ldy, float* ws, int b, int H, int W, int C, int k, int st,
                         hipStream_t s) {
  const DwGeom g = dw_geom(H, W, C, k, st);
  if (is_bf16) dwbn_fwd<bf16_t>((const bf16_t*)x, kern, gamma, beta, mov_mean, mov_var, training, eps, conv, stats, (bf16_t*)y, ldy, ws, b, g, s);
  else dwbn_fwd<float>((const float*)x, kern, gamma, beta, mov_mean, mov_var, training, eps, conv, stats, (float*)y, ldy, ws, b, g, s);
}

template <typename T>
static void bn_bwd(const T* dy, int64_t lddy, const float* conv, const double* stats, const float* gamma, float* dgamma, float* dbeta, float* dconv, float* ws_f,
                   int64_t rows, int C, hipStream_t s) {
  if (!rows || !C) return;
  const int slices = slices_of(rows);
  const int64_t per_slice = ceil_div(rows, slices), total = rows * C;
  double* ws = (double*)ws_f;
  double* sums = ws + (int64_t)slices * 2 * C;
  hipLaunchKernelGGL((cvt_bn_bwd_part_kernel<T>), dim3(grid256((int64_t)slices * C)), dim3(256), 0, s, dy, lddy, conv, stats, ws, rows, per_slice, slices, C);
  hipLaunchKernelGGL(cvt_bn_bwd_sum_kernel, dim3(grid256(C)), dim3(256), 0, s, (const double*)ws, sums, dgamma, dbeta, slices, C);
  hipLaunchKernelGGL((cvt_bn_bwd_dx_kernel<T>), dim3(grid256(total)), dim3(256), 0, s, dy, lddy, conv, stats, gamma, (const double*)sums, dconv, total, C,
                     1.0 / (double)rows);
}

void launch_cvt_bn_bwd(const void* dy, int is_bf16, int64_t lddy, const float* conv, const double* stats, const float* gamma, float* dgamma, float* dbeta,
                       float* dconv, float* ws, int64_t rows, int C, hipStream_t s) {
  if (is_bf16) bn_bwd<bf16_t>((const bf16_t*)dy, lddy, conv, stats, gamma, dgamma, dbeta, dconv, ws, rows, C, s);
  else bn_bwd<float>((const float*)dy, lddy, conv, stats, gamma, dgamma, dbeta, dconv, ws, rows, C, s);
}

void launch_cvt_dw_bwd_dkern(const void* x, int is_bf16, const float* dconv, float* ws, float* dkern, int b, int H, int W, int C, int k, int st, hipStream_t s) {
  const DwGeom g = dw_geom(H, W, C, k, st);
  const int64_t rows = (int64_t)b * g.oh * g.ow;
  const int n = k * k * C;
  if (!rows || !n) return;
  const int slices = slices_of(rows);
  const int64_t per_slice = ceil_div(rows, slices);
  const dim3 grid(grid256((int64_t)slices * n));
  if (is_bf16) hipLaunchKernelGGL((cvt_dw_dkern_part_kernel<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)x, dconv, ws, rows, per_slice, slices, g);
  else hipLaunchKernelGGL((cvt_dw_dkern_part_kernel<float>), grid, dim3(256), 0, s, (const float*)x, dconv, ws, rows, per_slice, slices, g);
  hipLaunchKernelGGL(cvt_sum_slices_kernel, dim3(grid256(n)), dim3(256), 0, s, (const float*)ws, dkern, slices, n);
}

void launch_cvt_dw_bwd_dx(const float* dconv_q, const float* kern_q, const float* dconv_kv, const float* kern_kv, int st_kv, void* dx, int is_bf16, int b, int H,
                          int W, int C, int k, hipStream_t s) {
  const DwGeom gq = dw_geom(H, W, C, k, 1), gkv = dw_geom(H, W, C, k, st_kv);
  const int64_t total = (int64_t)b * H * W * C;
  if (!total) return;
  if (is_bf16) hipLaunchKernelGGL((cvt_dw_dx_kernel<bf16_t>), dim3(grid256(total)), dim3(256), 0, s, dconv_q, kern_q, gq, dconv_kv, kern_kv, gkv, (bf16_t*)dx, total);
  else hipLaunchKernelGGL((cvt_dw_dx_kernel<float>), dim3(grid256(total)), dim3(256), 0, s, dconv_q, kern_q, gq, dconv_kv, kern_kv, gkv, (float*)dx, total);
}
