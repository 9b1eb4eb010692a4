// Shifted patch tokenization (vit_for_small_dataset.py:15-47,142-157): the image is concatenated along channels with four copies of itself
// shifted by one pixel (+1 / -1 along the width, +1 / -1 along the height, the vacated column or row zero), unfolded into patch rows and
// layer-normalised in front of the patch Dense.  The shifted copies are never materialised: feature f of a row is
//   f = ((r * p + s) * 5 + k) * C + c   ->   img[y + dy_k][x + dx_k][c],  (y, x) = (hi p + r, wi p + s),  zero outside the image
// with (dy, dx) = (0,0), (0,-1), (0,+1), (-1,0), (+1,0) for k = 0..4 (the concat order of vit_for_small_dataset.py:154).  The shifts act on the
// whole image, so a patch's edge pixels read their neighbours from the adjacent patch.
#include "kernels.h"

namespace {

constexpr int SPT_CHUNKS = 256;   // row chunks of the dgamma / dbeta partials

struct SptGeom { int H, W, C, p, Hp, Wp, F; };

__device__ __forceinline__ float spt_value(const float* __restrict__ img_b, const SptGeom& g, int hi, int wi, int f) {
  const int c5 = 5 * g.C;
  const int pix = f / c5, cc = f - pix * c5;
  const int k = cc / g.C, ch = cc - k * g.C;
  const int r = pix / g.p, s = pix - r * g.p;
  int y = hi * g.p + r, x = wi * g.p + s;
  if (k == 1) x -= 1;
  else if (k == 2) x += 1;
  else if (k == 3) y -= 1;
  else if (k == 4) y += 1;
  if (x < 0 || x >= g.W || y < 0 || y >= g.H) return 0.f;
  return img_b[((int64_t)y * g.W + x) * g.C + ch];
}

// one wave per row (the reduction idiom of layernorm_fwd_kernel: two-pass statistics in fp32, biased variance)
template <typename TO>
__global__ __launch_bounds__(256) void spt_fwd_kernel(const float* __restrict__ img, TO* __restrict__ out, int64_t ldo, float* __restrict__ mean,
                                                      float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int rows, SptGeom g, float eps) {
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;   // (wave-uniform)
  const int wi = row % g.Wp, t = row / g.Wp, hi = t % g.Hp, bi = t / g.Hp;
  const float* img_b = img + (int64_t)bi * g.H * g.W * g.C;
  float s = 0.f;
  for (int f = lane; f < g.F; f += 64) s += spt_value(img_b, g, hi, wi, f);
  const float mu = wave_sum(s) / (float)g.F;
  float q = 0.f;
  for (int f = lane; f < g.F; f += 64) {
    const float v = spt_value(img_b, g, hi, wi, f) - mu;
    q = fmaf(v, v, q);
  }
  const float rs = rsqrtf(wave_sum(q) / (float)g.F + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  TO* o = out + (int64_t)row * ldo;
  for (int f = lane; f < (int)ldo; f += 64)
    stf<TO>(o + f, f < g.F ? (spt_value(img_b, g, hi, wi, f) - mu) * rs * gamma[f] + beta[f] : 0.f);
}

// partial[chunk][0][f] = sum over the chunk's rows of dy * xhat, partial[chunk][1][f] = sum of dy (one thread per feature column)
__global__ __launch_bounds__(256) void spt_bwd_cols_kernel(const float* __restrict__ img, const float* __restrict__ dy, int64_t ld,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ partial, int rows, int rows_per_chunk, SptGeom g) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= g.F) return;
  const int r_begin = blockIdx.y * rows_per_chunk, r_end = min(rows, r_begin + rows_per_chunk);
  float a = 0.f, bsum = 0.f;
  for (int row = r_begin; row < r_end; ++row) {
    const int wi = row % g.Wp, t = row / g.Wp, hi = t % g.Hp, bi = t / g.Hp;
    const float xh = (spt_value(img + (int64_t)bi * g.H * g.W * g.C, g, hi, wi, f) - mean[row]) * rstd[row];
    const float d = dy[(int64_t)row * ld + f];
    a = fmaf(d, xh, a);
    bsum += d;
  }
  partial[((int64_t)blockIdx.y * 2 + 0) * g.F + f] = a;
  partial[((int64_t)blockIdx.y * 2 + 1) * g.F + f] = bsum;
}

// dx = rstd * (gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat)), in place, one wave per row
__global__ __launch_bounds__(256) void spt_bwd_rows_kernel(const float* __restrict__ img, float* __restrict__ dy, int64_t ld,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, int rows, SptGeom g) {
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;   // (wave-uniform)
  const int wi = row % g.Wp, t = row / g.Wp, hi = t % g.Hp, bi = t / g.Hp;
  const float* img_b = img + (int64_t)bi * g.H * g.W * g.C;
  const float mu = mean[row], rs = rstd[row];
  float* d = dy + (int64_t)row * ld;
  float s1 = 0.f, s2 = 0.f;
  for (int f = lane; f < g.F; f += 64) {
    const float gd = gamma[f] * d[f];
    s1 += gd;
    s2 = fmaf(gd, (spt_value(img_b, g, hi, wi, f) - mu) * rs, s2);
  }
  const float c1 = wave_sum(s1) / (float)g.F, c2 = wave_sum(s2) / (float)g.F;
  for (int f = lane; f < g.F; f += 64) {
    const float xh = (spt_value(img_b, g, hi, wi, f) - mu) * rs;
    d[f] = rs * (gamma[f] * d[f] - c1 - xh * c2);
  }
}

// every pixel sums what read it: its own position (k = 0) and the four neighbours a shifted copy mapped onto it
__global__ void spt_dimg_kernel(const float* __restrict__ dx, int64_t ld, float* __restrict__ dimg, int b, SptGeom g) {
  const int64_t total = (int64_t)b * g.H * g.W * g.C;
  const int c5 = 5 * g.C;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % g.C);
    int64_t t = e / g.C;
    const int x = (int)(t % g.W);
    t /= g.W;
    const int y = (int)(t % g.H);
    const int64_t bi = t / g.H;
    auto at = [&](int yy, int xx, int k) -> float {   // d(row feature) of the shifted copy k at output pixel (yy, xx)
      if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) return 0.f;
      const int64_t row = (bi * g.Hp + yy / g.p) * g.Wp + xx / g.p;
      return dx[row * ld + ((yy % g.p) * g.p + xx % g.p) * c5 + k * g.C + ch];
    };
    dimg[e] = (((at(y, x, 0) + at(y, x + 1, 1)) + at(y, x - 1, 2)) + at(y + 1, x, 3)) + at(y - 1, x, 4);
  }
}

inline SptGeom spt_geom(int H, int W, int C, int p) { return SptGeom{H, W, C, p, H / p, W / p, 5 * p * p * C}; }

}  // namespace

void launch_spt_fwd(const float* img, void* rows_out, int rows_bf16, int64_t ldo, float* mean, float* rstd, const float* gamma, const float* beta, int b,
                    int H, int W, int C, int p, float eps, hipStream_t s) {
  const SptGeom g = spt_geom(H, W, C, p);
  const int rows = b * g.Hp * g.Wp;
  if (rows == 0) return;
  const dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
  if (rows_bf16) hipLaunchKernelGGL(spt_fwd_kernel<bf16_t>, grid, block, 0, s, img, (bf16_t*)rows_out, ldo, mean, rstd, gamma, beta, rows, g, eps);
  else hipLaunchKernelGGL(spt_fwd_kernel<float>, grid, block, 0, s, img, (float*)rows_out, ldo, mean, rstd, gamma, beta, rows, g, eps);
}

int64_t spt_bwd_ws_elems(int feat) { return (int64_t)(SPT_CHUNKS + 32) * 2 * feat; }

void launch_spt_bwd(const float* img, float* d_rows, int64_t ld, const float* mean, const float* rstd, const float* gamma, float* ws, float* dgamma,
                    float* dbeta, int want_dx, int b, int H, int W, int C, int p, hipStream_t s) {
  const SptGeom g = spt_geom(H, W, C, p);
  const int rows = b * g.Hp * g.Wp;
  if (rows == 0) return;
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(SPT_CHUNKS, ceil_div(rows, 16)));
  const int rpc = (int)ceil_div(rows, chunks);
  // (the column kernel runs first: the row kernel overwrites d_rows)
  hipLaunchKernelGGL(spt_bwd_cols_kernel, dim3((unsigned)ceil_div(g.F, 256), (unsigned)chunks), dim3(256), 0, s, img, d_rows, ld, mean, rstd, ws, rows, rpc, g);
  launch_reduce_partials3(ws, chunks, (int64_t)2 * g.F, g.F, 2, dgamma, dbeta, nullptr, ws + (int64_t)SPT_CHUNKS * 2 * g.F, 1.0f, s);
  if (want_dx) hipLaunchKernelGGL(spt_bwd_rows_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, img, d_rows, ld, mean, rstd, gamma, rows, g);
}

void launch_spt_dimg(const float* dx, int64_t ld, float* dimg, int b, int H, int W, int C, int p, hipStream_t s) {
  const SptGeom g = spt_geom(H, W, C, p);
  const int64_t total = (int64_t)b * H * W * C;
  if (total == 0) return;
  hipLaunchKernelGGL(spt_dimg_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 256 * 8)), dim3(256), 0, s, dx, ld, dimg, b, g);
}
