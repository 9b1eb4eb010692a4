// Kernels of CrossFormer (crossformer.py) outside its transformer blocks: the dilated ("long") window partition
// 'b (l1 h) (l2 w) d -> (b h w) l1 l2 d' (:146) and its inverse (:178) -- the window partition of nest_ops.hip with the roles of window index and
// in-window index exchanged; both are permutations, each the VJP of the other --, the column-block copies of the cross-scale embedding (:46-47), and
// the dynamic position bias (:51-71,126-131,159-163): the network on its (2 wsz + 1)^2 positions and the [n, n] gather.
//
// The bias index arithmetic is the reference's and asymmetric on purpose: rel_pos_indices has row stride 2 wsz - 1 (:131) while the table it
// indexes is built from positions -wsz .. wsz, (2 wsz + 1) per side (:159-161).  The largest index, (2 wsz - 2) * 2 wsz, stays inside the table.
#include "composite.h"

namespace {

template <int V> struct CfVec;
template <> struct CfVec<1> { using type = float; };
template <> struct CfVec<4> { using type = float4; };

// One thread per V channels of one token.  e walks the TOKEN layout [(b h w), (l1 l2), c]; the map element is x[b, l1 * Hg + h, l2 * Wg + w, c].
template <int V, bool TO_TOKENS>
__global__ __launch_bounds__(256) void cf_dilated_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int Hg, int Wg, int g, int CV) {
  using T = typename CfVec<V>::type;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int cv = (int)(e % CV);
  int64_t r = e / CV;
  const int l2 = (int)(r % g); r /= g;
  const int l1 = (int)(r % g); r /= g;
  const int w = (int)(r % Wg); r /= Wg;
  const int h = (int)(r % Hg);
  const int64_t bi = r / Hg;
  const int64_t m = (((bi * g + l1) * Hg + h) * ((int64_t)g * Wg) + (int64_t)l2 * Wg + w) * CV + cv;
  if (TO_TOKENS) reinterpret_cast<T*>(dst)[e] = reinterpret_cast<const T*>(src)[m];
  else reinterpret_cast<T*>(dst)[m] = reinterpret_cast<const T*>(src)[e];
}

template <bool TO_TOKENS>
void cf_dilated(const float* src, float* dst, int b, int H, int W, int g, int c, hipStream_t s) {
  const bool v4 = c % 4 == 0 && aligned16({src, dst});
  const int CV = v4 ? c / 4 : c;
  const int64_t total = (int64_t)b * H * W * CV;
  if (total <= 0) return;
  if (v4) hipLaunchKernelGGL((cf_dilated_kernel<4, TO_TOKENS>), dim3(grid256(total)), dim3(256), 0, s, src, dst, total, H / g, W / g, g, CV);
  else hipLaunchKernelGGL((cf_dilated_kernel<1, TO_TOKENS>), dim3(grid256(total)), dim3(256), 0, s, src, dst, total, H / g, W / g, g, CV);
}

// PUT: wide[r, col0 + j] = narrow[r, j]; else narrow[r, j] = wide[r, col0 + j]
template <bool PUT>
__global__ __launch_bounds__(256) void cf_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int w, int ld, int col0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / w;
  const int j = (int)(e - r * w);
  if (PUT) dst[r * ld + col0 + j] = src[e];
  else dst[e] = src[r * ld + col0 + j];
}

// LayerNormalization (Keras: eps 1e-3, biased variance) + ReLU of one row held in LDS, by one wave: in -> out
__device__ __forceinline__ void cf_ln_relu(const float* in, float* out, const float* __restrict__ gamma, const float* __restrict__ beta, int d4, int lane) {
  float a = 0.f;
  for (int f = lane; f < d4; f += 64) a += in[f];
  const float mean = wave_sum(a) / (float)d4;
  float v = 0.f;
  for (int f = lane; f < d4; f += 64) { const float t = in[f] - mean; v = fmaf(t, t, v); }
  const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)d4 + 1e-3f);
  for (int f = lane; f < d4; f += 64) out[f] = fmaxf((in[f] - mean) * rstd * gamma[f] + beta[f], 0.f);
}

// DynamicPositionBias.call (:69-71) on position `blockIdx.x` of the (2 wsz + 1)^2 grid ('c i j -> (i j) c' of meshgrid(pos, pos, 'ij'), :159-161):
// one wave per position, the row of at most d / 4 features in LDS, every sum in a fixed order.
__global__ __launch_bounds__(64) void cf_dpb_kernel(CfDpbParams P, int d4, int wsz, float* __restrict__ tab) {
  extern __shared__ float cf_sm[];
  float* h0 = cf_sm;
  float* h1 = cf_sm + d4;
  const int lane = threadIdx.x, side = 2 * wsz + 1, row = blockIdx.x;
  const float x0 = (float)(row / side - wsz), x1 = (float)(row % side - wsz);
  for (int f = lane; f < d4; f += 64) h1[f] = fmaf(x1, P.t[0][d4 + f], fmaf(x0, P.t[0][f], 0.f)) + P.t[1][f];
  __syncthreads();
  cf_ln_relu(h1, h0, P.t[2], P.t[3], d4, lane);
  __syncthreads();
  for (int layer = 1; layer < 3; ++layer) {
    const float* __restrict__ Wk = P.t[4 * layer];
    for (int f = lane; f < d4; f += 64) {
      float a = 0.f;
      for (int k = 0; k < d4; ++k) a = fmaf(h0[k], Wk[(int64_t)k * d4 + f], a);
      h1[f] = a + P.t[4 * layer + 1][f];
    }
    __syncthreads();
    cf_ln_relu(h1, h0, P.t[4 * layer + 2], P.t[4 * layer + 3], d4, lane);
    __syncthreads();
  }
  float a = 0.f;
  for (int f = lane; f < d4; f += 64) a = fmaf(h0[f], P.t[12][f], a);
  a = wave_sum(a);
  if (lane == 0) tab[row] = a + P.t[13][0];
}

// bias[i, j] = tab[rel_pos_indices[i, j]] (:126-131,163): i = (i1, i2), j = (j1, j2) on the wsz x wsz window,
// index = (i1 - j1 + wsz - 1) * (2 wsz - 1) + (i2 - j2 + wsz - 1)
__global__ __launch_bounds__(256) void cf_bias_gather_kernel(const float* __restrict__ tab, float* __restrict__ bias, int wsz) {
  const int n = wsz * wsz;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * n) return;
  const int i = e / n, j = e - i * n;
  const int r0 = i / wsz - j / wsz + wsz - 1, r1 = i % wsz - j % wsz + wsz - 1;
  bias[e] = tab[r0 * (2 * wsz - 1) + r1];
}

}  // namespace

void launch_cf_to_dilated(const float* x, float* tokens, int b, int H, int W, int g, int c, hipStream_t s) { cf_dilated<true>(x, tokens, b, H, W, g, c, s); }
void launch_cf_from_dilated(const float* tokens, float* x, int b, int H, int W, int g, int c, hipStream_t s) { cf_dilated<false>(tokens, x, b, H, W, g, c, s); }

void launch_cf_cols_put(const float* src, float* dst, int64_t rows, int w, int ld, int col0, hipStream_t s) {
  const int64_t total = rows * w;
  if (total > 0) hipLaunchKernelGGL(cf_cols_kernel<true>, dim3(grid256(total)), dim3(256), 0, s, src, dst, total, w, ld, col0);
}
void launch_cf_cols_get(const float* src, float* dst, int64_t rows, int w, int ld, int col0, hipStream_t s) {
  const int64_t total = rows * w;
  if (total > 0) hipLaunchKernelGGL(cf_cols_kernel<false>, dim3(grid256(total)), dim3(256), 0, s, src, dst, total, w, ld, col0);
}

int64_t cf_dpb_ws_elems(int wsz) { return (int64_t)(2 * wsz + 1) * (2 * wsz + 1); }

void launch_cf_dpb_bias(const CfDpbParams& p, int d4, int wsz, float* ws, float* bias, hipStream_t s) {
  const int side = 2 * wsz + 1, n = wsz * wsz;
  hipLaunchKernelGGL(cf_dpb_kernel, dim3(side * side), dim3(64), (size_t)2 * d4 * sizeof(float), s, p, d4, wsz, ws);
  hipLaunchKernelGGL(cf_bias_gather_kernel, dim3(grid256((int64_t)n * n)), dim3(256), 0, s, (const float*)ws, bias, wsz);
}
