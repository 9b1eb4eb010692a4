// Kernels of TwinsSVT (twins_svt.py) outside its GEMMs and attention products:
//   * PatchEmbedding's Rearrange 'b (h p1) (w p2) c -> b h w (c p1 p2)' (:103) as a gather of its own -- launch_unfold's feature order is
//     (p1 p2 c) -- and its VJP, the inverse permutation;
//   * the k-strided window unfold in front of GlobalAttention's to_kv (:168,180: a 'valid' Conv2D of kernel and stride k is a Dense on the
//     (p1 p2 c) rows of non-overlapping k x k windows) on the engine's storage type, and its VJP, which ADDS into the gradient of the
//     LayerNorm output the to_q path has already written (every pixel lies in exactly one window: no atomics);
//   * PEG (:108-115): x + depthwise Conv2D 'SAME' stride 1 with bias in one pass, NHWC fp32, with its three VJPs.  d(kernel) is a two-pass sum:
//     partials over fixed slices of the b * H * W pixels, then the slices in order (the same bits every run).
// Only odd PEG kernels are built: pad (k - 1) / 2 on every side, any k (taps outside the map contribute nothing, so a kernel larger than the
// map is just mostly padding).
#include <algorithm>

#include "composite.h"

namespace {

// e walks out[b, h, w, (c p1 p2)] (row stride ld); FWD: out = x[b, h p + p1, w p + p2, c]; else x[...] = out (the VJP: dx from dpatches)
template <bool FWD>
__global__ __launch_bounds__(256) void twins_patch_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int H, int W, int C, int p,
                                                          int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int f = (int)(e % (C * p * p));
  int64_t r = e / (C * p * p);                 // (b, h, w) row
  const int p2 = f % p, p1 = (f / p) % p, c = f / (p * p);
  const int wo = W / p, ho = H / p;
  const int w = (int)(r % wo), h = (int)((r / wo) % ho);
  const int64_t bi = r / ((int64_t)wo * ho);
  const int64_t xi = ((bi * H + (int64_t)h * p + p1) * W + (int64_t)w * p + p2) * C + c;
  const int64_t oi = r * ld + f;
  if (FWD) dst[oi] = src[xi]; else dst[xi] = src[oi];
}

// e walks x[b, y, x, c] in fours of c; its window row is (b, y / k, x / k), its feature ((y % k) k + x % k) C + c
template <typename T, bool FWD>
__global__ __launch_bounds__(256) void twins_kunfold_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t total, int H, int W, int C4, int k,
                                                            int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c4 = (int)(e % C4);
  int64_t r = e / C4;
  const int x = (int)(r % W), y = (int)((r / W) % H);
  const int64_t bi = r / ((int64_t)W * H);
  const int64_t row = (bi * (H / k) + y / k) * (W / k) + x / k;
  const int64_t wi = row * ld + ((int64_t)((y % k) * k + x % k) * C4 + c4) * 4;
  if (FWD) {
    st4<T>(dst + wi, ld4<T>(src + e * 4));
  } else {      // dx += dwindows
    const float4 a = ld4<T>(dst + e * 4), g = ld4<T>(src + wi);
    st4<T>(dst + e * 4, make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w));
  }
}
template <typename T, bool FWD>
__global__ __launch_bounds__(256) void twins_kunfold_scalar_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t total, int H, int W, int C, int k,
                                                                   int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  int64_t r = e / C;
  const int x = (int)(r % W), y = (int)((r / W) % H);
  const int64_t bi = r / ((int64_t)W * H);
  const int64_t row = (bi * (H / k) + y / k) * (W / k) + x / k;
  const int64_t wi = row * ld + (int64_t)((y % k) * k + x % k) * C + c;
  if (FWD) stf<T>(dst + wi, ldf<T>(src + e)); else stf<T>(dst + e, ldf<T>(dst + e) + ldf<T>(src + wi));
}

// FWD: out = x + bias + sum_taps kern[ty, tx, c] x[b, y + ty - pad, x + tx - pad, c]
// else (the VJP in x): out = dy + sum_taps kern[ty, tx, c] dy[b, y - ty + pad, x - tx + pad, c]   (correlation with the flipped kernel)
template <bool FWD>
__global__ __launch_bounds__(256) void twins_peg_kernel(const float* __restrict__ in, const float* __restrict__ kern, const float* __restrict__ bias,
                                                        float* __restrict__ out, int64_t total, int H, int W, int C, int kp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  int64_t r = e / C;
  const int x = (int)(r % W), y = (int)((r / W) % H);
  const int64_t bi = r / ((int64_t)W * H);
  const int pad = (kp - 1) / 2;
  const float* img = in + bi * H * W * C + c;
  float acc = in[e] + (FWD ? bias[c] : 0.f);
  // taps whose source pixel lies inside the map
  for (int ty = 0; ty < kp; ++ty) {
    const int yy = FWD ? y + ty - pad : y - ty + pad;
    if (yy < 0 || yy >= H) continue;
    for (int tx = 0; tx < kp; ++tx) {
      const int xx = FWD ? x + tx - pad : x - tx + pad;
      if (xx < 0 || xx >= W) continue;
      acc = fmaf(kern[(ty * kp + tx) * C + c], img[((int64_t)yy * W + xx) * C], acc);
    }
  }
  out[e] = acc;
}

// part[slice, tap, c] = sum over the slice's pixels (b, y, x) of dy[b, y, x, c] x[b, y + ty - pad, x + tx - pad, c]; grid (slices, ceil(taps C / 256))
__global__ __launch_bounds__(256) void twins_peg_dkern_part_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                                   int64_t pixels, int64_t per_slice, int H, int W, int C, int kp) {
  const int tc = blockIdx.y * blockDim.x + threadIdx.x;
  if (tc >= kp * kp * C) return;
  const int c = tc % C, tap = tc / C, ty = tap / kp, tx = tap % kp, pad = (kp - 1) / 2;
  const int64_t p0 = (int64_t)blockIdx.x * per_slice, p1 = min(pixels, p0 + per_slice);
  float acc = 0.f;
  for (int64_t p = p0; p < p1; ++p) {
    const int xq = (int)(p % W), y = (int)((p / W) % H);
    const int yy = y + ty - pad, xx = xq + tx - pad;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    acc = fmaf(dy[p * C + c], x[(p + (int64_t)(ty - pad) * W + (tx - pad)) * C + c], acc);
  }
  part[(int64_t)blockIdx.x * kp * kp * C + tc] = acc;
}
__global__ __launch_bounds__(256) void twins_peg_dkern_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int slices, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int s = 0; s < slices; ++s) acc += part[(int64_t)s * n + i];
  out[i] = acc;
}

constexpr int PEG_SLICES_MAX = 256;

}  // namespace

void launch_twins_patch_gather(const float* x, float* out, int b, int H, int W, int C, int p, int64_t ld, hipStream_t s) {
  const int64_t total = (int64_t)b * H * W * C;
  if (total) hipLaunchKernelGGL(twins_patch_kernel<true>, dim3(grid256(total)), dim3(256), 0, s, x, out, total, H, W, C, p, ld);
}
void launch_twins_patch_scatter(const float* dpatches, int64_t ld, float* dx, int b, int H, int W, int C, int p, hipStream_t s) {
  const int64_t total = (int64_t)b * H * W * C;
  if (total) hipLaunchKernelGGL(twins_patch_kernel<false>, dim3(grid256(total)), dim3(256), 0, s, dpatches, dx, total, H, W, C, p, ld);
}

template <typename T>
static void kunfold(const T* src, T* dst, bool fwd, int b, int H, int W, int C, int k, int64_t ld, hipStream_t s) {
  const int64_t elems = (int64_t)b * H * W * C;
  if (!elems) return;
  const int align = 4 * (int)sizeof(T);
  if (C % 4 == 0 && ld % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & (uintptr_t)(align - 1)) == 0) {
    if (fwd) hipLaunchKernelGGL((twins_kunfold_kernel<T, true>), dim3(grid256(elems / 4)), dim3(256), 0, s, src, dst, elems / 4, H, W, C / 4, k, ld);
    else hipLaunchKernelGGL((twins_kunfold_kernel<T, false>), dim3(grid256(elems / 4)), dim3(256), 0, s, src, dst, elems / 4, H, W, C / 4, k, ld);
  } else {
    if (fwd) hipLaunchKernelGGL((twins_kunfold_scalar_kernel<T, true>), dim3(grid256(elems)), dim3(256), 0, s, src, dst, elems, H, W, C, k, ld);
    else hipLaunchKernelGGL((twins_kunfold_scalar_kernel<T, false>), dim3(grid256(elems)), dim3(256), 0, s, src, dst, elems, H, W, C, k, ld);
  }
}
void launch_twins_kunfold(const void* x, void* out, int is_bf16, int b, int H, int W, int C, int k, int64_t ldo, hipStream_t s) {
  if (is_bf16) kunfold<bf16_t>((const bf16_t*)x, (bf16_t*)out, true, b, H, W, C, k, ldo, s);
  else kunfold<float>((const float*)x, (float*)out, true, b, H, W, C, k, ldo, s);
}
void launch_twins_kfold_add(const void* dwin, int64_t ld, void* dx, int is_bf16, int b, int H, int W, int C, int k, hipStream_t s) {
  if (is_bf16) kunfold<bf16_t>((const bf16_t*)dwin, (bf16_t*)dx, false, b, H, W, C, k, ld, s);
  else kunfold<float>((const float*)dwin, (float*)dx, false, b, H, W, C, k, ld, s);
}

void launch_twins_peg_fwd(const float* x, const float* kern, const float* bias, float* out, int b, int H, int W, int C, int kp, hipStream_t s) {
  const int64_t total = (int64_t)b * H * W * C;
  if (total) hipLaunchKernelGGL(twins_peg_kernel<true>, dim3(grid256(total)), dim3(256), 0, s, x, kern, bias, out, total, H, W, C, kp);
}
void launch_twins_peg_bwd_dx(const float* dy, const float* kern, float* dx, int b, int H, int W, int C, int kp, hipStream_t s) {
  const int64_t total = (int64_t)b * H * W * C;
  if (total) hipLaunchKernelGGL(twins_peg_kernel<false>, dim3(grid256(total)), dim3(256), 0, s, dy, kern, (const float*)nullptr, dx, total, H, W, C, kp);
}
int64_t twins_peg_ws_elems(int C, int kp) { return (int64_t)PEG_SLICES_MAX * kp * kp * C; }
void launch_twins_peg_bwd_dkern(const float* x, const float* dy, float* ws, float* dkern, int b, int H, int W, int C, int kp, hipStream_t s) {
  const int64_t pixels = (int64_t)b * H * W;
  const int n = kp * kp * C;
  if (!pixels || !n) return;
  const int slices = (int)std::min<int64_t>(PEG_SLICES_MAX, ceil_div(pixels, 32));
  const int64_t per_slice = ceil_div(pixels, slices);
  hipLaunchKernelGGL(twins_peg_dkern_part_kernel, dim3((unsigned)slices, (unsigned)ceil_div(n, 256)), dim3(256), 0, s, x, dy, ws, pixels, per_slice, H, W, C, kp);
  hipLaunchKernelGGL(twins_peg_dkern_sum_kernel, dim3(grid256(n)), dim3(256), 0, s, (const float*)ws, dkern, slices, n);
}
