// Kernels of PiT (pit.py): the overlapping tokenizer's unfold (tf.image.extract_patches, sizes p, strides p // 2, 'VALID', :110-122) with its
// VJP, the class / position rows (:211-213) with theirs, and Pool (:140-156) -- Dense on the class row, a depthwise 3x3 / stride 2 'SAME'
// convolution with a channel multiplier of 2 and a bias on the other rows read as the h x w map, a 1x1 convolution -- with its VJP.
//   * Token layout everywhere: [b, 1 + h w, d] fp32 rows, row 0 the class token.  The kernels read and write rows 1.. as the map IN PLACE; no
//     rearranged copy exists.  Buffers that feed a GEMM over token rows keep a row 0 of zeros per image (the unfolded patches, the depthwise
//     output), so that one Dense / one weight-gradient product runs over all b (1 + h w) rows and row 0 adds nothing to a weight gradient.
//   * Pool geometry is TensorFlow's 'SAME' for k = 3, s = 2: oh = ceil(h / 2), pad_total = max((oh - 1) 2 + 3 - h, 0), pad_top = pad_total / 2:
//     an odd extent pads 1 | 1, an even one 0 | 1.  Output channel o reads input channel o / 2 (Keras Conv2D(groups = d, filters = 2 d)).
//   * Four channels per thread with vector loads / stores when the width allows it (2 d % 4 == 0: d even, every tensor 16-B aligned), a scalar
//     form otherwise; 32-bit index arithmetic throughout -- the launchers refuse sizes past 2^31 elements (pit_ops_fits).
//   * Every sum over positions (d(kernel), the two biases, d(pos_embedding)) is taken as partials over fixed slices of the rows, added in slice
//     order; d(input) and d(img) are gathers that write every element once.  No atomics: a second backward gives the same bits.
//   * fp32 storage in every compute mode.
#include <algorithm>

#include "composite.h"

namespace {

constexpr int PIT_SLICES_MAX = 1024;

struct PoolGeom { int h, w, d, oh, ow, pt, pl, n, no, C2; };   // n = 1 + h w, no = 1 + oh ow, C2 = 2 d

PoolGeom pool_geom(int h, int w, int d) {
  PoolGeom g{h, w, d, (h + 1) / 2, (w + 1) / 2, 0, 0, 1 + h * w, 0, 2 * d};
  g.pt = std::max((g.oh - 1) * 2 + 3 - h, 0) / 2;
  g.pl = std::max((g.ow - 1) * 2 + 3 - w, 0) / 2;
  g.no = 1 + g.oh * g.ow;
  return g;
}

// ---------------------------------------------------------------------------------------------- tokenizer
// rows[bi, 0, :] = 0; rows[bi, 1 + py ow + px, (ky p + kx) C + c] = img[bi, py st + ky, px st + kx, c]; columns K .. Kp are zeros.  Four columns a thread.
__global__ __launch_bounds__(256) void pit_unfold_kernel(const float* __restrict__ img, float* __restrict__ rows, int total4, int H, int W, int C, int p, int st,
                                                         int oh, int ow, int K, int Kp) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total4) return;
  const int kq = Kp >> 2, n = 1 + oh * ow;
  const int col0 = (t % kq) << 2, r = t / kq, tok = r % n, bi = r / n;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (tok > 0) {
    const int py = (tok - 1) / ow, px = (tok - 1) % ow;
    const float* src = img + ((bi * H + py * st) * W + px * st) * C;
    const int pc = p * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + j;
      if (col < K) v[j] = src[(col / pc) * W * C + col % pc];
    }
  }
  *(float4*)(rows + r * Kp + col0) = make_float4(v[0], v[1], v[2], v[3]);
}

// dimg[bi, y, x, c] = sum over the patches (py, px) whose window covers the pixel of drows[bi, 1 + py ow + px, ((y - py st) p + x - px st) C + c]
__global__ __launch_bounds__(256) void pit_unfold_bwd_kernel(const float* __restrict__ drows, float* __restrict__ dimg, int total, int H, int W, int C, int p, int st,
                                                             int oh, int ow, int Kp) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = e % C, r = e / C, x = r % W, y = (r / W) % H, bi = r / (W * H);
  const int n = 1 + oh * ow;
  const int py0 = max(0, (y - p + st) / st), py1 = min(oh - 1, y / st), px0 = max(0, (x - p + st) / st), px1 = min(ow - 1, x / st);
  float acc = 0.f;
  for (int py = py0; py <= py1; ++py)
    for (int px = px0; px <= px1; ++px)
      acc += drows[(bi * n + 1 + py * ow + px) * Kp + ((y - py * st) * p + (x - px * st)) * C + c];
  dimg[e] = acc;
}

// x[bi, 0, :] = cls + pos[0]; x[bi, r, :] += pos[r]  (pit.py:211-213)
__global__ __launch_bounds__(256) void pit_cls_pos_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos, int total, int n, int d) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = e % d, r = (e / d) % n;
  x[e] = (r == 0 ? cls[c] : x[e]) + pos[r * d + c];
}

// dpos[r, c] = r < n ? sum over the images, in order, of g[bi, r, c] : 0, r < pos_rows; dcls[c] = dpos[0, c]
__global__ __launch_bounds__(256) void pit_pos_grad_kernel(const float* __restrict__ g, float* __restrict__ dpos, float* __restrict__ dcls, int total, int b, int n, int d) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int r = e / d;
  float acc = 0.f;
  if (r < n)
    for (int bi = 0; bi < b; ++bi) acc += g[bi * n * d + e];
  dpos[e] = acc;
  if (r == 0) dcls[e] = acc;
}

// ---------------------------------------------------------------------------------------------- sums over the token rows 1..
// part[slice, c] = sum over the slice's rows (bi, p), p >= 1 counted without the class rows, of v[bi, p, c]
__global__ __launch_bounds__(256) void pit_rowsum_part_kernel(const float* __restrict__ v, float* __restrict__ part, int rows, int per_slice, int slices, int ntok, int C) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= slices * C) return;
  const int c = t % C, sl = t / C, np = ntok - 1;
  const int r0 = sl * per_slice, r1 = min(rows, r0 + per_slice);
  float acc = 0.f;
  for (int r = r0; r < r1; ++r) acc += v[((r / np) * ntok + 1 + r % np) * C + c];
  part[t] = acc;
}
__global__ __launch_bounds__(256) void pit_sum_slices_kernel(const float* __restrict__ part, float* __restrict__ out, int slices, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int s = 0; s < slices; ++s) acc += part[s * n + i];
  out[i] = acc;
}

int slices_of(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(PIT_SLICES_MAX, ceil_div(rows, 32))); }

// ---------------------------------------------------------------------------------------------- Pool, depthwise part
// dw[bi, 0, :] = 0; dw[bi, 1 + oy ow + ox, o] = bias[o] + sum over the taps inside the map of K[ty, tx, o] x[bi, 1 + (2 oy + ty - pt) w + 2 ox + tx - pl, o / 2]
// One thread: output channels o0 .. o0 + 3 (input channels o0 / 2, o0 / 2 + 1).
template <bool VEC>
__global__ __launch_bounds__(256) void pit_pool_dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ kern, const float* __restrict__ bias,
                                                              float* __restrict__ dw, int total, PoolGeom g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int cq = (g.C2 + 3) >> 2;
  const int o0 = (t % cq) << 2, r = t / cq, tok = r % g.no, bi = r / g.no;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (tok > 0) {
    const int oy = (tok - 1) / g.ow, ox = (tok - 1) % g.ow;
    if (VEC) { const float4 bv = *(const float4*)(bias + o0); acc[0] = bv.x; acc[1] = bv.y; acc[2] = bv.z; acc[3] = bv.w; }
    else for (int j = 0; j < 4 && o0 + j < g.C2; ++j) acc[j] = bias[o0 + j];
    const float* xi = x + (bi * g.n + 1) * g.d;
    for (int ty = 0; ty < 3; ++ty) {
      const int yy = 2 * oy + ty - g.pt;
      if (yy < 0 || yy >= g.h) continue;
      for (int tx = 0; tx < 3; ++tx) {
        const int xx = 2 * ox + tx - g.pl;
        if (xx < 0 || xx >= g.w) continue;
        const float* xp = xi + (yy * g.w + xx) * g.d;
        const float* kp = kern + (ty * 3 + tx) * g.C2 + o0;
        if (VEC) {
          const float2 xv = *(const float2*)(xp + (o0 >> 1));
          const float4 kv = *(const float4*)kp;
          acc[0] = fmaf(kv.x, xv.x, acc[0]); acc[1] = fmaf(kv.y, xv.x, acc[1]); acc[2] = fmaf(kv.z, xv.y, acc[2]); acc[3] = fmaf(kv.w, xv.y, acc[3]);
        } else {
          for (int j = 0; j < 4 && o0 + j < g.C2; ++j) acc[j] = fmaf(kp[j], xp[(o0 + j) >> 1], acc[j]);
        }
      }
    }
  }
  float* o = dw + r * g.C2 + o0;
  if (VEC) *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
  else for (int j = 0; j < 4 && o0 + j < g.C2; ++j) o[j] = acc[j];
}

// part[slice, tap, o] = sum over the slice's output positions (bi, oy, ox) of ddw[bi, 1 + oy ow + ox, o] x[bi, 1 + (2 oy + ty - pt) w + 2 ox + tx - pl, o / 2]
template <bool VEC>
__global__ __launch_bounds__(256) void pit_pool_dkern_part_kernel(const float* __restrict__ x, const float* __restrict__ ddw, float* __restrict__ part, int rows,
                                                                  int per_slice, int slices, PoolGeom g) {
  const int cq = (g.C2 + 3) >> 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= slices * 9 * cq) return;
  const int o0 = (t % cq) << 2, tap = (t / cq) % 9, sl = t / (cq * 9), ty = tap / 3, tx = tap % 3;
  const int r0 = sl * per_slice, r1 = min(rows, r0 + per_slice), npo = g.oh * g.ow;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0; r < r1; ++r) {
    const int bi = r / npo, pix = r % npo, oy = pix / g.ow, ox = pix % g.ow;
    const int yy = 2 * oy + ty - g.pt, xx = 2 * ox + tx - g.pl;
    if (yy < 0 || yy >= g.h || xx < 0 || xx >= g.w) continue;
    const float* gp = ddw + (bi * g.no + 1 + pix) * g.C2 + o0;
    const float* xp = x + (bi * g.n + 1 + yy * g.w + xx) * g.d;
    if (VEC) {
      const float4 gv = *(const float4*)gp;
      const float2 xv = *(const float2*)(xp + (o0 >> 1));
      acc[0] = fmaf(gv.x, xv.x, acc[0]); acc[1] = fmaf(gv.y, xv.x, acc[1]); acc[2] = fmaf(gv.z, xv.y, acc[2]); acc[3] = fmaf(gv.w, xv.y, acc[3]);
    } else {
      for (int j = 0; j < 4 && o0 + j < g.C2; ++j) acc[j] = fmaf(gp[j], xp[(o0 + j) >> 1], acc[j]);
    }
  }
  float* o = part + (sl * 9 + tap) * g.C2 + o0;
  if (VEC) *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
  else for (int j = 0; j < 4 && o0 + j < g.C2; ++j) o[j] = acc[j];
}

// dx[bi, 1 + y w + x, c] = sum over the outputs (oy, ox) whose window covers (y, x) -- 2 oy + ty - pt == y -- and j in {0, 1} of
// K[ty, tx, 2 c + j] ddw[bi, 1 + oy ow + ox, 2 c + j].  One thread: input channels c0 .. c0 + 3 (output channels 2 c0 .. 2 c0 + 7).  Row 0 is not written.
template <bool VEC>
__global__ __launch_bounds__(256) void pit_pool_dx_kernel(const float* __restrict__ ddw, const float* __restrict__ kern, float* __restrict__ dx, int total, PoolGeom g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int dq = (g.d + 3) >> 2, np = g.h * g.w;
  const int c0 = (t % dq) << 2, r = t / dq, pix = r % np, bi = r / np, y = pix / g.w, x = pix % g.w;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ty = 0; ty < 3; ++ty) {
    const int ny = y + g.pt - ty;
    if (ny < 0 || (ny & 1) || (ny >> 1) >= g.oh) continue;
    for (int tx = 0; tx < 3; ++tx) {
      const int nx = x + g.pl - tx;
      if (nx < 0 || (nx & 1) || (nx >> 1) >= g.ow) continue;
      const float* gp = ddw + (bi * g.no + 1 + (ny >> 1) * g.ow + (nx >> 1)) * g.C2 + 2 * c0;
      const float* kp = kern + (ty * 3 + tx) * g.C2 + 2 * c0;
      if (VEC) {
        const float4 g0 = *(const float4*)gp, g1 = *(const float4*)(gp + 4), k0 = *(const float4*)kp, k1 = *(const float4*)(kp + 4);
        acc[0] = fmaf(k0.y, g0.y, fmaf(k0.x, g0.x, acc[0])); acc[1] = fmaf(k0.w, g0.w, fmaf(k0.z, g0.z, acc[1]));
        acc[2] = fmaf(k1.y, g1.y, fmaf(k1.x, g1.x, acc[2])); acc[3] = fmaf(k1.w, g1.w, fmaf(k1.z, g1.z, acc[3]));
      } else {
        for (int j = 0; j < 4 && c0 + j < g.d; ++j) acc[j] = fmaf(kp[2 * j + 1], gp[2 * j + 1], fmaf(kp[2 * j], gp[2 * j], acc[j]));
      }
    }
  }
  float* o = dx + (bi * g.n + 1 + pix) * g.d + c0;
  if (VEC) *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
  else for (int j = 0; j < 4 && c0 + j < g.d; ++j) o[j] = acc[j];
}

bool vec4_ok(std::initializer_list<const void*> ps, int d) { return d % 4 == 0 && aligned16(ps); }

}  // namespace

// every index the kernels form stays below 2^31
bool pit_ops_fits(int64_t elems) { return elems > 0 && elems < (1ll << 31) - 4096; }

void launch_pit_unfold(const float* img, float* rows, int b, int H, int W, int C, int p, int st, int oh, int ow, int Kp, hipStream_t s) {
  const int64_t total4 = (int64_t)b * (1 + oh * ow) * (Kp / 4);
  hipLaunchKernelGGL(pit_unfold_kernel, dim3(grid256(total4)), dim3(256), 0, s, img, rows, (int)total4, H, W, C, p, st, oh, ow, p * p * C, Kp);
}
void launch_pit_unfold_bwd(const float* drows, float* dimg, int b, int H, int W, int C, int p, int st, int oh, int ow, int Kp, hipStream_t s) {
  const int64_t total = (int64_t)b * H * W * C;
  hipLaunchKernelGGL(pit_unfold_bwd_kernel, dim3(grid256(total)), dim3(256), 0, s, drows, dimg, (int)total, H, W, C, p, st, oh, ow, Kp);
}
void launch_pit_cls_pos(float* x, const float* cls, const float* pos, int b, int n, int d, hipStream_t s) {
  const int64_t total = (int64_t)b * n * d;
  hipLaunchKernelGGL(pit_cls_pos_kernel, dim3(grid256(total)), dim3(256), 0, s, x, cls, pos, (int)total, n, d);
}
void launch_pit_pos_grad(const float* g, float* dpos, float* dcls, int b, int n, int pos_rows, int d, hipStream_t s) {
  const int64_t total = (int64_t)pos_rows * d;
  hipLaunchKernelGGL(pit_pos_grad_kernel, dim3(grid256(total)), dim3(256), 0, s, g, dpos, dcls, (int)total, b, n, d);
}
int64_t pit_rowsum_ws_elems(int C) { return (int64_t)PIT_SLICES_MAX * C; }
// out[c] = sum over bi and the rows 1 .. ntok - 1 of v[bi, row, c]
void launch_pit_rowsum(const float* v, float* ws, float* out, int b, int ntok, int C, hipStream_t s) {
  const int rows = b * (ntok - 1), slices = slices_of(rows), per_slice = (int)ceil_div(rows, slices);
  hipLaunchKernelGGL(pit_rowsum_part_kernel, dim3(grid256((int64_t)slices * C)), dim3(256), 0, s, v, ws, rows, per_slice, slices, ntok, C);
  hipLaunchKernelGGL(pit_sum_slices_kernel, dim3(grid256(C)), dim3(256), 0, s, (const float*)ws, out, slices, C);
}

int64_t pit_pool_ws_elems(int d) { return (int64_t)PIT_SLICES_MAX * 9 * round_up(2 * d, 4); }
void launch_pit_pool_dw_fwd(const float* x, const float* kern, const float* bias, float* dw, int b, int h, int w, int d, hipStream_t s) {
  const PoolGeom g = pool_geom(h, w, d);
  const int64_t total = (int64_t)b * g.no * ceil_div(g.C2, 4);
  if (d % 2 == 0 && aligned16({x, kern, bias, dw}))
    hipLaunchKernelGGL((pit_pool_dw_fwd_kernel<true>), dim3(grid256(total)), dim3(256), 0, s, x, kern, bias, dw, (int)total, g);
  else hipLaunchKernelGGL((pit_pool_dw_fwd_kernel<false>), dim3(grid256(total)), dim3(256), 0, s, x, kern, bias, dw, (int)total, g);
}
// d(kernel) [3, 3, 1, 2 d] and d(bias) [2 d] of the depthwise convolution from its input tokens x [b, 1 + h w, d] and ddw [b, 1 + oh ow, 2 d]
void launch_pit_pool_dw_bwd_params(const float* x, const float* ddw, float* ws, float* dkern, float* dbias, int b, int h, int w, int d, hipStream_t s) {
  const PoolGeom g = pool_geom(h, w, d);
  const int rows = b * g.oh * g.ow, slices = slices_of(rows), per_slice = (int)ceil_div(rows, slices);
  const int cq = (int)ceil_div(g.C2, 4);
  const int64_t threads = (int64_t)slices * 9 * cq;
  if (d % 2 == 0 && aligned16({x, ddw, ws}))
    hipLaunchKernelGGL((pit_pool_dkern_part_kernel<true>), dim3(grid256(threads)), dim3(256), 0, s, x, ddw, ws, rows, per_slice, slices, g);
  else hipLaunchKernelGGL((pit_pool_dkern_part_kernel<false>), dim3(grid256(threads)), dim3(256), 0, s, x, ddw, ws, rows, per_slice, slices, g);
  hipLaunchKernelGGL(pit_sum_slices_kernel, dim3(grid256(9 * g.C2)), dim3(256), 0, s, (const float*)ws, dkern, slices, 9 * g.C2);
  launch_pit_rowsum(ddw, ws, dbias, b, g.no, g.C2, s);
}
// rows 1.. of dx [b, 1 + h w, d]
void launch_pit_pool_dw_bwd_dx(const float* ddw, const float* kern, float* dx, int b, int h, int w, int d, hipStream_t s) {
  const PoolGeom g = pool_geom(h, w, d);
  const int64_t total = (int64_t)b * h * w * ceil_div(d, 4);
  if (vec4_ok({ddw, kern, dx}, d)) hipLaunchKernelGGL((pit_pool_dx_kernel<true>), dim3(grid256(total)), dim3(256), 0, s, ddw, kern, dx, (int)total, g);
  else hipLaunchKernelGGL((pit_pool_dx_kernel<false>), dim3(grid256(total)), dim3(256), 0, s, ddw, kern, dx, (int)total, g);
}
