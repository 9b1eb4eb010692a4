// What the composites with a 'SAME' convolution share (cct.hip: the tokenizer; nest.hip: Aggregate; cvt.hip: the stage embedding): the convolution is im2col rows (cct_tok.hip)
// times the HWIO kernel viewed as [k*k*Cin, Cout] on the GEMM launchers, in image chunks so that the row workspace is bounded.  Here: the
// weight-gradient product, the chunk accumulation and the workspace budget of one chunk.
#pragma once
#include "composite.h"

// dst = first ? src : dst + src   (weight-gradient partials of the image chunks, summed in chunk order)
static __global__ void conv_accum_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n, int first) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dst[e] = first ? src[e] : dst[e] + src[e];
}

// Weight gradient of a convolution: dWp[Kp, N] = rows[M, Kp]^T dY[M, N] over all Kp (>= 64) padded columns.  On the split-operand kernel the M token
// rows are cut into slices (the kernel's batch index, the last one shorter) so that tiles x slices fills the chip; the fp32 partials are summed in
// slice order by launch_reduce_partials.  `part` holds max_slices * Kp * N floats.  The first K * N floats of dWp are the kernel's gradient.
constexpr int CONV_WGRAD_SLICES = 32;
inline void conv_wgrad(const float* rows, int Kp, const float* dY, float* dWp, float* part, int M, int N, int x3, hipStream_t s) {
  GenericGemmArgs g;
  g.A = rows; g.B = dY; g.M = Kp; g.N = N; g.K = M; g.sam = 1; g.sak = Kp; g.sbk = N; g.sbn = 1; g.x3 = x3;
  EpiParams ep;
  ep.out = dWp; ep.ldo = N; ep.M = Kp; ep.N = N; ep.vec_ok = (N % 4 == 0) && aligned16({dWp, part});
  int slices = 1;
  if (x3 && gemm_bf16x3_supported(g, 0, 0, 0)) {
    const int64_t tiles = ceil_div(Kp, 128) * ceil_div(N, 128);
    const int64_t want = std::min<int64_t>({std::max<int64_t>(1, 1024 / tiles), std::max<int64_t>(1, M / 256), CONV_WGRAD_SLICES});
    if (want > 1) {
      const int ks = (int)round_up(ceil_div(M, want), 32);
      slices = (int)ceil_div(M, ks);
      if (slices > 1) {
        g.K = ks; g.nb = slices; g.sAb = (int64_t)ks * Kp; g.sBb = (int64_t)ks * N; g.k_last = M - (slices - 1) * ks;
        ep.out = part; ep.out_batch_stride = (int64_t)Kp * N;
      }
    }
  }
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
  if (slices > 1) launch_reduce_partials(part, slices, (int64_t)Kp * N, (int64_t)Kp * N, dWp, 1.0f, s);
}
constexpr int64_t IM2COL_BUDGET = 32ll << 20;   // floats of one im2col chunk (128 MB); a single image may exceed it
