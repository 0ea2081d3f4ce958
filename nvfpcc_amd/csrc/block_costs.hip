// Per-block costs of a frozen-decoder latent fit (nvf_block_costs): for every block of a batch its main focal term and
// its eval-mode latent bits, each as ONE float64 number.  Under frozen weights the objective is a plain sum of these
// per-block costs, so the encoder can keep, block by block, the best rounded latents it has seen (engine.fit_latents).
//
// One workgroup per block and nothing shared between workgroups: a row depends on neither the batch nor the block's
// place in it.  Terms are the float32 terms of the loss kernels (focal_elem, finals.h) and of the latent rate
// (rate_term, latent_tail.h: the arguments of latent_rate_body in mode 1); they are ADDED in float64 in a fixed order:
// per-lane partials over float4 groups kBcThreads apart (ascending), a fixed wave tree, waves in wave order.
#include "nvf_common.h"
#include "finals.h"
#include "latent_tail.h"

constexpr int kBcThreads = 256;                 // four whole waves
constexpr int kBcStride = kBcThreads * 4;       // floats one pass of the workgroup covers (16-byte loads)

__device__ __forceinline__ double bc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kBcThreads) void block_costs_kernel(const float* __restrict__ p,
                                                                 const float* __restrict__ gt,
                                                                 const float* __restrict__ dist, float alpha, float beta,
                                                                 const float* __restrict__ x_rounded,
                                                                 const float* __restrict__ sigma,
                                                                 const float* __restrict__ mu, double* __restrict__ out,
                                                                 int voxels, int c, int spatial) {
  __shared__ double red[kBcThreads / 64 + 1];
  const long b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* p4 = (const float4*)(p + b * voxels);
  const float4* g4 = (const float4*)(gt + b * voxels);
  const float4* d4 = dist ? (const float4*)(dist + b * voxels) : nullptr;
  const float a1 = alpha, a0 = 1.f - alpha;
  const bool has_dist = dist != nullptr;
  double s = 0.0;
  for (int i = threadIdx.x; i < (voxels >> 2); i += kBcThreads) {
    const float4 pv = p4[i], gv = g4[i];
    const float4 dv = d4 ? d4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float o;
    s += (double)focal_elem(pv.x, gv.x, dv.x, has_dist, a1, a0, beta, 0, o);
    s += (double)focal_elem(pv.y, gv.y, dv.y, has_dist, a1, a0, beta, 0, o);
    s += (double)focal_elem(pv.z, gv.z, dv.z, has_dist, a1, a0, beta, 0, o);
    s += (double)focal_elem(pv.w, gv.w, dv.w, has_dist, a1, a0, beta, 0, o);
  }
  s = bc_wave_sum(s);
  if (lane == 0) red[wave] = s;
  if (wave == kBcThreads / 64 - 1) {            // the block's c * spatial <= 64 latent symbols: the last wave's work
    const int n = c * spatial;
    double r = 0.0;
    if (lane < n) {
      const int ch = lane / spatial;
      r = (double)rate_term(x_rounded[b * n + lane], mu[ch], fabsf(sigma[ch]), 0.5f, 1.f, true).bits;
    }
    r = bc_wave_sum(r);
    if (lane == 0) red[kBcThreads / 64] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kBcThreads / 64; ++w) t += red[w];
    out[2 * b] = t;
    out[2 * b + 1] = red[kBcThreads / 64];
  }
}

extern "C" int nvf_block_costs(const float* p, const float* gt, const float* dist, float alpha, float beta,
                               const float* x_rounded, const float* sigma, const float* mu, double* out, int batch,
                               int voxels, int c, int spatial, void* stream) {
  if (!p || !gt || !x_rounded || !sigma || !mu || !out || batch < 1) return NVF_EINVAL;
  if (voxels < kBcStride || voxels % kBcStride != 0) return NVF_EINVAL;
  if (c < 1 || spatial < 1 || (long)c * spatial > 64) return NVF_EINVAL;
  if ((((uintptr_t)p | (uintptr_t)gt | (uintptr_t)dist) & 15) != 0) return NVF_EINVAL;      // float4 access
  block_costs_kernel<<<batch, kBcThreads, 0, nvf_stream(stream)>>>(p, gt, dist, alpha, beta, x_rounded, sigma, mu, out,
                                                                   voxels, c, spatial);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
