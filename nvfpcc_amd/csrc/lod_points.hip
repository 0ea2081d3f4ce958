// Level-of-detail decode: from the trunk activation a coarse classifier head reads (conv1_cls on [B, C, 16^3],
// conv0_cls on [B, C, 8^3]) to the points of the coarse cloud, without the probabilities ever reaching memory.
//
//   nvf_head_occ_bits      the head's forward accumulation (head_fwd.h: the body of the head forward kernel, so the same
//                          fmaf chain per voxel), bias, sigmoid, `p > t`, and the hits leave as occupancy words: bit k of
//                          word w of a block is its voxel 64 w + k in raster order.  A thread owns four consecutive x, so
//                          sixteen consecutive lanes own 64 consecutive voxels; each lane fetches the hit bit of "its"
//                          voxel of word j from lane 16 j + lane / 4 and ONE ballot of the wave is word j.  Counts are
//                          popcounts, added in integers.
//   nvf_points_from_bits   one wave per block walks the block's words in order (occ_coder.h: occ_walk_bits, the walk
//                          the lossless coder's cell lists share); lane k owns bit k, its output slot is the block's
//                          offset + the bits before it.  d = 8, 16 or 32: 8, 64 or 512 words per block, 64 at a time.
//                          No workgroup waits for another.
#include "head_fwd.h"
#include "occ_coder.h"

namespace {

// what the head forward does with a thread's four sums here (head_fwd_body's SINK): bits, not stores
template <int S>
struct OccBitsSink {
  const float* bias;
  const float* thh_v;
  float thh;
  unsigned long long* words;
  int32_t* counts;
  __device__ __forceinline__ void operator()(const float (&acc)[4], int b, int z, int y, int x) const {
    constexpr int WPB = S * S * S / 64;               // words per block
    const float bv = bias ? bias[0] : 0.f;
    const float t = thh_v ? thh_v[b] : thh;
    int nib = 0;
#pragma unroll
    for (int o = 0; o < 4; ++o) nib |= (nvf_act(acc[o] + bv, NVF_ACT_SIGMOID) > t ? 1 : 0) << o;
    const int lane = threadIdx.x & 63;
    // raster index of this thread's first voxel inside its block; lanes 16 j .. 16 j + 15 hold word (that index) / 64
    const int vox = (z * S + y) * S + x;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int src = __shfl(nib, 16 * j + (lane >> 2), 64);
      const unsigned long long word = __ballot((src >> (lane & 3)) & 1);
      cnt += __popcll(word);
      if (lane == 16 * j) words[(size_t)b * WPB + (vox >> 6)] = word;
    }
    if (lane == 0) atomicAdd(counts + b, cnt);        // integers: any order gives the same sum
  }
};

template <class H>
__global__ __launch_bounds__(H::NT) void head_occ_bits_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float thh,
                                                              const float* __restrict__ thh_v,
                                                              unsigned long long* __restrict__ words,
                                                              int32_t* __restrict__ counts) {
  // sixteen lanes = 64 consecutive voxels of the raster, starting at a multiple of 64: full-width rows, a tile's rows
  // of one z are consecutive y, and the sink runs in whole waves (NACT is a multiple of 64)
  static_assert(H::TY % (16 / H::XG) == 0 && (H::S * H::S) % 64 == 0 && H::NACT % 64 == 0, "a word lies inside one z of a tile");
  __shared__ __attribute__((aligned(16))) float smem[HFwdSmem<H>::WORDS];
  head_fwd_body<H, false>(x, w, nullptr, nullptr, nullptr, nullptr, NVF_ACT_SIGMOID, blockIdx.x, smem, nullptr,
                          OccBitsSink<H::S>{bias, thh_v, thh, words, counts});
}

// one wave per block, four blocks per workgroup
__global__ __launch_bounds__(256) void points_from_bits_kernel(const unsigned long long* __restrict__ words,
                                                               const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ origins,
                                                               int32_t* __restrict__ points, int batch, int d, int shift,
                                                               int n) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;
  const int ld = d == 8 ? 3 : (d == 16 ? 4 : 5);       // d is a power of two: shifts, the integers of / and %
  const int oz = origins ? origins[3 * b] >> shift : 0, oy = origins ? origins[3 * b + 1] >> shift : 0,
            ox = origins ? origins[3 * b + 2] >> shift : 0;
  occ_walk_bits(words, b, d * d * d / 64, offsets[b], lane, [=](int slot, int v) {
    if (slot < 0 || slot >= n) return;
    int32_t* o = points + (size_t)slot * 3;
    o[0] = oz + (v >> (2 * ld));
    o[1] = oy + ((v >> ld) & (d - 1));
    o[2] = ox + (v & (d - 1));
  });
}

}  // namespace

extern "C" int nvf_head_occ_bits(const float* x, const float* w_fwd, const float* bias, float thh, const float* thh_v,
                                 uint64_t* words, int32_t* counts, int batch, int c, int d, void* stream) {
  if (!x || !w_fwd || !words || !counts || batch <= 0) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
#define NVF_H(CC, SS, TZ, TY, CPS)                                                                                 \
  if (c == CC && d == SS) {                                                                                        \
    using H = HPCfg<CC, SS, TZ, TY, CPS>;                                                                          \
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)batch * sizeof(int32_t), st);                                 \
    if (e != hipSuccess) return (int)e;                                                                            \
    head_occ_bits_kernel<H><<<batch * (SS / TZ) * (SS / TY), H::NT, 0, st>>>(x, w_fwd, bias, thh, thh_v,           \
                                                                             (unsigned long long*)words, counts);  \
    NVF_LAUNCH_CHECK();                                                                                            \
    return NVF_OK;                                                                                                 \
  }
  // the tiles of the head forward (heads.hip: nvf_head_fwd_launch) for the same shapes
  NVF_H(8, 16, 8, 8, 2)
  NVF_H(16, 8, 8, 8, 4)
  NVF_H(16, 16, 8, 8, 2)
  NVF_H(32, 8, 8, 8, 4)
#undef NVF_H
  return NVF_EINVAL;
}

extern "C" int nvf_points_from_bits(const uint64_t* words, const int32_t* offsets, const int32_t* origins,
                                    int32_t* points, int n, int batch, int d, int shift, void* stream) {
  if (!words || !offsets || !points || n < 0 || batch <= 0 || (d != 8 && d != 16 && d != 32) || shift < 0 || shift > 2)
    return NVF_EINVAL;
  points_from_bits_kernel<<<(batch + 3) / 4, 256, 0, nvf_stream(stream)>>>((const unsigned long long*)words, offsets,
                                                                           origins, points, batch, d, shift, n);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
