// Occupancy selection: radix histograms of the decoder's probabilities (exact k-th largest value, per block or for
// the whole cloud, and the count / true-positive / squared-error curve over candidate thresholds) and thresholding
// with one threshold per block (nvfpcc_amd/thh_select.py).
//
// Sort key of a probability = its bit pattern (monotone for non-negative floats; -0.0 is folded onto +0.0).  Keys
// above the bits of 1.0f (NaN, negative, > 1) are input errors: they are counted into bad[b] and into no bin.
// Everything summed is an integer, so no result depends on the order of addition.  One workgroup owns one block and
// writes that block's rows, so there are no global atomics; the bins live in LDS (ds_add_u32 / ds_add_u64).
//
// Same-address LDS adds serialise, and trained decoders saturate (most voxels carry the key of 0.0, thousands that
// of 1.0).  Each wave therefore PEELS equal keys before it adds: the lanes that share the first live lane's bin are
// found with one ballot, their riders are reduced across the wave, and one lane adds the totals.  Peeling stops as
// soon as a round finds a lane alone in its bin (diverse data: one wasted ballot) or after OCC_PEEL rounds; what is
// left adds lane by lane.  A private histogram per wave was the alternative: 16 waves x 2048 bins x 16 B of riders
// is 512 KiB, over the 160 KiB of LDS, so it could only serve the count-only pass -- two code paths for one job.
#include "nvf_common.h"

#define OCC_THREADS 1024
#define OCC_MAX_BINS 2048
#define OCC_PEEL 4
#define OCC_KEY_ONE 0x3F800000u

template <bool EDGES, bool RIDERS>
__global__ __launch_bounds__(OCC_THREADS) void occ_hist_kernel(const float* __restrict__ p, int voxels, int shift,
                                                               int nbits, const uint32_t* __restrict__ prefix,
                                                               const float* __restrict__ edges, int nedges,
                                                               const int32_t* __restrict__ d2,
                                                               const uint8_t* __restrict__ gt,
                                                               uint32_t* __restrict__ count,
                                                               unsigned long long* __restrict__ sum_d2,
                                                               uint32_t* __restrict__ count_gt,
                                                               uint32_t* __restrict__ bad) {
  __shared__ uint32_t h_cnt[OCC_MAX_BINS];
  __shared__ uint32_t h_gt[RIDERS ? OCC_MAX_BINS : 1];
  __shared__ unsigned long long h_d2[RIDERS ? OCC_MAX_BINS : 1];
  __shared__ float s_edges[EDGES ? OCC_MAX_BINS : 1];
  __shared__ uint32_t h_bad;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nbins = EDGES ? nedges + 1 : 1 << nbits;
  for (int i = tid; i < nbins; i += OCC_THREADS) {
    h_cnt[i] = 0;
    if (RIDERS) { h_gt[i] = 0; h_d2[i] = 0ull; }
  }
  if (EDGES) for (int i = tid; i < nedges; i += OCC_THREADS) s_edges[i] = edges[i];
  if (tid == 0) h_bad = 0;
  __syncthreads();
  const size_t row = (size_t)b * voxels;
  const float* pb = p + row;
  const bool use_prefix = !EDGES && prefix != nullptr && shift + nbits < 32;
  const uint32_t want = use_prefix ? prefix[b] : 0u;
  const uint32_t mask = EDGES ? 0u : (uint32_t)((1u << nbits) - 1u);
  uint32_t nbad = 0;
  // every lane of a wave runs the same number of rounds: ballots and shuffles below need the whole wave
  for (int base = 0; base < voxels; base += OCC_THREADS) {
    const int i = base + tid;
    bool live = i < voxels;
    const float v = live ? pb[i] : 0.f;
    uint32_t key = __float_as_uint(v);
    if (key == 0x80000000u) key = 0u;
    if (live && key > OCC_KEY_ONE) { ++nbad; live = false; }
    if (use_prefix && (key >> (shift + nbits)) != want) live = false;
    uint32_t bin;
    if (EDGES) {           // bin = number of edges below v (edges ascending): lower bound of v among them
      int lo = 0, hi = nedges;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v > s_edges[mid]) lo = mid + 1; else hi = mid;
      }
      bin = (uint32_t)lo;
    } else {
      bin = (key >> shift) & mask;
    }
    uint32_t r_d2 = 0, r_gt = 0;
    if (RIDERS && live) {
      r_d2 = d2 ? (uint32_t)d2[row + i] : 0u;
      r_gt = gt ? (gt[row + i] != 0) : 0u;
    }
#pragma unroll 1
    for (int round = 0; round < OCC_PEEL; ++round) {
      const unsigned long long alive = __ballot(live);
      if (alive == 0ull) break;
      const int first = __ffsll((long long)alive) - 1;
      const uint32_t lead = (uint32_t)__shfl((int)bin, first, 64);
      const bool mine = live && bin == lead;
      const unsigned long long grp = __ballot(mine);
      const int n = __popcll(grp);
      if (n == 1) break;                                 // nothing to aggregate here: leave it to the plain adds
      if (RIDERS) {
        const uint32_t ngt = (uint32_t)__popcll(__ballot(mine && r_gt));
        uint32_t s = mine ? r_d2 : 0u;                   // <= 64 * 2^24: fits 32 bits
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
        if (lane == first) {
          atomicAdd(&h_cnt[lead], (uint32_t)n);
          if (ngt) atomicAdd(&h_gt[lead], ngt);
          if (s) atomicAdd(&h_d2[lead], (unsigned long long)s);
        }
      } else if (lane == first) {
        atomicAdd(&h_cnt[lead], (uint32_t)n);
      }
      if (mine) live = false;
    }
    if (live) {
      atomicAdd(&h_cnt[bin], 1u);
      if (RIDERS) {
        if (r_gt) atomicAdd(&h_gt[bin], 1u);
        if (r_d2) atomicAdd(&h_d2[bin], (unsigned long long)r_d2);
      }
    }
  }
  if (nbad) atomicAdd(&h_bad, nbad);
  __syncthreads();
  const size_t orow = (size_t)b * nbins;
  for (int i = tid; i < nbins; i += OCC_THREADS) {
    count[orow + i] = h_cnt[i];
    if (RIDERS) {
      if (count_gt) count_gt[orow + i] = h_gt[i];
      if (sum_d2) sum_d2[orow + i] = h_d2[i];
    }
  }
  if (tid == 0) bad[b] = h_bad;
}

static bool occ_riders_ok(const int32_t* d2, const uint8_t* gt, const uint64_t* sum_d2, const uint32_t* count_gt) {
  return (d2 != nullptr) == (sum_d2 != nullptr) && (gt != nullptr) == (count_gt != nullptr);
}

extern "C" int nvf_occ_hist(const float* p, int batch, int voxels, int shift, int nbits, const uint32_t* prefix,
                            const int32_t* d2, const uint8_t* gt, uint32_t* count, uint64_t* sum_d2,
                            uint32_t* count_gt, uint32_t* bad, void* stream) {
  if (!p || !count || !bad || batch <= 0 || voxels <= 0 || voxels > (1 << 24)) return NVF_EINVAL;
  if (nbits < 1 || nbits > 11 || shift < 0 || shift + nbits > 32) return NVF_EINVAL;
  if (!occ_riders_ok(d2, gt, sum_d2, count_gt)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  if (d2 || gt)
    occ_hist_kernel<false, true><<<batch, OCC_THREADS, 0, st>>>(p, voxels, shift, nbits, prefix, nullptr, 0, d2, gt, count,
                                                                (unsigned long long*)sum_d2, count_gt, bad);
  else
    occ_hist_kernel<false, false><<<batch, OCC_THREADS, 0, st>>>(p, voxels, shift, nbits, prefix, nullptr, 0, nullptr,
                                                                 nullptr, count, nullptr, nullptr, bad);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_hist_edges(const float* p, int batch, int voxels, const float* edges, int nedges,
                                  const int32_t* d2, const uint8_t* gt, uint32_t* count, uint64_t* sum_d2,
                                  uint32_t* count_gt, uint32_t* bad, void* stream) {
  if (!p || !count || !bad || !edges || batch <= 0 || voxels <= 0 || voxels > (1 << 24)) return NVF_EINVAL;
  if (nedges < 1 || nedges >= OCC_MAX_BINS) return NVF_EINVAL;
  if (!occ_riders_ok(d2, gt, sum_d2, count_gt)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  if (d2 || gt)
    occ_hist_kernel<true, true><<<batch, OCC_THREADS, 0, st>>>(p, voxels, 0, 0, nullptr, edges, nedges, d2, gt, count,
                                                               (unsigned long long*)sum_d2, count_gt, bad);
  else
    occ_hist_kernel<true, false><<<batch, OCC_THREADS, 0, st>>>(p, voxels, 0, 0, nullptr, edges, nedges, nullptr, nullptr,
                                                                count, nullptr, nullptr, bad);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

// ---------------------------------------------------------------------------
// thresholding with one threshold per block: the kernels of pointwise.hip (raster order, ballot prefix inside a
// wave, wave offsets through LDS, chunks walked in order) reading thh[b]; counts are integer sums.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void threshold_count_v_kernel(const float* __restrict__ p,
                                                                 const float* __restrict__ thh,
                                                                 int32_t* __restrict__ counts, int voxels) {
  __shared__ int wave_cnt[16];
  const float* pb = p + (size_t)blockIdx.x * voxels;
  const float t = thh[blockIdx.x];
  int c = 0;
  for (int i = threadIdx.x; i < voxels; i += blockDim.x) c += pb[i] > t ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += wave_cnt[k];
    counts[blockIdx.x] = s;
  }
}

extern "C" int nvf_threshold_count_v(const float* p, const float* thh, int32_t* counts, int batch, int voxels,
                                     void* stream) {
  if (!p || !thh || !counts || batch <= 0 || voxels <= 0 || voxels > (1 << 24)) return NVF_EINVAL;
  threshold_count_v_kernel<<<batch, 1024, 0, nvf_stream(stream)>>>(p, thh, counts, voxels);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

__global__ __launch_bounds__(1024) void threshold_compact_v_kernel(const float* __restrict__ p,
                                                                   const float* __restrict__ thh,
                                                                   const int32_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ origins,
                                                                   int32_t* __restrict__ coords, int dim) {
  __shared__ int wave_cnt[16];
  __shared__ int running;
  const int b = blockIdx.x, voxels = dim * dim * dim;
  const float* pb = p + (size_t)b * voxels;
  const float t = thh[b];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int oz = origins ? origins[3 * b] : 0, oy = origins ? origins[3 * b + 1] : 0, ox = origins ? origins[3 * b + 2] : 0;
  if (threadIdx.x == 0) running = offsets[b];
  __syncthreads();
  for (int base = 0; base < voxels; base += blockDim.x) {
    const int i = base + threadIdx.x;
    const bool hit = i < voxels && pb[i] > t;
    const unsigned long long mask = __ballot(hit);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    int off = running;
    for (int k = 0; k < wv; ++k) off += wave_cnt[k];
    if (hit) {
      const int z = i / (dim * dim), y = (i / dim) % dim, x = i % dim;
      int32_t* o = coords + (size_t)(off + before) * 3;
      o[0] = oz + z;
      o[1] = oy + y;
      o[2] = ox + x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int k = 0; k < nw; ++k) s += wave_cnt[k];
      running += s;
    }
    __syncthreads();
  }
}

extern "C" int nvf_threshold_compact_v(const float* p, const float* thh, const int32_t* offsets, const int32_t* origins,
                                       int32_t* coords, int batch, int dim, void* stream) {
  if (!p || !thh || !offsets || !coords || batch <= 0 || dim <= 0 || dim > 256) return NVF_EINVAL;
  threshold_compact_v_kernel<<<batch, 1024, 0, nvf_stream(stream)>>>(p, thh, offsets, origins, coords, dim);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
