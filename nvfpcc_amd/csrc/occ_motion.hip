// Block motion compensation in front of the inter contexts (nvfpcc_amd/lossless_mv_pack.py; include/nvf_hip.h, "scalable
// lossless geometry, motion-compensated reference", is the contract).  The version-4 coder only ever sees R, the
// reference words of this frame's blocks; here R is built by fetching each block's window of the reference displaced by
// the block's own integer vector, R'_b(v) = Ref(o_b + v - d_b), and the vectors are found by an exhaustive search.
//
//   nvf_occ_mv_words    one workgroup per block: the at most 2 x 2 x 2 source blocks resolved once by binary search among
//                       the reference's sorted block keys, every output row a 64-bit shift of one or two source rows
//   nvf_occ_mv_search   one workgroup per block: the exact Hamming distance of the block to its window under every vector
//                       of the cube [-r, r]^3, and the winner in the defined order
//
// The reference lives on its OWN blocks (ref_own uint64 [nref, 512], ref_keys sorted ascending); a block that is absent
// and a coordinate outside [0, 2^NVF_OCC_REF_COORD_BITS) read as 0.  A row is the uint32 of the 32 voxels along axis 2
// at one (v0, v1): two rows make one uint64 word of the gt_w0 format.  All window arithmetic is 64-bit, so no content of
// origins or mv overflows, and every index into ref_own comes out of the search, so none leaves [0, nref).
//
// Search: the window of all vectors is (32 + 2r)^2 rows of 32 + 2r bits, staged once as uint64 (18 KiB at r = 8) next to
// the block's own 1024 rows.  For one (d0, d1) the 2r + 1 vectors along axis 2 read the SAME window rows at another
// shift, so a wave takes a (d0, d1) pair, its lanes the rows, and every lane keeps 2r + 1 integer sums in registers; one
// wave reduction per pair leaves the costs in LDS, and one argmin pass over packed (cost, |d|^2, index) keys picks the
// winner: index order is the lexicographic order of (d0, d1, d2).  Integers only: every call gives the same bits.
#include "nvf_common.h"

#define MV_R NVF_OCC_MV_MAX_RADIUS
#define MV_ND (2 * MV_R + 1)                           // vectors per axis at the largest radius
#define MV_WIN (32 + 2 * MV_R)                         // window rows per axis, and bits per row
#define MV_THREADS 256
#define MV_COORD_BLOCKS (1 << (NVF_OCC_REF_COORD_BITS - 5))

namespace {

// the reference block with block coordinates (k0, k1, k2) -> its index in ref_own, -1 when absent or out of range
__device__ __forceinline__ int mv_find(const long long* __restrict__ keys, int nref, long long k0, long long k1, long long k2) {
  if (k0 < 0 || k1 < 0 || k2 < 0 || k0 >= MV_COORD_BLOCKS || k1 >= MV_COORD_BLOCKS || k2 >= MV_COORD_BLOCKS) return -1;
  const long long key = (k0 << 42) | (k1 << 21) | k2;
  int lo = 0, hi = nref;                               // the first entry >= key
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < nref && keys[lo] == key) ? lo : -1;     // lo < nref: whatever keys holds, inside ref_own
}

// row (c0 & 31, c1 & 31) of source block `src` (-1: absent) as uint32
__device__ __forceinline__ uint32_t mv_row(const uint32_t* __restrict__ ref32, int src, long long c0, long long c1) {
  return src < 0 ? 0u : ref32[(size_t)src * 1024 + (int)(c0 & 31) * 32 + (int)(c1 & 31)];
}

__global__ __launch_bounds__(MV_THREADS) void mv_words_kernel(const uint32_t* __restrict__ ref32,
                                                              const long long* __restrict__ keys, int nref,
                                                              const int32_t* __restrict__ origins,
                                                              const int32_t* __restrict__ mv,
                                                              unsigned long long* __restrict__ words,
                                                              int32_t* __restrict__ status) {
  __shared__ int src[8];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long* out = words + (size_t)b * 512;
  const int d0 = mv[3 * b], d1 = mv[3 * b + 1], d2 = mv[3 * b + 2];
  if (d0 < -MV_R || d0 > MV_R || d1 < -MV_R || d1 > MV_R || d2 < -MV_R || d2 > MV_R) {   // uniform over the workgroup
    out[tid] = 0ull;
    out[tid + MV_THREADS] = 0ull;
    if (tid == 0) atomicAdd(status, 1);
    return;
  }
  const long long a0 = (long long)origins[3 * b] - d0, a1 = (long long)origins[3 * b + 1] - d1,
                  a2 = (long long)origins[3 * b + 2] - d2;       // the window's first coordinate on each axis
  if (tid < 8)
    src[tid] = mv_find(keys, nref, (a0 >> 5) + (tid >> 2), (a1 >> 5) + ((tid >> 1) & 1), (a2 >> 5) + (tid & 1));
  __syncthreads();
  const int sh = (int)(a2 & 31);
#pragma unroll
  for (int w = tid; w < 512; w += MV_THREADS) {        // word w = rows (v0, v1) and (v0, v1 + 1), v1 even
    const int v0 = w >> 4, v1 = (w & 15) * 2;
    const long long c0 = a0 + v0;
    const int s0 = ((int)((c0 >> 5) - (a0 >> 5))) << 2;
    uint32_t row[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long c1 = a1 + v1 + h;
      const int s = s0 | (((int)((c1 >> 5) - (a1 >> 5))) << 1);
      const unsigned long long two = ((unsigned long long)(sh ? mv_row(ref32, src[s | 1], c0, c1) : 0u) << 32) |
                                     mv_row(ref32, src[s], c0, c1);
      row[h] = (uint32_t)(two >> sh);
    }
    out[w] = ((unsigned long long)row[1] << 32) | row[0];
  }
}

__global__ __launch_bounds__(MV_THREADS) void mv_search_kernel(const uint32_t* __restrict__ gt32,
                                                               const uint32_t* __restrict__ ref32,
                                                               const long long* __restrict__ keys, int nref,
                                                               const int32_t* __restrict__ origins, int r,
                                                               int32_t* __restrict__ mv, uint32_t* __restrict__ cost) {
  __shared__ unsigned long long win[MV_WIN * MV_WIN];  // row (i0, i1): bit j = Ref(o - r + (i0, i1, j))
  __shared__ uint32_t G[1024];
  __shared__ uint32_t costs[MV_ND * MV_ND * MV_ND];
  __shared__ unsigned long long best[MV_THREADS / 64];
  __shared__ int src[27];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = 2 * r + 1, nw = 32 + 2 * r;
  const long long a0 = (long long)origins[3 * b] - r, a1 = (long long)origins[3 * b + 1] - r,
                  a2 = (long long)origins[3 * b + 2] - r;
  if (tid < 27)
    src[tid] = mv_find(keys, nref, (a0 >> 5) + tid / 9, (a1 >> 5) + (tid / 3) % 3, (a2 >> 5) + tid % 3);
  for (int i = tid; i < 1024; i += MV_THREADS) G[i] = gt32[(size_t)b * 1024 + i];
  __syncthreads();
  const int sh = (int)(a2 & 31);
  const unsigned long long keep = (1ull << nw) - 1;    // nw <= 48
  for (int i = tid; i < nw * nw; i += MV_THREADS) {
    const int i0 = i / nw, i1 = i - i0 * nw;
    const long long c0 = a0 + i0, c1 = a1 + i1;
    const int s = ((int)((c0 >> 5) - (a0 >> 5))) * 9 + ((int)((c1 >> 5) - (a1 >> 5))) * 3;
    const unsigned long long lo = ((unsigned long long)mv_row(ref32, src[s + 1], c0, c1) << 32) | mv_row(ref32, src[s], c0, c1);
    unsigned long long v = lo >> sh;
    if (sh) v |= (unsigned long long)mv_row(ref32, src[s + 2], c0, c1) << (64 - sh);
    win[i0 * MV_WIN + i1] = v & keep;
  }
  __syncthreads();
  // vector (d0, d1, d2) = (e0, e1, e2) - r reads window row (v0 + 2r - e0, v1 + 2r - e1) shifted by 2r - e2
  for (int pair = wave; pair < nd * nd; pair += MV_THREADS / 64) {
    const int e0 = pair / nd, e1 = pair - e0 * nd;
    uint32_t sum[MV_ND];
#pragma unroll
    for (int j = 0; j < MV_ND; ++j) sum[j] = 0;
    for (int row = lane; row < 1024; row += 64) {
      const uint32_t g = G[row];
      const unsigned long long w = win[((row >> 5) + 2 * r - e0) * MV_WIN + (row & 31) + 2 * r - e1];
#pragma unroll
      for (int j = 0; j < MV_ND; ++j)
        if (j < nd) sum[j] += __popc(g ^ (uint32_t)(w >> (2 * r - j)));
    }
#pragma unroll
    for (int j = 0; j < MV_ND; ++j) {
      if (j < nd) {
        uint32_t s = sum[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) costs[pair * nd + j] = s;
      }
    }
  }
  __syncthreads();
  // the winner: smallest (cost, |d|^2, index); index order is (d0, d1, d2) lexicographic
  unsigned long long k = ~0ull;
  for (int i = tid; i < nd * nd * nd; i += MV_THREADS) {
    const int e0 = i / (nd * nd), e1 = (i / nd) % nd, e2 = i % nd;
    const int n2 = (e0 - r) * (e0 - r) + (e1 - r) * (e1 - r) + (e2 - r) * (e2 - r);
    const unsigned long long c = ((unsigned long long)costs[i] << 32) | ((unsigned long long)n2 << 16) | (unsigned)i;
    k = c < k ? c : k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o, 64);
    k = other < k ? other : k;
  }
  if (lane == 0) best[wave] = k;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < MV_THREADS / 64; ++w) k = best[w] < k ? best[w] : k;
    const int i = (int)(k & 0xFFFF);
    mv[3 * b] = i / (nd * nd) - r;
    mv[3 * b + 1] = (i / nd) % nd - r;
    mv[3 * b + 2] = i % nd - r;
    cost[2 * b] = (uint32_t)(k >> 32);
    cost[2 * b + 1] = costs[(r * nd + r) * nd + r];
  }
}

}  // namespace

extern "C" int nvf_occ_mv_words(const uint64_t* ref_own, const int64_t* ref_keys, int nref, const int32_t* origins,
                                const int32_t* mv, int nblocks, uint64_t* words, int32_t* status, void* stream) {
  if (!origins || !mv || !words || !status || nref < 0 || (nref > 0 && (!ref_own || !ref_keys)) || nblocks <= 0 ||
      nblocks > NVF_OCC_HIER_MAX_BATCH)
    return NVF_EINVAL;
  mv_words_kernel<<<nblocks, MV_THREADS, 0, nvf_stream(stream)>>>((const uint32_t*)ref_own, (const long long*)ref_keys, nref,
                                                                  origins, mv, (unsigned long long*)words, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_mv_search(const uint64_t* gt_w0, const uint64_t* ref_own, const int64_t* ref_keys, int nref,
                                 const int32_t* origins, int nblocks, int radius, int32_t* mv, uint32_t* cost,
                                 void* stream) {
  if (!gt_w0 || !origins || !mv || !cost || nref < 0 || (nref > 0 && (!ref_own || !ref_keys)) || nblocks <= 0 ||
      nblocks > NVF_OCC_HIER_MAX_BATCH || radius < 1 || radius > NVF_OCC_MV_MAX_RADIUS)
    return NVF_EINVAL;
  mv_search_kernel<<<nblocks, MV_THREADS, 0, nvf_stream(stream)>>>((const uint32_t*)gt_w0, (const uint32_t*)ref_own,
                                                                   (const long long*)ref_keys, nref, origins, radius, mv,
                                                                   cost);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
