// Pre-processing of a cloud on the device (nvfpcc_amd/preprocess.py: preprocess_device): octree partition, block-sorted
// points, the candidate lists of nvf_nearest_dist2 and the float grids the trainer reads, without a host pass over
// anything that scales with the points or with the voxels.
//
// The reference's child index is [x >= mid] + 2 [y >= mid] + 4 [z >= mid] (get_octree.cpp:354-411), so its traversal
// order of the nodes of a level is ascending Morton code (x in the lowest bit of each level).  The occupancy of level
// 6 (16^3 cells), indexed by that code, is a 32 KiB bitmap whose BYTE i holds the eight children of level-5 cell i;
// the bitmap of level L is "byte != 0" of level L + 1, the breadth-first bytes of level L are the non-zero bytes of
// the bitmap of level L + 1 in index order, the leaf blocks are the set bits of the level-5 bitmap and a leaf's block
// id is the number of set bits below it.  Everything is an OR or an integer count: no result depends on an order.
//
//   nvf_pp_keys        per point: range check, sort key (cell code << 15 | local voxel), level-6 bit (LDS bitmap per
//                      workgroup, flushed with one global OR per non-zero word)
//   (the caller sorts the keys)
//   nvf_pp_tree        one workgroup: level bitmaps, per-level bytes, origins, the rank table, neighbour counts and
//                      their prefix sum
//   nvf_pp_blocks      sorted keys -> points, blk_off (each row written by the first point of its block), voxel count
//   nvf_pp_neighbours  one wave per block: the occupied blocks within +-2 steps, own block first, then by distance
//   nvf_pp_grids       dist = sqrtf(d2) (correctly rounded), gt = (d2 == 0)
#include "nvf_common.h"

#define PP_CELLS 32768
#define PP_B6_WORDS 8192
#define PP_BAD_KEY 0x7fffffff
#define PP_META_N 0
#define PP_META_BAD 1
#define PP_META_LEVEL 2
#define PP_META_NB 8
#define PP_META_VOXELS 9

// 5 bits -> bits 0, 3, 6, 9, 12 and back
__device__ __forceinline__ uint32_t pp_spread5(uint32_t v) {
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}
__device__ __forceinline__ uint32_t pp_gather5(uint32_t m) {
  return (m & 1u) | ((m >> 2) & 2u) | ((m >> 4) & 4u) | ((m >> 6) & 8u) | ((m >> 8) & 16u);
}
__device__ __forceinline__ uint32_t pp_cell_code(uint32_t cx, uint32_t cy, uint32_t cz) {
  return pp_spread5(cx) | (pp_spread5(cy) << 1) | (pp_spread5(cz) << 2);
}
// block id of an occupied level-5 cell: tab[0:1024] the level-5 bitmap, tab[1024:2048] set bits before each word
__device__ __forceinline__ int pp_rank(const uint32_t* __restrict__ tab, uint32_t cell) {
  return (int)tab[1024 + (cell >> 5)] + __popc(tab[cell >> 5] & ((1u << (cell & 31u)) - 1u));
}

__global__ __launch_bounds__(1024) void pp_keys_kernel(const int32_t* __restrict__ pts, int npts,
                                                       int32_t* __restrict__ keys, uint32_t* __restrict__ bitmap6,
                                                       int32_t* __restrict__ meta) {
  __shared__ uint32_t s_bits[PP_B6_WORDS];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  for (int i = tid; i < PP_B6_WORDS; i += 1024) s_bits[i] = 0u;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  int nbad = 0;
  for (size_t i = (size_t)blockIdx.x * 1024 + tid; i < (size_t)npts; i += (size_t)gridDim.x * 1024) {
    const int x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if ((x | y | z) & ~1023) {          // negative or >= 1024 on some axis
      ++nbad;
      keys[i] = PP_BAD_KEY;
      continue;
    }
    const uint32_t cell = pp_cell_code(x >> 5, y >> 5, z >> 5);
    keys[i] = (int32_t)((cell << 15) | ((x & 31) << 10) | ((y & 31) << 5) | (z & 31));
    const uint32_t m18 = (cell << 3) | ((x >> 4) & 1) | (((y >> 4) & 1) << 1) | (((z >> 4) & 1) << 2);
    const uint32_t bit = 1u << (m18 & 31u);
    if (!(s_bits[m18 >> 5] & bit)) atomicOr(&s_bits[m18 >> 5], bit);   // surfaces hit the same few words: test first
  }
  if (nbad) atomicAdd(&s_bad, nbad);
  __syncthreads();
  for (int i = tid; i < PP_B6_WORDS; i += 1024) {
    const uint32_t v = s_bits[i];
    if (v) atomicOr(&bitmap6[i], v);
  }
  if (tid == 0 && s_bad) atomicAdd(&meta[PP_META_BAD], s_bad);
}

// exclusive prefix sum of one value per thread over the 1024 threads of the workgroup; *total = the sum
__device__ __forceinline__ int pp_scan1024(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                       // s_wave may still be read by the previous scan
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int s = s_wave[k];
    all += s;
    if (k < wave) before += s;
  }
  *total = all;
  return before + incl - v;
}

// bit 4k + j of the result = byte j of src[8t + k] is non-zero: word t of the bitmap one level up
__device__ __forceinline__ uint32_t pp_fold(const uint32_t* src, int nsrc, int t) {
  uint32_t w = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t s = 8 * t + k < nsrc ? src[8 * t + k] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((s >> (8 * j)) & 0xffu) w |= 1u << (4 * k + j);
  }
  return w;
}

// the bytes of one level: for every set bit of `parent` (nw words) the byte of `child` with the bit's index
__device__ __forceinline__ void pp_emit(const uint32_t* parent, int nw, const uint32_t* child, uint8_t* out,
                                        int* s_wave, int32_t* count) {
  const int t = threadIdx.x;
  uint32_t w = t < nw ? parent[t] : 0u;
  int total;
  int at = pp_scan1024(__popc(w), s_wave, &total);
  while (w) {
    const int bi = 32 * t + __ffs((int)w) - 1;
    w &= w - 1u;
    out[at++] = (uint8_t)((child[bi >> 2] >> (8 * (bi & 3))) & 0xffu);
  }
  if (t == 0) *count = total;
}

__global__ __launch_bounds__(1024) void pp_tree_kernel(const uint32_t* __restrict__ bitmap6, int32_t* origins,
                                                       uint32_t* __restrict__ tab, uint8_t* __restrict__ oct,
                                                       int32_t* nb_off, int32_t* __restrict__ meta) {
  __shared__ uint32_t s5[1024], s4[128], s3[16], s2[2], s1[1];
  __shared__ int s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // this thread's 32 bytes of the level-6 bitmap are 32 level-5 cells: one word of the level-5 bitmap
  uint32_t w6[8];
  {
    const uint4 a = ((const uint4*)bitmap6)[2 * tid], b = ((const uint4*)bitmap6)[2 * tid + 1];
    w6[0] = a.x; w6[1] = a.y; w6[2] = a.z; w6[3] = a.w;
    w6[4] = b.x; w6[5] = b.y; w6[6] = b.z; w6[7] = b.w;
  }
  uint32_t w5 = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((w6[k] >> (8 * j)) & 0xffu) w5 |= 1u << (4 * k + j);
  s5[tid] = w5;
  __syncthreads();
  if (tid < 128) s4[tid] = pp_fold(s5, 1024, tid);
  __syncthreads();
  if (tid < 16) s3[tid] = pp_fold(s4, 128, tid);
  __syncthreads();
  if (tid < 2) s2[tid] = pp_fold(s3, 16, tid);
  __syncthreads();
  if (tid < 1) s1[tid] = pp_fold(s2, 2, tid);
  __syncthreads();
  // level L starts at byte (8^L - 1) / 7 of oct
  if (tid == 0) {
    oct[0] = (uint8_t)(s1[0] & 0xffu);
    meta[PP_META_LEVEL] = 1;
  }
  pp_emit(s1, 1, s2, oct + 1, s_wave, &meta[PP_META_LEVEL + 1]);
  pp_emit(s2, 2, s3, oct + 9, s_wave, &meta[PP_META_LEVEL + 2]);
  pp_emit(s3, 16, s4, oct + 73, s_wave, &meta[PP_META_LEVEL + 3]);
  pp_emit(s4, 128, s5, oct + 585, s_wave, &meta[PP_META_LEVEL + 4]);
  int n;
  const int base = pp_scan1024(__popc(w5), s_wave, &n);
  tab[tid] = w5;
  tab[1024 + tid] = (uint32_t)base;
  {
    int r = base;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b = (w6[k] >> (8 * j)) & 0xffu;
        if (b) {
          const uint32_t cell = 32u * tid + 4 * k + j;
          oct[4681 + r] = (uint8_t)b;
          origins[3 * r] = (int32_t)(pp_gather5(cell) << 5);
          origins[3 * r + 1] = (int32_t)(pp_gather5(cell >> 1) << 5);
          origins[3 * r + 2] = (int32_t)(pp_gather5(cell >> 2) << 5);
          ++r;
        }
      }
  }
  if (tid == 0) {
    meta[PP_META_N] = n;
    meta[PP_META_LEVEL + 5] = n;
  }
  __syncthreads();                       // origins of every block are written
  // neighbour counts, one wave per block: nb_off[b + 1] = occupied cells among the 125 around block b
  for (int b = wave; b < n; b += 16) {
    const int cx = origins[3 * b] >> 5, cy = origins[3 * b + 1] >> 5, cz = origins[3 * b + 2] >> 5;
    int cnt = 0;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int j = lane + 64 * round;
      const int nx = cx + j / 25 - 2, ny = cy + (j / 5) % 5 - 2, nz = cz + j % 5 - 2;
      bool ok = j < 125 && ((nx | ny | nz) & ~31) == 0;
      if (ok) {
        const uint32_t m = pp_cell_code(nx, ny, nz);
        ok = (s5[m >> 5] >> (m & 31u)) & 1u;
      }
      cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) nb_off[b + 1] = cnt;
  }
  __syncthreads();
  // counts -> offsets: thread t owns entries 32 t + 1 .. 32 t + 32
  int sum = 0;
  for (int e = 32 * tid; e < min(32 * tid + 32, n); ++e) sum += nb_off[e + 1];
  int total;
  int run = pp_scan1024(sum, s_wave, &total);
  for (int e = 32 * tid; e < min(32 * tid + 32, n); ++e) {
    run += nb_off[e + 1];
    nb_off[e + 1] = run;
  }
  if (tid == 0) {
    nb_off[0] = 0;
    meta[PP_META_NB] = total;
  }
}

__global__ __launch_bounds__(256) void pp_blocks_kernel(const int32_t* __restrict__ skeys, int npts,
                                                        const uint32_t* __restrict__ tab, int32_t* __restrict__ meta,
                                                        int32_t* __restrict__ pts, int32_t* __restrict__ blk_off) {
  const int n = min(meta[PP_META_N], PP_CELLS);
  int uniq = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 256) {
    const uint32_t key = (uint32_t)skeys[i];
    if (i == (size_t)npts - 1) blk_off[n] = npts;
    if (key >> 30) {                     // a rejected point (they sort to the end): the caller raises
      pts[3 * i] = pts[3 * i + 1] = pts[3 * i + 2] = -1;
      continue;
    }
    const uint32_t prev = i ? (uint32_t)skeys[i - 1] : 0xffffffffu;
    const uint32_t cell = key >> 15;
    pts[3 * i] = (int32_t)((pp_gather5(cell) << 5) | ((key >> 10) & 31u));
    pts[3 * i + 1] = (int32_t)((pp_gather5(cell >> 1) << 5) | ((key >> 5) & 31u));
    pts[3 * i + 2] = (int32_t)((pp_gather5(cell >> 2) << 5) | (key & 31u));
    if (key != prev) ++uniq;
    if (i == 0 || (prev >> 15) != cell) {
      const int r = pp_rank(tab, cell);
      if (r < n) blk_off[r] = (int32_t)i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) uniq += __shfl_xor(uniq, o, 64);
  if ((threadIdx.x & 63) == 0 && uniq) atomicAdd(&meta[PP_META_VOXELS], uniq);
}

// the 125 block steps in the order preprocess._neighbour_lists gives them: by squared length, (dx, dy, dz)
// lexicographic inside a length (a stable sort of the lexicographic list)
struct PpSteps { int8_t d[125][3]; };
static constexpr PpSteps pp_make_steps() {
  PpSteps s{};
  int n = 0;
  for (int r2 = 0; r2 <= 12; ++r2)
    for (int dx = -2; dx <= 2; ++dx)
      for (int dy = -2; dy <= 2; ++dy)
        for (int dz = -2; dz <= 2; ++dz)
          if (dx * dx + dy * dy + dz * dz == r2) {
            s.d[n][0] = (int8_t)dx; s.d[n][1] = (int8_t)dy; s.d[n][2] = (int8_t)dz;
            ++n;
          }
  return s;
}
__constant__ PpSteps pp_steps = pp_make_steps();

__global__ __launch_bounds__(256) void pp_neighbours_kernel(const int32_t* __restrict__ origins,
                                                            const uint32_t* __restrict__ tab,
                                                            const int32_t* __restrict__ nb_off,
                                                            int32_t* __restrict__ nb_idx, int n) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n) return;                    // the whole wave leaves
  const int cx = origins[3 * b] >> 5, cy = origins[3 * b + 1] >> 5, cz = origins[3 * b + 2] >> 5;
  int at = nb_off[b];
  const int end = nb_off[b + 1];
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const int j = lane + 64 * round;
    bool ok = j < 125;
    int idx = 0;
    if (ok) {
      const int nx = cx + pp_steps.d[j][0], ny = cy + pp_steps.d[j][1], nz = cz + pp_steps.d[j][2];
      ok = ((nx | ny | nz) & ~31) == 0;
      if (ok) {
        const uint32_t m = pp_cell_code(nx, ny, nz);
        ok = (tab[m >> 5] >> (m & 31u)) & 1u;
        if (ok) idx = pp_rank(tab, m);
      }
    }
    const unsigned long long mask = __ballot(ok);
    const int pos = at + __popcll(mask & ((1ull << lane) - 1ull));
    if (ok && pos < end) nb_idx[pos] = idx;
    at += __popcll(mask);
  }
}

// d2 and dist may be the same buffer: every thread reads its four values before it writes them.  sqrtf, not
// __fsqrt_rn: in a build without fast-math the former compiles to v_sqrt_f32 plus the two residual checks that make it
// correctly rounded, the latter to the bare 1-ulp instruction.
__global__ __launch_bounds__(256) void pp_grids_kernel(const int32_t* d2, float* dist, float* gt, size_t n) {
  const size_t quads = n >> 2, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += stride) {
    const int4 v = ((const int4*)d2)[i];
    const float4 g = make_float4(v.x == 0 ? 1.f : 0.f, v.y == 0 ? 1.f : 0.f, v.z == 0 ? 1.f : 0.f, v.w == 0 ? 1.f : 0.f);
    const float4 d = make_float4(sqrtf((float)v.x), sqrtf((float)v.y), sqrtf((float)v.z),
                                 sqrtf((float)v.w));
    ((float4*)dist)[i] = d;
    ((float4*)gt)[i] = g;
  }
  const size_t t = (quads << 2) + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) {
    const int v = d2[t];
    dist[t] = sqrtf((float)v);
    gt[t] = v == 0 ? 1.f : 0.f;
  }
}

extern "C" int nvf_pp_keys(const int32_t* pts, int npts, int32_t* keys, uint32_t* bitmap6, int32_t* meta,
                           void* stream) {
  if (!pts || !keys || !bitmap6 || !meta || npts <= 0) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  hipError_t e = hipMemsetAsync(bitmap6, 0, PP_B6_WORDS * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, NVF_PP_META_INTS * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  const int grid = min((npts + 1023) / 1024, 256);
  pp_keys_kernel<<<grid, 1024, 0, st>>>(pts, npts, keys, bitmap6, meta);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_tree(const uint32_t* bitmap6, int32_t* origins, uint32_t* rank_tab, uint8_t* octree_bytes,
                           int32_t* nb_off, int32_t* meta, void* stream) {
  if (!bitmap6 || !origins || !rank_tab || !octree_bytes || !nb_off || !meta) return NVF_EINVAL;
  if ((uintptr_t)bitmap6 & 15) return NVF_EINVAL;
  pp_tree_kernel<<<1, 1024, 0, nvf_stream(stream)>>>(bitmap6, origins, rank_tab, octree_bytes, nb_off, meta);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_blocks(const int32_t* sorted_keys, int npts, const uint32_t* rank_tab, int32_t* meta,
                             int32_t* pts, int32_t* blk_off, void* stream) {
  if (!sorted_keys || !rank_tab || !meta || !pts || !blk_off || npts <= 0) return NVF_EINVAL;
  const int grid = min((npts + 255) / 256, 2048);
  pp_blocks_kernel<<<grid, 256, 0, nvf_stream(stream)>>>(sorted_keys, npts, rank_tab, meta, pts, blk_off);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_neighbours(const int32_t* origins, const uint32_t* rank_tab, const int32_t* nb_off,
                                 int32_t* nb_idx, int nblocks, void* stream) {
  if (!origins || !rank_tab || !nb_off || !nb_idx || nblocks <= 0 || nblocks > PP_CELLS) return NVF_EINVAL;
  pp_neighbours_kernel<<<(nblocks + 3) / 4, 256, 0, nvf_stream(stream)>>>(origins, rank_tab, nb_off, nb_idx, nblocks);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_grids(const int32_t* d2, float* dist, float* gt, int64_t n, void* stream) {
  if (!d2 || !dist || !gt || n <= 0) return NVF_EINVAL;
  if (((uintptr_t)d2 | (uintptr_t)dist | (uintptr_t)gt) & 15) return NVF_EINVAL;
  const int grid = (int)min((int64_t)2048, ((n >> 2) + 255) / 256 + 1);
  pp_grids_kernel<<<grid, 256, 0, nvf_stream(stream)>>>(d2, dist, gt, (size_t)n);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
