// Pre-processing of clouds with 11 or 12 bits per axis on the device (nvfpcc_amd/preprocess.py: preprocess_device with
// bits > 10).  The definitions are those of pp_device.hip, one or two octree levels deeper: leaf blocks stay 32^3, the
// leaves are the cells of level D = bits - 5 (6 or 7), a cell code is the 3 D-bit Morton code of (x >> 5, y >> 5,
// z >> 5) with x in the lowest bit of each level, the bitmap of level L is "byte != 0" of level L + 1, the breadth-first
// bytes of level L are the non-zero bytes of the bitmap of level L + 1 in index order, the leaves are the set bits of the
// level-D bitmap and a leaf's block id is the number of set bits below it.  Everything is an OR or an integer count.
//
// What changes is the size: the bitmap of level D + 1 is 256 KiB (11 bits) or 2 MiB (12 bits) and stays in global
// memory, a sort key needs up to 36 bits, and the level-D bitmap has up to 65536 words, so "set bits before each word"
// is a grid-wide exclusive scan.  Every scan here is three launches -- sums per workgroup, one workgroup scans the at
// most 1024 partial sums, emit -- ordered by the stream: no workgroup ever waits for another.
//
//   nvf_pp_keys_deep        per point: range check, int64 sort key, the point's bit in the level-(D + 1) bitmap
//                           (tested before the atomic OR: a surface hits the same few words again and again)
//   (the caller sorts the keys)
//   nvf_pp_tree_deep        D + 1 fold launches, then per level sums / scan / emit; neighbour counts, one wave per block,
//                           and their prefix sum
//   nvf_pp_blocks_deep      sorted keys -> points, blk_off, voxel count
//   nvf_pp_neighbours_deep  one wave per block: the occupied blocks within +-2 steps of the 2^D grid
#include "nvf_common.h"

#define PPD_BAD_KEY 0x7fffffffffffffffll
#define PPD_META_N 0
#define PPD_META_BAD 1
#define PPD_META_LEVEL 2
#define PPD_META_NB 10
#define PPD_META_VOXELS 11
// work: the bitmaps of levels 0 .. D - 1 from word 0 (at most 9364 words), the partial sums of a scan from PPD_PART_AT
#define PPD_PART_AT 10240
#define PPD_MAX_PARTS 1024

// D bits -> bits 0, 3, 6, ... and back
template <int D>
__device__ __forceinline__ uint32_t ppd_spread(uint32_t v) {
  uint32_t m = 0u;
#pragma unroll
  for (int b = 0; b < D; ++b) m |= ((v >> b) & 1u) << (3 * b);
  return m;
}
template <int D>
__device__ __forceinline__ uint32_t ppd_gather(uint32_t m) {
  uint32_t v = 0u;
#pragma unroll
  for (int b = 0; b < D; ++b) v |= ((m >> (3 * b)) & 1u) << b;
  return v;
}
template <int D>
__device__ __forceinline__ uint32_t ppd_cell_code(uint32_t cx, uint32_t cy, uint32_t cz) {
  return ppd_spread<D>(cx) | (ppd_spread<D>(cy) << 1) | (ppd_spread<D>(cz) << 2);
}
// block id of an occupied level-D cell: tab[0:W] the level-D bitmap, tab[W:2W] set bits before each word, W = 8^D / 32
template <int D>
__device__ __forceinline__ int ppd_rank(const uint32_t* __restrict__ tab, uint32_t cell) {
  constexpr uint32_t W = 1u << (3 * D - 5);
  return (int)tab[W + (cell >> 5)] + __popc(tab[cell >> 5] & ((1u << (cell & 31u)) - 1u));
}

static inline int ppd_words(int level) { return level < 2 ? 1 : 1 << (3 * level - 5); }   // of the bitmap of a level
static inline int ppd_work_at(int level) {                                                   // its place in `work`
  int at = 0;
  for (int l = 0; l < level; ++l) at += ppd_words(l);
  return at;
}
static inline int ppd_cap(int level, int npts) {                // a level has at most min(8^level, points) nodes
  const int64_t full = (int64_t)1 << (3 * level);
  return full < npts ? (int)full : npts;
}

template <int D>
__global__ __launch_bounds__(256) void ppd_keys_kernel(const int32_t* __restrict__ pts, int npts,
                                                       int64_t* __restrict__ keys, uint32_t* bitmap,
                                                       int32_t* __restrict__ meta) {
  constexpr int OUTSIDE = ~((1 << (D + 5)) - 1);
  int nbad = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 256) {
    const int x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if ((x | y | z) & OUTSIDE) {        // negative or >= 2^bits on some axis
      ++nbad;
      keys[i] = PPD_BAD_KEY;
      continue;
    }
    const uint32_t cell = ppd_cell_code<D>(x >> 5, y >> 5, z >> 5);
    keys[i] = ((int64_t)cell << 15) | (int64_t)(((x & 31) << 10) | ((y & 31) << 5) | (z & 31));
    const uint32_t m = (cell << 3) | ((x >> 4) & 1) | (((y >> 4) & 1) << 1) | (((z >> 4) & 1) << 2);
    const uint32_t bit = 1u << (m & 31u);
    uint32_t* w = bitmap + (m >> 5);
    if (!(*w & bit)) atomicOr(w, bit);   // a stale read costs one OR too many, never a wrong bit
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&meta[PPD_META_BAD], nbad);
}

// exclusive prefix sum of one value per thread over the 1024 threads of the workgroup; *total = the sum
__device__ __forceinline__ int ppd_scan1024(int v, int* s_wave, int* total) {
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

// word t of the bitmap one level up: bit 4k + j = byte j of src[8t + k] is non-zero
__global__ __launch_bounds__(256) void ppd_fold_kernel(const uint32_t* __restrict__ src, int nsrc,
                                                       uint32_t* __restrict__ dst, int ndst) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ndst) return;
  uint32_t w = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t s = 8 * t + k < nsrc ? src[8 * t + k] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((s >> (8 * j)) & 0xffu) w |= 1u << (4 * k + j);
  }
  dst[t] = w;
}

// scan pass 1 over a bitmap: part[g] = set bits of the 1024 words of workgroup g
__global__ __launch_bounds__(1024) void ppd_level_sums_kernel(const uint32_t* __restrict__ bm, int nw,
                                                              int32_t* __restrict__ part) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  int total;
  ppd_scan1024(i < nw ? __popc(bm[i]) : 0, s_wave, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// scan pass 2, one workgroup: part[0:nparts] -> its exclusive prefix sum; the sum goes to *total and, if given, *total2
__global__ __launch_bounds__(1024) void ppd_parts_scan_kernel(int32_t* part, int nparts, int32_t* total,
                                                              int32_t* total2) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  int all;
  const int before = ppd_scan1024(t < nparts ? part[t] : 0, s_wave, &all);
  if (t < nparts) part[t] = before;
  if (t == 0) {
    *total = all;
    if (total2) *total2 = all;
  }
}

// scan pass 3 over the bitmap of a level: for every set bit the byte of `child` with the bit's index, at the bit's rank.
// D != 0: the level of the leaves -- also the prefix half of the rank table and the origins.
template <int D>
__global__ __launch_bounds__(1024) void ppd_level_emit_kernel(const uint32_t* __restrict__ parent, int nw,
                                                              const uint32_t* __restrict__ child,
                                                              const int32_t* __restrict__ part,
                                                              uint8_t* __restrict__ out, int cap,
                                                              uint32_t* __restrict__ prefix,
                                                              int32_t* __restrict__ origins) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  uint32_t w = i < nw ? parent[i] : 0u;
  int total;
  int at = part[blockIdx.x] + ppd_scan1024(__popc(w), s_wave, &total);
  if (D && i < nw) prefix[i] = (uint32_t)at;
  while (w) {
    const uint32_t bi = 32u * i + __ffs((int)w) - 1;
    w &= w - 1u;
    if (at < cap) {
      out[at] = (uint8_t)((child[bi >> 2] >> (8 * (bi & 3u))) & 0xffu);
      if (D) {
        origins[3 * at] = (int32_t)(ppd_gather<D ? D : 1>(bi) << 5);
        origins[3 * at + 1] = (int32_t)(ppd_gather<D ? D : 1>(bi >> 1) << 5);
        origins[3 * at + 2] = (int32_t)(ppd_gather<D ? D : 1>(bi >> 2) << 5);
      }
    }
    ++at;
  }
}

// neighbour counts, one wave per block: nb_off[b + 1] = occupied cells among the 125 around block b
template <int D>
__global__ __launch_bounds__(256) void ppd_nb_count_kernel(const int32_t* __restrict__ origins,
                                                           const uint32_t* __restrict__ tab,
                                                           const int32_t* __restrict__ meta, int cap,
                                                           int32_t* __restrict__ nb_off) {
  const int n = min(meta[PPD_META_N], cap);
  const int lane = threadIdx.x & 63;
  for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < n; b += gridDim.x * 4) {     // wave-uniform
    const int cx = origins[3 * b] >> 5, cy = origins[3 * b + 1] >> 5, cz = origins[3 * b + 2] >> 5;
    int cnt = 0;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int j = lane + 64 * round;
      const int nx = cx + j / 25 - 2, ny = cy + (j / 5) % 5 - 2, nz = cz + j % 5 - 2;
      bool ok = j < 125 && ((nx | ny | nz) & ~((1 << D) - 1)) == 0;
      if (ok) {
        const uint32_t m = ppd_cell_code<D>(nx, ny, nz);
        ok = (tab[m >> 5] >> (m & 31u)) & 1u;
      }
      cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) nb_off[b + 1] = cnt;
  }
}

// counts -> offsets in place, the same three passes: thread t of workgroup g owns entries (1024 g + t) ipt + [0, ipt)
__global__ __launch_bounds__(1024) void ppd_nb_sums_kernel(const int32_t* __restrict__ nb_off,
                                                           const int32_t* __restrict__ meta, int cap, int ipt,
                                                           int32_t* __restrict__ part) {
  __shared__ int s_wave[16];
  const int n = min(meta[PPD_META_N], cap);
  const int e0 = min((blockIdx.x * 1024 + threadIdx.x) * ipt, n), e1 = min(e0 + ipt, n);
  int sum = 0;
  for (int e = e0; e < e1; ++e) sum += nb_off[e + 1];
  int total;
  ppd_scan1024(sum, s_wave, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void ppd_nb_offsets_kernel(int32_t* nb_off, const int32_t* __restrict__ meta,
                                                              int cap, int ipt, const int32_t* __restrict__ part) {
  __shared__ int s_wave[16];
  const int n = min(meta[PPD_META_N], cap);
  const int e0 = min((blockIdx.x * 1024 + threadIdx.x) * ipt, n), e1 = min(e0 + ipt, n);
  int sum = 0;
  for (int e = e0; e < e1; ++e) sum += nb_off[e + 1];
  int total;
  int run = part[blockIdx.x] + ppd_scan1024(sum, s_wave, &total);
  for (int e = e0; e < e1; ++e) {
    run += nb_off[e + 1];
    nb_off[e + 1] = run;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) nb_off[0] = 0;
}

template <int D>
__global__ __launch_bounds__(256) void ppd_blocks_kernel(const int64_t* __restrict__ skeys, int npts,
                                                         const uint32_t* __restrict__ tab, int32_t* __restrict__ meta,
                                                         int cap, int32_t* __restrict__ pts,
                                                         int32_t* __restrict__ blk_off) {
  const int n = min(meta[PPD_META_N], cap);
  int uniq = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 256) {
    const int64_t key = skeys[i];
    if (i == (size_t)npts - 1) blk_off[n] = npts;
    if (key >> 40) {                     // a rejected point (they sort to the end): the caller raises
      pts[3 * i] = pts[3 * i + 1] = pts[3 * i + 2] = -1;
      continue;
    }
    const int64_t prev = i ? skeys[i - 1] : -1;
    const uint32_t cell = (uint32_t)(key >> 15), low = (uint32_t)key & 0x7fffu;
    pts[3 * i] = (int32_t)((ppd_gather<D>(cell) << 5) | ((low >> 10) & 31u));
    pts[3 * i + 1] = (int32_t)((ppd_gather<D>(cell >> 1) << 5) | ((low >> 5) & 31u));
    pts[3 * i + 2] = (int32_t)((ppd_gather<D>(cell >> 2) << 5) | (low & 31u));
    if (key != prev) ++uniq;
    if (i == 0 || (uint32_t)(prev >> 15) != cell) {
      const int r = ppd_rank<D>(tab, cell);
      if (r < n) blk_off[r] = (int32_t)i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) uniq += __shfl_xor(uniq, o, 64);
  if ((threadIdx.x & 63) == 0 && uniq) atomicAdd(&meta[PPD_META_VOXELS], uniq);
}

// the 125 block steps in the order preprocess._neighbour_lists gives them: by squared length, (dx, dy, dz)
// lexicographic inside a length
struct PpdSteps { int8_t d[125][3]; };
static constexpr PpdSteps ppd_make_steps() {
  PpdSteps s{};
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
static __constant__ PpdSteps ppd_steps = ppd_make_steps();

template <int D>
__global__ __launch_bounds__(256) void ppd_neighbours_kernel(const int32_t* __restrict__ origins,
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
      const int nx = cx + ppd_steps.d[j][0], ny = cy + ppd_steps.d[j][1], nz = cz + ppd_steps.d[j][2];
      ok = ((nx | ny | nz) & ~((1 << D) - 1)) == 0;
      if (ok) {
        const uint32_t m = ppd_cell_code<D>(nx, ny, nz);
        ok = (tab[m >> 5] >> (m & 31u)) & 1u;
        if (ok) idx = ppd_rank<D>(tab, m);
      }
    }
    const unsigned long long mask = __ballot(ok);
    const int pos = at + __popcll(mask & ((1ull << lane) - 1ull));
    if (ok && pos < end) nb_idx[pos] = idx;
    at += __popcll(mask);
  }
}

extern "C" int nvf_pp_keys_deep(const int32_t* pts, int npts, int bits, int64_t* keys, uint32_t* bitmap, int32_t* meta,
                                void* stream) {
  if (!pts || !keys || !bitmap || !meta || npts <= 0 || (bits != 11 && bits != 12)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  const int d = bits - 5;
  hipError_t e = hipMemsetAsync(bitmap, 0, (size_t)ppd_words(d + 1) * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, NVF_PP_META_INTS * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  const int grid = min((npts + 255) / 256, 2048);
  if (d == 6) ppd_keys_kernel<6><<<grid, 256, 0, st>>>(pts, npts, keys, bitmap, meta);
  else ppd_keys_kernel<7><<<grid, 256, 0, st>>>(pts, npts, keys, bitmap, meta);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_tree_deep(const uint32_t* bitmap, int bits, int npts, int32_t* origins, uint32_t* rank_tab,
                                uint8_t* octree_bytes, int32_t* nb_off, uint32_t* work, int32_t* meta, void* stream) {
  if (!bitmap || !origins || !rank_tab || !octree_bytes || !nb_off || !work || !meta || npts <= 0 ||
      (bits != 11 && bits != 12))
    return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  const int d = bits - 5;
  int32_t* part = (int32_t*)(work + PPD_PART_AT);
  // level d + 1 is the caller's bitmap, level d the first half of the rank table, the levels above live in `work`
  auto level = [&](int l) -> const uint32_t* {
    return l == d + 1 ? bitmap : l == d ? rank_tab : work + ppd_work_at(l);
  };
  for (int l = d; l >= 0; --l) {
    const int ndst = ppd_words(l);
    ppd_fold_kernel<<<(ndst + 255) / 256, 256, 0, st>>>(level(l + 1), ppd_words(l + 1), (uint32_t*)level(l), ndst);
    NVF_LAUNCH_CHECK();
  }
  size_t at = 0;
  for (int l = 0; l <= d; ++l) {
    const int nw = ppd_words(l), groups = (nw + 1023) / 1024, cap = ppd_cap(l, npts);
    ppd_level_sums_kernel<<<groups, 1024, 0, st>>>(level(l), nw, part);
    NVF_LAUNCH_CHECK();
    ppd_parts_scan_kernel<<<1, 1024, 0, st>>>(part, groups, &meta[PPD_META_LEVEL + l], l == d ? &meta[PPD_META_N] : nullptr);
    NVF_LAUNCH_CHECK();
    if (l < d)
      ppd_level_emit_kernel<0><<<groups, 1024, 0, st>>>(level(l), nw, level(l + 1), part, octree_bytes + at, cap, nullptr,
                                                        nullptr);
    else if (d == 6)
      ppd_level_emit_kernel<6><<<groups, 1024, 0, st>>>(level(l), nw, level(l + 1), part, octree_bytes + at, cap,
                                                        rank_tab + nw, origins);
    else
      ppd_level_emit_kernel<7><<<groups, 1024, 0, st>>>(level(l), nw, level(l + 1), part, octree_bytes + at, cap,
                                                        rank_tab + nw, origins);
    NVF_LAUNCH_CHECK();
    at += (size_t)cap;
  }
  const int cap = ppd_cap(d, npts);
  const int ipt = (cap + 1024 * PPD_MAX_PARTS - 1) / (1024 * PPD_MAX_PARTS), groups = (cap + 1024 * ipt - 1) / (1024 * ipt);
  const int count_grid = min((cap + 3) / 4, 4096);
  if (d == 6) ppd_nb_count_kernel<6><<<count_grid, 256, 0, st>>>(origins, rank_tab, meta, cap, nb_off);
  else ppd_nb_count_kernel<7><<<count_grid, 256, 0, st>>>(origins, rank_tab, meta, cap, nb_off);
  NVF_LAUNCH_CHECK();
  ppd_nb_sums_kernel<<<groups, 1024, 0, st>>>(nb_off, meta, cap, ipt, part);
  NVF_LAUNCH_CHECK();
  ppd_parts_scan_kernel<<<1, 1024, 0, st>>>(part, groups, &meta[PPD_META_NB], nullptr);
  NVF_LAUNCH_CHECK();
  ppd_nb_offsets_kernel<<<groups, 1024, 0, st>>>(nb_off, meta, cap, ipt, part);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_blocks_deep(const int64_t* sorted_keys, int npts, int bits, const uint32_t* rank_tab,
                                  int32_t* meta, int32_t* pts, int32_t* blk_off, void* stream) {
  if (!sorted_keys || !rank_tab || !meta || !pts || !blk_off || npts <= 0 || (bits != 11 && bits != 12))
    return NVF_EINVAL;
  const int grid = min((npts + 255) / 256, 2048), cap = ppd_cap(bits - 5, npts);
  hipStream_t st = nvf_stream(stream);
  if (bits == 11) ppd_blocks_kernel<6><<<grid, 256, 0, st>>>(sorted_keys, npts, rank_tab, meta, cap, pts, blk_off);
  else ppd_blocks_kernel<7><<<grid, 256, 0, st>>>(sorted_keys, npts, rank_tab, meta, cap, pts, blk_off);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_neighbours_deep(const int32_t* origins, int bits, const uint32_t* rank_tab, const int32_t* nb_off,
                                      int32_t* nb_idx, int nblocks, void* stream) {
  if (!origins || !rank_tab || !nb_off || !nb_idx || nblocks <= 0 || (bits != 11 && bits != 12)) return NVF_EINVAL;
  if (nblocks > 1 << (3 * (bits - 5))) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  if (bits == 11) ppd_neighbours_kernel<6><<<(nblocks + 3) / 4, 256, 0, st>>>(origins, rank_tab, nb_off, nb_idx, nblocks);
  else ppd_neighbours_kernel<7><<<(nblocks + 3) / 4, 256, 0, st>>>(origins, rank_tab, nb_off, nb_idx, nblocks);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
