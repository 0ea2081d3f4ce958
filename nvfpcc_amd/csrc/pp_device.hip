// Pre-processing of a cloud on the device (nvfpcc_amd/preprocess.py: preprocess_device): octree partition, block-sorted
// points, the candidate lists of nvf_nearest_dist2 and the float grids the trainer reads, without a host pass over
// anything that scales with the points or with the voxels.  One implementation for 10, 11 and 12 bits per axis,
// parameterised by the level D = bits - 5 (5, 6 or 7) of the 32^3 leaf blocks.
//
// The reference's child index is [x >= mid] + 2 [y >= mid] + 4 [z >= mid] (get_octree.cpp:354-411), so its traversal
// order of the nodes of a level is ascending Morton code (x in the lowest bit of each level).  A cell code is the
// 3 D-bit Morton code of (x >> 5, y >> 5, z >> 5).  The occupancy of level D + 1 (16^3 cells), indexed by that code, is
// a bitmap whose BYTE i holds the eight children of level-D cell i (32 KiB, 256 KiB or 2 MiB, in global memory); the
// bitmap of level L is "byte != 0" of level L + 1, the breadth-first bytes of level L are the non-zero bytes of the
// bitmap of level L + 1 in index order, the leaf blocks are the set bits of the level-D bitmap and a leaf's block id is
// the number of set bits below it.  Everything is an OR or an integer count: no result depends on an order.
//
// The level-D bitmap has up to 65536 words, so "set bits before each word" is a grid-wide exclusive scan.  Every scan
// here is three launches -- sums per workgroup, one workgroup scans the at most 1024 partial sums, emit -- ordered by
// the stream: no workgroup ever waits for another.  A level has at most min(8^L, points) nodes; buffers are sized so.
//
//   nvf_pp_keys        per point: range check, sort key (cell code << 15 | local voxel: int32 at D = 5, int64 above),
//                      the point's bit in the level-(D + 1) bitmap (tested before the atomic OR: a surface hits the
//                      same few words again and again; at D = 5 through an LDS copy of the bitmap per workgroup)
//   (the caller sorts the keys)
//   nvf_pp_tree        D + 1 fold launches, then per level sums / scan / emit: bytes, origins, the rank table;
//                      neighbour counts, one wave per block, and their prefix sum
//   nvf_pp_blocks      sorted keys -> points, blk_off (each row written by the first point of its block), voxel count
//   nvf_pp_neighbours  one wave per block: the occupied blocks within +-2 steps of the 2^D grid, own block first, then
//                      by distance
//   nvf_pp_grids       dist = sqrtf(d2) (correctly rounded), gt = (d2 == 0)
#include "nvf_common.h"

#define PP_META_N 0
#define PP_META_BAD 1
#define PP_META_LEVEL 2
#define PP_META_NB 10
#define PP_META_VOXELS 11
// work: the bitmaps of levels 0 .. D - 1 from word 0 (at most 9364 words), the partial sums of a scan from PP_PART_AT
#define PP_PART_AT 10240
#define PP_MAX_PARTS 1024
static_assert(PP_PART_AT + PP_MAX_PARTS == NVF_PP_WORK_WORDS, "work layout");

// the sort key: 3 D + 15 bits.  30 fit int32 (torch.sort of int64 costs radix passes the 10-bit cloud need not pay)
template <int D> struct PpKey { typedef int64_t type; static constexpr int64_t bad = 0x7fffffffffffffffll; };
template <> struct PpKey<5> { typedef int32_t type; static constexpr int32_t bad = 0x7fffffff; };

// D bits -> bits 0, 3, 6, ... and back
template <int D>
__device__ __forceinline__ uint32_t pp_spread(uint32_t v) {
  uint32_t m = 0u;
#pragma unroll
  for (int b = 0; b < D; ++b) m |= ((v >> b) & 1u) << (3 * b);
  return m;
}
template <int D>
__device__ __forceinline__ uint32_t pp_gather(uint32_t m) {
  uint32_t v = 0u;
#pragma unroll
  for (int b = 0; b < D; ++b) v |= ((m >> (3 * b)) & 1u) << b;
  return v;
}
template <int D>
__device__ __forceinline__ uint32_t pp_cell_code(uint32_t cx, uint32_t cy, uint32_t cz) {
  return pp_spread<D>(cx) | (pp_spread<D>(cy) << 1) | (pp_spread<D>(cz) << 2);
}
// block id of an occupied level-D cell: tab[0:W] the level-D bitmap, tab[W:2W] set bits before each word, W = 8^D / 32
template <int D>
__device__ __forceinline__ int pp_rank(const uint32_t* __restrict__ tab, uint32_t cell) {
  constexpr uint32_t W = 1u << (3 * D - 5);
  return (int)tab[W + (cell >> 5)] + __popc(tab[cell >> 5] & ((1u << (cell & 31u)) - 1u));
}
// is the level-D cell (nx, ny, nz) inside the 2^D grid and occupied?  *code = its cell code if so
template <int D>
__device__ __forceinline__ bool pp_occupied(const uint32_t* __restrict__ tab, int nx, int ny, int nz, uint32_t* code) {
  if ((nx | ny | nz) & ~((1 << D) - 1)) return false;
  *code = pp_cell_code<D>(nx, ny, nz);
  return (tab[*code >> 5] >> (*code & 31u)) & 1u;
}

static inline int pp_words(int level) { return level < 2 ? 1 : 1 << (3 * level - 5); }   // of the bitmap of a level
static inline int pp_work_at(int level) {                                                   // its place in `work`
  int at = 0;
  for (int l = 0; l < level; ++l) at += pp_words(l);
  return at;
}
static inline int pp_cap(int level, int npts) {                 // a level has at most min(8^level, points) nodes
  const int64_t full = (int64_t)1 << (3 * level);
  return full < npts ? (int)full : npts;
}

// one point: its sort key and the index of its bit in the level-(D + 1) bitmap; false (and the bad key) if a coordinate
// is negative or >= 2^bits
template <int D>
__device__ __forceinline__ bool pp_point(const int32_t* __restrict__ pts, size_t i, typename PpKey<D>::type* key,
                                         uint32_t* m) {
  typedef typename PpKey<D>::type Key;
  const int x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  *key = PpKey<D>::bad;
  if ((x | y | z) & ~((1 << (D + 5)) - 1)) return false;
  const uint32_t cell = pp_cell_code<D>(x >> 5, y >> 5, z >> 5);
  *key = ((Key)cell << 15) | (Key)(((x & 31) << 10) | ((y & 31) << 5) | (z & 31));
  *m = (cell << 3) | ((x >> 4) & 1) | (((y >> 4) & 1) << 1) | (((z >> 4) & 1) << 2);
  return true;
}
__device__ __forceinline__ void pp_count_bad(int nbad, int32_t* __restrict__ meta) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&meta[PP_META_BAD], nbad);
}

template <int D>
__global__ __launch_bounds__(256) void pp_keys_kernel(const int32_t* __restrict__ pts, int npts,
                                                      typename PpKey<D>::type* __restrict__ keys, uint32_t* bitmap,
                                                      int32_t* __restrict__ meta) {
  int nbad = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 256) {
    uint32_t m;
    const bool ok = pp_point<D>(pts, i, &keys[i], &m);
    nbad += !ok;
    if (!ok) continue;
    const uint32_t bit = 1u << (m & 31u);
    uint32_t* w = bitmap + (m >> 5);
    if (!(*w & bit)) atomicOr(w, bit);   // a stale read costs one OR too many, never a wrong bit
  }
  pp_count_bad(nbad, meta);
}

// D = 5 only: the 32 KiB bitmap fits LDS, so the points of a workgroup meet in an LDS copy that is flushed with one
// global OR per non-zero word.  Kept because it was measured (pre-processing, *Measured*): in the kernel above
// the atomics of a surface's points queue on the few words they all hit.
#define PP_B6_WORDS 8192
__global__ __launch_bounds__(1024) void pp_keys_lds_kernel(const int32_t* __restrict__ pts, int npts,
                                                           int32_t* __restrict__ keys, uint32_t* __restrict__ bitmap,
                                                           int32_t* __restrict__ meta) {
  __shared__ uint32_t s_bits[PP_B6_WORDS];
  for (int i = threadIdx.x; i < PP_B6_WORDS; i += 1024) s_bits[i] = 0u;
  __syncthreads();
  int nbad = 0;
  for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 1024) {
    uint32_t m;
    const bool ok = pp_point<5>(pts, i, &keys[i], &m);
    nbad += !ok;
    if (!ok) continue;
    const uint32_t bit = 1u << (m & 31u);
    if (!(s_bits[m >> 5] & bit)) atomicOr(&s_bits[m >> 5], bit);       // surfaces hit the same few words: test first
  }
  pp_count_bad(nbad, meta);
  __syncthreads();
  for (int i = threadIdx.x; i < PP_B6_WORDS; i += 1024) {
    const uint32_t v = s_bits[i];
    if (v) atomicOr(&bitmap[i], v);
  }
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

// word t of the bitmap one level up: bit 4k + j = byte j of src[8t + k] is non-zero
__global__ __launch_bounds__(256) void pp_fold_kernel(const uint32_t* __restrict__ src, int nsrc,
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
__global__ __launch_bounds__(1024) void pp_level_sums_kernel(const uint32_t* __restrict__ bm, int nw,
                                                             int32_t* __restrict__ part) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  int total;
  pp_scan1024(i < nw ? __popc(bm[i]) : 0, s_wave, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// scan pass 2, one workgroup: part[0:nparts] -> its exclusive prefix sum; the sum goes to *total and, if given, *total2
__global__ __launch_bounds__(1024) void pp_parts_scan_kernel(int32_t* part, int nparts, int32_t* total,
                                                             int32_t* total2) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  int all;
  const int before = pp_scan1024(t < nparts ? part[t] : 0, s_wave, &all);
  if (t < nparts) part[t] = before;
  if (t == 0) {
    *total = all;
    if (total2) *total2 = all;
  }
}

// scan pass 3 over the bitmap of a level: for every set bit the byte of `child` with the bit's index, at the bit's rank.
// LEAF_D != 0: the level of the leaves -- also the prefix half of the rank table and the origins.
template <int LEAF_D>
__global__ __launch_bounds__(1024) void pp_level_emit_kernel(const uint32_t* __restrict__ parent, int nw,
                                                             const uint32_t* __restrict__ child,
                                                             const int32_t* __restrict__ part,
                                                             uint8_t* __restrict__ out, int cap,
                                                             uint32_t* __restrict__ prefix,
                                                             int32_t* __restrict__ origins) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  uint32_t w = i < nw ? parent[i] : 0u;
  int total;
  int at = part[blockIdx.x] + pp_scan1024(__popc(w), s_wave, &total);
  if (LEAF_D && i < nw) prefix[i] = (uint32_t)at;
  while (w) {
    const uint32_t bi = 32u * i + __ffs((int)w) - 1;
    w &= w - 1u;
    if (at < cap) {
      out[at] = (uint8_t)((child[bi >> 2] >> (8 * (bi & 3u))) & 0xffu);
      if constexpr (LEAF_D != 0) {
        origins[3 * at] = (int32_t)(pp_gather<LEAF_D>(bi) << 5);
        origins[3 * at + 1] = (int32_t)(pp_gather<LEAF_D>(bi >> 1) << 5);
        origins[3 * at + 2] = (int32_t)(pp_gather<LEAF_D>(bi >> 2) << 5);
      }
    }
    ++at;
  }
}

// neighbour counts, one wave per block: nb_off[b + 1] = occupied cells among the 125 around block b
template <int D>
__global__ __launch_bounds__(256) void pp_nb_count_kernel(const int32_t* __restrict__ origins,
                                                          const uint32_t* __restrict__ tab,
                                                          const int32_t* __restrict__ meta, int cap,
                                                          int32_t* __restrict__ nb_off) {
  const int n = min(meta[PP_META_N], cap);
  const int lane = threadIdx.x & 63;
  for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < n; b += gridDim.x * 4) {     // wave-uniform
    const int cx = origins[3 * b] >> 5, cy = origins[3 * b + 1] >> 5, cz = origins[3 * b + 2] >> 5;
    int cnt = 0;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int j = lane + 64 * round;
      uint32_t m;
      const bool ok = j < 125 && pp_occupied<D>(tab, cx + j / 25 - 2, cy + (j / 5) % 5 - 2, cz + j % 5 - 2, &m);
      cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) nb_off[b + 1] = cnt;
  }
}

// counts -> offsets in place, scan passes 1 (EMIT = false: part[g] = the sum of workgroup g's counts) and 3; thread t
// of workgroup g owns entries (1024 g + t) ipt + [0, ipt)
template <bool EMIT>
__global__ __launch_bounds__(1024) void pp_nb_scan_kernel(int32_t* nb_off, const int32_t* __restrict__ meta, int cap,
                                                          int ipt, int32_t* part) {
  __shared__ int s_wave[16];
  const int n = min(meta[PP_META_N], cap);
  const int e0 = min((blockIdx.x * 1024 + threadIdx.x) * ipt, n), e1 = min(e0 + ipt, n);
  int sum = 0;
  for (int e = e0; e < e1; ++e) sum += nb_off[e + 1];
  int total;
  int run = pp_scan1024(sum, s_wave, &total);
  if (!EMIT) {
    if (threadIdx.x == 0) part[blockIdx.x] = total;
    return;
  }
  run += part[blockIdx.x];
  for (int e = e0; e < e1; ++e) {
    run += nb_off[e + 1];
    nb_off[e + 1] = run;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) nb_off[0] = 0;
}

template <int D>
__global__ __launch_bounds__(256) void pp_blocks_kernel(const typename PpKey<D>::type* __restrict__ skeys, int npts,
                                                        const uint32_t* __restrict__ tab, int32_t* __restrict__ meta,
                                                        int cap, int32_t* __restrict__ pts,
                                                        int32_t* __restrict__ blk_off) {
  typedef typename PpKey<D>::type Key;
  const int n = min(meta[PP_META_N], cap);
  int uniq = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)npts; i += (size_t)gridDim.x * 256) {
    const Key key = skeys[i];
    if (i == (size_t)npts - 1) blk_off[n] = npts;
    if (key == PpKey<D>::bad) {          // a rejected point (they sort to the end): the caller raises
      pts[3 * i] = pts[3 * i + 1] = pts[3 * i + 2] = -1;
      continue;
    }
    const Key prev = i ? skeys[i - 1] : (Key)-1;
    const uint32_t cell = (uint32_t)(key >> 15), low = (uint32_t)key & 0x7fffu;
    pts[3 * i] = (int32_t)((pp_gather<D>(cell) << 5) | ((low >> 10) & 31u));
    pts[3 * i + 1] = (int32_t)((pp_gather<D>(cell >> 1) << 5) | ((low >> 5) & 31u));
    pts[3 * i + 2] = (int32_t)((pp_gather<D>(cell >> 2) << 5) | (low & 31u));
    if (key != prev) ++uniq;
    if (i == 0 || (uint32_t)(prev >> 15) != cell) {
      const int r = pp_rank<D>(tab, cell);
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

template <int D>
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
    uint32_t m;
    const bool ok = j < 125 && pp_occupied<D>(tab, cx + pp_steps.d[j][0], cy + pp_steps.d[j][1], cz + pp_steps.d[j][2], &m);
    const int idx = ok ? pp_rank<D>(tab, m) : 0;
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

// the host side of an entry point is a function template of D; the entry point checks its arguments and picks D
#define PP_DISPATCH(bits, fn, ...)            \
  switch (bits) {                             \
    case 10: return fn<5>(__VA_ARGS__);       \
    case 11: return fn<6>(__VA_ARGS__);       \
    case 12: return fn<7>(__VA_ARGS__);       \
    default: return NVF_EINVAL;               \
  }

template <int D>
static int pp_keys(const int32_t* pts, int npts, void* keys, uint32_t* bitmap, int32_t* meta, hipStream_t st) {
  hipError_t e = hipMemsetAsync(bitmap, 0, (size_t)pp_words(D + 1) * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(meta, 0, NVF_PP_META_INTS * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  if constexpr (D == 5)
    pp_keys_lds_kernel<<<min((npts + 1023) / 1024, 256), 1024, 0, st>>>(pts, npts, (int32_t*)keys, bitmap, meta);
  else
    pp_keys_kernel<D><<<min((npts + 255) / 256, 2048), 256, 0, st>>>(pts, npts, (typename PpKey<D>::type*)keys, bitmap, meta);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_keys(const int32_t* pts, int npts, int bits, void* keys, uint32_t* bitmap, int32_t* meta,
                           void* stream) {
  if (!pts || !keys || !bitmap || !meta || npts <= 0) return NVF_EINVAL;
  PP_DISPATCH(bits, pp_keys, pts, npts, keys, bitmap, meta, nvf_stream(stream));
}

template <int D>
static int pp_tree(const uint32_t* bitmap, int npts, int32_t* origins, uint32_t* rank_tab, uint8_t* octree_bytes,
                   int32_t* nb_off, uint32_t* work, int32_t* meta, hipStream_t st) {
  int32_t* part = (int32_t*)(work + PP_PART_AT);
  // level D + 1 is the caller's bitmap, level D the first half of the rank table, the levels above live in `work`
  auto level = [&](int l) -> const uint32_t* {
    return l == D + 1 ? bitmap : l == D ? rank_tab : work + pp_work_at(l);
  };
  for (int l = D; l >= 0; --l) {
    const int ndst = pp_words(l);
    pp_fold_kernel<<<(ndst + 255) / 256, 256, 0, st>>>(level(l + 1), pp_words(l + 1), (uint32_t*)level(l), ndst);
    NVF_LAUNCH_CHECK();
  }
  size_t at = 0;
  for (int l = 0; l <= D; ++l) {
    const int nw = pp_words(l), groups = (nw + 1023) / 1024, cap = pp_cap(l, npts);
    pp_level_sums_kernel<<<groups, 1024, 0, st>>>(level(l), nw, part);
    NVF_LAUNCH_CHECK();
    pp_parts_scan_kernel<<<1, 1024, 0, st>>>(part, groups, &meta[PP_META_LEVEL + l], l == D ? &meta[PP_META_N] : nullptr);
    NVF_LAUNCH_CHECK();
    if (l < D)
      pp_level_emit_kernel<0><<<groups, 1024, 0, st>>>(level(l), nw, level(l + 1), part, octree_bytes + at, cap, nullptr,
                                                       nullptr);
    else
      pp_level_emit_kernel<D><<<groups, 1024, 0, st>>>(level(l), nw, level(l + 1), part, octree_bytes + at, cap,
                                                       rank_tab + nw, origins);
    NVF_LAUNCH_CHECK();
    at += (size_t)cap;
  }
  const int cap = pp_cap(D, npts);
  const int ipt = (cap + 1024 * PP_MAX_PARTS - 1) / (1024 * PP_MAX_PARTS), groups = (cap + 1024 * ipt - 1) / (1024 * ipt);
  pp_nb_count_kernel<D><<<min((cap + 3) / 4, 4096), 256, 0, st>>>(origins, rank_tab, meta, cap, nb_off);
  NVF_LAUNCH_CHECK();
  pp_nb_scan_kernel<false><<<groups, 1024, 0, st>>>(nb_off, meta, cap, ipt, part);
  NVF_LAUNCH_CHECK();
  pp_parts_scan_kernel<<<1, 1024, 0, st>>>(part, groups, &meta[PP_META_NB], nullptr);
  NVF_LAUNCH_CHECK();
  pp_nb_scan_kernel<true><<<groups, 1024, 0, st>>>(nb_off, meta, cap, ipt, part);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_tree(const uint32_t* bitmap, int bits, int npts, int32_t* origins, uint32_t* rank_tab,
                           uint8_t* octree_bytes, int32_t* nb_off, uint32_t* work, int32_t* meta, void* stream) {
  if (!bitmap || !origins || !rank_tab || !octree_bytes || !nb_off || !work || !meta || npts <= 0) return NVF_EINVAL;
  PP_DISPATCH(bits, pp_tree, bitmap, npts, origins, rank_tab, octree_bytes, nb_off, work, meta, nvf_stream(stream));
}

template <int D>
static int pp_blocks(const void* sorted_keys, int npts, const uint32_t* rank_tab, int32_t* meta, int32_t* pts,
                     int32_t* blk_off, hipStream_t st) {
  pp_blocks_kernel<D><<<min((npts + 255) / 256, 2048), 256, 0, st>>>((const typename PpKey<D>::type*)sorted_keys, npts,
                                                                     rank_tab, meta, pp_cap(D, npts), pts, blk_off);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_blocks(const void* sorted_keys, int npts, int bits, const uint32_t* rank_tab, int32_t* meta,
                             int32_t* pts, int32_t* blk_off, void* stream) {
  if (!sorted_keys || !rank_tab || !meta || !pts || !blk_off || npts <= 0) return NVF_EINVAL;
  PP_DISPATCH(bits, pp_blocks, sorted_keys, npts, rank_tab, meta, pts, blk_off, nvf_stream(stream));
}

template <int D>
static int pp_neighbours(const int32_t* origins, const uint32_t* rank_tab, const int32_t* nb_off, int32_t* nb_idx,
                         int nblocks, hipStream_t st) {
  if (nblocks > 1 << (3 * D)) return NVF_EINVAL;
  pp_neighbours_kernel<D><<<(nblocks + 3) / 4, 256, 0, st>>>(origins, rank_tab, nb_off, nb_idx, nblocks);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pp_neighbours(const int32_t* origins, int bits, const uint32_t* rank_tab, const int32_t* nb_off,
                                 int32_t* nb_idx, int nblocks, void* stream) {
  if (!origins || !rank_tab || !nb_off || !nb_idx || nblocks <= 0) return NVF_EINVAL;
  PP_DISPATCH(bits, pp_neighbours, origins, rank_tab, nb_off, nb_idx, nblocks, nvf_stream(stream));
}

extern "C" int nvf_pp_grids(const int32_t* d2, float* dist, float* gt, int64_t n, void* stream) {
  if (!d2 || !dist || !gt || n <= 0) return NVF_EINVAL;
  if (((uintptr_t)d2 | (uintptr_t)dist | (uintptr_t)gt) & 15) return NVF_EINVAL;
  const int grid = (int)min((int64_t)2048, ((n >> 2) + 255) / 256 + 1);
  pp_grids_kernel<<<grid, 256, 0, nvf_stream(stream)>>>(d2, dist, gt, (size_t)n);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
