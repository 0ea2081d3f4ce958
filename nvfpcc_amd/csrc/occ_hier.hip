// Scalable lossless geometry: the occupancy of every leaf block coded coarse to fine (nvfpcc_amd/lossless_lod_pack.py;
// include/nvf_hip.h, "scalable lossless geometry", is the contract).  A block's 8^3 max-pool is coded first, then the
// 16^3 cells under occupied 8^3 cells, then the voxels under occupied 16^3 cells: everything under an empty parent is
// known, and a decoder that stops after the first or second section holds the exact max-pooled occupancy.
//
//   nvf_occ_hier_pyramid   p -> P1, K1, P2, K2 (the maxima and the clipped counts of the eight children above 0.5), the
//                          input errors over ALL voxels, and with gt the ground truth's occupancy words of the three levels
//   nvf_occ_hier_cells     occupancy words of a level -> set bits per block and the list of occupied cells in (block,
//                          raster) order, entry = block * cells per block + cell
//   nvf_occ_hier_hist      per context the coded symbols of one level and the occupied ones, exact integers
//   nvf_occ_hier_encode    one 64-lane wave per group: sections 0, 1, 2, each backwards, ONE stream
//   nvf_occ_hier_decode    one section per launch, states and word position in and out; a cell-list launch in between
//   nvf_occ_nbr_hist / _encode / _decode   the second context model: a voxel is coded under the 16^3 occupancy of its
//                          parent's neighbours as well (NBR below).  Sections 2 and 1 are the first model's
//
// Symbol i of a section belongs to lane i % 64 at step i / 64; a lane past the section's end is idle: it neither codes
// nor renormalises.  Frequencies depend on the pyramid alone, so a wave fetches OCC_AHEAD steps before it enters the
// serial chain, as occ_rans.hip does; the gathers of a parent's eight children are four rows of two adjacent floats.
// The chain itself -- the step with its idle lanes, the word window, the status -- and the walk behind the cell lists
// are occ_coder.h's.
//
// NBR: the level-0 contexts grow by the class n in [0, 32) of the parent's seven neighbours on the voxel's side, read
// from the block's own 64 level-1 words: the ground truth's at the encoder, the ones section 1 left at the decoder, so
// they are known before the first voxel and are gathered with the probabilities, HIER_AHEAD steps before the chain.
// A row of 16 cells along x is one uint16 of those words, so a voxel gathers four rows: (Z, Y), (Z + sz, Y), (Z, Y + sy),
// (Z + sz, Y + sy).  The 32 x 1024 level-0 frequencies sit in LDS as uint16 (64 KiB; a frequency is in [1, 65535]) next
// to the 3072 uint32 entries the other two sections use; the histogram counts a block in ONE uint32 per context, symbols
// in the low half and occupied ones in the high half (128 KiB): a block codes at most 32768 voxels, so neither half
// can carry.
//
//   nvf_occ_ref_words      a reference cloud rasterised onto this frame's blocks: one thread per point, a binary search
//                          of its block among the sorted origin keys, an integer OR of one bit
//   nvf_occ_inter_hist / _encode / _decode   the third context model (INTER below).  Sections 2 and 1 are the first model's
//
// INTER: the level-0 contexts are t = r * 16 + s in [0, 48): r in {0, 1, 2} from the reference words R of the SAME block
// (2: the voxel itself is in the reference, 1: a face neighbour of it is, 0: neither), s in [0, 16) the neighbour class
// with the edge count folded to a bit, (F * 2 + (E > 0)) * 2 + C.  R is read as uint32 rows of 32 voxels along x, five
// per voxel: its own, z - 1, z + 1, y - 1, y + 1 (a row outside the block is empty), gathered with the probabilities
// ahead of the chain.  The 48 x 1024 level-0 frequencies sit in LDS as uint16 (96 KiB) next to the 12 KiB of the other
// sections; the histogram runs one workgroup per (block, r) over the block's symbols and counts those of its r in one
// uint32 per context (16384 of them, 64 KiB), as NBR does.
#include "occ_coder.h"

#define HIER_CTX 3072                                  // 3 levels x 4 child counts x 256
#define NBR_CTX0 32768                                 // 32 neighbour classes x 4 child counts x 256, from context 3072 on
#define INTER_CTX0 49152                               // 3 temporal x 16 spatial classes x 4 child counts x 256
#define INTER_CTX_R 16384                              // the level-0 contexts of one temporal class
#define HIER_AHEAD 8
#define HIER_BLOCK_WORDS NVF_OCC_HIER_BLOCK_WORDS      // 512 + 4096 + 32768: an all-full block
#define HIER_THREADS 1024

namespace {

// the context model of a level-0 symbol: the field alone, with the parent's neighbours, with a reference cloud as well
enum HierCtx { CTX_FIELD = 0, CTX_NBR = 1, CTX_INTER = 2 };

__device__ __forceinline__ int hier_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of c[lo .. hi), the same value in every lane of the wave
__device__ __forceinline__ int hier_sum(const int32_t* __restrict__ c, int lo, int hi, int lane) {
  int s = 0;
  for (int i = lo + lane; i < hi; i += 64) s += c[i];
  return hier_wave_sum(s);
}

// symbol i of a section -> the cell whose value and occupancy bit it codes (index into the level's [batch, cells]
// arrays) and the cell whose K gives its child count.  parents: the group's (or block's) occupied cells of the level
// above; b0: the first block of the section (level 2 only, dense raster).
template <int LEVEL>
__device__ __forceinline__ void hier_where(int i, const int32_t* __restrict__ parents, int b0, int& cell, int& kcell) {
  if constexpr (LEVEL == 2) {
    cell = kcell = b0 * 512 + i;
  } else {
    const int e = parents[i >> 3], j = i & 7;
    const int dz = j >> 2, dy = (j >> 1) & 1, dx = j & 1;
    if constexpr (LEVEL == 1) {
      const int b = e >> 9, c = e & 511;
      const int z = 2 * (c >> 6) + dz, y = 2 * ((c >> 3) & 7) + dy, x = 2 * (c & 7) + dx;
      cell = kcell = b * 4096 + (z * 16 + y) * 16 + x;
    } else {
      const int b = e >> 12, c = e & 4095;
      const int z = 2 * (c >> 8) + dz, y = 2 * ((c >> 4) & 15) + dy, x = 2 * (c & 15) + dx;
      cell = b * 32768 + (z * 32 + y) * 32 + x;
      kcell = e;
    }
  }
}

__device__ __forceinline__ int hier_ctx(int level, int k, float v) { return (level * 4 + (k & 3)) * OCC_CTX + occ_ctx(v); }

// the four rows of 16^3 cells a voxel's neighbour class is read from; a row outside the block is empty
struct NbrRows {
  uint32_t r00, r10, r01, r11;
};

__device__ __forceinline__ uint32_t nbr_row(const uint16_t* __restrict__ rows, int b, int Z, int Y) {
  const bool in = (unsigned)Z < 16u && (unsigned)Y < 16u;
  const uint32_t r = rows[(size_t)b * 256 + (in ? Z * 16 + Y : 0)];
  return in ? r : 0u;
}

// e = block * 4096 + parent cell (hier_where's kcell at level 0), j = the voxel's child index: its odd coordinates
__device__ __forceinline__ NbrRows nbr_gather(const uint16_t* __restrict__ rows, int e, int j) {
  const int b = e >> 12, Z = (e >> 8) & 15, Y = (e >> 4) & 15;
  const int Zs = Z + ((j & 4) ? 1 : -1), Ys = Y + ((j & 2) ? 1 : -1);
  return NbrRows{nbr_row(rows, b, Z, Y), nbr_row(rows, b, Zs, Y), nbr_row(rows, b, Z, Ys), nbr_row(rows, b, Zs, Ys)};
}

// n = (F * 4 + E) * 2 + C: the occupied face, edge and corner neighbours
__device__ __forceinline__ int nbr_class(const NbrRows& r, int e, int j) {
  const int X = e & 15, Xs = X + ((j & 1) ? 1 : -1);
  const uint32_t in = (unsigned)Xs < 16u ? 1u : 0u;
  const int xs = Xs & 15;
  const uint32_t F = ((r.r10 >> X) & 1u) + ((r.r01 >> X) & 1u) + ((r.r00 >> xs) & in);
  const uint32_t E = ((r.r11 >> X) & 1u) + ((r.r10 >> xs) & in) + ((r.r01 >> xs) & in);
  return (int)((F * 4u + E) * 2u + ((r.r11 >> xs) & in));
}

// the five rows of 32 reference voxels a voxel's temporal class is read from; a row outside the block is empty
struct InterRows {
  uint32_t own, zm, zp, ym, yp;
};

__device__ __forceinline__ uint32_t inter_row(const uint32_t* __restrict__ ref, int b, int z, int y) {
  const bool in = (unsigned)z < 32u && (unsigned)y < 32u;
  const uint32_t r = ref[(size_t)b * 1024 + (in ? z * 32 + y : 0)];
  return in ? r : 0u;
}

// cell = block * 32768 + voxel (hier_where's cell at level 0)
__device__ __forceinline__ InterRows inter_gather(const uint32_t* __restrict__ ref, int cell) {
  const int b = cell >> 15, z = (cell >> 10) & 31, y = (cell >> 5) & 31;
  return InterRows{inter_row(ref, b, z, y), inter_row(ref, b, z - 1, y), inter_row(ref, b, z + 1, y),
                   inter_row(ref, b, z, y - 1), inter_row(ref, b, z, y + 1)};
}

// r = 2: the voxel is in the reference; 1: one of its six face neighbours is; 0: neither.  x = the voxel's x
__device__ __forceinline__ int inter_temporal(const InterRows& q, int x) {
  const unsigned long long o = q.own;                  // 64 bits: x - 1 = -1 and x + 1 = 32 read zeros
  const unsigned long long faces = ((unsigned long long)(q.zm | q.zp | q.ym | q.yp) | (o >> 1) | (o << 1)) >> x;
  return ((q.own >> x) & 1u) ? 2 : (int)(faces & 1ull);
}

// t = r * 16 + s, s = (F * 2 + (E > 0)) * 2 + C: the neighbour class n = F << 3 | E << 1 | C with E folded to a bit
__device__ __forceinline__ int inter_class(const InterRows& q, const NbrRows& r, int e, int j, int x) {
  const int n = nbr_class(r, e, j);
  return inter_temporal(q, x) * 16 + ((n >> 3) * 2 + ((n & 6) ? 1 : 0)) * 2 + (n & 1);
}

// index into the level-0 frequencies: context - 3072
__device__ __forceinline__ int nbr_ctx0(int n, int k, float v) { return (n * 4 + (k & 3)) * OCC_CTX + occ_ctx(v); }

// the N (NBR_CTX0 or INTER_CTX0) level-0 frequencies f0 (16-byte aligned) as uint16 in LDS, pulled into [1, 65535].
// One wave.
template <int N = NBR_CTX0>
__device__ __forceinline__ void nbr_load_table(const int32_t* __restrict__ f0, uint16_t* tab0, int lane) {
  const auto pull = [](int v) { return (uint32_t)(v < 1 ? 1 : (v > 65535 ? 65535 : v)); };
#pragma unroll 8
  for (int i = lane * 4; i < N; i += 256) {
    const int4 v = *(const int4*)(f0 + i);
    *(uint2*)(tab0 + i) = make_uint2(pull(v.x) | (pull(v.y) << 16), pull(v.z) | (pull(v.w) << 16));
  }
  __syncthreads();
}

// m = c0; m = cj > m ? cj : m in child order: exact comparisons, the first of equal values (and of +-0) stays
__device__ __forceinline__ void hier_fold(float c, float& m, int& k) {
  m = c > m ? c : m;
  k += c > 0.5f ? 1 : 0;
}

// one workgroup per block.  A: the input errors and the occupancy words of gt; B: the 16^3 level from p; C: the 8^3
// level from P1 in LDS.  The coarse occupancy words come from the finer ones in LDS: a cell is occupied when a child is.
__global__ __launch_bounds__(HIER_THREADS) void hier_pyramid_kernel(const float* __restrict__ p, const float* __restrict__ gt,
                                                                    float* __restrict__ p1, uint8_t* __restrict__ k1,
                                                                    float* __restrict__ p2, uint8_t* __restrict__ k2,
                                                                    unsigned long long* __restrict__ bad,
                                                                    unsigned long long* __restrict__ w0,
                                                                    unsigned long long* __restrict__ w1,
                                                                    unsigned long long* __restrict__ w2) {
  __shared__ unsigned long long w0s[512];
  __shared__ unsigned long long w1s[64];
  __shared__ float p1s[4096];
  __shared__ uint32_t nbad_s;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const float* pb = p + (size_t)b * 32768;
  if (tid == 0) nbad_s = 0;
  __syncthreads();
  uint32_t nbad = 0;
  for (int it = 0; it < 32; ++it) {
    const int v = it * HIER_THREADS + tid;
    nbad += occ_bad(pb[v]) ? 1u : 0u;
    if (gt) {
      const unsigned long long word = __ballot(gt[(size_t)b * 32768 + v] != 0.f);
      if (lane == 0) {
        w0s[v >> 6] = word;
        w0[(size_t)b * 512 + (v >> 6)] = word;
      }
    }
  }
  nbad = (uint32_t)hier_wave_sum((int)nbad);
  if (lane == 0 && nbad) atomicAdd(&nbad_s, nbad);
  __syncthreads();
  if (tid == 0 && nbad_s) atomicAdd(bad, (unsigned long long)nbad_s);
  for (int it = 0; it < 4; ++it) {
    const int c = it * HIER_THREADS + tid;
    const int Z = c >> 8, Y = (c >> 4) & 15, X = c & 15;
    float m = 0.f;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                     // four rows of two adjacent floats, in child order
      const float2 v = *(const float2*)(pb + ((2 * Z + (r >> 1)) * 32 + 2 * Y + (r & 1)) * 32 + 2 * X);
      if (r == 0) { m = v.x; k = v.x > 0.5f ? 1 : 0; } else hier_fold(v.x, m, k);
      hier_fold(v.y, m, k);
    }
    p1s[c] = m;
    p1[(size_t)b * 4096 + c] = m;
    k1[(size_t)b * 4096 + c] = (uint8_t)(k > 3 ? 3 : k);
    if (gt) {
      const unsigned long long two = w0s[(2 * Z) * 16 + Y] | w0s[(2 * Z + 1) * 16 + Y];
      const unsigned long long word = __ballot((((two >> (2 * X)) | (two >> (32 + 2 * X))) & 3ull) != 0ull);
      if (lane == 0) {
        w1s[c >> 6] = word;
        w1[(size_t)b * 64 + (c >> 6)] = word;
      }
    }
  }
  __syncthreads();
  if (tid < 512) {                                     // waves 0..7, whole
    const int c = tid;
    const int Z = c >> 6, Y = (c >> 3) & 7, X = c & 7;
    float m = 0.f;
    int k = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = p1s[((2 * Z + (j >> 2)) * 16 + 2 * Y + ((j >> 1) & 1)) * 16 + 2 * X + (j & 1)];
      if (j == 0) { m = v; k = v > 0.5f ? 1 : 0; } else hier_fold(v, m, k);
    }
    p2[(size_t)b * 512 + c] = m;
    k2[(size_t)b * 512 + c] = (uint8_t)(k > 3 ? 3 : k);
    if (gt) {
      const unsigned long long two = w1s[(2 * Z) * 4 + (Y >> 1)] | w1s[(2 * Z + 1) * 4 + (Y >> 1)];
      const int sh = 32 * (Y & 1) + 2 * X;
      const unsigned long long word = __ballot((((two >> sh) | (two >> (sh + 16))) & 3ull) != 0ull);
      if (lane == 0) w2[(size_t)b * 8 + (c >> 6)] = word;
    }
  }
}

// one wave per block, four blocks per workgroup
__global__ __launch_bounds__(256) void hier_count_kernel(const unsigned long long* __restrict__ words, int batch, int wpb,
                                                         int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;
  int n = 0;
  for (int w = lane; w < wpb; w += 64) n += __popcll(words[(size_t)b * wpb + w]);
  n = hier_wave_sum(n);
  if (lane == 0) counts[b] = n;
}

// occ_walk_bits with the cell list as its sink; a block's slots start at the set bits of the blocks before it, so every
// slot is below the set bits of the call, and the list holds batch * wpb * 64 entries
__global__ __launch_bounds__(256) void hier_cells_kernel(const unsigned long long* __restrict__ words, int batch, int wpb,
                                                         const int32_t* __restrict__ counts, int32_t* __restrict__ cells) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;
  occ_walk_bits(words, b, wpb, hier_sum(counts, 0, b, lane), lane,
                [=](int slot, int cell) { cells[slot] = b * (wpb * 64) + cell; });
}

// one workgroup per block over the block's coded symbols of the level
template <int LEVEL>
__global__ __launch_bounds__(HIER_THREADS) void hier_hist_kernel(const float* __restrict__ pv, const uint8_t* __restrict__ kv,
                                                                 const unsigned long long* __restrict__ gw,
                                                                 const int32_t* __restrict__ cells,
                                                                 const int32_t* __restrict__ counts,
                                                                 unsigned long long* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ occ) {
  __shared__ uint32_t h_cnt[4 * OCC_CTX];              // the level's own 1024 contexts
  __shared__ uint32_t h_occ[4 * OCC_CTX];
  const int tid = threadIdx.x, b = blockIdx.x;
  h_cnt[tid] = 0;
  h_occ[tid] = 0;
  __syncthreads();
  int n = 512;
  const int32_t* parents = nullptr;
  if constexpr (LEVEL < 2) {
    parents = cells + hier_sum(counts, 0, b, tid & 63);
    n = 8 * counts[b];
  }
  for (int i = tid; i < n; i += HIER_THREADS) {
    int cell, kcell;
    hier_where<LEVEL>(i, parents, b, cell, kcell);
    const int c = hier_ctx(0, kv[kcell], pv[cell]);
    atomicAdd(&h_cnt[c], 1u);
    if ((gw[cell >> 6] >> (cell & 63)) & 1ull) atomicAdd(&h_occ[c], 1u);
  }
  __syncthreads();
  // integers: any order of these adds gives the same totals
  if (h_cnt[tid]) atomicAdd(cnt + LEVEL * 4 * OCC_CTX + tid, (unsigned long long)h_cnt[tid]);
  if (h_occ[tid]) atomicAdd(occ + LEVEL * 4 * OCC_CTX + tid, (unsigned long long)h_occ[tid]);
}

// the level-0 symbols of one block under the neighbour contexts: one workgroup per block, one uint32 per context
__global__ __launch_bounds__(HIER_THREADS) void nbr_hist_kernel(const float* __restrict__ p, const uint8_t* __restrict__ k1,
                                                                const unsigned long long* __restrict__ w0,
                                                                const uint16_t* __restrict__ rows,
                                                                const int32_t* __restrict__ cells1,
                                                                const int32_t* __restrict__ counts1,
                                                                unsigned long long* __restrict__ cnt,
                                                                unsigned long long* __restrict__ occ) {
  __shared__ uint32_t h[NBR_CTX0];                     // occupied << 16 | symbols, each <= 32768
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int c = tid; c < NBR_CTX0; c += HIER_THREADS) h[c] = 0;
  __syncthreads();
  const int32_t* parents = cells1 + hier_sum(counts1, 0, b, tid & 63);
  const int n = 8 * counts1[b];
  for (int i = tid; i < n; i += HIER_THREADS) {
    int cell, e;
    hier_where<0>(i, parents, b, cell, e);
    const int c = nbr_ctx0(nbr_class(nbr_gather(rows, e, i & 7), e, i & 7), k1[e], p[cell]);
    atomicAdd(&h[c], 1u + ((uint32_t)((w0[cell >> 6] >> (cell & 63)) & 1ull) << 16));
  }
  __syncthreads();
  // integers: any order of these adds gives the same totals
  for (int c = tid; c < NBR_CTX0; c += HIER_THREADS) {
    const uint32_t v = h[c];
    if (v & 0xFFFFu) atomicAdd(cnt + HIER_CTX + c, (unsigned long long)(v & 0xFFFFu));
    if (v >> 16) atomicAdd(occ + HIER_CTX + c, (unsigned long long)(v >> 16));
  }
}

// one section of a group, backwards.  The words written so far are wg[ptr .. region).  CTX_NBR (level 0 only): the
// frequency comes from tab0 under the neighbour class read from `rows`, the ground truth's level-1 words.  CTX_INTER:
// under the temporal class read from `ref`, the reference words, as well.
template <int LEVEL, HierCtx CTX = CTX_FIELD>
__device__ __forceinline__ void hier_encode_section(int n, const int32_t* __restrict__ parents, int b0,
                                                    const float* __restrict__ pv, const uint8_t* __restrict__ kv,
                                                    const unsigned long long* __restrict__ gw, const uint32_t* tab,
                                                    int lane, unsigned long long& x, int& ptr, uint32_t* __restrict__ wg,
                                                    const uint16_t* __restrict__ rows = nullptr,
                                                    const uint16_t* tab0 = nullptr,
                                                    const uint32_t* __restrict__ ref = nullptr) {
  static_assert(CTX == CTX_FIELD || LEVEL == 0, "only voxels have neighbour contexts");
  constexpr bool NBR = CTX != CTX_FIELD, INTER = CTX == CTX_INTER;
  const int steps = (n + 63) >> 6;
  for (int t0 = (steps + HIER_AHEAD - 1) / HIER_AHEAD * HIER_AHEAD - HIER_AHEAD; t0 >= 0; t0 -= HIER_AHEAD) {
    float val[HIER_AHEAD];
    int kk[HIER_AHEAD], bit[HIER_AHEAD];
    unsigned long long gword[HIER_AHEAD];
    NbrRows nr[NBR ? HIER_AHEAD : 1];
    int ee[NBR ? HIER_AHEAD : 1];
    InterRows ir[INTER ? HIER_AHEAD : 1];
#pragma unroll
    for (int k = 0; k < HIER_AHEAD; ++k) {
      const int i = (t0 + k) * 64 + lane;
      int cell = 0, kcell = 0;
      if (i < n) hier_where<LEVEL>(i, parents, b0, cell, kcell);
      val[k] = pv[cell];
      kk[k] = kv[kcell];
      gword[k] = gw[cell >> 6];
      bit[k] = cell & 63;
      if constexpr (NBR) {
        nr[k] = nbr_gather(rows, kcell, lane & 7);     // i & 7: a step is 64 symbols
        ee[k] = kcell;
      }
      if constexpr (INTER) ir[k] = inter_gather(ref, cell);
    }
    uint32_t fr[HIER_AHEAD], st[HIER_AHEAD];           // fr = 0: an idle lane
#pragma unroll
    for (int k = 0; k < HIER_AHEAD; ++k) {
      uint32_t one;
      if constexpr (INTER) one = tab0[nbr_ctx0(inter_class(ir[k], nr[k], ee[k], lane & 7, bit[k] & 31), kk[k], val[k])];
      else if constexpr (NBR) one = tab0[nbr_ctx0(nbr_class(nr[k], ee[k], lane & 7), kk[k], val[k])];
      else one = tab[hier_ctx(LEVEL, kk[k], val[k])];
      const bool s = (gword[k] >> bit[k]) & 1ull;
      const bool live = (t0 + k) * 64 + lane < n;
      fr[k] = !live ? 0u : (s ? one : 65536u - one);
      st[k] = s ? 0u : one;
    }
#pragma unroll
    for (int k = HIER_AHEAD - 1; k >= 0; --k)
      occ_encode_step<true>(x, fr[k], st[k], ptr, wg, lane);
  }
}

// one wave per group.  CTX_NBR: section 0 under the neighbour contexts, f1 holds NVF_OCC_NBR_CONTEXTS entries;
// CTX_INTER: under the inter contexts, f1 holds NVF_OCC_INTER_CONTEXTS entries and ref the reference words
template <HierCtx CTX>
__global__ __launch_bounds__(64) void hier_encode_kernel(const float* __restrict__ p, const float* __restrict__ p1,
                                                         const uint8_t* __restrict__ k1, const float* __restrict__ p2,
                                                         const uint8_t* __restrict__ k2,
                                                         const unsigned long long* __restrict__ w0,
                                                         const unsigned long long* __restrict__ w1,
                                                         const unsigned long long* __restrict__ w2,
                                                         const int32_t* __restrict__ cells2, const int32_t* __restrict__ counts2,
                                                         const int32_t* __restrict__ cells1, const int32_t* __restrict__ counts1,
                                                         const int32_t* __restrict__ f1, int batch, int G,
                                                         unsigned long long* __restrict__ states, uint32_t* __restrict__ words,
                                                         uint32_t* __restrict__ nwords,
                                                         const uint32_t* __restrict__ ref = nullptr) {
  __shared__ uint32_t tab[HIER_CTX];
  const int lane = threadIdx.x, g = blockIdx.x;
  occ_load_table<HIER_CTX>(f1, tab, lane);
  const uint16_t* tab0 = nullptr;
  if constexpr (CTX != CTX_FIELD) {
    constexpr int N0 = CTX == CTX_INTER ? INTER_CTX0 : NBR_CTX0;
    __shared__ __attribute__((aligned(16))) uint16_t t0[N0];
    nbr_load_table<N0>(f1 + HIER_CTX, t0, lane);
    tab0 = t0;
  }
  const int b0 = g * G, nb = min(G, batch - b0);
  const int region = nb * HIER_BLOCK_WORDS;            // a symbol emits one word at the most
  uint32_t* wg = words + (size_t)g * G * HIER_BLOCK_WORDS;
  unsigned long long x = OCC_RANS_L;
  int ptr = region;
  hier_encode_section<0, CTX>(8 * hier_sum(counts1, b0, b0 + nb, lane), cells1 + hier_sum(counts1, 0, b0, lane), b0, p, k1,
                              w0, tab, lane, x, ptr, wg, (const uint16_t*)w1, tab0, ref);
  hier_encode_section<1>(8 * hier_sum(counts2, b0, b0 + nb, lane), cells2 + hier_sum(counts2, 0, b0, lane), b0, p1, k1, w1,
                         tab, lane, x, ptr, wg);
  hier_encode_section<2>(nb * 512, nullptr, b0, p2, k2, w2, tab, lane, x, ptr, wg);
  states[(size_t)g * 64 + lane] = x;
  if (lane == 0) nwords[g] = (uint32_t)(region - ptr);
}

// one section of a group, forwards: what the decoder kernels below share.  CTX_NBR (level 0 only): the frequency comes
// from tab0 under the neighbour class read from `rows`, the level-1 words section 1 decoded.  CTX_INTER: under the
// temporal class read from `ref`, the reference words, as well.
template <int LEVEL, HierCtx CTX>
__device__ __forceinline__ void hier_decode_group(const float* __restrict__ pv, const uint8_t* __restrict__ kv,
                                                  const int32_t* __restrict__ cells, const int32_t* __restrict__ counts,
                                                  const uint32_t* tab, const uint16_t* tab0,
                                                  const uint16_t* __restrict__ rows,
                                                  unsigned long long* __restrict__ states, long long* __restrict__ pos_io,
                                                  const uint32_t* __restrict__ words,
                                                  const long long* __restrict__ word_off,
                                                  const uint32_t* __restrict__ nwords, long long total_words,
                                                  int batch, int G, unsigned long long* __restrict__ occ_words,
                                                  int32_t* __restrict__ status,
                                                  const uint32_t* __restrict__ ref = nullptr) {
  static_assert(CTX == CTX_FIELD || LEVEL == 0, "only voxels have neighbour contexts");
  constexpr bool NBR = CTX != CTX_FIELD, INTER = CTX == CTX_INTER;
  const int lane = threadIdx.x, g = blockIdx.x;
  const int b0 = g * G, nb = min(G, batch - b0);
  // a stop before level 0 needs only a prefix of the group's words: there the cut alone is no damage
  OccWindow w = occ_window_open(words, word_off[g], (long long)nwords[g], total_words, LEVEL == 0);
  unsigned long long x = states[(size_t)g * 64 + lane];
  w.pos = max(pos_io[g], 0ll);
  int n = nb * 512;
  const int32_t* parents = nullptr;
  if constexpr (LEVEL < 2) {
    n = 8 * hier_sum(counts, b0, b0 + nb, lane);
    parents = cells + hier_sum(counts, 0, b0, lane);
  }
  const int steps = (n + 63) >> 6;
  for (int t0 = 0; t0 < steps; t0 += HIER_AHEAD) {
    float val[HIER_AHEAD];
    int kk[HIER_AHEAD], where[HIER_AHEAD];
    NbrRows nr[NBR ? HIER_AHEAD : 1];
    int ee[NBR ? HIER_AHEAD : 1];
    InterRows ir[INTER ? HIER_AHEAD : 1];
#pragma unroll
    for (int k = 0; k < HIER_AHEAD; ++k) {
      const int i = (t0 + k) * 64 + lane;
      int cell = 0, kcell = 0;
      if (i < n) hier_where<LEVEL>(i, parents, b0, cell, kcell);
      val[k] = pv[cell];
      kk[k] = kv[kcell];
      where[k] = cell;
      if constexpr (NBR) {
        nr[k] = nbr_gather(rows, kcell, lane & 7);     // i & 7: a step is 64 symbols
        ee[k] = kcell;
      }
      if constexpr (INTER) ir[k] = inter_gather(ref, cell);
    }
    uint32_t one[HIER_AHEAD];
#pragma unroll
    for (int k = 0; k < HIER_AHEAD; ++k) {
      if constexpr (INTER) one[k] = tab0[nbr_ctx0(inter_class(ir[k], nr[k], ee[k], lane & 7, where[k] & 31), kk[k], val[k])];
      else if constexpr (NBR) one[k] = tab0[nbr_ctx0(nbr_class(nr[k], ee[k], lane & 7), kk[k], val[k])];
      else one[k] = tab[hier_ctx(LEVEL, kk[k], val[k])];
    }
#pragma unroll
    for (int k = 0; k < HIER_AHEAD; ++k) {
      const bool s = occ_decode_step<true>(x, one[k], (t0 + k) * 64 + lane < n, w, lane);
      if constexpr (LEVEL == 2) {                      // dense raster: the ballot is the word
        const unsigned long long word = __ballot(s);
        if (lane == 0 && t0 + k < steps) occ_words[(size_t)b0 * 8 + t0 + k] = word;
      } else {
        if (s) atomicOr(&occ_words[where[k] >> 6], 1ull << (where[k] & 63));   // integer OR: any order, the same word
      }
    }
  }
  states[(size_t)g * 64 + lane] = x;
  // the final states and the word count are the whole stream's: only level 0 has them behind it
  const int st = occ_window_status(w, x, (long long)nwords[g]) & (LEVEL == 0 ? ~0 : NVF_OCC_RANS_PAST_END);
  if (lane == 0) {
    pos_io[g] = w.pos;
    status[g] |= st;
  }
}

// one section of every group.  states, pos and status carry the coder from one section's launch to the next.
template <int LEVEL>
__global__ __launch_bounds__(64) void hier_decode_kernel(const float* __restrict__ pv, const uint8_t* __restrict__ kv,
                                                         const int32_t* __restrict__ cells, const int32_t* __restrict__ counts,
                                                         const int32_t* __restrict__ f1,
                                                         unsigned long long* __restrict__ states, long long* __restrict__ pos_io,
                                                         const uint32_t* __restrict__ words,
                                                         const long long* __restrict__ word_off,
                                                         const uint32_t* __restrict__ nwords, long long total_words,
                                                         int batch, int G, unsigned long long* __restrict__ occ_words,
                                                         int32_t* __restrict__ status) {
  __shared__ uint32_t tab[HIER_CTX];
  occ_load_table<HIER_CTX>(f1, tab, threadIdx.x);
  hier_decode_group<LEVEL, CTX_FIELD>(pv, kv, cells, counts, tab, nullptr, nullptr, states, pos_io, words, word_off, nwords,
                                  total_words, batch, G, occ_words, status);
}

// section 0 of every group under the neighbour contexts: f0 = the level-0 frequencies, w1 = the decoded level-1 words
__global__ __launch_bounds__(64) void nbr_decode_kernel(const float* __restrict__ p, const uint8_t* __restrict__ k1,
                                                        const int32_t* __restrict__ cells1, const int32_t* __restrict__ counts1,
                                                        const uint16_t* __restrict__ rows, const int32_t* __restrict__ f0,
                                                        unsigned long long* __restrict__ states, long long* __restrict__ pos_io,
                                                        const uint32_t* __restrict__ words,
                                                        const long long* __restrict__ word_off,
                                                        const uint32_t* __restrict__ nwords, long long total_words,
                                                        int batch, int G, unsigned long long* __restrict__ occ_words,
                                                        int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint16_t tab0[NBR_CTX0];
  nbr_load_table(f0, tab0, threadIdx.x);
  hier_decode_group<0, CTX_NBR>(p, k1, cells1, counts1, nullptr, tab0, rows, states, pos_io, words, word_off, nwords,
                                total_words, batch, G, occ_words, status);
}

// section 0 of every group under the inter contexts: nbr_decode_kernel with the reference words
__global__ __launch_bounds__(64) void inter_decode_kernel(const float* __restrict__ p, const uint8_t* __restrict__ k1,
                                                          const int32_t* __restrict__ cells1, const int32_t* __restrict__ counts1,
                                                          const uint16_t* __restrict__ rows, const uint32_t* __restrict__ ref,
                                                          const int32_t* __restrict__ f0,
                                                          unsigned long long* __restrict__ states, long long* __restrict__ pos_io,
                                                          const uint32_t* __restrict__ words,
                                                          const long long* __restrict__ word_off,
                                                          const uint32_t* __restrict__ nwords, long long total_words,
                                                          int batch, int G, unsigned long long* __restrict__ occ_words,
                                                          int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint16_t tab0[INTER_CTX0];
  nbr_load_table<INTER_CTX0>(f0, tab0, threadIdx.x);
  hier_decode_group<0, CTX_INTER>(p, k1, cells1, counts1, nullptr, tab0, rows, states, pos_io, words, word_off, nwords,
                                  total_words, batch, G, occ_words, status, ref);
}

// a reference cloud onto the blocks: one thread per point.  keys: the blocks' origin keys ascending, perm[i] the block
// whose key is keys[i].  A point under no block (or outside the key's range) is counted in dropped[0].
__device__ __forceinline__ long long ref_key(int q0, int q1, int q2) {
  return ((long long)(q0 >> 5) << 42) | ((long long)(q1 >> 5) << 21) | (long long)(q2 >> 5);
}

__global__ __launch_bounds__(256) void ref_words_kernel(const int32_t* __restrict__ pts, long long npts,
                                                        const long long* __restrict__ keys, const int32_t* __restrict__ perm,
                                                        int nblocks, unsigned long long* __restrict__ words,
                                                        unsigned long long* __restrict__ dropped) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool drop = false;
  if (i < npts) {
    const int q0 = pts[3 * i], q1 = pts[3 * i + 1], q2 = pts[3 * i + 2];
    drop = true;
    if ((unsigned)q0 < (1u << NVF_OCC_REF_COORD_BITS) && (unsigned)q1 < (1u << NVF_OCC_REF_COORD_BITS) &&
        (unsigned)q2 < (1u << NVF_OCC_REF_COORD_BITS)) {
      const long long key = ref_key(q0, q1, q2);
      int lo = 0, hi = nblocks;                        // the first entry >= key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < nblocks && keys[lo] == key) {
        const int b = perm[lo];
        if ((unsigned)b < (unsigned)nblocks) {         // a permutation cannot fail this; no content of perm writes outside
          const int v = ((q0 & 31) * 32 + (q1 & 31)) * 32 + (q2 & 31);
          atomicOr(&words[(size_t)b * 512 + (v >> 6)], 1ull << (v & 63));   // integer OR: any order, the same words
          drop = false;
        }
      }
    }
  }
  const unsigned long long m = __ballot(drop);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(dropped, (unsigned long long)__popcll(m));
}

// the level-0 symbols of one block under the inter contexts: one workgroup per (block, temporal class r = blockIdx.y),
// which counts the symbols of its r alone, one uint32 per context as nbr_hist_kernel
__global__ __launch_bounds__(HIER_THREADS) void inter_hist_kernel(const float* __restrict__ p, const uint8_t* __restrict__ k1,
                                                                  const unsigned long long* __restrict__ w0,
                                                                  const uint16_t* __restrict__ rows,
                                                                  const uint32_t* __restrict__ ref,
                                                                  const int32_t* __restrict__ cells1,
                                                                  const int32_t* __restrict__ counts1,
                                                                  unsigned long long* __restrict__ cnt,
                                                                  unsigned long long* __restrict__ occ) {
  __shared__ uint32_t h[INTER_CTX_R];                  // occupied << 16 | symbols, each <= 32768
  const int tid = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
  for (int c = tid; c < INTER_CTX_R; c += HIER_THREADS) h[c] = 0;
  __syncthreads();
  const int32_t* parents = cells1 + hier_sum(counts1, 0, b, tid & 63);
  const int n = 8 * counts1[b];
  for (int i = tid; i < n; i += HIER_THREADS) {
    int cell, e;
    hier_where<0>(i, parents, b, cell, e);
    const int t = inter_class(inter_gather(ref, cell), nbr_gather(rows, e, i & 7), e, i & 7, cell & 31);
    if ((t >> 4) != r) continue;
    const int c = nbr_ctx0(t & 15, k1[e], p[cell]);
    atomicAdd(&h[c], 1u + ((uint32_t)((w0[cell >> 6] >> (cell & 63)) & 1ull) << 16));
  }
  __syncthreads();
  // integers: any order of these adds gives the same totals
  for (int c = tid; c < INTER_CTX_R; c += HIER_THREADS) {
    const uint32_t v = h[c];
    if (v & 0xFFFFu) atomicAdd(cnt + HIER_CTX + r * INTER_CTX_R + c, (unsigned long long)(v & 0xFFFFu));
    if (v >> 16) atomicAdd(occ + HIER_CTX + r * INTER_CTX_R + c, (unsigned long long)(v >> 16));
  }
}

}  // namespace

extern "C" int nvf_occ_hier_pyramid(const float* p, const float* gt, int batch, float* p1, uint8_t* k1, float* p2,
                                    uint8_t* k2, uint64_t* bad, uint64_t* gt_w0, uint64_t* gt_w1, uint64_t* gt_w2,
                                    void* stream) {
  if (!p || !p1 || !k1 || !p2 || !k2 || !bad || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH) return NVF_EINVAL;
  if (gt && (!gt_w0 || !gt_w1 || !gt_w2)) return NVF_EINVAL;
  hier_pyramid_kernel<<<batch, HIER_THREADS, 0, nvf_stream(stream)>>>(
      p, gt, p1, k1, p2, k2, (unsigned long long*)bad, (unsigned long long*)gt_w0, (unsigned long long*)gt_w1,
      (unsigned long long*)gt_w2);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_hier_cells(const uint64_t* words, int batch, int wpb, int32_t* counts, int32_t* cells,
                                  void* stream) {
  if (!words || !counts || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || (wpb != 8 && wpb != 64 && wpb != 512))
    return NVF_EINVAL;
  if (cells && wpb == 512) return NVF_EINVAL;          // voxels have no children: their list is the point cloud
  hier_count_kernel<<<(batch + 3) / 4, 256, 0, nvf_stream(stream)>>>((const unsigned long long*)words, batch, wpb, counts);
  NVF_LAUNCH_CHECK();
  if (cells) {
    hier_cells_kernel<<<(batch + 3) / 4, 256, 0, nvf_stream(stream)>>>((const unsigned long long*)words, batch, wpb, counts,
                                                                       cells);
    NVF_LAUNCH_CHECK();
  }
  return NVF_OK;
}

extern "C" int nvf_occ_hier_hist(int level, const float* pv, const uint8_t* kv, const uint64_t* gt_words,
                                 const int32_t* cells, const int32_t* counts, int batch, uint64_t* cnt, uint64_t* occ,
                                 void* stream) {
  if (!pv || !kv || !gt_words || !cnt || !occ || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || level < 0 || level > 2 ||
      (level < 2 && (!cells || !counts)))
    return NVF_EINVAL;
  const unsigned long long* gw = (const unsigned long long*)gt_words;
  unsigned long long *c = (unsigned long long*)cnt, *o = (unsigned long long*)occ;
  hipStream_t s = nvf_stream(stream);
  if (level == 2) hier_hist_kernel<2><<<batch, HIER_THREADS, 0, s>>>(pv, kv, gw, cells, counts, c, o);
  if (level == 1) hier_hist_kernel<1><<<batch, HIER_THREADS, 0, s>>>(pv, kv, gw, cells, counts, c, o);
  if (level == 0) hier_hist_kernel<0><<<batch, HIER_THREADS, 0, s>>>(pv, kv, gw, cells, counts, c, o);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_hier_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                                   const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2,
                                   const int32_t* cells2, const int32_t* counts2, const int32_t* cells1,
                                   const int32_t* counts1, const int32_t* f1, int batch, int group, uint64_t* states,
                                   uint32_t* words, uint32_t* nwords, void* stream) {
  if (!p || !p1 || !k1 || !p2 || !k2 || !gt_w0 || !gt_w1 || !gt_w2 || !cells2 || !counts2 || !cells1 || !counts1 || !f1 ||
      !states || !words || !nwords || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || group < 1 ||
      group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  hier_encode_kernel<CTX_FIELD><<<groups, 64, 0, nvf_stream(stream)>>>(
      p, p1, k1, p2, k2, (const unsigned long long*)gt_w0, (const unsigned long long*)gt_w1,
      (const unsigned long long*)gt_w2, cells2, counts2, cells1, counts1, f1, batch, group, (unsigned long long*)states,
      words, nwords);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_hier_decode(int level, const float* pv, const uint8_t* kv, const int32_t* cells,
                                   const int32_t* counts, const int32_t* f1, uint64_t* states, int64_t* pos,
                                   const uint32_t* words, const int64_t* word_off, const uint32_t* nwords,
                                   int64_t total_words, int batch, int group, uint64_t* occ_words, int32_t* status,
                                   void* stream) {
  if (!pv || !kv || !f1 || !states || !pos || !words || !word_off || !nwords || !occ_words || !status || total_words < 0 ||
      batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || group < 1 || group > NVF_OCC_RANS_MAX_GROUP || level < 0 ||
      level > 2 || (level < 2 && (!cells || !counts)))
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  hipStream_t s = nvf_stream(stream);
  unsigned long long *x = (unsigned long long*)states, *ow = (unsigned long long*)occ_words;
  const long long* wo = (const long long*)word_off;
  long long* ps = (long long*)pos;
  const long long tw = (long long)total_words;
  if (level == 2)
    hier_decode_kernel<2><<<groups, 64, 0, s>>>(pv, kv, cells, counts, f1, x, ps, words, wo, nwords, tw, batch, group, ow, status);
  if (level == 1)
    hier_decode_kernel<1><<<groups, 64, 0, s>>>(pv, kv, cells, counts, f1, x, ps, words, wo, nwords, tw, batch, group, ow, status);
  if (level == 0)
    hier_decode_kernel<0><<<groups, 64, 0, s>>>(pv, kv, cells, counts, f1, x, ps, words, wo, nwords, tw, batch, group, ow, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_nbr_hist(const float* p, const uint8_t* k1, const uint64_t* gt_w0, const uint64_t* gt_w1,
                                const int32_t* cells1, const int32_t* counts1, int batch, uint64_t* cnt, uint64_t* occ,
                                void* stream) {
  if (!p || !k1 || !gt_w0 || !gt_w1 || !cells1 || !counts1 || !cnt || !occ || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH)
    return NVF_EINVAL;
  nbr_hist_kernel<<<batch, HIER_THREADS, 0, nvf_stream(stream)>>>(p, k1, (const unsigned long long*)gt_w0,
                                                                  (const uint16_t*)gt_w1, cells1, counts1,
                                                                  (unsigned long long*)cnt, (unsigned long long*)occ);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_nbr_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                                  const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2,
                                  const int32_t* cells2, const int32_t* counts2, const int32_t* cells1,
                                  const int32_t* counts1, const int32_t* f1, int batch, int group, uint64_t* states,
                                  uint32_t* words, uint32_t* nwords, void* stream) {
  if (!p || !p1 || !k1 || !p2 || !k2 || !gt_w0 || !gt_w1 || !gt_w2 || !cells2 || !counts2 || !cells1 || !counts1 || !f1 ||
      ((uintptr_t)f1 & 15) || !states || !words || !nwords || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || group < 1 ||
      group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  hier_encode_kernel<CTX_NBR><<<groups, 64, 0, nvf_stream(stream)>>>(
      p, p1, k1, p2, k2, (const unsigned long long*)gt_w0, (const unsigned long long*)gt_w1,
      (const unsigned long long*)gt_w2, cells2, counts2, cells1, counts1, f1, batch, group, (unsigned long long*)states,
      words, nwords);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_nbr_decode(const float* p, const uint8_t* k1, const int32_t* cells1, const int32_t* counts1,
                                  const uint64_t* w1, const int32_t* f1, uint64_t* states, int64_t* pos,
                                  const uint32_t* words, const int64_t* word_off, const uint32_t* nwords,
                                  int64_t total_words, int batch, int group, uint64_t* occ_words, int32_t* status,
                                  void* stream) {
  if (!p || !k1 || !cells1 || !counts1 || !w1 || !f1 || ((uintptr_t)f1 & 15) || !states || !pos || !words || !word_off ||
      !nwords || !occ_words || !status || total_words < 0 || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH || group < 1 ||
      group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  nbr_decode_kernel<<<groups, 64, 0, nvf_stream(stream)>>>(
      p, k1, cells1, counts1, (const uint16_t*)w1, f1 + HIER_CTX, (unsigned long long*)states, (long long*)pos, words,
      (const long long*)word_off, nwords, (long long)total_words, batch, group, (unsigned long long*)occ_words, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_ref_words(const int32_t* points, int64_t npts, const int64_t* keys, const int32_t* perm, int nblocks,
                                 uint64_t* words, uint64_t* dropped, void* stream) {
  if (!keys || !perm || !words || !dropped || npts < 0 || (npts > 0 && !points) || nblocks <= 0 ||
      nblocks > NVF_OCC_HIER_MAX_BATCH || npts > ((int64_t)1 << 31) * 256)
    return NVF_EINVAL;
  if (npts == 0) return NVF_OK;
  ref_words_kernel<<<(unsigned)((npts + 255) / 256), 256, 0, nvf_stream(stream)>>>(
      points, (long long)npts, (const long long*)keys, perm, nblocks, (unsigned long long*)words,
      (unsigned long long*)dropped);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_inter_hist(const float* p, const uint8_t* k1, const uint64_t* gt_w0, const uint64_t* gt_w1,
                                  const uint64_t* ref_words, const int32_t* cells1, const int32_t* counts1, int batch,
                                  uint64_t* cnt, uint64_t* occ, void* stream) {
  if (!p || !k1 || !gt_w0 || !gt_w1 || !ref_words || !cells1 || !counts1 || !cnt || !occ || batch <= 0 ||
      batch > NVF_OCC_HIER_MAX_BATCH)
    return NVF_EINVAL;
  inter_hist_kernel<<<dim3(batch, 3), HIER_THREADS, 0, nvf_stream(stream)>>>(
      p, k1, (const unsigned long long*)gt_w0, (const uint16_t*)gt_w1, (const uint32_t*)ref_words, cells1, counts1,
      (unsigned long long*)cnt, (unsigned long long*)occ);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_inter_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                                    const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2,
                                    const uint64_t* ref_words, const int32_t* cells2, const int32_t* counts2,
                                    const int32_t* cells1, const int32_t* counts1, const int32_t* f1, int batch, int group,
                                    uint64_t* states, uint32_t* words, uint32_t* nwords, void* stream) {
  if (!p || !p1 || !k1 || !p2 || !k2 || !gt_w0 || !gt_w1 || !gt_w2 || !ref_words || !cells2 || !counts2 || !cells1 ||
      !counts1 || !f1 || ((uintptr_t)f1 & 15) || !states || !words || !nwords || batch <= 0 ||
      batch > NVF_OCC_HIER_MAX_BATCH || group < 1 || group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  hier_encode_kernel<CTX_INTER><<<groups, 64, 0, nvf_stream(stream)>>>(
      p, p1, k1, p2, k2, (const unsigned long long*)gt_w0, (const unsigned long long*)gt_w1,
      (const unsigned long long*)gt_w2, cells2, counts2, cells1, counts1, f1, batch, group, (unsigned long long*)states,
      words, nwords, (const uint32_t*)ref_words);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_inter_decode(const float* p, const uint8_t* k1, const int32_t* cells1, const int32_t* counts1,
                                    const uint64_t* w1, const uint64_t* ref_words, const int32_t* f1, uint64_t* states,
                                    int64_t* pos, const uint32_t* words, const int64_t* word_off, const uint32_t* nwords,
                                    int64_t total_words, int batch, int group, uint64_t* occ_words, int32_t* status,
                                    void* stream) {
  if (!p || !k1 || !cells1 || !counts1 || !w1 || !ref_words || !f1 || ((uintptr_t)f1 & 15) || !states || !pos || !words ||
      !word_off || !nwords || !occ_words || !status || total_words < 0 || batch <= 0 || batch > NVF_OCC_HIER_MAX_BATCH ||
      group < 1 || group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  inter_decode_kernel<<<groups, 64, 0, nvf_stream(stream)>>>(
      p, k1, cells1, counts1, (const uint16_t*)w1, (const uint32_t*)ref_words, f1 + HIER_CTX, (unsigned long long*)states,
      (long long*)pos, words, (const long long*)word_off, nwords, (long long)total_words, batch, group,
      (unsigned long long*)occ_words, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
