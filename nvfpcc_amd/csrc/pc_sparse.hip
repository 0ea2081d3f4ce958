// The geometry metrics of pc_metrics.hip for clouds of 10, 11 and 12 bits per axis: the same exact 1-NN and k-NN + PCA
// normals, on a SPARSE hierarchical cell index whose memory follows the points and the occupied cells, never the
// volume (a dense cell_start of a 4096^3 volume would be 512 MiB per cloud).  ABI: include/nvf_hip.h "point-cloud
// metrics, sparse index"; Python: nvfpcc_amd/pc_metrics.py (_SparseCloud).
//
// Index.  Cells stay 8^3 voxels.  Above them sit 64-voxel super-cells, 512-voxel hyper-cells and the root of 2, 4 or
// 8 hyper-cells per axis.  The cell key nests the levels, hyper << 18 | super-in-hyper << 9 | cell-in-super (each
// 9-bit field is x << 6 | y << 3 | z of the 3-bit position inside the parent), so the points of any node of any level
// are one contiguous range of the sorted cloud.  cell_start [M + 1] runs over the M OCCUPIED cells in key order.  An
// occupied super-cell has a record: a 512-bit mask of its cells (8 x uint64, word = x, bit = y << 3 | z) and the
// index of its first occupied cell; the cell of bit b of word w is cell first + popcount(words below w) +
// popcount(word w below b).  super_table [(2^bits / 64)^3] maps key >> 9 to the record or -1, hyper_table
// [(2^bits / 512)^3] says which hyper-cells hold a point.
//
// Search.  One lane per query, the queries themselves a sorted cloud.  Near phase: Chebyshev shells 0..kNearR of
// cells around the query's cell, each cell found through super_table and one mask word.  A shell loop stops only when
// the next shell's lower bound is GREATER than the current bound, and candidates compare as (d2 << 32 | input index):
// ties go to the lowest input index whatever order cells are met in (the arguments of pc_metrics.hip, unchanged).
// A query the near phase leaves unresolved descends top-down: hyper-cell shells around its own hyper-cell, empty
// hyper-cells skipped in one read, then the occupied super-cells of a surviving hyper-cell, then their occupied
// cells, with the box lower-bound test at every level.  Cells of the near phase are skipped there (the k-NN list
// must not meet a point twice).  The k-NN kernel takes the same descent: its work is bounded by the occupied
// structure, not by the 512 cell shells a tiny cloud in a 4096^3 volume would otherwise walk.
//
// Ranges.  d2 <= 3 * 4095^2 = 50 307 075 < 2^31, so the (d2, index) key and the int32 nn_d2 hold at 12 bits.  The k-NN
// scatter sums k * sum(p p^T) - sum(p) sum(p)^T have terms below 32 * 32 * 4095^2 < 2^35 and stay in int64.
// nvf_pc_error_sums (pc_metrics.hip) takes coordinates and indices only and is reused unchanged: its int64 D1 sum
// holds 2^31 points * 2^26, its per-point dot product is fp64.
#include "nvf_common.h"

namespace {

constexpr int kNearR = 2;                   // cell shells searched before the top-down descent
constexpr int kThreads = 256;
constexpr uint64_t kNone = ~0ull;

struct Index {
  const int4* pts;
  const int32_t* start;
  const uint64_t* mask;
  const int32_t* first;
  const int32_t* stab;
  const int32_t* htab;
  int hb;                                   // bits of a hyper-cell coordinate: 1, 2, 3 at 10, 11, 12 bits per axis
};

__device__ __forceinline__ int gap(int q, int lo, int w) { return max(0, max(lo - q, q - (lo + w - 1))); }

// least squared distance from q to the box [b, b + w)^3
__device__ __forceinline__ int64_t box_lb(int qx, int qy, int qz, int bx, int by, int bz, int w) {
  const int gx = gap(qx, bx, w), gy = gap(qy, by, w), gz = gap(qz, bz, w);
  return gx * gx + gy * gy + gz * gz;
}

// least squared distance from q to any voxel of Chebyshev shell s >= 1 of boxes of edge w around q's own box
__device__ __forceinline__ int64_t shell_lb(int qx, int qy, int qz, int s, int w) {
  const int fx = qx & (w - 1), fy = qy & (w - 1), fz = qz & (w - 1);
  const int m = min(min(min(fx + w * (s - 1) + 1, w * s - fx), min(fy + w * (s - 1) + 1, w * s - fy)),
                    min(fz + w * (s - 1) + 1, w * s - fz));
  return (int64_t)m * m;
}

__device__ __forceinline__ uint64_t cand(int4 p, int qx, int qy, int qz) {
  const int dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
  return ((uint64_t)(uint32_t)(dx * dx + dy * dy + dz * dz) << 32) | (uint32_t)p.w;
}

__device__ __forceinline__ int64_t d2_of(uint64_t key) { return (int64_t)(key >> 32); }   // kNone -> 2^32 - 1

// visits the boxes (x, y, z) of Chebyshev shell s around (cx, cy, cz) inside [0, n)^3
template <typename F>
__device__ __forceinline__ void for_shell(int cx, int cy, int cz, int s, int n, F&& f) {
  for (int dx = -s; dx <= s; ++dx) {
    const int x = cx + dx;
    if (x < 0 || x >= n) continue;
    for (int dy = -s; dy <= s; ++dy) {
      const int y = cy + dy;
      if (y < 0 || y >= n) continue;
      const int step = (dx == -s || dx == s || dy == -s || dy == s) ? 1 : 2 * s;   // interior column: dz = +-s only
      for (int dz = -s; dz <= s; dz += step) {
        const int z = cz + dz;
        if (z >= 0 && z < n) f(x, y, z);
      }
    }
  }
}

// the point range [b, e) of cell (x, y, z) (cell coordinates); false when the cell is empty
__device__ __forceinline__ bool cell_range(const Index& ix, int x, int y, int z, int& b, int& e) {
  const int h = ((x >> 6) << (2 * ix.hb)) | ((y >> 6) << ix.hb) | (z >> 6);
  const int l = (((x >> 3) & 7) << 6) | (((y >> 3) & 7) << 3) | ((z >> 3) & 7);
  const int r = ix.stab[(h << 9) | l];
  if (r < 0) return false;
  const uint64_t* mw = ix.mask + 8 * (size_t)r;
  const int w = x & 7, bit = ((y & 7) << 3) | (z & 7);
  const uint64_t word = mw[w];
  if (!((word >> bit) & 1)) return false;
  int rank = __popcll(word & ((1ull << bit) - 1));
  for (int j = 0; j < w; ++j) rank += __popcll(mw[j]);
  const int m = ix.first[r] + rank;
  b = ix.start[m];
  e = ix.start[m + 1];
  return true;
}

// The search of one query q whose cell is (cx, cy, cz): bound() is the squared distance above which nothing can
// enter the answer any more, offer(p) takes a candidate point.  Every cell whose box is within bound() is offered
// exactly once.
template <typename Bound, typename Offer>
__device__ __forceinline__ void search(const Index& ix, int4 q, int cx, int cy, int cz, Bound&& bound, Offer&& offer) {
  const int cgrid = 64 << ix.hb, hgrid = 1 << ix.hb;
  for (int s = 0; s <= kNearR; ++s) {
    if (s > 0 && shell_lb(q.x, q.y, q.z, s, 8) > bound()) return;
    for_shell(cx, cy, cz, s, cgrid, [&](int x, int y, int z) {
      int b, e;
      if (box_lb(q.x, q.y, q.z, 8 * x, 8 * y, 8 * z, 8) > bound() || !cell_range(ix, x, y, z, b, e)) return;
      for (int j = b; j < e; ++j) offer(ix.pts[j]);
    });
  }
  if (shell_lb(q.x, q.y, q.z, kNearR + 1, 8) > bound()) return;
  // unresolved (no early return above, so shells 0..kNearR were scanned whole): descend from the root
  const int hx = cx >> 6, hy = cy >> 6, hz = cz >> 6;
  for (int s = 0; s < hgrid; ++s) {
    if (s > 0 && shell_lb(q.x, q.y, q.z, s, 512) > bound()) return;
    for_shell(hx, hy, hz, s, hgrid, [&](int X, int Y, int Z) {
      const int h = (X << (2 * ix.hb)) | (Y << ix.hb) | Z;
      if (!ix.htab[h] || box_lb(q.x, q.y, q.z, 512 * X, 512 * Y, 512 * Z, 512) > bound()) return;
      for (int l = 0; l < 512; ++l) {
        const int r = ix.stab[(h << 9) | l];
        if (r < 0) continue;
        const int sx = 8 * X + (l >> 6), sy = 8 * Y + ((l >> 3) & 7), sz = 8 * Z + (l & 7);
        if (box_lb(q.x, q.y, q.z, 64 * sx, 64 * sy, 64 * sz, 64) > bound()) continue;
        int m = ix.first[r];
        for (int w = 0; w < 8; ++w) {
          uint64_t word = ix.mask[8 * (size_t)r + w];
          while (word) {
            const int bit = __builtin_ctzll(word), c = m++;
            word &= word - 1;
            const int x = 8 * sx + w, y = 8 * sy + (bit >> 3), z = 8 * sz + (bit & 7);
            if (max(max(abs(x - cx), abs(y - cy)), abs(z - cz)) <= kNearR) continue;     // met in the near phase
            if (box_lb(q.x, q.y, q.z, 8 * x, 8 * y, 8 * z, 8) > bound()) continue;
            const int e = ix.start[c + 1];
            for (int j = ix.start[c]; j < e; ++j) offer(ix.pts[j]);
          }
        }
      }
    });
  }
}

__global__ __launch_bounds__(kThreads) void pc_nearest_sparse_kernel(const int4* __restrict__ query, int nq, Index ix,
                                                                    int32_t* __restrict__ nn_idx,
                                                                    int32_t* __restrict__ nn_d2) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nq) return;
  const int4 q = query[i];
  const int top = (64 << ix.hb) - 1;
  const int cx = min(max(q.x >> 3, 0), top), cy = min(max(q.y >> 3, 0), top), cz = min(max(q.z >> 3, 0), top);
  uint64_t best = kNone;
  search(ix, q, cx, cy, cz, [&]() { return d2_of(best); },
         [&](int4 p) { best = min(best, cand(p, q.x, q.y, q.z)); });
  nn_idx[q.w] = (int32_t)(uint32_t)best;
  nn_d2[q.w] = (int32_t)(best >> 32);
}

// one cyclic-Jacobi rotation zeroing a[p][q] of a symmetric 3x3 (v accumulates the eigenvectors as columns)
template <int p, int q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int r = 3 - p - q;
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double arp = a[r][p], arq = a[r][q];
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
  a[r][p] = a[p][r] = c * arp - s * arq;
  a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double vp = v[j][p], vq = v[j][q];
    v[j][p] = c * vp - s * vq;
    v[j][q] = s * vp + c * vq;
  }
}

// k-NN of every point of a sorted cloud within the same cloud (itself included), then the unit eigenvector of the
// smallest eigenvalue of the neighbourhood's covariance: pc_metrics.hip's kernel, statement for statement after the
// search (the same integer sums and the same Jacobi give the same bits).  The top-k lives in registers as K sorted
// keys; k <= K.
template <int K>
__global__ __launch_bounds__(kThreads) void pc_knn_normals_sparse_kernel(Index ix, const int32_t* __restrict__ xyz,
                                                                        int n, int k, float* __restrict__ normals,
                                                                        int32_t* __restrict__ knn_idx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int4 q = ix.pts[i];
  const int top_cell = (64 << ix.hb) - 1;
  const int cx = min(max(q.x >> 3, 0), top_cell), cy = min(max(q.y >> 3, 0), top_cell),
            cz = min(max(q.z >> 3, 0), top_cell);
  uint64_t top[K];
#pragma unroll
  for (int j = 0; j < K; ++j) top[j] = kNone;
  uint64_t kth = kNone;                 // top[k - 1]
  search(ix, q, cx, cy, cz, [&]() { return d2_of(kth); }, [&](int4 p) {
    uint64_t c = cand(p, q.x, q.y, q.z);
    if (c >= kth) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {       // sorted insert: constant indices only, so the array stays in registers
      const uint64_t a = top[j];
      const bool lt = c < a;
      top[j] = lt ? c : a;
      c = lt ? a : c;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) kth = (j == k - 1) ? top[j] : kth;
  });
  // k * scatter matrix, exactly: k * sum(p p^T) - sum(p) sum(p)^T in int64
  int64_t s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j < k && top[j] != kNone) {     // n >= k and the search is exhaustive: always filled (guards the read below)
      const int idx = (int)(uint32_t)top[j];
      if (knn_idx) knn_idx[(size_t)q.w * k + j] = idx;
      const int64_t x = xyz[3 * idx], y = xyz[3 * idx + 1], z = xyz[3 * idx + 2];
      s1[0] += x; s1[1] += y; s1[2] += z;
      s2[0] += x * x; s2[1] += x * y; s2[2] += x * z; s2[3] += y * y; s2[4] += y * z; s2[5] += z * z;
    }
  }
  double a[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  a[0][0] = (double)(k * s2[0] - s1[0] * s1[0]);
  a[0][1] = a[1][0] = (double)(k * s2[1] - s1[0] * s1[1]);
  a[0][2] = a[2][0] = (double)(k * s2[2] - s1[0] * s1[2]);
  a[1][1] = (double)(k * s2[3] - s1[1] * s1[1]);
  a[1][2] = a[2][1] = (double)(k * s2[4] - s1[1] * s1[2]);
  a[2][2] = (double)(k * s2[5] - s1[2] * s1[2]);
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (off <= 1e-30 * diag || off == 0.0) break;
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  const int m = (a[0][0] <= a[1][1] && a[0][0] <= a[2][2]) ? 0 : (a[1][1] <= a[2][2] ? 1 : 2);
  double nx = m == 0 ? v[0][0] : (m == 1 ? v[0][1] : v[0][2]);
  double ny = m == 0 ? v[1][0] : (m == 1 ? v[1][1] : v[1][2]);
  double nz = m == 0 ? v[2][0] : (m == 1 ? v[2][1] : v[2][2]);
  const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
  normals[3 * (size_t)q.w] = (float)(nx * inv);
  normals[3 * (size_t)q.w + 1] = (float)(ny * inv);
  normals[3 * (size_t)q.w + 2] = (float)(nz * inv);
}

// One thread per occupied cell: its bit into its super-cell's mask (an integer OR: any order gives the same bits);
// the first cell of a super-cell writes that record's first-cell index and table entry, the first cell of a
// hyper-cell its flag.  The tables were cleared by the memsets of nvf_pc_sparse_build on the same stream.
__global__ __launch_bounds__(kThreads) void pc_sparse_fill_kernel(const int32_t* __restrict__ cell_key,
                                                                 const int32_t* __restrict__ cell_super, int m,
                                                                 int n_supers, int table_size, uint64_t* mask,
                                                                 int32_t* __restrict__ first,
                                                                 int32_t* __restrict__ stab,
                                                                 int32_t* __restrict__ htab) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int key = cell_key[i], r = cell_super[i];
  if ((unsigned)(key >> 9) >= (unsigned)table_size || (unsigned)r >= (unsigned)n_supers) return;   // not a key of this index
  const int c = key & 511;
  atomicOr((unsigned long long*)&mask[8 * (size_t)r + (c >> 6)], 1ull << (c & 63));
  const int prev = i > 0 ? cell_key[i - 1] : -1;
  if (i == 0 || (prev >> 9) != (key >> 9)) {
    first[r] = i;
    stab[key >> 9] = r;
  }
  if (i == 0 || (prev >> 18) != (key >> 18)) htab[key >> 18] = 1;
}

bool valid(const NvfPcSparseIndex* x) {
  return x && x->sorted && x->cell_start && x->super_mask && x->super_first && x->super_table && x->hyper_table &&
         x->bits >= 10 && x->bits <= 12 && x->n > 0 && x->n_cells > 0 && x->n_cells <= x->n && x->n_supers > 0 &&
         x->n_supers <= x->n_cells && x->n_supers <= NVF_PC_SPARSE_SUPERS(x->bits);
}

Index device_index(const NvfPcSparseIndex* x) {
  return Index{(const int4*)x->sorted, x->cell_start, x->super_mask, x->super_first, x->super_table, x->hyper_table,
               x->bits - 9};
}

}  // namespace

extern "C" int nvf_pc_sparse_build(const NvfPcSparseIndex* index, const int32_t* cell_key, const int32_t* cell_super,
                                   void* stream) {
  if (!valid(index) || !cell_key || !cell_super) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  const int supers = NVF_PC_SPARSE_SUPERS(index->bits), hypers = NVF_PC_SPARSE_HYPERS(index->bits);
  hipError_t e = hipMemsetAsync(index->super_mask, 0, (size_t)index->n_supers * 8 * sizeof(uint64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(index->super_table, 0xff, (size_t)supers * sizeof(int32_t), st);   // -1
  if (e == hipSuccess) e = hipMemsetAsync(index->hyper_table, 0, (size_t)hypers * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  pc_sparse_fill_kernel<<<(index->n_cells + kThreads - 1) / kThreads, kThreads, 0, st>>>(
      cell_key, cell_super, index->n_cells, index->n_supers, supers, index->super_mask, index->super_first,
      index->super_table, index->hyper_table);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pc_nearest_sparse(const int32_t* query_sorted, int n_query, const NvfPcSparseIndex* target,
                                     int32_t* nn_idx, int32_t* nn_d2, void* stream) {
  if (!query_sorted || !valid(target) || !nn_idx || !nn_d2 || n_query <= 0) return NVF_EINVAL;
  pc_nearest_sparse_kernel<<<(n_query + kThreads - 1) / kThreads, kThreads, 0, nvf_stream(stream)>>>(
      (const int4*)query_sorted, n_query, device_index(target), nn_idx, nn_d2);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pc_knn_normals_sparse(const NvfPcSparseIndex* cloud, const int32_t* cloud_xyz, int k,
                                         float* normals, int32_t* knn_idx, void* stream) {
  if (!valid(cloud) || !cloud_xyz || !normals || k < 3 || k > 32 || cloud->n < k) return NVF_EINVAL;
  const int n = cloud->n;
  const dim3 grid((n + kThreads - 1) / kThreads);
  if (k <= 16)
    pc_knn_normals_sparse_kernel<16><<<grid, kThreads, 0, nvf_stream(stream)>>>(device_index(cloud), cloud_xyz, n, k,
                                                                                normals, knn_idx);
  else
    pc_knn_normals_sparse_kernel<32><<<grid, kThreads, 0, nvf_stream(stream)>>>(device_index(cloud), cloud_xyz, n, k,
                                                                                normals, knn_idx);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
