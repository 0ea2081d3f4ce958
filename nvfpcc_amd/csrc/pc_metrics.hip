// Geometry-quality metrics of a decoded cloud against its reference: exact 1-NN, k-NN + PCA normals, and the
// D1 (point-to-point) / D2 (point-to-plane) error sums behind MPEG's geometry PSNR (pc_error's definitions; the
// Python side is nvfpcc_amd/pc_metrics.py, the ABI include/nvf_hip.h "point-cloud metrics").
//
// Index.  Coordinates are 10-bit integers.  A cloud is bucketed into cells of 8^3 voxels (a dense 128^3 grid) and
// the cells into super-cells of 64^3 voxels (16^3).  The cell key puts the super-cell in the high bits
// (super << 9 | cell-in-super), so the points of one super-cell are one contiguous range of the sorted cloud and
// cell_start[super << 9] .. cell_start[(super + 1) << 9] delimits it.  A sorted cloud is int4 (x, y, z, input index).
//
// Search.  One lane per query; the queries are themselves a sorted cloud, so the 64 lanes of a wave search
// neighbouring cells.  A lane visits Chebyshev shells of cells around its own cell and stops once the lower bound of
// the next shell is GREATER than its current best squared distance (not merely equal: a point at the same distance
// with a lower input index may sit in that shell).  Candidates compare as (d2 << 32 | input index), so ties go to the
// lowest input index whatever order the cells are scanned in, and the result does not depend on the sort.
// The 1-NN search looks at most kNearR shells far; a query still unresolved there (its nearest target is more than
// 16 voxels away: an empty decoded block, a far cluster) walks the super-cells shell by shell instead, skipping empty
// super-cells in one read each and scanning only cells whose box can still hold a better point.
#include "nvf_common.h"

namespace {

constexpr int kGrid = 128;                  // cells per axis (edge 8 voxels)
constexpr int kSGrid = 16;                  // super-cells per axis (edge 64 voxels)
constexpr int kNearR = 2;                   // cell shells searched before the super-cell walk
constexpr int kThreads = 256;
constexpr int kSumThreads = 256;
constexpr int kSumMaxBlocks = 1024;
constexpr uint64_t kNone = ~0ull;
static_assert(NVF_PC_CELLS == kGrid * kGrid * kGrid, "cell grid of the ABI");

__device__ __forceinline__ int cell_key(int cx, int cy, int cz) {
  return ((((cx >> 3) << 8) | ((cy >> 3) << 4) | (cz >> 3)) << 9) | ((cx & 7) << 6) | ((cy & 7) << 3) | (cz & 7);
}

__device__ __forceinline__ int gap(int q, int lo, int w) { return max(0, max(lo - q, q - (lo + w - 1))); }

// least squared distance from q to the box [b, b + w)^3
__device__ __forceinline__ int64_t box_lb(int qx, int qy, int qz, int bx, int by, int bz, int w) {
  const int gx = gap(qx, bx, w), gy = gap(qy, by, w), gz = gap(qz, bz, w);
  return gx * gx + gy * gy + gz * gz;
}

// least squared distance from q to any voxel of Chebyshev shell s >= 1 of boxes of edge w around q's own box:
// along one axis the box at -s starts f + w (s - 1) + 1 away and the box at +s starts w s - f away (f = q mod w)
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

// visits the cells (x, y, z) of Chebyshev shell s around (cx, cy, cz) inside [0, n)^3
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

__global__ __launch_bounds__(kThreads) void pc_nearest_kernel(const int4* __restrict__ query, int nq,
                                                             const int4* __restrict__ tgt,
                                                             const int32_t* __restrict__ start,
                                                             int32_t* __restrict__ nn_idx, int32_t* __restrict__ nn_d2) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nq) return;
  const int4 q = query[i];
  const int cx = min(max(q.x >> 3, 0), kGrid - 1), cy = min(max(q.y >> 3, 0), kGrid - 1),
            cz = min(max(q.z >> 3, 0), kGrid - 1);
  uint64_t best = kNone;
  auto scan_cell = [&](int x, int y, int z) {
    if (box_lb(q.x, q.y, q.z, 8 * x, 8 * y, 8 * z, 8) > d2_of(best)) return;
    const int key = cell_key(x, y, z);
    const int e = start[key + 1];
    for (int j = start[key]; j < e; ++j) best = min(best, cand(tgt[j], q.x, q.y, q.z));
  };
  for (int s = 0; s <= kNearR; ++s) {
    if (s > 0 && shell_lb(q.x, q.y, q.z, s, 8) > d2_of(best)) break;
    for_shell(cx, cy, cz, s, kGrid, scan_cell);
  }
  if (shell_lb(q.x, q.y, q.z, kNearR + 1, 8) <= d2_of(best)) {
    // unresolved: walk the super-cells (scanning a cell twice changes nothing: the minimum is exact)
    const int sx = cx >> 3, sy = cy >> 3, sz = cz >> 3;
    for (int s = 0; s < kSGrid; ++s) {
      if (s > 0 && shell_lb(q.x, q.y, q.z, s, 64) > d2_of(best)) break;
      for_shell(sx, sy, sz, s, kSGrid, [&](int x, int y, int z) {
        const int base = ((x << 8) | (y << 4) | z) << 9;
        if (start[base] == start[base + 512] || box_lb(q.x, q.y, q.z, 64 * x, 64 * y, 64 * z, 64) > d2_of(best))
          return;
        for (int l = 0; l < 512; ++l) {
          const int b = start[base + l], e = start[base + l + 1];
          if (b == e) continue;
          const int x8 = 8 * (x * 8 + (l >> 6)), y8 = 8 * (y * 8 + ((l >> 3) & 7)), z8 = 8 * (z * 8 + (l & 7));
          if (box_lb(q.x, q.y, q.z, x8, y8, z8, 8) > d2_of(best)) continue;
          for (int j = b; j < e; ++j) best = min(best, cand(tgt[j], q.x, q.y, q.z));
        }
      });
    }
  }
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
// smallest eigenvalue of the neighbourhood's covariance.  The top-k lives in registers as K sorted keys; k <= K.
template <int K>
__global__ __launch_bounds__(kThreads) void pc_knn_normals_kernel(const int4* __restrict__ pts,
                                                                 const int32_t* __restrict__ start,
                                                                 const int32_t* __restrict__ xyz, int n, int k,
                                                                 float* __restrict__ normals,
                                                                 int32_t* __restrict__ knn_idx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int4 q = pts[i];
  const int cx = min(max(q.x >> 3, 0), kGrid - 1), cy = min(max(q.y >> 3, 0), kGrid - 1),
            cz = min(max(q.z >> 3, 0), kGrid - 1);
  uint64_t top[K];
#pragma unroll
  for (int j = 0; j < K; ++j) top[j] = kNone;
  uint64_t kth = kNone;                 // top[k - 1]
  auto scan_cell = [&](int x, int y, int z) {
    if (box_lb(q.x, q.y, q.z, 8 * x, 8 * y, 8 * z, 8) > d2_of(kth)) return;
    const int key = cell_key(x, y, z);
    const int e = start[key + 1];
    for (int jj = start[key]; jj < e; ++jj) {
      uint64_t c = cand(pts[jj], q.x, q.y, q.z);
      if (c >= kth) continue;
#pragma unroll
      for (int j = 0; j < K; ++j) {     // sorted insert: constant indices only, so the array stays in registers
        const uint64_t a = top[j];
        const bool lt = c < a;
        top[j] = lt ? c : a;
        c = lt ? a : c;
      }
#pragma unroll
      for (int j = 0; j < K; ++j) kth = (j == k - 1) ? top[j] : kth;
    }
  };
  for (int s = 0; s < kGrid; ++s) {
    if (s > 0 && shell_lb(q.x, q.y, q.z, s, 8) > d2_of(kth)) break;
    for_shell(cx, cy, cz, s, kGrid, scan_cell);
  }
  // k * scatter matrix, exactly: k * sum(p p^T) - sum(p) sum(p)^T in int64
  int64_t s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j < k) {
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

int sum_blocks(int n) { return min(kSumMaxBlocks, (n + 4 * kSumThreads - 1) / (4 * kSumThreads)); }

size_t sum_workspace(int n) {
  return n <= 0 ? 0 : (size_t)sum_blocks(n) * (sizeof(int64_t) + sizeof(double) + sizeof(int32_t));
}

struct ErrPartials {
  int64_t* d1;
  double* d2;
  int32_t* mx;
  static ErrPartials at(void* ws, int blocks) {
    ErrPartials p;
    p.d1 = (int64_t*)ws;
    p.d2 = (double*)(p.d1 + blocks);
    p.mx = (int32_t*)(p.d2 + blocks);
    return p;
  }
};

// fixed-order block reduction (the partition depends on n only), so every call gives the same bits
__global__ __launch_bounds__(kSumThreads) void pc_error_partial_kernel(const int32_t* __restrict__ q, int n, int chunk,
                                                                      const int32_t* __restrict__ t,
                                                                      const int32_t* __restrict__ nn,
                                                                      const float* __restrict__ normals,
                                                                      int normals_of_target, ErrPartials out) {
  __shared__ int64_t r1[kSumThreads];
  __shared__ double r2[kSumThreads];
  __shared__ int32_t rm[kSumThreads];
  const int tid = threadIdx.x, lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  int64_t s1 = 0;
  double s2 = 0.0;
  int32_t mx = 0;
  for (int i = lo + tid; i < hi; i += kSumThreads) {
    const int j = nn[i];
    const int ex = t[3 * j] - q[3 * i], ey = t[3 * j + 1] - q[3 * i + 1], ez = t[3 * j + 2] - q[3 * i + 2];
    const int d = ex * ex + ey * ey + ez * ez;
    s1 += d;
    mx = max(mx, d);
    if (normals) {
      const float* nv = normals + 3 * (size_t)(normals_of_target ? j : i);
      const double dot = (double)ex * (double)nv[0] + (double)ey * (double)nv[1] + (double)ez * (double)nv[2];
      s2 += dot * dot;
    }
  }
  r1[tid] = s1;
  r2[tid] = s2;
  rm[tid] = mx;
  for (int o = kSumThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
      rm[tid] = max(rm[tid], rm[tid + o]);
    }
  }
  if (tid == 0) {
    out.d1[blockIdx.x] = r1[0];
    out.d2[blockIdx.x] = r2[0];
    out.mx[blockIdx.x] = rm[0];
  }
}

__global__ __launch_bounds__(kSumThreads) void pc_error_final_kernel(ErrPartials in, int blocks, int64_t* sums,
                                                                    double* d2_sum) {
  __shared__ int64_t r1[kSumThreads];
  __shared__ double r2[kSumThreads];
  __shared__ int32_t rm[kSumThreads];
  const int tid = threadIdx.x;
  int64_t s1 = 0;
  double s2 = 0.0;
  int32_t mx = 0;
  for (int b = tid; b < blocks; b += kSumThreads) {
    s1 += in.d1[b];
    s2 += in.d2[b];
    mx = max(mx, in.mx[b]);
  }
  r1[tid] = s1;
  r2[tid] = s2;
  rm[tid] = mx;
  for (int o = kSumThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
      rm[tid] = max(rm[tid], rm[tid + o]);
    }
  }
  if (tid == 0) {
    sums[0] = r1[0];
    sums[1] = rm[0];
    if (d2_sum) d2_sum[0] = r2[0];
  }
}

}  // namespace

extern "C" size_t nvf_pc_workspace_bytes(int n_query, int n_target) {
  return sum_workspace(max(n_query, n_target));
}

extern "C" int nvf_pc_nearest(const int32_t* query_sorted, int n_query, const int32_t* target_sorted,
                              const int32_t* cell_start, int n_target, int32_t* nn_idx, int32_t* nn_d2, void* stream) {
  if (!query_sorted || !target_sorted || !cell_start || !nn_idx || !nn_d2 || n_query <= 0 || n_target <= 0)
    return NVF_EINVAL;
  pc_nearest_kernel<<<(n_query + kThreads - 1) / kThreads, kThreads, 0, nvf_stream(stream)>>>(
      (const int4*)query_sorted, n_query, (const int4*)target_sorted, cell_start, nn_idx, nn_d2);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pc_knn_normals(const int32_t* cloud_sorted, const int32_t* cell_start, const int32_t* cloud_xyz,
                                  int n, int k, float* normals, int32_t* knn_idx, void* stream) {
  if (!cloud_sorted || !cell_start || !cloud_xyz || !normals || k < 3 || k > 32 || n < k) return NVF_EINVAL;
  const dim3 grid((n + kThreads - 1) / kThreads);
  if (k <= 16)
    pc_knn_normals_kernel<16><<<grid, kThreads, 0, nvf_stream(stream)>>>((const int4*)cloud_sorted, cell_start,
                                                                         cloud_xyz, n, k, normals, knn_idx);
  else
    pc_knn_normals_kernel<32><<<grid, kThreads, 0, nvf_stream(stream)>>>((const int4*)cloud_sorted, cell_start,
                                                                         cloud_xyz, n, k, normals, knn_idx);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_pc_error_sums(const int32_t* query_xyz, int n_query, const int32_t* target_xyz,
                                 const int32_t* nn_idx, const float* normals, int normals_of_target, int64_t* sums,
                                 double* d2_sum, void* workspace, size_t workspace_bytes, void* stream) {
  if (!query_xyz || !target_xyz || !nn_idx || !sums || (normals && !d2_sum) || n_query <= 0) return NVF_EINVAL;
  if (!workspace || workspace_bytes < sum_workspace(n_query)) return NVF_EWORKSPACE;
  const int blocks = sum_blocks(n_query), chunk = (n_query + blocks - 1) / blocks;
  const ErrPartials p = ErrPartials::at(workspace, blocks);
  pc_error_partial_kernel<<<blocks, kSumThreads, 0, nvf_stream(stream)>>>(query_xyz, n_query, chunk, target_xyz,
                                                                          nn_idx, normals, normals_of_target, p);
  NVF_LAUNCH_CHECK();
  pc_error_final_kernel<<<1, kSumThreads, 0, nvf_stream(stream)>>>(p, blocks, sums, normals ? d2_sum : nullptr);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
