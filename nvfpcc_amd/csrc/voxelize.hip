// Voxelisation of a float cloud on the device (nvfpcc_amd/voxelize.py): float64 [P,3] points under a lattice
// L = (bits, o[3], s) -> the distinct lattice points in ascending key order, how many input points fell on each, and
// the quantisation error.  The definition is the format: both sides of a pack must agree to the bit.
//
//   forward   t = x - o;  u = t * inv;  q = floor(u + 0.5)       inv = 1.0 / s, one division, on the host
//   inverse   x = o + q * s                                     a multiply, then an add
//   error     e2 = sum over axes 0, 1, 2 of (x - (o + q s))^2    in that order
//
// Every operation above is rounded to float64 on its own: a fused multiply-add would round u + 0.5 or o + q s once
// instead of twice and move a point that sits within an ulp of a cell boundary -- about one point in 10^13, which no
// random test can show.  It is therefore ensured by construction: this whole file is compiled with floating-point
// contraction off (the pragma below, at file scope, and again in the three functions that hold the arithmetic), and the
// kernels' code holds no double-precision fused multiply-add.
//
//   nvf_vox_bounds      per-axis minimum and maximum over the finite points, count and lowest index of the others: a
//                       grid of partial records and one workgroup that folds them.  min and max are exact in any
//                       order, so no atomics on floats are needed and none are used.
//   nvf_vox_quantize    per point: class (non-finite, outside, inside -- decided in float64 before any conversion to an
//                       integer), q, the sort key, e2.  max e2 is a maximum of non-negative doubles, taken on their
//                       bit patterns as integers; sum e2 is one partial per workgroup, every partial summed in a fixed
//                       order.  A point that is not inside gets q = -1 and the largest key, so it sorts last.
//   (the caller sorts the keys)
//   nvf_vox_unique      over the sorted keys: head flags, a grid-wide exclusive scan in the house form of pp_device.hip
//                       (sums per workgroup, one workgroup scans the at most 1024 sums, emit: three launches ordered
//                       by the stream, no workgroup waits for another), then the point of every head at its rank.  A
//                       run's count is (index after its tail) - (index of its head): the two ends may lie in
//                       different workgroups, so each adds its term to counts[rank] -- integer adds, exact in any
//                       order -- and a run of one point is a plain store.
//   nvf_vox_dequantize  q -> o + q s
//
// All four are memory-bound (24 bytes in and 20 out per point for the quantiser) and hold a few dozen registers: the
// grids are capped at 1024 workgroups and stride over the rest.
#include <math.h>

#include "nvf_common.h"

#pragma clang fp contract(off)

#define VOX_BAD_KEY 0x7fffffffffffffffll
#define VOX_NONE 0xffffffffffffffffull          // "no such point" in a lowest-index word: -1, the largest unsigned
// the status record of nvf_vox_quantize / nvf_vox_unique, 8-byte words
#define VOX_ST_NONFINITE 0
#define VOX_ST_OUTSIDE 1
#define VOX_ST_FIRST_NONFINITE 2
#define VOX_ST_FIRST_OUTSIDE 3
#define VOX_ST_MAX_ERR2 4
#define VOX_ST_VOXELS 5
#define VOX_ST_GROUPS 6
#define VOX_ST_PARTIALS 8
static_assert(VOX_ST_PARTIALS + NVF_VOX_MAX_GROUPS == NVF_VOX_STATUS_WORDS, "status layout");

// ---- the arithmetic of the definition ---------------------------------------------------------------------------------
// u + 0.5 of one coordinate; the caller classifies it and floors it
__device__ __forceinline__ double vox_forward(double x, double o, double inv) {
#pragma clang fp contract(off)
  const double t = x - o;
  const double u = t * inv;
  return u + 0.5;
}
__device__ __forceinline__ double vox_inverse(int q, double o, double s) {
#pragma clang fp contract(off)
  const double p = (double)q * s;
  return o + p;
}
__device__ __forceinline__ double vox_err2(double x, double y, double z, double rx, double ry, double rz) {
#pragma clang fp contract(off)
  const double dx = x - rx, dy = y - ry, dz = z - rz;
  const double ex = dx * dx, ey = dy * dy, ez = dz * dz;
  const double e = ex + ey;
  return e + ez;
}

__device__ __forceinline__ bool vox_finite(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- bounds -----------------------------------------------------------------------------------------------------------
// One record of eight 8-byte words: lo[3], hi[3] (doubles), the count of non-finite points, the lowest index of one
struct VoxBounds {
  double lo[3], hi[3];
  unsigned long long bad, first;
};
__device__ __forceinline__ void vox_bounds_merge(VoxBounds& a, const VoxBounds& b) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = fmin(a.lo[k], b.lo[k]);
    a.hi[k] = fmax(a.hi[k], b.hi[k]);
  }
  a.bad += b.bad;
  a.first = min(a.first, b.first);
}
__device__ __forceinline__ VoxBounds vox_bounds_empty() {
  VoxBounds r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = INFINITY;
    r.hi[k] = -INFINITY;
  }
  r.bad = 0ull;
  r.first = VOX_NONE;
  return r;
}
// over the NT threads of the workgroup; the result is valid in thread 0
template <int NT>
__device__ __forceinline__ VoxBounds vox_bounds_reduce(VoxBounds v, VoxBounds* s_wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VoxBounds w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w.lo[k] = __shfl_xor(v.lo[k], o, 64);
      w.hi[k] = __shfl_xor(v.hi[k], o, 64);
    }
    w.bad = __shfl_xor(v.bad, o, 64);
    w.first = __shfl_xor(v.first, o, 64);
    vox_bounds_merge(v, w);
  }
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < NT / 64; ++k) vox_bounds_merge(v, s_wave[k]);
  return v;
}

__global__ __launch_bounds__(256) void vox_bounds_kernel(const double* __restrict__ xyz, int n, VoxBounds* __restrict__ part) {
  __shared__ VoxBounds s_wave[4];
  VoxBounds v = vox_bounds_empty();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (vox_finite(p[0], p[1], p[2])) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v.lo[k] = fmin(v.lo[k], p[k]);
        v.hi[k] = fmax(v.hi[k], p[k]);
      }
    } else {
      ++v.bad;
      v.first = min(v.first, (unsigned long long)i);      // i ascends in a thread: the first hit is its lowest
    }
  }
  v = vox_bounds_reduce<256>(v, s_wave);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one workgroup: part[0:nparts] -> *out
__global__ __launch_bounds__(1024) void vox_bounds_fold_kernel(const VoxBounds* __restrict__ part, int nparts,
                                                               VoxBounds* __restrict__ out) {
  __shared__ VoxBounds s_wave[16];
  VoxBounds v = (int)threadIdx.x < nparts ? part[threadIdx.x] : vox_bounds_empty();
  v = vox_bounds_reduce<1024>(v, s_wave);
  if (threadIdx.x == 0) *out = v;
}

// ---- quantise ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vox_quantize_kernel(const double* __restrict__ xyz, int n, int bits, double ox,
                                                           double oy, double oz, double s, double inv,
                                                           int32_t* __restrict__ q, int64_t* __restrict__ keys,
                                                           int64_t* status) {
  __shared__ double s_sum[4], s_max[4];
  const double top = (double)(1 << bits);
  unsigned long long n_nf = 0ull, n_out = 0ull, first_nf = VOX_NONE, first_out = VOX_NONE;
  double sum = 0.0, mx = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const double v0 = vox_forward(x, ox, inv), v1 = vox_forward(y, oy, inv), v2 = vox_forward(z, oz, inv);
    // float64 decides: a comparison with a NaN is false, so nothing but a value in [0, 2^bits) is ever converted
    const bool inside = v0 >= 0.0 && v0 < top && v1 >= 0.0 && v1 < top && v2 >= 0.0 && v2 < top;
    int q0 = -1, q1 = -1, q2 = -1;
    int64_t key = VOX_BAD_KEY;
    if (!vox_finite(x, y, z)) {
      ++n_nf;
      first_nf = min(first_nf, (unsigned long long)i);
    } else if (!inside) {
      ++n_out;
      first_out = min(first_out, (unsigned long long)i);
    } else {
      q0 = (int)floor(v0);
      q1 = (int)floor(v1);
      q2 = (int)floor(v2);
      key = ((int64_t)q0 << (2 * bits)) | ((int64_t)q1 << bits) | (int64_t)q2;
      const double e2 = vox_err2(x, y, z, vox_inverse(q0, ox, s), vox_inverse(q1, oy, s), vox_inverse(q2, oz, s));
      sum += e2;
      mx = fmax(mx, e2);
    }
    q[3 * i] = q0;
    q[3 * i + 1] = q1;
    q[3 * i + 2] = q2;
    keys[i] = key;
  }
  // the butterfly leaves one value in all 64 lanes: the order of the adds is fixed by the lane numbers
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    mx = fmax(mx, __shfl_xor(mx, o, 64));
    n_nf += __shfl_xor(n_nf, o, 64);
    n_out += __shfl_xor(n_out, o, 64);
    first_nf = min(first_nf, __shfl_xor(first_nf, o, 64));
    first_out = min(first_out, __shfl_xor(first_out, o, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* st = (unsigned long long*)status;
  if (lane == 0) {
    s_sum[wave] = sum;
    s_max[wave] = mx;
    if (n_nf) {
      atomicAdd(&st[VOX_ST_NONFINITE], n_nf);
      atomicMin(&st[VOX_ST_FIRST_NONFINITE], first_nf);
    }
    if (n_out) {
      atomicAdd(&st[VOX_ST_OUTSIDE], n_out);
      atomicMin(&st[VOX_ST_FIRST_OUTSIDE], first_out);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    ((double*)status)[VOX_ST_PARTIALS + blockIdx.x] = total;
    const double m = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    // non-negative doubles order as their bit patterns do
    if (m > 0.0) atomicMax((long long*)&status[VOX_ST_MAX_ERR2], __double_as_longlong(m));
    if (blockIdx.x == 0) status[VOX_ST_GROUPS] = (int64_t)gridDim.x;
  }
}

// ---- unique -----------------------------------------------------------------------------------------------------------
// exclusive prefix sum of one value per thread over the 1024 threads of the workgroup; *total = the sum (pp_scan1024 of
// pp_device.hip, restated: that file is a translation unit of its own)
__device__ __forceinline__ int vox_scan1024(int v, int* s_wave, int* total) {
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

// Workgroup g owns the sorted keys [g span, (g + 1) span), span = 1024 rounds; in round r thread t looks at key
// g span + 1024 r + t, so a wave reads 512 contiguous bytes.  EMIT = false: part[g] = heads of the span.  EMIT = true:
// part[g] = heads before the span; the point of every head goes to its rank and both ends of a run add to its count.
template <bool EMIT>
__global__ __launch_bounds__(1024) void vox_unique_kernel(const int64_t* __restrict__ skeys, int n, int bits, int rounds,
                                                          int32_t* part, int32_t* __restrict__ pts, int32_t* counts) {
  __shared__ int s_wave[16];
  const int64_t base = (int64_t)blockIdx.x * 1024 * rounds;
  const int mask = (1 << bits) - 1;
  int carry = EMIT ? part[blockIdx.x] : 0, heads = 0;
  for (int r = 0; r < rounds; ++r) {            // the same trip count in every thread: the scans' barriers meet
    const int64_t i = base + (int64_t)r * 1024 + threadIdx.x;
    const int64_t key = i < n ? skeys[i] : VOX_BAD_KEY;
    const bool valid = key != VOX_BAD_KEY;      // the rejected points sort last and belong to no run
    const bool head = valid && (i == 0 || skeys[i - 1] != key);
    if (!EMIT) {
      heads += head;
      continue;
    }
    int total;
    const int rank = carry + vox_scan1024(head, s_wave, &total) + (int)head - 1;
    carry += total;
    if (!valid || rank < 0) continue;           // (rank < 0: keys that were not sorted; nothing is written out of bounds)
    const bool tail = i == n - 1 || skeys[i + 1] != key;
    if (head) {
      pts[3 * (size_t)rank] = (int32_t)(key >> (2 * bits)) & mask;
      pts[3 * (size_t)rank + 1] = (int32_t)(key >> bits) & mask;
      pts[3 * (size_t)rank + 2] = (int32_t)key & mask;
    }
    if (head && tail) counts[rank] = 1;
    else if (head) atomicAdd(&counts[rank], -(int)i);
    else if (tail) atomicAdd(&counts[rank], (int)i + 1);
  }
  if (!EMIT) {
    int total;
    vox_scan1024(heads, s_wave, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
  }
}

// one workgroup: part[0:nparts] -> its exclusive prefix sum; the sum is the number of voxels
__global__ __launch_bounds__(1024) void vox_parts_scan_kernel(int32_t* part, int nparts, int64_t* voxels) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  int all;
  const int before = vox_scan1024(t < nparts ? part[t] : 0, s_wave, &all);
  if (t < nparts) part[t] = before;
  if (t == 0) *voxels = (int64_t)all;
}

// ---- dequantise -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vox_dequantize_kernel(const int32_t* __restrict__ q, int n, double ox, double oy,
                                                             double oz, double s, double* __restrict__ xyz) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    xyz[3 * i] = vox_inverse(q[3 * i], ox, s);
    xyz[3 * i + 1] = vox_inverse(q[3 * i + 1], oy, s);
    xyz[3 * i + 2] = vox_inverse(q[3 * i + 2], oz, s);
  }
}

// ---- entry points -----------------------------------------------------------------------------------------------------
static inline bool vox_count_ok(int n) { return n >= 1 && n < (1 << 30); }
static inline bool vox_bits_ok(int bits) { return bits >= 10 && bits <= 12; }
static inline bool vox_step_ok(double s) { return isfinite(s) && s > 0.0; }
static inline bool vox_origin_ok(double ox, double oy, double oz) { return isfinite(ox) && isfinite(oy) && isfinite(oz); }
static inline int vox_groups(int n) { return min((n + 255) / 256, NVF_VOX_MAX_GROUPS); }

static_assert(sizeof(VoxBounds) == 8 * NVF_VOX_BOUNDS_WORDS, "bounds record");
static_assert(sizeof(VoxBounds) * NVF_VOX_MAX_GROUPS == 8 * NVF_VOX_BOUNDS_WORK_WORDS, "bounds work");

extern "C" int nvf_vox_bounds(const double* xyz, int n, int64_t* bounds, int64_t* work, void* stream) {
  if (!xyz || !bounds || !work || !vox_count_ok(n)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  const int groups = vox_groups(n);
  vox_bounds_kernel<<<groups, 256, 0, st>>>(xyz, n, (VoxBounds*)work);
  NVF_LAUNCH_CHECK();
  vox_bounds_fold_kernel<<<1, 1024, 0, st>>>((const VoxBounds*)work, groups, (VoxBounds*)bounds);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_vox_quantize(const double* xyz, int n, int bits, double ox, double oy, double oz, double s, double inv,
                                int32_t* q, int64_t* keys, int64_t* status, void* stream) {
  if (!xyz || !q || !keys || !status || !vox_count_ok(n) || !vox_bits_ok(bits) || !vox_step_ok(s) || !vox_step_ok(inv) ||
      !vox_origin_ok(ox, oy, oz))
    return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  hipError_t e = hipMemsetAsync(status, 0, NVF_VOX_STATUS_WORDS * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(status + VOX_ST_FIRST_NONFINITE, 0xff, 2 * sizeof(int64_t), st);   // -1: none
  if (e != hipSuccess) return (int)e;
  vox_quantize_kernel<<<vox_groups(n), 256, 0, st>>>(xyz, n, bits, ox, oy, oz, s, inv, q, keys, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_vox_unique(const int64_t* sorted_keys, int n, int bits, int32_t* pts, int32_t* counts, int64_t* status,
                              int32_t* work, void* stream) {
  if (!sorted_keys || !pts || !counts || !status || !work || !vox_count_ok(n) || !vox_bits_ok(bits)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  const int rounds = (n + 1024 * NVF_VOX_MAX_GROUPS - 1) / (1024 * NVF_VOX_MAX_GROUPS);
  const int groups = (n + 1024 * rounds - 1) / (1024 * rounds);
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  vox_unique_kernel<false><<<groups, 1024, 0, st>>>(sorted_keys, n, bits, rounds, work, pts, counts);
  NVF_LAUNCH_CHECK();
  vox_parts_scan_kernel<<<1, 1024, 0, st>>>(work, groups, &status[VOX_ST_VOXELS]);
  NVF_LAUNCH_CHECK();
  vox_unique_kernel<true><<<groups, 1024, 0, st>>>(sorted_keys, n, bits, rounds, work, pts, counts);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_vox_dequantize(const int32_t* q, int n, double ox, double oy, double oz, double s, double* xyz,
                                  void* stream) {
  if (!q || !xyz || !vox_count_ok(n) || !vox_step_ok(s) || !vox_origin_ok(ox, oy, oz)) return NVF_EINVAL;
  vox_dequantize_kernel<<<vox_groups(n), 256, 0, nvf_stream(stream)>>>(q, n, ox, oy, oz, s, xyz);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
