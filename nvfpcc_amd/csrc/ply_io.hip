// ASCII PLY bodies on the device: text -> int32 coordinates and int32 coordinates -> text (the Python side is
// nvfpcc_amd/ply_io.py, the ABI include/nvf_hip.h "PLY text").  Headers stay on the host; so does binary PLY.
//
// Text to integers, three launches around one device scan:
//   nvf_ply_count_lines   one wave per chunk of `chunk` bytes counts its '\n' (a ballot per 64 bytes).
//   nvf_ply_line_starts   the same walk again with the number of '\n' before the chunk (the caller's exclusive scan of
//                         the counts): the '\n' at byte p that has k '\n' before it ends line k, so line k + 1 starts at
//                         p + 1.  Line 0 starts at 0.  A line that ends the text without '\n' is a line like any other.
//   nvf_ply_parse_xyz     one thread per vertex line walks the bytes of its line once.  Tokens are maximal runs of bytes
//                         other than space, tab, CR, LF; the tokens of the three coordinate columns must match
//                         [+-]?[0-9]{1,10}(\.0*)? with a magnitude of at most 2^31 - 1, the others are skipped.  A line
//                         with fewer tokens than properties, and a line that is not in the text at all (its start is
//                         negative or >= nbytes), is SHORT; a coordinate token outside the grammar makes the line
//                         FOREIGN, and so does a byte that a host reader might take for a line break or a separator
//                         where this walk does not (a control byte other than tab / LF / CR-before-LF, or a byte >= 0x7f):
//                         the caller hands such a file to the host reader.  Counts and lowest indices of both kinds go
//                         to `status` through atomics on global memory (rare events).
//
// Integers to text:
//   nvf_ply_format_sizes  bytes of "%d %d %d\n" per point.
//   nvf_ply_format_xyz    a workgroup formats its 256 lines into LDS, at the 16-byte phase its text has in global memory,
//                         and stores the text in 16-byte pieces (single bytes at the two ragged ends).
//
// Bounds.  No kernel reads at or beyond text + nbytes or writes at or beyond text + nbytes, whatever the bytes, the
// line starts or the offsets say: every index that comes from memory is range-checked before it is used.
// Indices of lines, vertices and chunks live in grid dimension x only (2^31 - 1 workgroups), as 64-bit values.
#include "nvf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLineMax = 36;                          // 3 * 11 characters ("-2147483648"), two spaces, '\n'
constexpr int kFmtBytes = kThreads * kLineMax;        // text of one workgroup's points
constexpr unsigned long long kMaxMag = 2147483647ull;

// ---- lines ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ply_count_lines_kernel(const unsigned char* __restrict__ text, int64_t nbytes,
                                                                   int64_t chunk, int64_t nchunks,
                                                                   int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const int64_t lo = c * chunk, hi = min(lo + chunk, nbytes);
  int64_t cnt = 0;
  for (int64_t p = lo; p < hi; p += 64) {             // wave-uniform bounds
    const int64_t q = p + lane;
    cnt += __popcll(__ballot(q < hi && text[q] == '\n'));
  }
  if (lane == 0) counts[c] = cnt;
}

__global__ __launch_bounds__(kThreads) void ply_line_starts_kernel(const unsigned char* __restrict__ text, int64_t nbytes,
                                                                   int64_t chunk, int64_t nchunks,
                                                                   const int64_t* __restrict__ chunk_first,
                                                                   int64_t* __restrict__ starts, int64_t nlines) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const int64_t lo = c * chunk, hi = min(lo + chunk, nbytes);
  int64_t before = chunk_first[c];                    // '\n' before this chunk
  if (c == 0 && lane == 0 && nlines > 0) starts[0] = 0;
  for (int64_t p = lo; p < hi; p += 64) {
    const int64_t q = p + lane;
    const bool nl = q < hi && text[q] == '\n';
    const unsigned long long m = __ballot(nl);
    const int64_t line = before + __popcll(m & ((1ull << lane) - 1ull)) + 1;      // the line this '\n' opens
    if (nl && line >= 1 && line < nlines) starts[line] = q + 1;
    before += __popcll(m);
  }
}

// ---- parse ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ply_parse_xyz_kernel(const unsigned char* __restrict__ text, int64_t nbytes,
                                                                 const int64_t* __restrict__ starts, int64_t first_line,
                                                                 int64_t n, int nprops, int cx, int cy, int cz,
                                                                 int32_t* __restrict__ xyz,
                                                                 unsigned long long* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int64_t p = starts[first_line + i];
  int32_t out[3] = {0, 0, 0};
  int tokens = 0;
  bool foreign = false;
  if (p < 0) p = nbytes;                              // a line the text does not have: no tokens
  // state of the token under the cursor: kind 0 = between tokens, 1 = a skipped column, 2 = sign or digits of a
  // coordinate, 3 = its zeros after the point, 4 = a coordinate that has left the grammar
  int kind = 0, axis = 0, digits = 0;
  bool neg = false;
  unsigned long long mag = 0;
  for (;; ++p) {
    const int ch = p < nbytes ? text[p] : '\n';       // the end of the text ends the line
    const bool cr_eol = ch == '\r' && (p + 1 >= nbytes || text[p + 1] == '\n');
    const bool space = ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n';
    if ((ch < 0x20 && ch != '\t' && ch != '\n' && !cr_eol) || ch >= 0x7f) foreign = true;
    if (space) {
      if (kind >= 2) {                                // a coordinate token ends here
        if (kind == 4 || digits < 1 || digits > 10 || mag > kMaxMag) foreign = true;
        else out[axis] = neg ? -(int32_t)mag : (int32_t)mag;
      }
      kind = 0;
      if (ch == '\n') break;
      continue;
    }
    if (kind == 0) {                                  // a token starts
      const int col = tokens++;
      kind = 1;
      if (col < nprops && (col == cx || col == cy || col == cz)) {
        kind = 2; axis = col == cx ? 0 : (col == cy ? 1 : 2); digits = 0; neg = false; mag = 0;
        if (ch == '+' || ch == '-') { neg = ch == '-'; continue; }
      }
    }
    if (kind == 2) {
      if (ch >= '0' && ch <= '9') { if (++digits <= 10) mag = mag * 10 + (unsigned)(ch - '0'); }
      else if (ch == '.' && digits >= 1) kind = 3;
      else kind = 4;
    } else if (kind == 3) {
      if (ch != '0') kind = 4;
    }
  }
  xyz[3 * i] = out[0]; xyz[3 * i + 1] = out[1]; xyz[3 * i + 2] = out[2];
  if (tokens < nprops) {
    atomicAdd(status + 0, 1ull);
    atomicMin(status + 2, (unsigned long long)i);
  }
  if (foreign) {
    atomicAdd(status + 1, 1ull);
    atomicMin(status + 3, (unsigned long long)i);
  }
}

// ---- format ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t magnitude(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

__device__ __forceinline__ int dec_digits(uint32_t m) {
  int d = 1;
  d += m >= 10u; d += m >= 100u; d += m >= 1000u; d += m >= 10000u; d += m >= 100000u; d += m >= 1000000u;
  d += m >= 10000000u; d += m >= 100000000u; d += m >= 1000000000u;
  return d;
}

__device__ __forceinline__ int field_bytes(int32_t v) { return dec_digits(magnitude(v)) + (v < 0 ? 1 : 0); }

// writes v and the byte `after` at dst -> the next free byte
__device__ __forceinline__ unsigned char* put_field(unsigned char* dst, int32_t v, unsigned char after) {
  uint32_t m = magnitude(v);
  const int d = dec_digits(m);
  if (v < 0) *dst++ = '-';
  for (int k = d - 1; k >= 0; --k) { dst[k] = (unsigned char)('0' + m % 10u); m /= 10u; }
  dst[d] = after;
  return dst + d + 1;
}

__global__ __launch_bounds__(kThreads) void ply_format_sizes_kernel(const int32_t* __restrict__ xyz, int64_t n,
                                                                    int32_t* __restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  sizes[i] = field_bytes(xyz[3 * i]) + field_bytes(xyz[3 * i + 1]) + field_bytes(xyz[3 * i + 2]) + 3;
}

__global__ __launch_bounds__(kThreads) void ply_format_xyz_kernel(const int32_t* __restrict__ xyz,
                                                                  const int64_t* __restrict__ offsets, int64_t n,
                                                                  unsigned char* __restrict__ text, int64_t nbytes) {
  __shared__ __attribute__((aligned(16))) unsigned char buf[kFmtBytes + 16];
  const int64_t i0 = (int64_t)blockIdx.x * kThreads;
  const int cnt = (int)min((int64_t)kThreads, n - i0);
  const int64_t base = offsets[i0];
  // the workgroup's text is text[base .. base + len); inconsistent offsets shrink it, they never widen it
  int64_t len = offsets[i0 + cnt] - base;
  if (base < 0 || base >= nbytes || len < 0) len = 0;
  len = min(min(len, (int64_t)kFmtBytes), nbytes - max(base, (int64_t)0));
  const int phase = (int)((uintptr_t)(text + base) & 15);   // LDS byte phase + j <-> text[base + j]
  const int t = threadIdx.x;
  if (t < cnt) {
    const int64_t i = i0 + t;
    const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const int size = field_bytes(x) + field_bytes(y) + field_bytes(z) + 3;
    const int64_t rel = offsets[i] - base;
    if (rel >= 0 && rel + size <= len) {
      unsigned char* d = buf + phase + rel;
      d = put_field(d, x, ' ');
      d = put_field(d, y, ' ');
      put_field(d, z, '\n');
    }
  }
  __syncthreads();
  if (len <= 0) return;
  unsigned char* g0 = text + base - phase;                  // 16-byte aligned; piece k is g0[16 k .. 16 k + 16)
  const int lo = phase, hi = phase + (int)len;              // the live bytes of buf
  for (int k = t; 16 * k < hi; k += kThreads) {
    const int b = 16 * k;
    if (b >= lo && b + 16 <= hi) {
      *(uint4*)(g0 + b) = *(const uint4*)(buf + b);
    } else {
      for (int j = max(b, lo); j < min(b + 16, hi); ++j) g0[j] = buf[j];
    }
  }
}

inline bool fits_grid(int64_t blocks) { return blocks >= 1 && blocks <= 0x7fffffffll; }

}  // namespace

extern "C" int nvf_ply_count_lines(const uint8_t* text, int64_t nbytes, int64_t chunk, int64_t* counts, void* stream) {
  if (!text || !counts || nbytes < 0 || chunk < 1) return NVF_EINVAL;
  if (nbytes == 0) return NVF_OK;
  const int64_t nchunks = (nbytes + chunk - 1) / chunk, blocks = (nchunks + kWaves - 1) / kWaves;
  if (!fits_grid(blocks)) return NVF_EINVAL;
  ply_count_lines_kernel<<<(unsigned)blocks, kThreads, 0, nvf_stream(stream)>>>(text, nbytes, chunk, nchunks, counts);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_ply_line_starts(const uint8_t* text, int64_t nbytes, int64_t chunk, const int64_t* chunk_first,
                                   int64_t* starts, int64_t nlines, void* stream) {
  if (!text || !chunk_first || !starts || nbytes < 0 || chunk < 1 || nlines < 0) return NVF_EINVAL;
  if (nbytes == 0 || nlines == 0) return NVF_OK;
  const int64_t nchunks = (nbytes + chunk - 1) / chunk, blocks = (nchunks + kWaves - 1) / kWaves;
  if (!fits_grid(blocks)) return NVF_EINVAL;
  ply_line_starts_kernel<<<(unsigned)blocks, kThreads, 0, nvf_stream(stream)>>>(text, nbytes, chunk, nchunks, chunk_first,
                                                                                starts, nlines);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_ply_parse_xyz(const uint8_t* text, int64_t nbytes, const int64_t* starts, int64_t first_line, int64_t n,
                                 int nprops, int cx, int cy, int cz, int32_t* xyz, int64_t* status, void* stream) {
  if (!text || !starts || !xyz || !status || nbytes < 0 || first_line < 0 || n < 0 || nprops < 3) return NVF_EINVAL;
  if (cx < 0 || cy < 0 || cz < 0 || cx >= nprops || cy >= nprops || cz >= nprops || cx == cy || cy == cz || cx == cz)
    return NVF_EINVAL;
  if (n == 0) return NVF_OK;
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  if (!fits_grid(blocks)) return NVF_EINVAL;
  hipStream_t st = nvf_stream(stream);
  // counts 0, lowest indices "none" (all bits set: -1 as the int64 the caller reads, the greatest value for atomicMin)
  hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(status + 2, 0xff, 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  ply_parse_xyz_kernel<<<(unsigned)blocks, kThreads, 0, st>>>(text, nbytes, starts, first_line, n, nprops, cx, cy, cz, xyz,
                                                              (unsigned long long*)status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_ply_format_sizes(const int32_t* xyz, int64_t n, int32_t* sizes, void* stream) {
  if (!xyz || !sizes || n < 0) return NVF_EINVAL;
  if (n == 0) return NVF_OK;
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  if (!fits_grid(blocks)) return NVF_EINVAL;
  ply_format_sizes_kernel<<<(unsigned)blocks, kThreads, 0, nvf_stream(stream)>>>(xyz, n, sizes);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_ply_format_xyz(const int32_t* xyz, const int64_t* offsets, int64_t n, uint8_t* text, int64_t nbytes,
                                  void* stream) {
  if (!xyz || !offsets || !text || n < 0 || nbytes < 0) return NVF_EINVAL;
  if (n == 0 || nbytes == 0) return NVF_OK;
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  if (!fits_grid(blocks)) return NVF_EINVAL;
  ply_format_xyz_kernel<<<(unsigned)blocks, kThreads, 0, nvf_stream(stream)>>>(xyz, offsets, n, text, nbytes);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
