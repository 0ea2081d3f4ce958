// What the four Winograd (y, x) convolution kernels share (conv_wino.hip, conv_wino1.hip: 8 -> 8 channels; conv16_wino.hip,
// conv16_wino1.hip: 16 -> 16): the tile / LDS geometry, the work-unit mapping, the staging of raw planes through a per-wave
// LDS image, the window transform, the 25-MFMA block, the DMA copy of the A fragments and the epilogue.  A kernel file keeps
// its accumulator sets and its SCHEDULE -- which plane feeds which set, and when a set is emitted -- and calls these pieces.
// Everything here is force-inlined and takes accumulators and staging registers by reference to a caller's local: the
// kernels sit close to their register limits (245 of 256 VGPRs at two waves per SIMD), and their machine code is checked
// against the previous build's instruction by instruction ("Checking a refactor of the Winograd kernels").
#pragma once
#include "wino_common.h"
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wino_u4 __attribute__((ext_vector_type(4)));
typedef unsigned wino_u2 __attribute__((ext_vector_type(2)));

constexpr int kWinoOob = 0x7ffffff0;        // an offset beyond every buffer descriptor: loads read 0, stores do nothing

// ---- the `ppc` argument of nvf_conv3d_k4_wino_* / nvf_conv3d_k4_wino16_* (include/nvf_hip.h) --------------------------------
constexpr int kWinoPpcCount = 0xff;         // bits 0-7: pairs (one-plane wide kernel: planes) per work unit, 0 = the default
constexpr int kWinoPpcDbgShift = 8;         // bits 8-15: WinoDims::dbg of NVF_WINO_DBG builds (conv_wino.hip), else ignored
constexpr int kWinoPpcOne = 1 << 16;        // bit 16: the one-set (narrow) / one-plane (wide) kernel
struct WinoPpc {
  int count, dbg;
  bool one;
};
// `one_by_default`: the shape runs the one-set / one-plane kernel when the caller names neither a count nor that kernel
static inline WinoPpc wino_ppc(int ppc, bool one_by_default) {
  const bool one = (ppc & kWinoPpcOne) || (one_by_default && (ppc & kWinoPpcCount) == 0);
  return WinoPpc{ppc & kWinoPpcCount, ppc >> kWinoPpcDbgShift, one};
}
// the tail of every entry point
static inline int wino_launched(int rc) {
  if (rc != NVF_OK) return rc;
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

struct WinoDims {
  int batch, units, ppc;        // work units = (block, z chunk, column group); ppc pairs (or planes) per chunk
  int dbg;                      // conv_wino.hip's tuning builds only
  float* bias_part;             // optional: per unit the channel sums of what it stored
};

// DIN: input extent; PAD: zero padding of the gather (3: backward-data = full correlation of the output gradient, 0: the
// forward pass); output extent DIN + 2 PAD - 3.  The kernels work in PADDED input coordinates p = input index + PAD.
// CH: channels of one staged LDS image (per wave); NWAVE: waves per workgroup; AFLOATS: the A fragments in front of the images.
template <int DIN_, int PAD_, int CH_, int NWAVE_, int AFLOATS_>
struct WinoCfg {
  static constexpr int DIN = DIN_, PAD = PAD_, CH = CH_, NWAVE = NWAVE_, AFLOATS = AFLOATS_;
  static constexpr int DOUT = DIN_ + 2 * PAD_ - 3, TPR = (DOUT + 1) / 2, NTILE = TPR * TPR;
  static constexpr int NCG = (NTILE + 15) / 16, NPAIR = TPR;
  // tile rows a group of 16 consecutive flattened tiles can touch: 16 | 16 tiles per row: 1; 8: 2; 18: 2; 10: 3
  static constexpr int SPAN = TPR % 16 == 0 ? 1 : (16 % TPR == 0 ? 16 / TPR : (14 + TPR) / TPR + 1);
  static constexpr int NR = 2 * SPAN + 3;                 // raw rows staged per plane and channel
  static constexpr int SEGS = (DIN + 3) / 4, RPI = 64 / SEGS, NROW = CH * NR, NLD = (NROW + RPI - 1) / RPI;
  static constexpr int rs_for() {
    int r = 2 * TPR + 4 > PAD + 4 * SEGS ? 2 * TPR + 4 : PAD + 4 * SEGS;
    while (r % 32 != TPR % 32) ++r;
    return r;
  }
  static constexpr int RS = rs_for();                     // 2 RS = 2 TPR (mod 64): window address linear in the tile index
  static constexpr int cs_for() { int c = NR * RS; while (c % 64 != 32) ++c; return c; }
  static constexpr int CS = cs_for();                     // the second channel of a 32-lane read group: banks + 32
  static constexpr int BUF = CH * CS, LDS = AFLOATS + NWAVE * BUF;
  static_assert(RS % 2 == 0 && CS % 2 == 0, "8-byte window reads");
  static_assert(LDS * 4 <= 160 * 1024, "LDS");
};

// ---- a wave's work unit: (block b, z chunk [q0, q1), column group cg); lane (j, kq) owns tile (R, X) and K index kq -----------
template <class C>
struct WinoWave {
  int tid, lane, wave, j, kq, unit_, unit, b, q0, q1, R, X, R0;
  bool idle, tvalid;            // idle: a wave past the last unit (zero partials, no work)
  float* raw;                   // the wave's own LDS image of a plane
  const float *win, *abase;     // this lane's window in the image; this lane's column of the A fragments

  __device__ __forceinline__ explicit WinoWave(float* lds) {
    tid = threadIdx.x, lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    raw = lds + C::AFLOATS + wave * C::BUF;
  }
  __device__ __forceinline__ void zero_image() const {     // the margins stay zero for the whole launch
    for (int i = lane; i < C::BUF; i += 64) raw[i] = 0.f;
  }
  // `count` planes or pairs along z in chunks of `ppc`
  __device__ __forceinline__ void decode(float* lds, int units, int count, int ppc) {
    // XCD k (workgroups k, k + 8, ...) takes a CONTIGUOUS range of work units: neighbouring column groups and z chunks of a
    // block share input rows / planes, and each XCD has its own L2 (round-robin units made every XCD fetch every block)
    const int per = (int)(gridDim.x >> 3);                         // the grid is a multiple of 8
    const int wg = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    unit_ = __builtin_amdgcn_readfirstlane(wg * C::NWAVE + wave);
    j = lane & 15, kq = lane >> 4;
    idle = unit_ >= units;
    unit = idle ? 0 : unit_;
    const int nchunk = (count + ppc - 1) / ppc;
    const int cg = unit % C::NCG, zc = (unit / C::NCG) % nchunk;
    b = unit / (C::NCG * nchunk);
    q0 = zc * ppc, q1 = min(q0 + ppc, count);
    const int tl = 16 * cg + j;
    tvalid = tl < C::NTILE;
    const int t = tvalid ? tl : C::NTILE - 1;
    R = t / C::TPR, X = t % C::TPR, R0 = (16 * cg) / C::TPR;
    win = raw + 2 * (R - R0) * C::RS + 2 * X + kq * C::CS;
    abase = lds + lane;
  }
};

// ---- staging: a plane of C::CH channels, 16-byte buffer loads held in registers (fetch) and written to the image (commit) ----
template <class C, int NCH>                // NCH: channels of the tensor
struct WinoStage {
  static constexpr int DIN = C::DIN, PAD = C::PAD, NLD = C::NLD;
  int voff[NLD], ldst[NLD];
  __amdgpu_buffer_rsrc_t rsrc;
  wino_u4 st[NLD];
  float* raw;

  // staging descriptors: load k covers rows (k RPI + lane / SEGS) of the (channel, row) list, 16 bytes per lane
  __device__ __forceinline__ WinoStage(const WinoWave<C>& w, const float* g) {
    const int lane = w.lane, R0 = w.R0;
    raw = w.raw;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int ri = k * C::RPI + lane / C::SEGS, seg = lane % C::SEGS;
      const int co = ri / C::NR, row = ri % C::NR, yd = 2 * R0 + row - PAD;
      const bool live = ri < C::NROW && lane < C::RPI * C::SEGS;
      const bool ok = live && yd >= 0 && yd < DIN;
      voff[k] = ok ? ((co * DIN * DIN + yd) * DIN + 4 * seg) * 4 : kWinoOob;        // beyond the descriptor: reads 0
      ldst[k] = live ? co * C::CS + row * C::RS + PAD + 4 * seg : -1;
    }
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(g + (size_t)w.b * NCH * DIN * DIN * DIN), 0, NCH * DIN * DIN * DIN * 4,
                                             0x00020000);
  }
  // plane p (padded coordinate), channels c0 .. c0 + C::CH - 1.
  // (unconditional loads: a plane outside the tensor takes the out-of-range offset in every lane and reads zeros -- a
  // branch here makes the loaded registers a phi, which the compiler resolves with a wait right behind the loads; the
  // plane offset is forced into an SGPR or every load becomes a waterfall loop)
  __device__ __forceinline__ void fetch(int p, int c0 = 0) {
    const int pz = p - PAD;
    const bool pin = pz >= 0 && pz < DIN;
    const int so = __builtin_amdgcn_readfirstlane(pin ? ((c0 * DIN + pz) * DIN * DIN) * 4 : 0);
#pragma unroll
    for (int k = 0; k < NLD; ++k) st[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, pin ? voff[k] : kWinoOob, so, 0);
  }
  __device__ __forceinline__ void commit() const {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      if (ldst[k] < 0) continue;
      float* o = raw + ldst[k];
      if constexpr (PAD & 1) {                                    // odd word: 4 + 8 + 4 bytes
        o[0] = __uint_as_float(st[k].x);
        *(float2*)(o + 1) = float2{__uint_as_float(st[k].y), __uint_as_float(st[k].z)};
        o[3] = __uint_as_float(st[k].w);
      } else {                                                    // (a row's last segment may run one word past the
        *(float2*)o = float2{__uint_as_float(st[k].x), __uint_as_float(st[k].y)};       // row: no window reads it)
        *(float2*)(o + 2) = float2{__uint_as_float(st[k].z), __uint_as_float(st[k].w)};
      }
    }
  }
};

// V = B^T (5 x 5 window at p, row stride RS) B: the y pass on the packed pipe -- the window's x pairs (0,1) and (2,3) are the
// 8-byte LDS reads themselves -- then the x pass row by row (wino_common.h): 57 vector instructions
template <int RS>
__device__ __forceinline__ void wino_transform(const float* p, float (&V)[25]) {
  wino_f2 a[5], bb[5], ea[5], eb[5];
  float c[5], ec[5];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    a[dy] = *(const wino_f2*)(p + dy * RS);
    bb[dy] = *(const wino_f2*)(p + dy * RS + 2);
    c[dy] = p[dy * RS + 4];
  }
  wino_bt2(a[0], a[1], a[2], a[3], a[4], ea[0], ea[1], ea[2], ea[3], ea[4]);
  wino_bt2(bb[0], bb[1], bb[2], bb[3], bb[4], eb[0], eb[1], eb[2], eb[3], eb[4]);
  wino_bt(c[0], c[1], c[2], c[3], c[4], ec[0], ec[1], ec[2], ec[3], ec[4]);
#pragma unroll
  for (int fy = 0; fy < 5; ++fy)
    wino_bt_row(ea[fy], eb[fy], ec[fy], V[5 * fy], V[5 * fy + 1], V[5 * fy + 2], V[5 * fy + 3], V[5 * fy + 4]);
}

// one block: the 25 frequencies of one (accumulator set, tap, channel group); ap = this lane's column of that block's A
// fragments.  FIRST: the first block of a set starts from zero (no clearing pass)
template <bool FIRST>
__device__ __forceinline__ void wino_mfma25(f32x4 (&acc)[25], const float* ap, const float (&V)[25]) {
  __builtin_amdgcn_sched_barrier(0);        // keeps the A reads of other (set, tap) blocks out of this one: registers
#pragma unroll
  for (int f = 0; f < 25; ++f)
    acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[f * 64], V[f], FIRST ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[f], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void wino_clear(f32x4 (&acc)[25]) {
#pragma unroll
  for (int f = 0; f < 25; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the A fragments, L2 -> LDS by DMA (1 KB per wave instruction, no registers)
template <class C>
__device__ __forceinline__ void wino_copy_a(float* lds, const float* wp, int tid, int wave) {
  constexpr int NT = C::NWAVE * 64, NV = C::AFLOATS / 4, NI = (NV + NT - 1) / NT;
  typedef __attribute__((address_space(3))) void* lds_vp;
  typedef const __attribute__((address_space(1))) void* glb_vp;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i * NT + tid < NV)
      __builtin_amdgcn_global_load_lds((glb_vp)(wp + (size_t)(i * NT + tid) * 4), (lds_vp)(lds + (i * NT + wave * 64) * 4), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- a finished accumulator set: A^T M A per row, ReLU mask or bias, stores, channel sums ---------------------------------------
// EPI 1: y = mask > 0 ? acc : 0 (backward-data through the ReLU of the layer below; `mask` = that layer's output)
// EPI 0: y = relu(acc + bias[channel])  (forward; `mask` = the biases)
// CPL (channels per lane) is the row mapping of the MFMA: 2 -- rows (channel 2 kq + (r >> 1), plane 2 zq + (r & 1)) of PAIR zq
// (the 8-channel kernels); 4 -- rows = channels 4 kq + r of PLANE zq (the 16-channel kernels).  ZEDGE: zq may name a plane
// beyond the tensor.  BIAS: keep the channel sums of what was stored (a masked-out or out-of-range output is 0 and adds
// nothing) -- a switch because the adds cost the wide backward-data kernel 2-3 us whether anyone reads the sums or not.
// Mask / output addressing goes through buffer descriptors (out-of-range lanes read 0 and store nothing: no divergent
// branches): the lane part of the offset per output row yo; the (channel, plane) part is scalar.
template <class C, int EPI, int CPL, bool ZEDGE, bool BIAS>
struct WinoEpilogue {
  static constexpr int DOUT = C::DOUT, NCH = 4 * CPL;
  size_t cstride;
  __amdgpu_buffer_rsrc_t rs_m, rs_y;
  float bias[CPL], bsum[CPL];                             // EPI 0: the biases of this lane's channels
  bool full;                                              // the tile's second x output exists
  int vo[2], vs64[2], vs32[2];
  wino_u2 mk[8];                                          // the ReLU mask of the set being finished, fetched a plane ahead

  __device__ __forceinline__ WinoEpilogue(const WinoWave<C>& w, float* y, const float* mask) {
    const int b = w.b, kq = w.kq, R = w.R, X = w.X;
    const bool tvalid = w.tvalid;
    cstride = (size_t)DOUT * DOUT * DOUT;
    rs_m = __builtin_amdgcn_make_buffer_rsrc((void*)(EPI == 1 ? mask + (size_t)b * NCH * cstride : mask), 0,
                                             EPI == 1 ? (int)(NCH * cstride * 4) : NCH * 4, 0x00020000);
#pragma unroll
    for (int h = 0; h < CPL; ++h) bias[h] = 0.f, bsum[h] = 0.f;
    if constexpr (EPI == 0) {
#pragma unroll
      for (int h = 0; h < CPL; ++h) bias[h] = mask[CPL * kq + h];
    }
    rs_y = __builtin_amdgcn_make_buffer_rsrc((void*)(y + (size_t)b * NCH * cstride), 0, (int)(NCH * cstride * 4), 0x00020000);
    full = 2 * X + 1 < DOUT;
#pragma unroll
    for (int yo = 0; yo < 2; ++yo) {
      const bool ok = tvalid && 2 * R + yo < DOUT;
      const int o = (int)(((size_t)(CPL * kq) * cstride + (size_t)(2 * R + yo) * DOUT + 2 * X) * 4);
      vo[yo] = ok ? o : kWinoOob;
      vs64[yo] = ok && full ? o : kWinoOob;
      vs32[yo] = ok && !full ? o : kWinoOob;
    }
  }
  static __device__ __forceinline__ int chan(int r) { return CPL == 2 ? r >> 1 : r; }
  static __device__ __forceinline__ int plane(int r, int zq) { return CPL == 2 ? 2 * zq + (r & 1) : zq; }
  // the scalar (channel, plane) part of row r's offset; zin (wave-uniform): the plane exists
  __device__ __forceinline__ int row_offset(int r, int zq, bool zin) const {
    return __builtin_amdgcn_readfirstlane(zin ? (int)(((size_t)chan(r) * cstride + (size_t)plane(r, zq) * DOUT * DOUT) * 4) : 0);
  }
  __device__ __forceinline__ void mask_fetch(int zq) {
    if constexpr (EPI != 1) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool zin = !ZEDGE || plane(r, zq) < DOUT;
      const int so = row_offset(r, zq, zin);
#pragma unroll
      for (int yo = 0; yo < 2; ++yo) mk[2 * r + yo] = __builtin_amdgcn_raw_buffer_load_b64(rs_m, zin ? vo[yo] : kWinoOob, so, 0);
    }
  }
  __device__ __forceinline__ void emit(const f32x4 (&acc)[25], int zq) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float c[2][5];
#pragma unroll
      for (int fx = 0; fx < 5; ++fx) {
        const float m0 = acc[fx][r], m1 = acc[5 + fx][r], m2 = acc[10 + fx][r], m3 = acc[15 + fx][r], m4 = acc[20 + fx][r];
        c[0][fx] = (m0 + m1) + (m2 + m3);
        c[1][fx] = (m1 - m2) + fmaf(2.f, m3, m4);
      }
      const bool zin = !ZEDGE || plane(r, zq) < DOUT;
      const int so = row_offset(r, zq, zin);
#pragma unroll
      for (int yo = 0; yo < 2; ++yo) {
        float o0 = (c[yo][0] + c[yo][1]) + (c[yo][2] + c[yo][3]);
        float o1 = (c[yo][1] - c[yo][2]) + fmaf(2.f, c[yo][3], c[yo][4]);
        if constexpr (EPI == 1) {
          const wino_u2 m = mk[2 * r + yo];
          o0 = __uint_as_float(m.x) > 0.f ? o0 : 0.f;
          o1 = (full && __uint_as_float(m.y) > 0.f) ? o1 : 0.f;
        } else {
          o0 = fmaxf(o0 + bias[chan(r)], 0.f);
          o1 = fmaxf(o1 + bias[chan(r)], 0.f);
        }
        // (a plane beyond the tensor: its mask was read as zeros, so o0 = o1 = 0; the stores take the out-of-range offset)
        __builtin_amdgcn_raw_buffer_store_b64(wino_u2{__float_as_uint(o0), __float_as_uint(o1)}, rs_y, zin ? vs64[yo] : kWinoOob, so, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o0), rs_y, zin ? vs32[yo] : kWinoOob, so, 0);
        if constexpr (BIAS) bsum[chan(r)] += o0 + o1;
      }
    }
  }
  // the unit's channel sums (the bias gradient of the layer below): a 16-lane shuffle reduction over the unit's tiles
  __device__ __forceinline__ void store_sums(const WinoWave<C>& w, float* bias_part) const {
#pragma unroll
    for (int h = 0; h < CPL; ++h) {
      float v = bsum[h];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (w.j == 0) bias_part[(size_t)w.unit * NCH + CPL * w.kq + h] = v;
    }
  }
};
// an idle wave's sums
template <int NCH, class C>
__device__ __forceinline__ void wino_zero_sums(const WinoWave<C>& w, float* bias_part) {
  if (w.j == 0) {
#pragma unroll
    for (int h = 0; h < NCH / 4; ++h) bias_part[(size_t)w.unit_ * NCH + NCH / 4 * w.kq + h] = 0.f;
  }
}
