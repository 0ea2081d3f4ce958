// The forward of a one-channel classifier head (Conv3d(C -> 1, k = 3, padding 1)): the kernels that write the
// probabilities (heads.hip) and the kernel that turns them into occupancy bits without storing them (lod_points.hip)
// run this one body, so every voxel's logit is the same chain of fmaf in both.
#pragma once
#include "nvf_common.h"
#include "step_ctx.h"      // what stem_bwd.h builds on
#include "stem_bwd.h"      // nvf_coop_signal

// Six consecutive words x-1 .. x+4 of a staged row for the thread that owns x .. x+3 (xg = its float4 group, threads of
// a row are consecutive lanes): ONE aligned ds_read_b128; the two halo words come from the neighbour lanes by DPP (the
// row ends are the zero padding).  Scalar LDS reads at a lane stride of four words would hit 8 of the 32 banks.
typedef float hf4 __attribute__((ext_vector_type(4)));
template <int XG>
__device__ __forceinline__ void head_row6(const float* row, int xg, float (&v)[6]) {
  const hf4 m = *(const hf4*)(row + 4);
  const int left = __builtin_amdgcn_update_dpp(0, __float_as_int(m.w), 0x111, 0xf, 0xf, true);    // row_shr:1
  const int right = __builtin_amdgcn_update_dpp(0, __float_as_int(m.x), 0x101, 0xf, 0xf, true);   // row_shl:1
  v[0] = xg == 0 ? 0.f : __int_as_float(left);
  v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w;
  v[5] = xg == XG - 1 ? 0.f : __int_as_float(right);
}

// ---- forward, channel-pipelined: the tile of ONE input channel (with its y / z halo rows; the x halo comes from the
// neighbour lanes, head_row6) is staged by LDS-DMA into one of two buffers while the previous channel's 27 taps are
// being accumulated.  A workgroup needs 8-20 KB of LDS instead of the whole C-channel tile (61-102 KB), so up to
// eight of them share a CU and one's staging overlaps another's arithmetic; tiles are TZ x TY = 4 x 8 / 8 x 8 whatever
// C is.  Rows are S words apart (a wave reads 1 KB of consecutive LDS per ds_read_b128, a DMA instruction fills two
// rows); rows outside the tensor are zeroed once.  Per output the fmaf order is (c, kz, ky, kx) as before.
template <int C_, int S_, int TZ_, int TY_, int CPS_ = 1>
struct HPCfg {
  static constexpr int C = C_, S = S_, TZ = TZ_, TY = TY_, CPS = CPS_;   // CPS channels per pipeline step (small tiles:
  static_assert(C % CPS == 0, "whole steps");                            //  a step costs ~1 us of latency whatever its size)
  static constexpr int XG = S / 4, IZ = TZ + 2, IY = TY + 2;
  static constexpr int WORDS = IZ * IY * S;            // one channel's tile
  static constexpr int NACT = TZ * TY * XG;            // one thread per four outputs
  static constexpr int NT = 256, NW = 4;
  static constexpr int NIT = (WORDS + NT - 1) / NT;    // (dword DMA instructions per wave per channel: no longer used)
  static_assert(S % 4 == 0 && NACT <= NT && NACT % 64 == 0 && WORDS % 4 == 0, "tile");
};
template <class H>
struct HFwdSmem { static constexpr int WORDS = 2 * H::CPS * H::WORDS + H::C * 9 * 4; };

// 16-byte device-scope accesses (sc1: the store goes through to memory, the load never hits a stale line of this XCD's
// L2) for values that cross workgroups INSIDE a launch (heads3_fwd_loss_bwd_data_kernel).  The compiler does not track an
// asm load: the caller waits (nvf_wait_dev4) before it touches the registers.
constexpr int kHeadFlagStride = 64;     // words between two counters: 256 B, so the pollers of different blocks hit different lines
#ifndef NVF_HC_SLEEP
#define NVF_HC_SLEEP 32                 // s_sleep argument of a polling consumer (x 64 cycles)
#endif

#ifndef NVF_HC_DBG
#define NVF_HC_DBG 0     // tuning builds (wrong results): 1 = plain stores / loads, 2 = consumers do not wait, 4 = no signal
#endif
__device__ __forceinline__ void nvf_store_dev4(float* p, hf4 v) {
  if (NVF_HC_DBG & 1) { *(hf4*)p = v; return; }
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void nvf_load_dev4_issue(hf4& v, const float* p) {
  if (NVF_HC_DBG & 1) { asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(p) : "memory"); return; }
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(v) : "v"(p) : "memory");
}
template <int N>
__device__ __forceinline__ void nvf_wait_dev4(hf4 (&v)[N]) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));      // (ordered behind the wait: volatile asms keep their order)
}

// COOP (the forward inside the launch that also runs the loss and the backward-data): p leaves with device-scope stores
// and the workgroup signals done[b] -- every thread reaches the signal, so no early return.
// SINK (lod_points.hip): instead of storing anything, the active threads hand their four sums to
// sink(acc, b, z, y, x) -- block, and the voxel of acc[0]; acc[o] is the logit of (z, y, x + o) before the bias.
struct HeadStoreP {};
template <class H, bool COOP = false, class SINK = HeadStoreP>
__device__ __forceinline__ void head_fwd_body(const float* __restrict__ x, const float* __restrict__ w,
                                              const float* __restrict__ bias, float* __restrict__ y,
                                              const float* __restrict__ addend, const float* __restrict__ mask, int act,
                                              int bid, float* smem, unsigned* done = nullptr, SINK sink = SINK()) {
  constexpr int C = H::C, S = H::S, TZ = H::TZ, TY = H::TY, IY = H::IY, XG = H::XG, NT = H::NT, NIT = H::NIT,
                WORDS = H::WORDS, CPS = H::CPS;
  float* xs = smem;
  float* ws = smem + 2 * CPS * WORDS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int TILES_Y = S / TY, TILES_Z = S / TZ;
  const int tile = bid % (TILES_Y * TILES_Z), b = bid / (TILES_Y * TILES_Z);
  const int y0 = (tile % TILES_Y) * TY, z0 = (tile / TILES_Y) * TZ;
  for (int i = tid; i < C * 9 * 4; i += NT) ws[i] = (i & 3) < 3 ? w[(i >> 2) * 3 + (i & 3)] : 0.f;
  // which 16-byte piece of a channel volume each of this lane's DMA instructions fetches (the same for every channel).
  // global_load_lds_dwordx4: a wave-instruction moves 1 KiB (64 lanes x 16 B, LDS destination = wave base + 16 lane); the
  // tile image is rows of S words with nothing between them, so 64 consecutive pieces are 64 consecutive LDS quadwords;
  // the per-lane SOURCE follows the (z, y) of the piece's row.  (The dword form was four times the instructions: the
  // DMA issue rate, not its latency, bound this kernel.)
  constexpr int NPC = WORDS / 4, NI4 = (NPC + NT - 1) / NT;       // pieces per channel tile, instructions per wave
  unsigned soff[NI4];
  bool sok[NI4];
#pragma unroll
  for (int i = 0; i < NI4; ++i) {
    const int pc = i * NT + tid, wd = 4 * pc;
    const int r = wd / S, xx = wd - r * S, yi = r % IY, zi = r / IY;
    const int gz = z0 - 1 + zi, gy = y0 - 1 + yi;
    const bool live = pc < NPC;
    sok[i] = live && gz >= 0 && gz < S && gy >= 0 && gy < S;
    soff[i] = sok[i] ? (unsigned)((gz * S + gy) * S + xx) : 0u;
    if (live && !sok[i]) {
#pragma unroll
      for (int q = 0; q < 2 * CPS; ++q) *(float4*)(xs + q * WORDS + wd) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float* xb = x + (size_t)b * C * S * S * S;
  typedef __attribute__((address_space(3))) void* lds_vp;
  typedef const __attribute__((address_space(1))) void* glb_vp;
  auto stage = [&](int step, int buf) {
#pragma unroll
    for (int cc = 0; cc < CPS; ++cc) {
      const float* src = xb + (size_t)(step * CPS + cc) * S * S * S;
#pragma unroll
      for (int i = 0; i < NI4; ++i) {
        // wave-uniform LDS base of this instruction's 64 pieces
        float* dst = xs + (buf * CPS + cc) * WORDS + (i * NT + wave * 64) * 4;
        if (sok[i]) __builtin_amdgcn_global_load_lds((glb_vp)(src + soff[i]), (lds_vp)dst, 16, 0, 0);
      }
    }
  };
  stage(0, 0);
  const bool active = tid < H::NACT;
  const int xg = tid % XG, ty = (tid / XG) % TY, tz = tid / (XG * TY);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int step = 0; step < C / CPS; ++step) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // this wave's share of the step has landed
    __syncthreads();                                              // ... everyone's; the other buffer is free
    if (step + 1 < C / CPS) stage(step + 1, (step + 1) & 1);
    if (active) {
#pragma unroll 1
      for (int cc = 0; cc < CPS; ++cc) {
        const int c = step * CPS + cc;
        const float* xc = xs + ((step & 1) * CPS + cc) * WORDS;
#pragma unroll
        for (int kz = 0; kz < 3; ++kz)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const float* row = xc + ((tz + kz) * IY + ty + ky) * S + 4 * xg - 4;     // head_row6 reads row + 4
            float v[6];
            head_row6<XG>(row, xg, v);
            const float4 wv = *(const float4*)(ws + (c * 9 + kz * 3 + ky) * 4);
            const float wk[3] = {wv.x, wv.y, wv.z};
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
              for (int o = 0; o < 4; ++o) acc[o] = fmaf(v[o + kx], wk[kx], acc[o]);
          }
      }
    }
  }
  if constexpr (!__is_same(SINK, HeadStoreP)) {
    if (active) sink(acc, b, z0 + tz, y0 + ty, 4 * xg);
    return;
  }
  if (COOP) {
    if (active) {
      const float bv = bias ? bias[0] : 0.f;
      const size_t off = (((size_t)b * S + z0 + tz) * S + y0 + ty) * S + 4 * xg;
      nvf_store_dev4(y + off, hf4{nvf_act(acc[0] + bv, act), nvf_act(acc[1] + bv, act), nvf_act(acc[2] + bv, act),
                                  nvf_act(acc[3] + bv, act)});
    }
    if (!(NVF_HC_DBG & 4)) nvf_coop_signal(done + b * kHeadFlagStride);
    return;
  }
  if (!active) return;
  const float bv = bias ? bias[0] : 0.f;
  const size_t off = (((size_t)b * S + z0 + tz) * S + y0 + ty) * S + 4 * xg;
  float o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = nvf_act(acc[i] + bv, act);
  if (addend) {
    const float4 a = *(const float4*)(addend + off);
    o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
  }
  if (mask) {
    const float4 m = *(const float4*)(mask + off);
    o[0] = m.x > 0.f ? o[0] : 0.f; o[1] = m.y > 0.f ? o[1] : 0.f;
    o[2] = m.z > 0.f ? o[2] : 0.f; o[3] = m.w > 0.f ? o[3] : 0.f;
  }
  *(float4*)(y + off) = make_float4(o[0], o[1], o[2], o[3]);
}
