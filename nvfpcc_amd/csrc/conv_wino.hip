// Backward-data (and the training-step forward) of the 4x4x4 convolutions (conv2: 32^3 <-> 35^3, conv1: 16^3 <-> 19^3;
// 8 -> 8 channels) in a reduced-multiplication form: Winograd F(2x2, 4x4) over (y, x), direct over z with the pair trick of conv_mfma.hip.
// Reference site: F.conv3d in mode 'train' and its autograd backward, utils/network.py:687 (NVFPCC.py:160, 197).  Training
// steps only: the eval / encode / decode forward keeps the direct fixed-order form (bit-exact batch invariance, the 2e-6
// occupancy contract).
//
//   out[ci, z, y, x] = sum_co sum_{tz,ty,tx} g[co, z + tz, y + ty, x + tx] w'[co][tz,ty,tx][ci]        (gather form: g is
//   the zero-padded output gradient, w' = w_bwd, the flipped kernel).  For the 2 x 2 outputs of tile (R, X) on plane z:
//
//   out_tile = A^T [ sum_co sum_tz U[f][tz][co][ci] * V[f][z + tz][co][tile] ] A,     f = (fy, fx) in 5 x 5
//   V = B^T g_tile B  (5 x 5 window at (2R, 2X)),   U = G w'_{tz} G^T  (packed once per step: nvf_pack kind 40)
//
// with the Cook-Toom matrices on {0, 1, -1, 2, inf}, the rational factors moved into G so that B^T is small integers:
// 25 products per 2 x 2 outputs and tz instead of 64 -- 2.56 x fewer multiplications.  fp32 error against fp64:
// 1.0e-6 of max |out| (direct form 6.0e-7; tools/winograd_probe.py, /tmp-probe in DESIGN section 12).
//
// Matrix-core mapping (v_mfma_f32_16x16x4_f32): rows (ci, s) = two output planes z = 2q + s of a PAIR q, columns = 16
// tiles, K = four gradient channels; a plane p = 2q + zw (zw = 0..4) feeds pair q with A[(ci,s)][co] = U[f][zw - s][co][ci]
// (zero where zw - s is no tap: 4/5 of every MFMA useful).  The B operand of lane (tile j, co kq) is V[f] of ITS tile
// and channel, so the transformed data never leaves the registers of the lane that computed it: raw 5 x 5 windows are
// read from the wave's own LDS image of the plane (flattened tiles: 16 consecutive tiles of the 18 x 18 tile plane; row
// stride 50 = 18 (mod 32) makes the window reads of 16 tiles x 2 channels conflict-free 8-byte reads), transformed by
// 57 vector instructions per (plane, channel group) (wino_common.h) and multiplied into up to three live pairs (75 MFMAs).  A
// wave walks a chunk of pairs down z with TWO accumulator sets (25 frequencies x 4 registers each; the plane that completes a
// pair is multiplied into its set first, the pair is emitted, and the same set starts the next pair); a finished pair goes
// through the inverse transform in registers and leaves as 8-byte stores behind the ReLU mask.  (conv_wino1.hip is the
// one-set, two-waves-per-SIMD form of the same arithmetic and the default for conv2 and conv1's backward-data.)  Planes are fetched one
// ahead with 16-byte buffer loads (8 rows per instruction) held in registers and committed to LDS after the current
// plane's reads; no barrier after the prologue -- waves share only the A fragments (64 KB of LDS per workgroup).
#include "wino_conv.h"

constexpr int kWinoAFloats = 2 * 5 * 25 * 64;     // [g][zw][f][lane]

#ifndef NVF_WINO_DBG
#define NVF_WINO_DBG 0        // tuning builds (tools/ab_build.py .. -DNVF_WINO_DBG=1): WinoDims::dbg switches phases off.  In the
#endif                        // regular build the switches are compiled out (as run-time tests they cost 150 moves per step)
// d.dbg (ppc >> 8), tuning runs only: 1 no MFMAs, 2 no emit, 4 no transform, 8 no staging, 16 no A copy, 32 no zero fill;
// results meaningless
#define WDBG(bit) (NVF_WINO_DBG && (d.dbg & (bit)))

extern "C" size_t nvf_pack_wino_k4_floats(void) { return (size_t)kWinoAFloats; }

template <int DIN, int PAD>                      // (a type of its own: the kernels keep their names in profiles)
struct WCfg : WinoCfg<DIN, PAD, 8, 4, kWinoAFloats> {};

template <class C, int EPI>
__global__ __launch_bounds__(256) void conv_k4_wino(const float* __restrict__ g, const float* __restrict__ wp,
                                                    float* __restrict__ y, const float* __restrict__ mask, WinoDims d) {
  constexpr int DIN = C::DIN, PAD = C::PAD;
  __shared__ __attribute__((aligned(16))) float lds[C::LDS];
  WinoWave<C> w(lds);
  if (!WDBG(32)) w.zero_image();
  w.decode(lds, d.units, C::NPAIR, d.ppc);
  WinoStage<C, 8> stage(w, g);
  auto fetch = [&](int p) { if (!WDBG(8)) stage.fetch(p); };
  auto commit = [&]() { if (!WDBG(8)) stage.commit(); };

  // two accumulator sets: pair q lives in set q & 1 (25 frequencies x 4 registers); the matrix cores' accumulators are
  // the AGPR half of the register file, which 3 x 100 would overflow -- so the plane that completes pair s - 2 (tap 4)
  // is multiplied into that set FIRST, the pair is emitted, and the same set then starts pair s with the same V
  f32x4 acc[2][25];
  wino_clear(acc[0]);
  wino_clear(acc[1]);

  // V = B^T (5 x 5 window of channel 4 gi + kq) B
  auto transform = [&](auto gi, float (&V)[25]) {
    if (WDBG(4)) {
#pragma unroll
      for (int f = 0; f < 25; ++f) V[f] = 1.f + f;
      return;
    }
    wino_transform<C::RS>(w.win + decltype(gi)::value * 4 * C::CS, V);
  };
  auto mfma25 = [&](auto slot, auto zwc, auto gi, const float (&V)[25]) {
    constexpr int S = decltype(slot)::value, ZW = decltype(zwc)::value, G = decltype(gi)::value;
    if (!WDBG(1)) wino_mfma25<ZW == 0 && G == 0>(acc[S], w.abase + (G * 5 + ZW) * 25 * 64, V);
  };
  WinoEpilogue<C, EPI, 2, true, true> epi(w, y, mask);
  auto emit = [&](auto slot, int q) { if (!WDBG(2)) epi.emit(acc[decltype(slot)::value], q); };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;
  // one pair step: planes 2s (taps 4 / 0 / 2 of pairs s-2, s, s-1) and 2s + 1 (taps 1 / 3 of pairs s, s-1); SA = set of s
  auto step = [&](auto sa, int s) -> bool {
    constexpr int SA = decltype(sa)::value;
    using A = std::integral_constant<int, SA>;
    using B = std::integral_constant<int, 1 - SA>;
    const bool hA = s < w.q1, hB = s - 1 >= w.q0 && s - 1 < w.q1, hC = s - 2 >= w.q0;
    const bool last = s == w.q1 + 1;
    if (hC) epi.mask_fetch(s - 2);
    if (!last) fetch(2 * s + 1);
    const bool pin = 2 * s - PAD >= 0 && 2 * s - PAD < DIN;
    float V0[25], V1[25];
    if (pin) {
      transform(I0{}, V0);
      transform(I1{}, V1);
      if (hC) { mfma25(A{}, I4{}, I0{}, V0); mfma25(A{}, I4{}, I1{}, V1); }
    }
    if (hC) emit(A{}, s - 2);
    if (pin) {
      if (hA) { mfma25(A{}, I0{}, I0{}, V0); mfma25(A{}, I0{}, I1{}, V1); }
      if (hB) { mfma25(B{}, I2{}, I0{}, V0); mfma25(B{}, I2{}, I1{}, V1); }
    }
    if (last) return false;
    commit();
    fetch(2 * s + 2);
    if (2 * s + 1 - PAD >= 0 && 2 * s + 1 - PAD < DIN) {
      transform(I0{}, V0);
      if (hA) mfma25(A{}, I1{}, I0{}, V0);
      if (hB) mfma25(B{}, I3{}, I0{}, V0);
      transform(I1{}, V1);
      if (hA) mfma25(A{}, I1{}, I1{}, V1);
      if (hB) mfma25(B{}, I3{}, I1{}, V1);
    }
    commit();
    return true;
  };
  // prologue: the first plane's loads go out BEFORE the A fragments are copied, so that their latency (HBM on a cold
  // tile) passes under the 64 KB copy instead of after it
  if (!w.idle) fetch(2 * w.q0);
  if (!WDBG(16)) wino_copy_a<C>(lds, wp, w.tid, w.wave);
  __syncthreads();
  if (w.idle) {
    if (d.bias_part) wino_zero_sums<8>(w, d.bias_part);
    return;
  }
  commit();
  int s = w.q0;                                       // q0 is even (ppc is): the set of pair q is q & 1
#pragma unroll 1
  for (;;) {
    s = __builtin_amdgcn_readfirstlane(s);
    if (!step(I0{}, s++)) break;
    if (!step(I1{}, s++)) break;
  }
  if (d.bias_part) epi.store_sums(w, d.bias_part);
}

// p.count pairs per work unit, `dflt` when the caller names none
template <class C, int EPI>
static int launch_wino(const float* x, const float* wp, float* y, const float* aux, int batch, WinoPpc p, int dflt,
                       float* bias_part, int* bias_nparts, hipStream_t s) {
  const int ppc = p.count ? p.count : dflt;
  if (ppc & 1) return NVF_EINVAL;       // chunks start at even pairs (two alternating accumulator sets)
  const int nchunk = (C::NPAIR + ppc - 1) / ppc;
  WinoDims d{batch, batch * nchunk * C::NCG, ppc, p.dbg, bias_part};
  const int grid = ((d.units + 3) / 4 + 7) / 8 * 8;      // a multiple of the 8 XCDs (idle workgroups write zero partials)
  if (bias_nparts) *bias_nparts = grid * 4;
  conv_k4_wino<C, EPI><<<grid, 256, 0, s>>>(x, wp, y, aux, d);
  return NVF_OK;
}

// conv_wino1.hip: p.count pairs per work unit (0 = that kernel's default)
int nvf_wino1_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, float* bias_part,
                  int* bias_nparts, hipStream_t s);
int nvf_wino1_bwd16(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, float* bias_part,
                    int* bias_nparts, hipStream_t s);
int nvf_wino1_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s);
int nvf_wino1_fwd19(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s);

// dx[b, ci, :] = relu-mask( sum_co conv_full(dy[b, co], w) ): backward-data of a valid 4^3 convolution with 8 -> 8 channels
// through the ReLU of the layer below.  dy [batch, 8, din^3] (din = 32: conv2, 16: conv1), dx / mask [batch, 8, (din + 3)^3];
// wp = nvf_pack_mfma_all kind 40 of the layer's w_bwd (nvf_pack_wino_k4_floats() floats).  bias_part (optional):
// *bias_nparts slabs of 8 channel sums of dx (the bias gradient of the layer below).  ppc: include/nvf_hip.h, wino_ppc().
// NVF_EINVAL for shapes without an instantiation.
// Both shapes run, by default, the one-accumulator-set kernel with two waves per SIMD (conv_wino1.hip: the same bits, conv2
// 44.1 -> 42.8 us in the step, conv1 18.8 -> 16.7 us); a caller that wants the two-set kernel of this file names a count.
extern "C" int nvf_conv3d_k4_wino_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int din,
                                      int ppc, float* bias_part, int* bias_nparts, void* stream) {
  if (!dy || !wp || !dx || !mask || batch <= 0 || (bias_part && !bias_nparts)) return NVF_EINVAL;
  hipStream_t s = nvf_stream(stream);
  const WinoPpc p = wino_ppc(ppc, din == 32 || din == 16);
  int rc = NVF_EINVAL;
  if (p.one) {
    if (din == 32) rc = nvf_wino1_bwd(dy, wp, dx, mask, batch, p.count, bias_part, bias_nparts, s);
    else if (din == 16) rc = nvf_wino1_bwd16(dy, wp, dx, mask, batch, p.count, bias_part, bias_nparts, s);
  } else if (din == 32) {
    rc = launch_wino<WCfg<32, 3>, 1>(dy, wp, dx, mask, batch, p, 6, bias_part, bias_nparts, s);
  } else if (din == 16) {
    rc = launch_wino<WCfg<16, 3>, 1>(dy, wp, dx, mask, batch, p, 2, bias_part, bias_nparts, s);
  }
  return wino_launched(rc);
}

// y = relu(conv3d(x, w) + bias): the FORWARD pass of the same layers in the Winograd form -- for training steps only (its
// results differ from the direct fixed-order kernel by fp32 rounding, 1e-6 of max |y|: the eval / encode / decode forward,
// whose occupancy must be batch-invariant bit for bit, never uses it).  x [batch, 8, din^3] (din = 35: conv2, 19: conv1),
// y [batch, 8, (din - 3)^3]; wp = kind 40 of the layer's w_fwd.  conv2's forward runs the one-set kernel by default
// (31.3 -> 30.4 us), conv1's the two-set kernel.
extern "C" int nvf_conv3d_k4_wino_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int din,
                                      int ppc, void* stream) {
  if (!x || !wp || !bias || !y || batch <= 0) return NVF_EINVAL;
  hipStream_t s = nvf_stream(stream);
  const WinoPpc p = wino_ppc(ppc, din == 35);
  int rc = NVF_EINVAL;
  if (p.one) {
    if (din == 35) rc = nvf_wino1_fwd(x, wp, bias, y, batch, p.count, s);
    else if (din == 19) rc = nvf_wino1_fwd19(x, wp, bias, y, batch, p.count, s);
  } else if (din == 35) {
    rc = launch_wino<WCfg<35, 0>, 0>(x, wp, y, bias, batch, p, 4, nullptr, nullptr, s);
  } else if (din == 19) {
    rc = launch_wino<WCfg<19, 0>, 0>(x, wp, y, bias, batch, p, 2, nullptr, nullptr, s);
  }
  return wino_launched(rc);
}
