// The 4x4x4 convolutions of the WIDE decoder (chanstr 16,32,16,16: conv2 32^3 <-> 35^3, conv1 16^3 <-> 19^3; 16 -> 16
// channels) in the reduced-multiplication form of conv_wino.hip: Winograd F(2x2, 4x4) over (y, x), direct over z.
// Reference site: F.conv3d, utils/network.py:687, and its autograd backward (NVFPCC.py:197).  Training steps only: the
// eval / encode / decode forward keeps the direct fixed-order kernel (conv16_mfma.hip).
//
//   out[o, z, y, x] = sum_c sum_{tz,ty,tx} in[c, z + tz, y + ty, x + tx] w[c][tz,ty,tx][o]     (gather form; `in` zero-padded
//   by PAD).  For the 2 x 2 outputs of tile (R, X) on plane z:
//   out_tile = A^T [ sum_c sum_tz U[f][tz][c][o] * V[f][z + tz][c][tile] ] A,   V = B^T in_tile B,   U = G w_{tz} G^T
//
// Matrix-core mapping (v_mfma_f32_16x16x4_f32): rows = the 16 OUTPUT channels (every lane useful -- no plane pairing as
// in the 8-channel kernel), K = four input channels (four groups), columns = 16 tiles.  The accumulators of one output
// plane are 25 frequencies x 4 registers; two planes (a PAIR 2q, 2q + 1) are in flight -- the 200 accumulation registers --
// and the five input planes 2q .. 2q + 4 of a pair are walked once per pair: plane t feeds tap t of the first and tap
// t - 1 of the second plane of the pair.  (A plane therefore meets 2.5 pairs and is fetched and transformed once for
// each: with 16 x 16 channels a transform of 57 vector instructions feeds up to 50 MFMAs, so the repeated transforms are
// ~20 % on top of the MFMAs, against the 2.56 x fewer MFMAs of the form.)  The lane that owns column j (tile) and K index
// k (channel) transforms the window it feeds; raw planes pass through a per-wave LDS image of EIGHT channels (two phases
// per plane), fetched one phase ahead by 16-byte buffer loads.  U (100 KB: [g][tz][f][lane]) is copied to LDS once per
// workgroup by DMA.  No barrier after the prologue.
#include "wino_conv.h"

constexpr int kWino16AFloats = 4 * 4 * 25 * 64;     // [g][tz][f][lane]

extern "C" size_t nvf_pack_wino16_k4_floats(void) { return (size_t)kWino16AFloats; }

template <int DIN, int PAD>
struct W16Cfg : WinoCfg<DIN, PAD, 8, 4, kWino16AFloats> {};     // an LDS image holds EIGHT channels of one plane

// BIAS (EPI 1 only): also leave the channel sums of what was stored (d.bias_part); a template switch, see WinoEpilogue
template <class C, int EPI, bool BIAS = false>
__global__ __launch_bounds__(256) void conv16_k4_wino(const float* __restrict__ g, const float* __restrict__ wp,
                                                      float* __restrict__ y, const float* __restrict__ mask, WinoDims d) {
  constexpr int DIN = C::DIN, PAD = C::PAD;
  __shared__ __attribute__((aligned(16))) float lds[C::LDS];
  WinoWave<C> w(lds);
  w.zero_image();
  w.decode(lds, d.units, C::NPAIR, d.ppc);
  WinoStage<C, 16> stage(w, g);          // one eight-channel phase per fetch: channels 8 h .. 8 h + 7

  // two accumulator sets = the two output planes of the pair in flight
  f32x4 acc[2][25];
  // one block: the 25 frequencies of (output plane set S, tap TZ, channel group G)
  auto mfma25 = [&](auto slot, auto tzc, auto gi, auto firstc, const float (&V)[25]) {
    constexpr int S = decltype(slot)::value, TZ = decltype(tzc)::value, G = decltype(gi)::value;
    wino_mfma25<decltype(firstc)::value>(acc[S], w.abase + (G * 4 + TZ) * 25 * 64, V);
  };
  // a finished plane: lane holds channels 4 kq + r (r = 0..3) of its tile
  WinoEpilogue<C, EPI, 4, true, BIAS> epi(w, y, mask);

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;
  using Yes = std::true_type;
  using No = std::false_type;
  // blocks of input plane T of a pair: tap T of the pair's first output plane (set 0), tap T - 1 of its second (set 1)
  auto blocks = [&](auto tc, auto gi, const float (&V)[25]) {
    constexpr int T = decltype(tc)::value, G = decltype(gi)::value;
    if constexpr (T <= 3) {
      if constexpr (T == 0 && G == 0) mfma25(I0{}, I0{}, gi, Yes{}, V);
      else mfma25(I0{}, std::integral_constant<int, T>{}, gi, No{}, V);
    }
    if constexpr (T >= 1) {
      if constexpr (T == 1 && G == 0) mfma25(I1{}, I0{}, gi, Yes{}, V);
      else mfma25(I1{}, std::integral_constant<int, (T >= 1 ? T - 1 : 0)>{}, gi, No{}, V);
    }
  };
  // one input plane = two staging phases of eight channels.  The data of phase (T, 0) is in `st` on entry; on exit `st`
  // holds phase (T + 1, 0) -- or the first phase of the next pair
  auto plane = [&](auto tc, int q) {
    constexpr int T = decltype(tc)::value;
    const int p = 2 * q + T;
    const bool pin = p - PAD >= 0 && p - PAD < DIN;      // wave-uniform
    if constexpr (T == 3) epi.mask_fetch(2 * q);
    if constexpr (T == 4) epi.mask_fetch(2 * q + 1);
    float V[25];
    stage.commit();
    stage.fetch(p, 8);
    if (pin) {
      wino_transform<C::RS>(w.win, V); blocks(tc, I0{}, V);
      wino_transform<C::RS>(w.win + 4 * C::CS, V); blocks(tc, I1{}, V);
    } else {
      if constexpr (T == 0) wino_clear(acc[0]);                  // the plane that would have started the set does not exist
      if constexpr (T == 1) wino_clear(acc[1]);
    }
    stage.commit();
    if constexpr (T < 4) stage.fetch(p + 1);
    else if (q + 1 < w.q1) stage.fetch(2 * q + 2);
    if (pin) {
      wino_transform<C::RS>(w.win, V); blocks(tc, I2{}, V);
      wino_transform<C::RS>(w.win + 4 * C::CS, V); blocks(tc, I3{}, V);
    }
  };

  // prologue: the first phase's loads go out before the A fragments are copied
  if (!w.idle) stage.fetch(2 * w.q0);
  wino_copy_a<C>(lds, wp, w.tid, w.wave);
  __syncthreads();
  if (w.idle) {
    if (BIAS && d.bias_part) wino_zero_sums<16>(w, d.bias_part);
    return;
  }
#pragma unroll 1
  for (int q = w.q0; q < w.q1; ++q) {
    plane(I0{}, q);
    plane(I1{}, q);
    plane(I2{}, q);
    plane(I3{}, q);
    epi.emit(acc[0], 2 * q);
    plane(I4{}, q);
    epi.emit(acc[1], 2 * q + 1);
  }
  if (BIAS && d.bias_part) epi.store_sums(w, d.bias_part);
}

template <class C, int EPI>
static int launch_wino16(const float* x, const float* wp, float* y, const float* aux, int batch, int ppc, float* bias_part,
                         int* bias_nparts, hipStream_t s) {
  if (ppc <= 0) return NVF_EINVAL;
  const int nchunk = (C::NPAIR + ppc - 1) / ppc;
  WinoDims d{batch, batch * nchunk * C::NCG, ppc, 0, bias_part};
  const int grid = ((d.units + 3) / 4 + 7) / 8 * 8;      // a multiple of the 8 XCDs (idle waves write zero partials)
  if (bias_nparts) *bias_nparts = grid * 4;
  if (EPI == 1 && bias_part) conv16_k4_wino<C, EPI, EPI == 1><<<grid, 256, 0, s>>>(x, wp, y, aux, d);
  else conv16_k4_wino<C, EPI, false><<<grid, 256, 0, s>>>(x, wp, y, aux, d);
  return NVF_OK;
}

// conv16_wino1.hip: ppc OUTPUT PLANES per work unit (0 = that kernel's default)
int nvf_wino16_1_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, hipStream_t s);
int nvf_wino16_1_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s);

// dx[b, ci, :] = relu-mask( sum_co conv_full(dy[b, co], w) ): backward-data of a valid 4^3 convolution with 16 -> 16
// channels through the ReLU of the layer below.  dy [batch, 16, din^3] (din = 32: conv2, 16: conv1), dx / mask
// [batch, 16, (din + 3)^3]; wp = nvf_pack_mfma_all kind 41 of the layer's w_bwd (nvf_pack_wino16_k4_floats() floats).
// ppc: include/nvf_hip.h, wino_ppc() -- the two-plane kernel of this file has no debug switches and takes every bit below
// bit 16 as its count of pairs.  bias_part (optional): *bias_nparts slabs of 16 channel sums of dx (the bias gradient of the
// layer below; a jtotal = 16 job of nvf_wgrad_reduce_multi*).  NVF_EINVAL for shapes without an instantiation.
// conv2's backward-data (din 32) without bias sums runs, by default, the kernel with one output plane in flight and two waves
// per SIMD (conv16_wino1.hip: the same bits, 140 -> 133 us at batch 16, 534 -> 479 at 64; the forward is faster in the
// two-plane kernel of this file: 88 vs 100 us); a caller that wants the two-plane kernel there as well names a count.
extern "C" int nvf_conv3d_k4_wino16_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int din,
                                        int ppc, float* bias_part, int* bias_nparts, void* stream) {
  if (!dy || !wp || !dx || !mask || batch <= 0 || ppc < 0 || (bias_part && !bias_nparts)) return NVF_EINVAL;
  hipStream_t s = nvf_stream(stream);
  const bool has_one = din == 32 && !bias_part;       // the one-plane kernel's only backward instantiation
  const WinoPpc p = wino_ppc(ppc, has_one);
  int rc = NVF_EINVAL;
  if (p.one) {
    if (has_one) rc = nvf_wino16_1_bwd(dy, wp, dx, mask, batch, p.count, s);
  } else if (din == 32) {
    rc = launch_wino16<W16Cfg<32, 3>, 1>(dy, wp, dx, mask, batch, ppc ? ppc : 6, bias_part, bias_nparts, s);
  } else if (din == 16) {
    rc = launch_wino16<W16Cfg<16, 3>, 1>(dy, wp, dx, mask, batch, ppc ? ppc : 1, bias_part, bias_nparts, s);
  }
  return wino_launched(rc);
}

// y = relu(conv3d(x, w) + bias): the FORWARD pass of the same layers in the Winograd form -- for training steps only.
// x [batch, 16, din^3] (din = 35: conv2, 19: conv1), y [batch, 16, (din - 3)^3]; wp = kind 41 of the layer's w_fwd.
extern "C" int nvf_conv3d_k4_wino16_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int din,
                                        int ppc, void* stream) {
  if (!x || !wp || !bias || !y || batch <= 0 || ppc < 0) return NVF_EINVAL;
  hipStream_t s = nvf_stream(stream);
  const WinoPpc p = wino_ppc(ppc, false);
  int rc = NVF_EINVAL;
  if (p.one) {
    if (din == 35) rc = nvf_wino16_1_fwd(x, wp, bias, y, batch, p.count, s);
  } else if (din == 35) {
    rc = launch_wino16<W16Cfg<35, 0>, 0>(x, wp, y, bias, batch, ppc ? ppc : 4, nullptr, nullptr, s);
  } else if (din == 19) {
    rc = launch_wino16<W16Cfg<19, 0>, 0>(x, wp, y, bias, batch, ppc ? ppc : 1, nullptr, nullptr, s);
  }
  return wino_launched(rc);
}
