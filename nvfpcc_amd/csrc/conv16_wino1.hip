// conv16_wino.hip's Winograd (y, x) convolution for the wide decoder (16 -> 16 channels) with ONE output plane in flight
// per wave (100 accumulation registers) and two waves per SIMD -- the step conv_wino1.hip takes for the narrow decoder:
// an output plane reads its four input planes, each staged and transformed one channel GROUP at a time (a per-wave LDS image
// of four channels: eight waves fit beside the 100 KB of U), 25 MFMAs per (tap, group).  A plane is transformed for each of
// the four output planes it meets instead of 2.5 pairs, at half the price per vector instruction.  Per output the sum has
// conv16_k4_wino's order -- taps 0..3, groups 0..3 -- so the results are the same bits.
#include "wino_conv.h"

constexpr int kWino161AFloats = 4 * 4 * 25 * 64;     // [g][tz][f][lane] (pack kind 41)

template <int DIN, int PAD>
struct W161Cfg : WinoCfg<DIN, PAD, 4, 8, kWino161AFloats> {};   // an LDS image holds FOUR channels of one plane

// d.ppc: OUTPUT PLANES per chunk; no channel sums (d.bias_part is not read)
template <class C, int EPI>
__global__ __launch_bounds__(512, 2) void conv16_k4_wino1(const float* __restrict__ g, const float* __restrict__ wp,
                                                          float* __restrict__ y, const float* __restrict__ mask, WinoDims d) {
  constexpr int DIN = C::DIN, PAD = C::PAD;
  __shared__ __attribute__((aligned(16))) float lds[C::LDS];
  WinoWave<C> w(lds);
  w.zero_image();
  w.decode(lds, d.units, C::DOUT, d.ppc);             // q0, q1: the chunk's output PLANES
  WinoStage<C, 16> stage(w, g);
  f32x4 acc[25];
  WinoEpilogue<C, EPI, 4, false, false> epi(w, y, mask);
  // one staging phase = (input plane z + T, channel group G): its data is in `stage.st` on entry, the next phase's on exit
  auto phase = [&](auto tc, auto gc, int z) {
    constexpr int T = decltype(tc)::value, G = decltype(gc)::value;
    const int p = z + T;
    const bool pin = p - PAD >= 0 && p - PAD < DIN;      // wave-uniform
    if constexpr (T == 3 && G == 0) epi.mask_fetch(z);
    stage.commit();
    if constexpr (G < 3) stage.fetch(p, 4 * (G + 1));
    else if constexpr (T < 3) stage.fetch(p + 1);
    else if (z + 1 < w.q1) stage.fetch(z + 1);
    if (pin) {
      float V[25];
      wino_transform<C::RS>(w.win, V);
      wino_mfma25<T == 0 && G == 0>(acc, w.abase + (G * 4 + T) * 25 * 64, V);
    } else if constexpr (T == 0 && G == 0) {
      wino_clear(acc);
    }
  };
  if (!w.idle) stage.fetch(w.q0);
  wino_copy_a<C>(lds, wp, w.tid, w.wave);
  __syncthreads();
  if (w.idle) return;

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
#pragma unroll 1
  for (int z = w.q0; z < w.q1; ++z) {
    phase(I0{}, I0{}, z); phase(I0{}, I1{}, z); phase(I0{}, I2{}, z); phase(I0{}, I3{}, z);
    phase(I1{}, I0{}, z); phase(I1{}, I1{}, z); phase(I1{}, I2{}, z); phase(I1{}, I3{}, z);
    phase(I2{}, I0{}, z); phase(I2{}, I1{}, z); phase(I2{}, I2{}, z); phase(I2{}, I3{}, z);
    phase(I3{}, I0{}, z); phase(I3{}, I1{}, z); phase(I3{}, I2{}, z); phase(I3{}, I3{}, z);
    epi.emit(acc, z);
  }
}

template <class C, int EPI>
static int launch_wino161(const float* x, const float* wp, float* y, const float* aux, int batch, int ppc, hipStream_t s) {
  if (ppc <= 0) return NVF_EINVAL;
  const int nchunk = (C::DOUT + ppc - 1) / ppc;
  WinoDims d{batch, batch * nchunk * C::NCG, ppc, 0, nullptr};
  const int grid = ((d.units + C::NWAVE - 1) / C::NWAVE + 7) / 8 * 8;
  conv16_k4_wino1<C, EPI><<<grid, 512, 0, s>>>(x, wp, y, aux, d);
  return NVF_OK;
}

// called by nvf_conv3d_k4_wino16_bwd / _fwd (conv16_wino.hip) for conv2's shapes; ppc = output planes per work unit
int nvf_wino16_1_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, hipStream_t s) {
  return launch_wino161<W161Cfg<32, 3>, 1>(dy, wp, dx, mask, batch, ppc ? ppc : 6, s);
}
int nvf_wino16_1_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s) {
  return launch_wino161<W161Cfg<35, 0>, 0>(x, wp, y, bias, batch, ppc ? ppc : 4, s);
}
