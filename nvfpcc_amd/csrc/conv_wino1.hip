// conv_wino.hip's Winograd (y, x) convolution (conv2: 8 -> 8 channels, 32^3 <-> 35^3) with ONE accumulator set per wave and
// two waves per SIMD: a wave finishes one pair of output planes at a time from its five input planes (each plane is fetched
// and transformed for the 2.5 pairs it meets, as in conv16_wino.hip), which halves the accumulation registers (100) so that
// eight waves share a CU -- vector instructions then cost ~2.5 instead of ~5.3 cycles each (profiles/r04_mfma_valu_overlap.md)
// and one wave's LDS / memory latencies pass under the other's MFMAs.  The order of every output's sum -- taps zw = 0..4,
// channel group 0 then 1 -- is the two-set kernel's: the results are the same BITS (tests/test_gpu_ops.py).  With the 57-
// instruction transforms of wino_common.h the repeated transforms cost less than the cheaper issue returns: conv2
// backward-data 44.1 -> 42.8 us, forward 31.3 -> 30.4 us in the step (with the 115-instruction transforms the same idea --
// the "team" variant of DESIGN.md section 12(c) -- lost 15 %).  Default for conv2 (nvf_conv3d_k4_wino_*, ppc 0) and for conv1's
// backward-data (its 10 x 10 tiles need 13 KB of LDS per wave: six waves per workgroup fit beside the A fragments, not eight).
#include "wino_conv.h"

constexpr int kWino1AFloats = 2 * 5 * 25 * 64;     // [g][zw][f][lane] (pack kind 40)

template <int DIN, int PAD, int NWAVE = 8>
struct W1Cfg : WinoCfg<DIN, PAD, 8, NWAVE, kWino1AFloats> {};

template <class C, int EPI>
__global__ __launch_bounds__(C::NWAVE * 64, 2) void conv_k4_wino1(const float* __restrict__ g, const float* __restrict__ wp,
                                                        float* __restrict__ y, const float* __restrict__ mask, WinoDims d) {
  constexpr int DIN = C::DIN, PAD = C::PAD;
  __shared__ __attribute__((aligned(16))) float lds[C::LDS];
  WinoWave<C> w(lds);
  w.zero_image();
  w.decode(lds, d.units, C::NPAIR, d.ppc);
  WinoStage<C, 8> stage(w, g);
  f32x4 acc[25];
  WinoEpilogue<C, EPI, 2, true, true> epi(w, y, mask);
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // input plane T of pair q feeds tap zw = T of the pair's row pairs (ci, s); G: the channel group of V
  auto block = [&](auto tc, auto gi, const float (&V)[25]) {
    constexpr int T = decltype(tc)::value, G = decltype(gi)::value;
    wino_mfma25<T == 0 && G == 0>(acc, w.abase + (G * 5 + T) * 25 * 64, V);
  };
  auto plane = [&](auto tc, int q) {
    constexpr int T = decltype(tc)::value;
    const int p = 2 * q + T;
    const bool pin = p - PAD >= 0 && p - PAD < DIN;
    if constexpr (T == 3) epi.mask_fetch(q);
    float V[25];
    stage.commit();
    if constexpr (T < 4) stage.fetch(p + 1);
    else if (q + 1 < w.q1) stage.fetch(2 * q + 2);
    if (pin) {
      wino_transform<C::RS>(w.win, V);
      block(tc, I0{}, V);
      wino_transform<C::RS>(w.win + 4 * C::CS, V);
      block(tc, I1{}, V);
    } else if constexpr (T == 0) {
      wino_clear(acc);
    }
  };
  if (!w.idle) stage.fetch(2 * w.q0);
  wino_copy_a<C>(lds, wp, w.tid, w.wave);
  __syncthreads();
  if (w.idle) {
    if (d.bias_part) wino_zero_sums<8>(w, d.bias_part);
    return;
  }
#pragma unroll 1
  for (int q = w.q0; q < w.q1; ++q) {
    plane(std::integral_constant<int, 0>{}, q);
    plane(std::integral_constant<int, 1>{}, q);
    plane(std::integral_constant<int, 2>{}, q);
    plane(std::integral_constant<int, 3>{}, q);
    plane(std::integral_constant<int, 4>{}, q);
    epi.emit(acc, q);
  }
  if (d.bias_part) epi.store_sums(w, d.bias_part);
}

template <class C, int EPI>
static int launch_wino1(const float* x, const float* wp, float* y, const float* aux, int batch, int ppc, float* bias_part,
                        int* bias_nparts, hipStream_t s) {
  if (ppc <= 0) return NVF_EINVAL;
  const int nchunk = (C::NPAIR + ppc - 1) / ppc;
  WinoDims d{batch, batch * nchunk * C::NCG, ppc, 0, bias_part};
  const int grid = ((d.units + C::NWAVE - 1) / C::NWAVE + 7) / 8 * 8;
  if (bias_nparts) *bias_nparts = grid * C::NWAVE;
  conv_k4_wino1<C, EPI><<<grid, C::NWAVE * 64, 0, s>>>(x, wp, y, aux, d);
  return NVF_OK;
}

// called by nvf_conv3d_k4_wino_bwd / _fwd (conv_wino.hip): the shape's default, or bit 16 of ppc; ppc = pairs per work unit
int nvf_wino1_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, float* bias_part,
                  int* bias_nparts, hipStream_t s) {
  return launch_wino1<W1Cfg<32, 3>, 1>(dy, wp, dx, mask, batch, ppc ? ppc : 3, bias_part, bias_nparts, s);
}
int nvf_wino1_bwd16(const float* dy, const float* wp, float* dx, const float* mask, int batch, int ppc, float* bias_part,
                    int* bias_nparts, hipStream_t s) {       // conv1 (16^3 -> 19^3): six waves per workgroup fit the LDS
  return launch_wino1<W1Cfg<16, 3, 6>, 1>(dy, wp, dx, mask, batch, ppc ? ppc : 1, bias_part, bias_nparts, s);
}
int nvf_wino1_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s) {
  return launch_wino1<W1Cfg<35, 0>, 0>(x, wp, y, bias, batch, ppc ? ppc : 2, nullptr, nullptr, s);
}
int nvf_wino1_fwd19(const float* x, const float* wp, const float* bias, float* y, int batch, int ppc, hipStream_t s) {
  return launch_wino1<W1Cfg<19, 0>, 0>(x, wp, y, bias, batch, ppc ? ppc : 1, nullptr, nullptr, s);
}
