/*
 * nvf_hip.h -- C ABI of libnvf_hip.so: the gfx950 (MI355X) kernels under NVFPCC's
 * per-block neural-volumetric-field hot path.
 *
 * The reference has NO native boundary on this path: NVFPCC.py calls the Python
 * operator classes of utils/network.py, gdn_3d.py and utils/loss.py, which call
 * torch aten ops.  This header is the boundary this build introduces underneath
 * those classes; every entry point names the reference call site it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every tensor is fp32, contiguous, NCDHW, resident in device memory;
 *   - the caller owns every buffer (inputs, outputs, workspace); the library
 *     never allocates, frees or keeps a pointer after returning, and holds NO state of its own between
 *     calls: work that one call hands to a later one (the deferred final passes, the queued latent
 *     tail) travels in a caller-owned NvfStepCtx, so any number of engines, streams and threads can
 *     use the library at once, each with its own context;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no call
 *     synchronises; outputs are overwritten unless the argument says accumulate;
 *   - return 0 on success, a positive hipError_t from the launch, or a negative
 *     NVF_E* code for a rejected argument; no C++ exception crosses the ABI;
 *   - summation order inside a kernel depends only on the output element, never
 *     on the batch size or grid, so results are batch- and rank-count-invariant.
 */
#ifndef NVF_HIP_H
#define NVF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVF_OK 0
#define NVF_EINVAL (-1)      /* bad shape / null pointer / unsupported combination */
#define NVF_EWORKSPACE (-2)  /* workspace too small */

#define NVF_ACT_NONE 0
#define NVF_ACT_RELU 1
#define NVF_ACT_SIGMOID 2

int nvf_version(void);

/* ---- step context ---------------------------------------------------------------
 * Host-side state of ONE training step in flight: the queue of deferred final passes (nvf_finals_*) and the
 * queued latent tail (nvf_latent_tail_queue).  Opaque; the caller allocates nvf_step_ctx_bytes() bytes of host
 * memory (8-byte aligned), calls nvf_step_ctx_init once, and passes the pointer to every entry point that takes
 * an `NvfStepCtx* ctx`.  ctx == NULL everywhere means "defer nothing": every final pass is launched by the call
 * that produces its partial sums.  A context must not be used from two threads at the same time; different
 * contexts are independent (tests/test_gpu_engine.py::test_two_step_contexts_do_not_interfere). */
typedef struct NvfStepCtx NvfStepCtx;
size_t nvf_step_ctx_bytes(void);
int nvf_step_ctx_init(NvfStepCtx* ctx);
/* on != 0: launches given this context keep the direct summation order (no Winograd form of a weight gradient): the
 * arithmetic that follows the reference's training trajectory to 1e-7 (torch's conv backward, NVFPCC.py:164-172);
 * 0 (default): the reduced-multiplication forms, statistically equivalent training. */
int nvf_step_ctx_set_direct(NvfStepCtx* ctx, int on);
/* Forms of the merged weight-gradient launches (nvf_wgrad_trunk_partial) when the context does not
 * ask for the direct ones: conv2_zsplit in 0..8 (0 = default 1): z work items of conv2's Winograd gradient; conv1_wino
 * != 0: conv1's gradient in the Winograd form as well.  Each choice is another summation order (agreement to fp32
 * rounding): it belongs to the caller's context, the library reads no environment variable for it.  NVF_EINVAL outside
 * the ranges. */
int nvf_step_ctx_set_wgrad_forms(NvfStepCtx* ctx, int conv2_zsplit, int conv1_wino);

/* Adam fused into the launch that produces a gradient: an element g_base[i] written by that launch is followed by the
 * nvf_step_tail update of p_base[i], m_base[i], v_base[i] (same coefficients, same arithmetic, same non-finite rule;
 * bad_count, if non-NULL, is nvf_step_tail's acc + 6).  Applies to outputs inside [g_base, g_base + n) only. */
typedef struct NvfAdamFuse {
  const float* g_base;
  float* p_base;
  float* m_base;
  float* v_base;
  int64_t n;
  const float* coef_dev;
  float coef0_host, coef1_host, beta1, beta2, eps, reserved;
  float* bad_count;
} NvfAdamFuse;

/* ---- weight packing -------------------------------------------------------
 * Re-lays an effective kernel into the two layouts the direct-conv kernels read
 * from scalar registers: w_fwd[ci][k][co] and w_bwd[co][k'][ci].
 * conv  : w is [Cout][Cin][K^3] (F.conv3d, network.py:687,741); w_bwd taps are flipped.
 * convT : w is [Cin][Cout][K^3] (F.conv_transpose3d, network.py:621); w_bwd keeps tap order.
 * Either output may be NULL. */
int nvf_pack_conv_weight(const float* w, int cout, int cin, int k, float* w_fwd, float* w_bwd, void* stream);
int nvf_pack_convT_weight(const float* w, int cin, int cout, int k, float* w_fwd, float* w_bwd, void* stream);

/* ---- effective parameters (network.py:611-620, 677-686, 735-740) ------------
 * w_eff = f_q(kernel) + kernel_init, b_eff = b + b_init for one layer.
 * q = 1: kernel + (U-.5)/16 with U from `u` if non-NULL else Philox(seed, stream_id);
 * q = 2: round(16 k)/16 (half-to-even); any other q: raw kernel. */
int nvf_effective_params(const float* kernel, const float* kernel_init, const float* u, float* w_eff, int n,
                         const float* b, const float* b_init, float* b_eff, int nb, int q, uint64_t seed,
                         uint64_t stream_id, void* stream);

/* All layers of a decoder in one launch.  `table_dev` is a device array of `nlayers` NvfLayerDesc records
 * (nvf_layer_desc_size() bytes each).  Writes w_eff = f_q(kernel) + kernel_init directly in the packed
 * layouts and b_eff = b + b_init.  Weight noise (q = 1): Philox(seed, ((step + *step_dev) << 8) | layer_id). */
typedef struct NvfLayerDesc {
  const float* kernel;
  const float* kernel_init;
  const float* b;
  const float* b_init;
  float* w_fwd;
  float* w_bwd;
  float* b_eff;
  int32_t dim0, dim1, k3;   /* kernel is [dim0][dim1][k3] */
  int32_t kind;             /* 0: conv [cout][cin][k] (w_bwd taps flipped); 1: convT [cin][cout][k] */
  int32_t quantised;        /* 1: Q-layer (q applies); 0: I-layer (raw kernel) */
  int32_t layer_id;         /* weight-noise stream id */
  int32_t nbias, pad_;
} NvfLayerDesc;
size_t nvf_layer_desc_size(void);
int nvf_prepare_weights(const void* table_dev, int nlayers, int q, uint64_t seed, uint64_t step,
                        const uint64_t* step_dev, void* stream);

/* ---- gather convolution (F.conv3d fwd; bwd-data of conv3d and conv_transpose3d) --
 * y[b,co,o] = act(bias[co] + sum_{ci,k} x[b,ci, stride*o - pad + k] * w[ci][k][co])
 *             (+ addend[b,co,o]) (* (mask[b,co,o] > 0))
 * w is a packed w_fwd (forward) or w_bwd (backward-data; then cin/cout are swapped
 * by the caller and pad = K-1-p for conv, pad = p with stride 2 for convT).
 * bias, addend, mask may be NULL.  variant: 0 = tuned LDS-tiled kernel (falls back to 1 for shapes without a
 * tiled instantiation), 1 = one-thread-per-output kernel (same fmaf order: bit-identical), >= 2 = tuning alternates.
 * Replaces F.conv3d at network.py:687,741 and the
 * autograd backward of network.py:621,687. */
int nvf_conv3d_gather(const float* x, const float* w, const float* bias, float* y, const float* addend,
                      const float* mask, int batch, int cin, int cout, int k, int stride, int pad, int din,
                      int hin, int win, int dout, int hout, int wout, int act, int variant, void* stream);

/* ---- transposed convolution k5 s2 forward (F.conv_transpose3d, network.py:621) ---
 * y[b,co,o] = act(bias[co] + sum_{ci,k : o+pad-k = 2i} x[b,ci,i] * w[ci][k][co]),
 * dout = 2*din + 3 (pad 0) or 2*din (pad 2, output_padding 1).  w is w_fwd. */
int nvf_convT3d_k5s2_fwd(const float* x, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                         int pad, int din, int hin, int win, int dout, int hout, int wout, int act, int variant,
                         void* stream);

/* ---- matrix-core (v_mfma_f32_16x16x4_f32, exact fp32) form of the 4^3 convolutions with 8 output channels
 * (conv1 / conv2 of chanstr 8,16,8,8: F.conv3d network.py:687 and its autograd backward-data).  Same contract
 * as nvf_conv3d_gather with k = 4, stride 1, but the weights are pre-packed MFMA A-fragments:
 *   nvf_pack_mfma_k4(gather_w [cin][64][8] (= w_fwd, or w_bwd for the backward-data pass), cin, 8, pair_axis, wp)
 *   pair_axis 0: rows pair outputs along x (forward, pad 0); 2: along z (backward-data, pad 3)
 * wp holds nvf_pack_mfma_k4_floats(cin, pair_axis) floats (layout [ci group][ky][kx][kz][lane]).  Per-output accumulation order is fixed
 * (input-channel group, ky, kx, kz), so results do not depend on batch size or tiling; they differ from
 * nvf_conv3d_gather's order by fp32 rounding only.  NVF_EINVAL = no instantiation for this shape. */
size_t nvf_pack_mfma_k4_floats(int cin, int pair_axis);
int nvf_pack_mfma_k4(const float* gather_w, int cin, int cout, int pair_axis, float* wp, void* stream);
/* up to 8 packings (8 output channels each) in one launch */
int nvf_pack_mfma_k4_multi(const float* const* gather_ws, float* const* wps, const int* cins, const int* pair_axes,
                           int n, void* stream);
int nvf_conv3d_k4_mfma(const float* x, const float* wp, const float* bias, float* y, const float* addend,
                       const float* mask, int batch, int cin, int cout, int pad, int pair_axis, int din, int hin,
                       int win, int dout, int hout, int wout, int act, int variant, void* stream);
/* ... with bias_part (backward-data through a ReLU mask: bias NULL, act NVF_ACT_NONE, addend NULL, mask given): the
 * launch also leaves, per (workgroup, wave), the 8 channel sums of the outputs it stored -- *bias_nparts (<= 2048) slabs
 * of 8 floats whose sum (a jtotal = 8 job of nvf_wgrad_reduce_multi) is the bias gradient of the layer below. */
int nvf_conv3d_k4_mfma_bias(const float* x, const float* wp, const float* bias, float* y, const float* addend,
                            const float* mask, int batch, int cin, int cout, int pad, int pair_axis, int din, int hin,
                            int win, int dout, int hout, int wout, int act, int variant, float* bias_part,
                            int* bias_nparts, void* stream);

/* ---- reduced-multiplication backward-data of the valid 4^3 convolutions with 8 -> 8 channels (conv2 of chanstr
 * 8,16,8,8: the autograd backward of F.conv3d, network.py:687, NVFPCC.py:197): Winograd F(2x2, 4x4) over (y, x), direct
 * over z on the matrix cores (conv_wino.hip) -- 2.56 x fewer multiplications than nvf_conv3d_k4_mfma's gather form.
 * BACKWARD PASSES ONLY: fp32 error 1e-6 of max |dx| against 6e-7 for the direct form, but not a fixed fmaf chain per
 * output, so the forward (bit-exact batch invariance) never uses it.
 * dy [batch, 8, din^3]; dx, mask [batch, 8, (din + 3)^3]: dx = mask > 0 ? conv_full(dy, w) : 0 (the ReLU of the layer
 * below).  wp = nvf_pack_mfma_all kind 40 (c0 = c1 = 8) of the layer's gather-form backward weights w_bwd,
 * nvf_pack_wino_k4_floats() floats.  bias_part (optional): *bias_nparts slabs of 8 floats, the channel sums of dx per work
 * unit (the bias gradient of the layer below, a jtotal = 8 job of nvf_wgrad_reduce_multi).  NVF_EINVAL = no instantiation
 * (din 32: conv2, 16: conv1).
 * ppc, for these and the three entry points below, names the kernel and its work units.  Every shape has up to two kernels
 * that give the same bits: "one" (conv_wino1.hip / conv16_wino1.hip: one accumulator set or output plane per wave, two waves
 * per SIMD) and "two" (conv_wino.hip / conv16_wino.hip: two sets or planes, every input plane walked once per pair).
 *   bits 0-7   count: pairs of output planes per work unit (output planes in conv16_wino1.hip); 0 = the kernel's default.
 *              conv_wino.hip takes even counts only (NVF_EINVAL otherwise).
 *   bits 8-15  debug switches of -DNVF_WINO_DBG=1 tuning builds of conv_wino.hip; ignored by the "one" kernels.  The
 *              16-channel "two" kernel has none: it reads every bit below bit 16 as its count.
 *   bit 16     the "one" kernel.  NVF_EINVAL where the shape has none: 16 channels with din 16 or 19, or with bias_part.
 *   ppc = 0 (count 0 without bit 16) is each shape's default kernel: "one" for 8 channels except the forward with din 19,
 *   and for 16 channels with din 32 backward without bias_part; "two" elsewhere.  The 16-channel entries reject ppc < 0. */
size_t nvf_pack_wino_k4_floats(void);
int nvf_conv3d_k4_wino_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int din, int ppc,
                           float* bias_part, int* bias_nparts, void* stream);
/* The FORWARD of the same layers in the same form, y = relu(conv3d(x, w) + bias), for TRAINING steps only (NVFPCC.py:160,
 * 234): x [batch, 8, din^3] (din 35: conv2, 19: conv1), y [batch, 8, (din - 3)^3], wp = kind 40 of the layer's w_fwd.  Its
 * outputs differ from nvf_conv3d_k4_mfma's by fp32 rounding (1e-6 of max |y|) and are not a fixed fmaf chain per output:
 * eval / encode / decode (NVFPCC.py:316, 516, 628), whose occupancy must be batch-invariant bit for bit, never use it. */
int nvf_conv3d_k4_wino_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int din, int ppc,
                           void* stream);

/* The same form for the WIDE decoder's 4^3 layers (16 -> 16 channels; conv16_wino.hip): rows = the 16 output channels,
 * two output planes in flight, the five input planes of a pair walked once per pair.  Training steps only, as above.
 * wp = nvf_pack_mfma_all kind 41 (c0 = c1 = 16) of w_bwd (backward-data) / w_fwd (forward), nvf_pack_wino16_k4_floats()
 * floats.  bwd: dy [batch, 16, din^3] (din 32 / 16), dx, mask [batch, 16, (din + 3)^3]; fwd: x [batch, 16, din^3]
 * (din 35 / 19), y [batch, 16, (din - 3)^3].  ppc: as above.  bias_part (optional, bwd): *bias_nparts slabs of 16 floats,
 * the channel sums of dx per work unit (a jtotal = 16 job of nvf_wgrad_reduce_multi*). */
size_t nvf_pack_wino16_k4_floats(void);
int nvf_conv3d_k4_wino16_bwd(const float* dy, const float* wp, float* dx, const float* mask, int batch, int din, int ppc,
                             float* bias_part, int* bias_nparts, void* stream);
int nvf_conv3d_k4_wino16_fwd(const float* x, const float* wp, const float* bias, float* y, int batch, int din, int ppc,
                             void* stream);

/* ... and their WEIGHT gradient (wgrad16_wino.hip: Winograd F(4x4, 2x2) over (y, x), rows = the 16 dY channels, columns =
 * the 16 X channels, two z taps per pass): partial sums only -- *nslab <= max_slabs slabs of 16384 floats, layout
 * [co][ci][kz][ky][kx], for a jtotal = 16384 job of nvf_wgrad_reduce_multi*.  dy [batch, 16, w^3] (w 32 / 16), x [batch, 16,
 * (w + 3)^3]; zsplit: z steps of an item split over this many work items (0: default; <= 8). */
int nvf_wgrad16_k4_wino_partial(const float* dy, const float* x, float* slabs, int batch, int w, int zsplit, int max_slabs,
                                int* nslab, void* stream);

/* ... and conv2's WEIGHT gradient in the corresponding form (wgrad_wino.h: Winograd F(4x4, 2x2) over (y, x) -- the taps
 * are the output, 2 x 2 tiles of dy the filter -- direct over z on the matrix cores, every MFMA lane useful): the weight
 * half of the autograd backward of F.conv3d, network.py:687.  dy [batch, 8, 32^3], x [batch, 8, 35^3] -> dw [8][8][4][4][4]
 * (and db [8] = channel sums of dy when db is not NULL).  One launch of per-workgroup slabs + the fixed-order reduction
 * (deterministic; fp32 error 4e-6 of max |dw| against 1e-6 for the direct form).  workspace: 512 * (4096 + 8) floats.
 * zsplit: the z steps of a (block, tile group) are split over this many work items (1..8).  In the training step the same
 * body runs as job 0 of nvf_wgrad_trunk_partial (NVF_WGRAD_WINO=0 selects the direct form there). */
int nvf_wgrad_k4_wino(const float* dy, const float* x, float* dw, float* db, void* workspace, size_t workspace_bytes,
                      int batch, int zsplit, void* stream);

/* ---- matrix-core form of the transposed convolutions k5 s2 with 8 output channels and padding 0 (up1, up2 of
 * chanstr 8,16,8,8; F.conv_transpose3d network.py:621).  Same contract as nvf_convT3d_k5s2_fwd; the weights are
 * MFMA A-fragments: nvf_pack_convT_mfma(w_fwd [cin][125][8], cin, 8, wp), nvf_pack_convT_mfma_floats(cin) floats.
 * Fixed per-output accumulation order (input-channel group, jy, jx, jz): independent of batch and tiling.
 * NVF_EINVAL = no instantiation for this shape. */
size_t nvf_pack_convT_mfma_floats(int cin);
int nvf_pack_convT_mfma(const float* w_fwd, int cin, int cout, float* wp, void* stream);
int nvf_convT3d_k5s2_mfma(const float* x, const float* wp, const float* bias, float* y, int batch, int cin, int cout,
                          int din, int act, int variant, void* stream);

/* ---- matrix-core backward-data of those transposed convolutions (a stride-2 gather convolution, autograd
 * backward of network.py:621): dx[b,ci,i] = (sum_{co,k} g[b,co,2i+k] w[ci][co][k] (+ addend)) (* (mask > 0)),
 * din = 2 dout + 3, cog = 8 (up2) or 16 (up1) output channels, cig channels of g.  Weights:
 * nvf_pack_s2k5_mfma(w_bwd [cig][125][cog], cig, cog, wp), nvf_pack_s2k5_mfma_floats(cig, cog) floats.
 * Fixed per-output accumulation order (channel group, ky, kx window, kz).  NVF_EINVAL = no instantiation. */
size_t nvf_pack_s2k5_mfma_floats(int cig, int cog);
int nvf_pack_s2k5_mfma(const float* gather_w, int cig, int cog, float* wp, void* stream);
int nvf_conv3d_s2k5_mfma(const float* g, const float* wp, float* dx, const float* addend, const float* mask,
                         int batch, int cig, int cog, int din, int dout, int variant, void* stream);

/* ---- matrix-core gather convolutions for 16 / 32 OUTPUT channels (the wide decoder, chanstr 16,32,16,16:
 * F.conv3d network.py:687 forward and backward-data, and the backward-data of the stride-2 transposed convolutions
 * network.py:621).  Rows of the MFMA tile are the output channels (no pairing), K = four input channels.  Same
 * contract as nvf_conv3d_gather; the weights are A fragments of the packed gather weight:
 *   nvf_pack_g16_mfma(gather_w [cin][k^3][cout] (= w_fwd, or w_bwd for a backward-data pass), cin, cout, k, wp),
 *   nvf_pack_g16_mfma_floats(cin, cout, k) floats, layout [ceil(cout/16)][cin/4][tap][lane]; cout = 8 is accepted too
 *   (rows 8..15 of the tile are zero weights and are not stored).
 * Fixed per-output accumulation order (channel group, kz, ky, kx): independent of batch and tiling.
 * NVF_EINVAL = no instantiation for this shape (the caller then uses nvf_conv3d_gather). */
size_t nvf_pack_g16_mfma_floats(int cin, int cout, int k);
int nvf_pack_g16_mfma(const float* gather_w, int cin, int cout, int k, float* wp, void* stream);
int nvf_conv3d_g16_mfma(const float* x, const float* wp, const float* bias, float* y, const float* addend,
                        const float* mask, int batch, int cin, int cout, int k, int stride, int pad, int din, int hin,
                        int win, int dout, int hout, int wout, int act, int variant, void* stream);

/* ---- matrix-core form of the transposed convolutions k5 s2 with 16 / 32 output channels (all four of chanstr
 * 16,32,16,16: up1 / up2 with padding 0, conv0 / up0 with padding 2 and output_padding 1; F.conv_transpose3d
 * network.py:621): the output channels are the MFMA rows, the eight sub-pixel parity classes separate accumulators
 * fed by one B fragment.  Same contract as nvf_convT3d_k5s2_fwd; weights: nvf_pack_convT16_mfma(w_fwd
 * [cin][125][cout], cin, cout, wp), nvf_pack_convT16_mfma_floats(cin, cout) floats, layout [cout/16][cin/4][125][lane].
 * Fixed per-output accumulation order (input-channel group, jy, jx, jz).  NVF_EINVAL = no instantiation. */
size_t nvf_pack_convT16_mfma_floats(int cin, int cout);
int nvf_pack_convT16_mfma(const float* w_fwd, int cin, int cout, float* wp, void* stream);
int nvf_convT3d_k5s2_mfma16(const float* x, const float* wp, const float* bias, float* y, int batch, int cin, int cout,
                            int pad, int din, int act, int variant, void* stream);

/* every MFMA weight packing of a step in one launch (<= 16 jobs): kind 0 / 2 = nvf_pack_mfma_k4 with that pair
 * axis (c0 = cin), 10 = nvf_pack_convT_mfma (c0 = cin), 11 = nvf_pack_convT16_mfma (c0 = cin, c1 = cout),
 * 20 = nvf_pack_s2k5_mfma (c0 = cig, c1 = cog),
 * 30 / 31 = nvf_pack_g16_mfma with k = 4 / 5 (c0 = cin, c1 = cout), 40 / 41 = the Winograd packings of
 * nvf_conv3d_k4_wino_* (c0 = c1 = 8) / nvf_conv3d_k4_wino16_* (c0 = c1 = 16) */
int nvf_pack_mfma_all(const float* const* srcs, float* const* dsts, const int* kinds, const int* c0s, const int* c1s,
                      int n, void* stream);

/* ---- the three classifier heads of the narrow decoder in one launch each (conv0_cls on [16, 8^3], conv1_cls on
 * [8, 16^3], conv2_cls on [8, 32^3], in that order; IConv3d/QConv3d C -> 1, k 3, padding 1, network.py:4761-4768).
 * Same kernels, same results as three nvf_conv3d_gather / nvf_wgrad calls; the two small heads, latency-bound on a
 * few CUs, run beside the big one.  NVF_EINVAL for any other (channels, size) triple. */
int nvf_heads3_fwd(const float* const* xs, const float* const* w_fwds, const float* const* biases, float* const* ps,
                   const int* cs, const int* ss, int batch, int act, void* stream);
int nvf_heads3_bwd_data(const float* const* dlogits, const float* const* w_bwds, float* const* dxs,
                        const float* const* masks, const int* cs, const int* ss, int batch, void* stream);

/* nvf_focal_loss_multi (chain_sigmoid) of the three heads and nvf_heads3_bwd_data in ONE launch (NVFPCC.py:166-184
 * + the heads' backward-data): dls[h] = d term_h / d logit_h is computed while the tiles are staged, written for
 * the weight gradient, and loss[slots[h]] = term_h (final pass deferred while ctx has an open nvf_finals_begin).  dists[h] may be
 * NULL.  batch <= 32 (one loss partial per workgroup); otherwise NVF_EINVAL. */
int nvf_heads3_loss_bwd_data(const float* const* ps, const float* const* gts, const float* const* dists,
                             const float* alphas, const float* betas, const int* slots, float* loss,
                             float* const* dls, const float* const* wbs, float* const* dxs,
                             const float* const* masks, const int* cs, const int* ss, int batch, void* workspace,
                             size_t workspace_bytes, NvfStepCtx* ctx, void* stream);
/* ... and, with bias_outs (three pointers; NULL = the call above), the heads' bias gradients (autograd of the bias add,
 * utils/network.py:741): bias_outs[h][0] = sum of dls[h], from one partial per workgroup of the values it writes anyway;
 * the final pass is deferred like the loss terms' (or launched here). */
int nvf_heads3_loss_bwd_data_bias(const float* const* ps, const float* const* gts, const float* const* dists,
                                  const float* alphas, const float* betas, const int* slots, float* loss,
                                  float* const* dls, const float* const* wbs, float* const* dxs,
                                  const float* const* masks, const int* cs, const int* ss, int batch,
                                  float* const* bias_outs, void* workspace, size_t workspace_bytes, NvfStepCtx* ctx,
                                  void* stream);
/* nvf_heads3_fwd (ps[h] = act(conv(xs[h], ws[h]) + biases[h]): network.py:4761-4768 in mode 'train') and
 * nvf_heads3_loss_bwd_data_bias on those ps (NVFPCC.py:166-184 and the heads' autograd backward-data) in ONE launch: the
 * forward workgroups hand p to the loss workgroups of their block through device-scope stores and arrival counters.  Same
 * bits as the two calls.  flags: 6 * batch * 64 32-bit words (one 256-byte line per counter), zero before the first call; a call leaves them zero (one buffer per
 * stream).  batch <= 32; NVF_EINVAL for other head shapes than nvf_heads3_fwd's. */
int nvf_heads3_fwd_loss_bwd_data(const float* const* xs, const float* const* ws, const float* const* biases,
                                 float* const* ps, int act, const float* const* gts, const float* const* dists,
                                 const float* alphas, const float* betas, const int* slots, float* loss,
                                 float* const* dls, const float* const* wbs, float* const* dxs,
                                 const float* const* masks, const int* cs, const int* ss, int batch,
                                 float* const* bias_outs, void* workspace, size_t workspace_bytes, uint32_t* flags,
                                 NvfStepCtx* ctx, void* stream);
/* partial sums only: slabs[h] receives nslabs[h] (<= max_slabs) slabs of cs[h] * 27 floats, to be added by
 * nvf_wgrad_reduce_multi */
int nvf_heads3_wgrad_partial(const float* const* dlogits, const float* const* xs, float* const* slabs, const int* cs,
                             const int* ss, int batch, int max_slabs, int* nslabs, void* stream);

/* ---- fused stem for chanstr (c0, c1) = (8, 16) or (16, 32), ch <= 8 (network.py:4759-4760; gdn_3d.py:137-159) ----
 * forward : a0 = up0(x0) (convT k5 s2 p2 op1), h0 = IGDN(a0), y1 = ReLU(conv0(h0)); all three are outputs.
 * backward: from g1 = dL/d(conv0 pre-activation): da0 (= dL/d a0, after the IGDN backward) and dx0; when
 *           dbeta_hat, dgamma_hat and dw_up0 are all non-NULL also the IGDN parameter gradients and up0's weight
 *           gradient [ch][c0][5][5][5] (overwritten).  Intermediates in LDS; the workspace (always required,
 *           nvf_stem_bwd_workspace_for bytes) also holds conv0's backward-data partials, batch x c1/2 x c0 x 64 floats.
 * Weights are the packed layouts: *_w_fwd = [cin][125][cout], *_w_bwd = [cout][125][cin]. */
int nvf_stem_fwd(const float* x0, const float* up0_w_fwd, const float* up0_b, const float* beta_hat,
                 const float* gamma_hat, const float* conv0_w_fwd, const float* conv0_b, float* a0, float* h0,
                 float* y1, int batch, int ch, int c0, int c1, void* stream);

/* nvf_latent_fwd and nvf_stem_fwd in ONE launch (the stem's workgroups compute their block's rounded latents themselves;
 * one more workgroup produces h, lat, x_rounded and the latent rate of the whole batch); results of the two calls, bit
 * for bit.  utils/network.py:4592-4612, 4514-4539, 4759-4760. */
int nvf_stem_latent_fwd(const float* e, const float* lat_w_fwd, const float* lat_bias, const float* lat_beta_hat,
                        const float* lat_gamma_hat, const int64_t* block_ids, const float* sigma, const float* mu,
                        float* h, float* lat, float* x_rounded, float* bits, int mode, uint64_t seed, uint64_t step,
                        const uint64_t* step_dev, const float* up0_w_fwd, const float* up0_b, const float* beta_hat,
                        const float* gamma_hat, const float* conv0_w_fwd, const float* conv0_b, float* a0, float* h0,
                        float* y1, int batch, int ch, int c0, int c1, void* stream);
size_t nvf_stem_bwd_workspace(int batch, int ch);                           /* (c0, c1) = (8, 16) */
size_t nvf_stem_bwd_workspace_for(int batch, int ch, int c0, int c1);       /* 0: no kernel for (c0, c1) */
int nvf_stem_bwd(const float* g1, const float* x0, const float* a0, const float* conv0_w_bwd,
                 const float* up0_w_bwd, const float* beta_hat, const float* gamma_hat, float* da0, float* dx0,
                 float* dbeta_hat, float* dgamma_hat, float* dw_up0, void* workspace, size_t workspace_bytes,
                 int batch, int ch, int c0, int c1, void* stream);

/* nvf_stem_bwd minus its final launch (training step): up0's weight-gradient slabs (*dw_slabs: *nslabs slabs of
 * ch * c0 * 125 floats inside `workspace`) are left to the caller's slab reduction (nvf_wgrad_reduce_multi*), the
 * IGDN parameter gradients to the deferred final passes (nvf_finals_begin; launched at once otherwise).  Same sums,
 * same order as nvf_stem_bwd.  h0 and dw_conv0_slabs (both or neither): the launch that computes conv0's backward-data
 * also leaves conv0's weight gradient (bwd-weight of network.py:621 for conv0) as `batch` slabs of c0 * c1 * 125 floats
 * ([ci][co][k], one per block, inside `workspace`) for the same reduction. */
int nvf_stem_bwd_partial(const float* g1, const float* x0, const float* a0, const float* conv0_w_bwd,
                         const float* up0_w_bwd, const float* beta_hat, const float* gamma_hat, float* da0, float* dx0,
                         float* dbeta_hat, float* dgamma_hat, float** dw_slabs, int* nslabs, void* workspace,
                         size_t workspace_bytes, int batch, int ch, int c0, int c1, const float* h0,
                         float** dw_conv0_slabs, NvfStepCtx* ctx, void* stream);

/* The same work with NO launch of its own (narrow decoder, c0 = 8, c1 = 16, batch <= 32): queued in `ctx`, it runs as the
 * first workgroups of the next five-job weight-gradient launch given that context (nvf_wgrad_trunk_partial), which must also
 * carry a queued latent tail (nvf_latent_tail_queue: the tail is the only consumer of dx0 inside that launch; its
 * dx_addend argument is ignored there).  The stem's backward depends on g1 alone, exactly like conv0's weight gradient
 * in that launch (autograd backward of network.py:4759-4760, gdn_3d.py:137-159).  Needs an open finals queue
 * (nvf_finals_begin).  Outputs as nvf_stem_bwd_partial (same sums, same order, same bits), plus *bias_slabs: `batch`
 * slabs of c0 floats inside `workspace` whose sum is up0's bias gradient (a jtotal = c0 job of nvf_wgrad_reduce_multi*).
 * da0 / dx0 exist once that launch has run.  flags: (batch + 1) * 64 uint32 words of device memory (one 256-byte line per arrival counter), zero before the first use
 * (the launch leaves them zero).  NVF_EINVAL: another shape, no open queue, or a stem backward already queued.
 * nvf_latent_tail_cancel also drops a queued stem backward. */
int nvf_stem_bwd_queue(NvfStepCtx* ctx, const float* g1, const float* x0, const float* a0, const float* conv0_w_bwd,
                       const float* up0_w_bwd, const float* beta_hat, const float* gamma_hat, float* da0, float* dx0,
                       float* dbeta_hat, float* dgamma_hat, float** dw_slabs, int* nslabs, float** bias_slabs,
                       void* workspace, size_t workspace_bytes, uint32_t* flags, int batch, int ch, int c0, int c1,
                       void* stream);
int nvf_stem_bwd_pending(const NvfStepCtx* ctx);

/* ---- weight gradient (autograd backward of network.py:621,687,741) --------------
 * dw[a][b][k] (+)= sum_{n,i} p[n,a,i] * q[n,b, stride*i - pad + k]      (out_mode 0)
 * dw[b][a][K^3-1-k] (+)= same sum                                        (out_mode 1)
 * conv  : p = dY, q = X, stride 1          -> dw[cout][cin][k]
 * convT : p = X,  q = dY, stride 2         -> dw[cin][cout][k]
 * head  : p = X,  q = dlogit, out_mode 1   -> dw[1][cin][k]
 * Two launches: per-workgroup partial sums into `workspace`, then a fixed-order
 * reduction (deterministic; no float atomics).  nvf_wgrad_workspace() gives the
 * byte size for a batch. */
size_t nvf_wgrad_workspace(int batch, int a, int b, int k, int dp, int hp, int wp);
int nvf_wgrad(const float* p, const float* q, float* dw, void* workspace, size_t workspace_bytes, int batch, int a,
              int b, int k, int stride, int pad, int dp, int hp, int wp, int dq, int hq, int wq, int out_mode,
              int accumulate, int variant, void* stream);
/* The same gradient in two separate steps, so that a whole backward pass needs ONE reduction launch:
 * nvf_wgrad_partial launches only the partial sums (slabs stay in `workspace`, which the caller must not reuse
 * until the reduction; *nslab = number of slabs, 0 when dw was written directly), nvf_wgrad_reduce_multi adds the
 * slabs of up to 16 gradients in the same fixed order as nvf_wgrad (results identical bit for bit). */
int nvf_wgrad_partial(const float* p, const float* q, float* dw, void* workspace, size_t workspace_bytes, int batch,
                      int a, int b, int k, int stride, int pad, int dp, int hp, int wp, int dq, int hq, int wq,
                      int out_mode, int variant, int* nslab, void* stream);
int nvf_wgrad_reduce_multi(const float* const* slabs, float* const* dws, const int* nslabs, const int* jtotals,
                           int n, void* stream);

/* up1's and conv0's weight gradients of the narrow trunk in one launch (partial sums): job 0 = up1 (p = X [B,16,8^3],
 * q = dY [B,8,19^3]), job 1 = conv0 (p = X [B,8,4^3], q = dY [B,16,8^3]).  slabs[j] must hold 512 slabs of 16000
 * floats; nslabs[j] <= 512 at every batch (above 512 work items a workgroup walks several).  Both jobs are VALU tile
 * kernels in the direct summation order. */
int nvf_wgrad_up1_conv0_partial(const float* const* ps, const float* const* qs, float* const* slabs, int batch,
                                int* nslabs, void* stream);

/* The weight gradients of the narrow trunk above the stem in ONE launch (partial sums only), with what rides along.
 * Jobs (ps[j], qs[j], slabs[j], nslabs[j]), in this order; slabs[j] must hold 512 slabs of the size given:
 *   0 conv2: p = dY [B,8,32^3], q = X [B,8,35^3],  4096 floats     1 up2: p = X [B,8,16^3], q = dY [B,8,35^3],  8000
 *   2 conv1: p = dY [B,8,16^3], q = X [B,8,19^3],  4096            3 up1: p = X [B,16,8^3], q = dY [B,8,19^3], 16000
 *   4 conv0: p = X [B,8,4^3],   q = dY [B,16,8^3], 16000
 * nslabs[j] receives the number written (<= 512 at every batch), to be added by nvf_wgrad_reduce_multi*.  njobs = 3:
 * jobs 0-2, the kernels and results of three nvf_wgrad_partial calls.  njobs = 5: all five, jobs 0-3 with the same
 * bits; the two small jobs fill the slots the short matrix-core workgroups leave while conv2's are still running.
 * conv0 takes one of two forms: on the matrix cores with one slab per block (nslabs[4] = batch) when batch <= 512 and
 * the context does not ask for the direct forms; otherwise the tile job of nvf_wgrad_up1_conv0_partial, capped at 512
 * slabs.  The matrix-core form sums in another order: it agrees with that launch to fp32 rounding, not bit for bit.
 * What rides along (a NULL / zero group is absent, a partly given one NVF_EINVAL; all but the first need njobs = 5):
 *   - a latent tail queued in ctx as the first workgroup, behind a queued stem backward (nvf_stem_bwd_queue) if any;
 *   - bias_slabs: three entries, entry 1 ignored; with bias_slabs[0] / bias_slabs[2] non-NULL the per-workgroup channel
 *     sums of conv2's / conv1's dY: nslabs[j] slabs of 8 floats each, whose sum (a jtotal = 8 reduction job) is that
 *     layer's bias gradient -- the kernel holds every dY tile in registers, and its tiles partition dY;
 *   - head_*: the weight gradients of the narrow decoder's three classifier heads (the contract of
 *     nvf_heads3_wgrad_partial: three entries each, at most head_max_slabs slabs of cs[h] * 27 floats) as further
 *     workgroups: they depend on nothing the launch produces and run in the slots its other jobs leave;
 *   - sum_* (needs head_*): the FIRST pass of nvf_multi_channel_sum over sum_xs (bias gradients sum_outs that no other
 *     kernel leaves behind) into sum_workspace (nvf_multi_channel_sum_workspace(total channels) bytes, NVF_EWORKSPACE
 *     if fewer; untouched until the flush); the final pass is queued in ctx (an open nvf_finals_begin) or launched
 *     here.  Then no final pass of the step reads what the slab reduction writes: nvf_wgrad_reduce_finals_tail;
 *   - coef_src / coef_live (both or neither; needs sum_*): two floats, the optimiser's step coefficients, copied.
 * A refused request launches nothing and leaves ctx as it was.  nvf_trunk_wgrads_bytes(): sizeof, for bindings. */
typedef struct NvfTrunkWgrads {
  const float* const* ps;
  const float* const* qs;
  float* const* slabs;
  int32_t* nslabs;
  float* const* bias_slabs;
  const float* const* head_dls;
  const float* const* head_xs;
  float* const* head_slabs;
  int32_t* head_nslabs;
  const float* const* sum_xs;
  float* const* sum_outs;
  const int32_t* sum_channels;
  const int32_t* sum_spatials;
  void* sum_workspace;
  uint64_t sum_workspace_bytes;
  const float* coef_src;
  float* coef_live;
  int32_t batch, njobs, head_max_slabs, sum_n;
} NvfTrunkWgrads;
size_t nvf_trunk_wgrads_bytes(void);
int nvf_wgrad_trunk_partial(const NvfTrunkWgrads* req, NvfStepCtx* ctx, void* stream);

/* per-channel sum over batch and space: out[c] (+)= sum x[b,c,:]  (bias gradients);
 * two launches through a caller-owned workspace of nvf_channel_sum_workspace(c) bytes */
size_t nvf_channel_sum_workspace(int c);
int nvf_channel_sum(const float* x, float* out, void* workspace, size_t workspace_bytes, int batch, int c,
                    int spatial, int accumulate, void* stream);

/* several bias gradients at once (<= 12 tensors of the same batch): outs[i][c] = sum xs[i][b,c,:]; two launches */
size_t nvf_multi_channel_sum_workspace(int total_channels);
int nvf_multi_channel_sum(const float* const* xs, float* const* outs, const int* channels, const int* spatials,
                          int ntensors, int batch, void* workspace, size_t workspace_bytes, NvfStepCtx* ctx,
                          void* stream);

/* nvf_wgrad_reduce_multi and the partial pass of nvf_multi_channel_sum in one launch (independent work), then the
 * bias sums' final pass; same results as the two separate calls.  Per-gradient addends (addends[i], or addends itself,
 * may be NULL: dws[i][j] = sum of slabs + addends[i][j] -- the weight-rate gradient of nvf_step_head's rate job) and,
 * optionally, the optimiser applied to every element it writes (adam NULL: none). */
int nvf_wgrad_reduce_multi_and_sums_fused(const float* const* slabs, float* const* dws, const int* nslabs,
                                          const int* jtotals, int n, const float* const* addends,
                                          const NvfAdamFuse* adam, const float* const* xs, float* const* outs,
                                          const int* channels, const int* spatials, int ntensors, int batch,
                                          void* workspace, size_t workspace_bytes, NvfStepCtx* ctx, void* stream);

/* The latent tail of a training step (backward of NVFPCC.py:186-196's latent generator on [batch, c <= 8, spatial]
 * tensors): gradient of the latent rate (+ dx_addend) -> GDN backward -> 1x1x1 weight and bias gradients, i.e.
 * nvf_latent_rate (want_grad) + nvf_gdn_bwd + nvf_wgrad + the bias sum.  Queued in `ctx`, it runs as ONE workgroup of
 * the next nvf_wgrad_trunk_partial or nvf_wgrad_reduce_multi_and_sums_fused call that is given the
 * same ctx, whichever comes first (every input must already be enqueued on that call's stream), instead of three
 * dependent launches.  NVF_EINVAL: ctx is not an initialised context, or another tail is pending in it. */
int nvf_latent_tail_queue(NvfStepCtx* ctx, const float* lat, const int64_t* block_ids, const float* sigma, const float* mu,
                          const float* dx_addend, float* dlat, float* dsigma, float* dmu, const float* g_dev,
                          float g_host, int mode, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                          const float* h, const float* beta_hat, const float* gamma_hat, float* dh, float* dbeta_hat,
                          float* dgamma_hat, const float* e, float* dw, float* db, int batch, int c, int spatial);
int nvf_latent_tail_pending(const NvfStepCtx* ctx);
void nvf_latent_tail_cancel(NvfStepCtx* ctx);

/* ---- GDN / IGDN (gdn_3d.py:72-95, 137-159; LowerBound gdn_3d.py:13-29) ----------
 * beta = max(beta_hat, beta_bound)^2 - 2^-36, gamma = max(gamma_hat, 2^-18)^2 - 2^-36;
 * norm[c] = sqrt(beta[c] + sum_j gamma[c][j] x[j]^2); y = x / norm (GDN) or x * norm (IGDN).
 * bwd overwrites dx, dbeta_hat[c], dgamma_hat[c][j] (LowerBound pass-through rule applied to
 * the summed gradient); workspace: nvf_gdn_bwd_workspace(c) bytes; c <= 32. */
int nvf_gdn_fwd(const float* x, const float* beta_hat, const float* gamma_hat, float* y, int batch, int c,
                int spatial, int inverse, void* stream);
size_t nvf_gdn_bwd_workspace(int c);
int nvf_gdn_bwd(const float* x, const float* beta_hat, const float* gamma_hat, const float* dy, float* dx,
                float* dbeta_hat, float* dgamma_hat, void* workspace, size_t workspace_bytes, int batch, int c,
                int spatial, int inverse, void* stream);

/* ---- latent generator + quantiser, forward, in one launch (SingleLayerLatentGen network.py:4592-4612 followed by
 * QuantGaussianLikelihood network.py:4514-4539): h = conv1x1(e) + bias, lat = GDN(h), x_rounded = round(lat),
 * bits[0] as nvf_latent_rate.  Same arithmetic and order as nvf_conv3d_gather(k = 1) + nvf_gdn_fwd +
 * nvf_latent_rate (bit-identical outputs); c <= 8; w_fwd is the packed [ci][1][co] layout. */
int nvf_latent_fwd(const float* e, const float* w_fwd, const float* bias, const float* beta_hat,
                   const float* gamma_hat, const int64_t* block_ids, const float* sigma, const float* mu, float* h,
                   float* lat, float* x_rounded, float* bits, int batch, int c, int spatial, int mode, uint64_t seed,
                   uint64_t step, const uint64_t* step_dev, void* stream);

/* ---- latent quantisation + Gaussian rate (network.py:4514-4539, 145-161) --------
 * x_rounded = round(x) (half-to-even); v = x + (U-.5) (mode 0 = train) or x_rounded (mode 1 = eval);
 * bits[0] = sum -log2(max(Phi((v-mu+.5)/|s|) - Phi((v-mu-.5)/|s|), 1e-8)).
 * U comes from `u` if non-NULL, else Philox keyed by (seed, block_ids[b], step + *step_dev): one stream per
 * leaf block, so the noise does not depend on how blocks are sharded over GPUs; block_ids NULL
 * means 0..B-1.  Gradients (each optional, overwritten) are already multiplied by the upstream
 * gradient g = g_host * (g_dev ? *g_dev : 1): dx = dx_addend + g dbits/dx (identity through the
 * round and the noise; dx_addend, optional, is the decoder's gradient w.r.t. x_rounded), dsigma[c], dmu[c].  The LowerBound at 1e-8 passes when like >= 1e-8 or the incoming
 * gradient is negative (network.py:66-72). */
int nvf_latent_rate(const float* x, const float* u, const int64_t* block_ids, const float* sigma, const float* mu,
                    float* x_rounded, float* bits, float* dx, const float* dx_addend, float* dsigma, float* dmu,
                    const float* g_dev, float g_host, int batch, int c, int spatial, int mode, uint64_t seed,
                    uint64_t step, const uint64_t* step_dev, void* stream);

/* ---- weight rate (network.py:4777-4778, 301-305): one quantised kernel ---------
 * bits[0] = sum -log2(max(Phi((w-mu+1/32)/|s|) - Phi((w-mu-1/32)/|s|), 1e-8)), w = round(16 k)/16.
 * dk[i], dsigma[0], dmu[0] (optional) get g * d bits / d(.), overwritten or accumulated. */
int nvf_weight_rate(const float* kernel, int n, const float* sigma, const float* mu, float* bits, float* dk,
                    float* dsigma, float* dmu, const float* g_dev, float g_host, int accumulate, void* stream);

/* all (<= 8) quantised kernels in two launches: bits[l] per layer; dks[l][i] += g dbits/dk (dks or entries may be
 * NULL); dsigma[0], dmu[0] overwritten with the sum over layers (network.py:4777-4778). */
size_t nvf_weight_rate_batch_workspace(void);
int nvf_weight_rate_batch(const float* const* kernels, float* const* dks, const int* ns, int nlayers,
                          const float* sigma, const float* mu, float* bits, float* dsigma, float* dmu,
                          const float* g_dev, float g_host, void* workspace, size_t workspace_bytes, NvfStepCtx* ctx,
                          void* stream);

/* The same rate term split so that its partial pass can ride in the step head (it depends on the parameters only, not
 * on the mini-batch): nvf_step_head given a job computes the per-workgroup partial sums into job->part
 * (nvf_weight_rate_batch_workspace() bytes) and WRITES g * dbits/dk to job->dk[l] (not accumulated: the caller hands
 * those buffers to nvf_wgrad_reduce_multi_and_sums_fused as addends); nvf_weight_rate_batch_final then adds the partials in
 * the usual fixed order (queued in ctx between nvf_finals_begin / nvf_finals_flush, like nvf_weight_rate_batch's). */
typedef struct NvfRateJob {
  const float* kernel[8];
  float* dk[8];            /* entries may be NULL */
  int32_t n[8];
  int32_t nlayers, reserved;
  const float* sigma;
  const float* mu;
  float* part;
  float g, reserved2;
} NvfRateJob;
int nvf_weight_rate_batch_final(const NvfRateJob* job, float* bits, float* dsigma, float* dmu, NvfStepCtx* ctx,
                                void* stream);


/* ---- deferred final passes ------------------------------------------------------
 * nvf_focal_loss_multi, nvf_multi_channel_sum / nvf_wgrad_reduce_multi_and_sums_fused and nvf_weight_rate_batch end with a
 * tiny launch that adds per-workgroup partial sums in a fixed order.  Between nvf_finals_begin(ctx) and
 * nvf_finals_flush(ctx, stream) the final passes of calls given that ctx (at most one of each kind; further ones are
 * launched as usual) are queued in the context and flush runs them in ONE launch on `stream`: their outputs (the loss
 * terms, the bias gradients, the weight-rate bits and d/dsigma, d/dmu) exist only after the flush.  Same device code:
 * identical results.  Used by the training step, where nothing reads those outputs before the optimiser
 * (NVFPCC.py:161-223).  nvf_finals_begin returns NVF_EINVAL when a queue is already open on ctx. */
int nvf_finals_begin(NvfStepCtx* ctx);
int nvf_finals_flush(NvfStepCtx* ctx, void* stream);
void nvf_finals_cancel(NvfStepCtx* ctx);   /* drop the queue without launching (error paths) */

/* workspace (bytes) for the two-stage reductions of nvf_focal_loss / nvf_metrics */
size_t nvf_reduce_workspace(void);

/* ---- losses (utils/loss.py:61-72, 94-111) fused with their gradient ------------
 * loss[0] (+)= sum -a_t (1-p_t)^2 w ln(p_t),  p_t = max(p or 1-p, 1e-9), a_t = alpha or 1-alpha,
 * w = 1 (dist NULL: get_focal_dense) or dist + gt*beta (get_surf_focal_dense).
 * dp (optional) receives g * d loss / d p with g = g_host * (g_dev ? *g_dev : 1); with chain_sigmoid
 * it is further multiplied by p (1 - p), i.e. it is the gradient w.r.t. the head's logit. */
int nvf_focal_loss(const float* p, const float* gt, const float* dist, float alpha, float beta, float* loss,
                   float* dp, const float* g_dev, float g_host, void* workspace, size_t workspace_bytes, int64_t n,
                   int accumulate, int chain_sigmoid, void* stream);

/* up to 3 focal terms (the objective's main output + two heads, NVFPCC.py:166-184) in one launch pair;
 * loss[t] overwritten; dps[t] (optional) = d loss_t / d p_t, times p(1-p) with chain_sigmoid. */
int nvf_focal_loss_multi(const float* const* ps, const float* const* gts, const float* const* dists,
                         float* const* dps, const float* alphas, const float* betas, const int64_t* ns, int nterm,
                         float* loss, int chain_sigmoid, void* workspace, size_t workspace_bytes, NvfStepCtx* ctx,
                         void* stream);

/* ---- per-block costs of a frozen-decoder latent fit (engine.fit_latents) --------
 * p, gt, dist [batch, voxels] (dist may be NULL), x_rounded [batch, c, spatial] (the eval-mode latents), sigma, mu [c].
 * out [batch][2], float64: out[b][0] = the focal sum of block b (the terms of nvf_focal_loss without chain_sigmoid),
 * out[b][1] = its eval-mode latent bits (the terms of nvf_latent_rate in mode 1).  Terms are float32; they are added in
 * float64 in a fixed order by ONE workgroup per block: a row depends neither on batch nor on the block's place in it.
 * NVF_EINVAL: a NULL required pointer, batch < 1, voxels not a multiple of 1024 (the workgroup's stride of 16-byte
 * loads), c * spatial > 64 (the symbols are one wave's work), p / gt / dist not 16-byte aligned. */
int nvf_block_costs(const float* p, const float* gt, const float* dist, float alpha, float beta,
                    const float* x_rounded, const float* sigma, const float* mu, double* out, int batch, int voxels,
                    int c, int spatial, void* stream);

/* metrics (utils/loss.py:74-84, 113-121): out[0..5] (+)= tp, ap, tn, an at thh_acc; sse, denom at thh_sse */
/* Exactness of the five counts: the per-workgroup partials are float32 and exact while a workgroup sees fewer than 2^24
 * elements, i.e. up to n = 2^34 per term (1024 workgroups); the final pass adds them in float64 and rounds once, so a
 * count is the true count rounded to float32 (equal to it below 2^24).  sse: float32 partials, float64 final sum. */
/* with ctx (an open nvf_finals_begin) the final pass joins the deferred ones: out exists after nvf_finals_flush, and
 * `workspace` must then be a buffer no other deferred pass uses */
int nvf_metrics(const float* p, const float* gt, const float* dist, float thh_acc, float thh_sse, float* out,
                void* workspace, size_t workspace_bytes, int64_t n, int accumulate, NvfStepCtx* ctx, void* stream);

/* the same six sums for up to three (prediction, ground truth[, dist]) pairs in one launch: out[6 t + k], overwritten
 * (the main output and the two coarse heads of the TRAIN / TEST log lines, NVFPCC.py:174-179, 214-221); dists or any
 * dists[t] may be NULL (sse = 0).  workspace: nvf_metrics_workspace() bytes (also enough for nvf_metrics). */
size_t nvf_metrics_workspace(void);
int nvf_metrics3(const float* const* ps, const float* const* gts, const float* const* dists, const int64_t* ns,
                 int nterm, float thh_acc, float thh_sse, float* out, void* workspace, size_t workspace_bytes,
                 NvfStepCtx* ctx, void* stream);

/* dlogit = dp * p * (1 - p)   (sigmoid backward of network.py:4761,4764,4768) */
int nvf_sigmoid_bwd(const float* dp, const float* p, float* dlogit, int64_t n, void* stream);

/* out = dy where y > 0 else 0   (ReLU backward of network.py:4760-4766) */
int nvf_relu_bwd(const float* dy, const float* y, float* out, int64_t n, void* stream);

/* get_se (utils/loss.py:123-128): out[b,0,:] = ((p > thh) * dist)^2, out[b,1,:] = p; out is [B,2,spatial] */
int nvf_squared_error_map(const float* p, const float* dist, float thh, float* out, int batch, int spatial,
                          void* stream);

/* 2x2x2 max pooling, stride 2 (MultiscaleProcessor, NVFPCC.py:76-88) */
int nvf_maxpool2(const float* x, float* y, int batch_channels, int d, int h, int w, void* stream);

/* ---- optimiser (torch.optim.Adam defaults, NVFPCC.py:116,124) -------------------
 * one fused update over a flat buffer; step counts from 1. */
int nvf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, int step, void* stream);

/* The tail of a training step with every per-step scalar in device memory (so it can be a node of a replayed HIP
 * graph, behind the data-parallel all-reduce).  One launch does
 *   - nvf_adam_step over n floats with coef_dev[0] = lr / (1 - beta1^t), coef_dev[1] = sqrt(1 - beta2^t) (coef_dev
 *     NULL: the host values coef0_host, coef1_host) -- nvf_adam_coefficients() gives exactly the two floats
 *     nvf_adam_step would use, so the updates are identical.  An element whose gradient is NaN / +-inf keeps its
 *     parameter and moments and is counted in acc[6] (the reference checks before opt.step(), NVFPCC.py:199-212);
 *   - when acc is non-NULL, the epoch's running sums behind the TRAIN log line (NVFPCC.py:190-221, 256-281, without
 *     the per-step .item() syncs): acc[0..2] += loss_terms[0..2]; acc[3] += lbits[0] * (inv_npts_dev ? *inv_npts_dev :
 *     inv_npts_host) (b_latent, :161); acc[4] += sum(nbits[0..nnb)) * nbits_scale (b_net, :162); acc[5] += number of
 *     non-finite terms among those; acc[7] += 1; and, when counts (the 18 floats of nvf_metrics3) is non-NULL, the
 *     per-step ratios the reference averages: acc[8 + 2t] += tp_t / ap_t, acc[9 + 2t] += tn_t / an_t for t = main
 *     output, head 0, head 1 (get_acc_dense, loss.py:74-84), acc[14] += sse, acc[15] += denom (get_sse1);
 *   - when sched_rows is non-NULL, the hand-over to the next step: row sched_cursor[0] of the caller's schedule
 *     (sched_words int64 words per row: whatever the step's kernels read from sched_buf -- block ids, noise step, rate
 *     coefficient, Adam coefficients) is copied over sched_buf and the cursor advances, so a replayed graph needs no
 *     host-to-device copy per step.
 * done: one uint32 of device memory, zero before the first call (the last workgroup to arrive does the scalars and
 * resets it); required when acc or sched_rows is given. */
typedef struct NvfStepTail {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  const float* coef_dev;
  float coef0_host, coef1_host, beta1, beta2, eps;
  int32_t nnb;
  const float* loss_terms;
  const float* lbits;
  const float* nbits;
  const float* inv_npts_dev;
  float inv_npts_host, nbits_scale;
  const float* counts;
  float* acc;
  int64_t* sched_buf;
  const int64_t* sched_rows;
  uint64_t* sched_cursor;
  uint32_t* done;
  int32_t sched_words, reserved;
} NvfStepTail;
int nvf_step_tail(const NvfStepTail* args, void* stream);

/* nvf_finals_flush and the tail of the training step in the same launch (single-GPU steps: nothing sits between the
 * gradients and the optimiser): every gradient element a queued final pass writes inside [tail->g, tail->g + tail->n)
 * -- bias sums, d/dsigma and d/dmu of the weight rate, the stem's GDN parameter gradients -- gets tail's Adam update on
 * the spot; the elements of the nranges half-open index ranges ranges[2 r], ranges[2 r + 1] (gradients that earlier
 * launches wrote directly, e.g. the latent tail's) get it from a workgroup of their own; the workgroup that ran the
 * loss / rate / metrics passes adds the epoch statistics; the last workgroup to arrive hands the step buffer over to
 * the next schedule row.  Together with nvf_wgrad_reduce_multi_and_sums_fused (the weight gradients) this covers what
 * nvf_step_tail does; the caller makes the ranges the exact complement. */
int nvf_finals_flush_tail(NvfStepCtx* ctx, const NvfStepTail* tail, const int64_t* ranges, int nranges, void* stream);
/* nvf_wgrad_reduce_multi_and_sums_fused with adam (required) and nvf_finals_flush_tail as ONE call, two launches: the
 * optimiser of such a step is split over both, and a caller that fails or is interrupted between two calls would hold
 * half-updated parameters.  Same arguments, same bits; what the second call would refuse is refused before the first
 * launch. */
int nvf_wgrad_reduce_sums_fused_flush_tail(const float* const* slabs, float* const* dws, const int* nslabs,
                                           const int* jtotals, int n, const float* const* addends,
                                           const NvfAdamFuse* adam, const float* const* xs, float* const* outs,
                                           const int* channels, const int* spatials, int ntensors, int batch,
                                           void* workspace, size_t workspace_bytes, NvfStepCtx* ctx,
                                           const NvfStepTail* tail, const int64_t* ranges, int nranges, void* stream);
/* nvf_wgrad_reduce_multi_and_sums_fused (slab reduction with addends and the fused optimiser; no channel sums) and
 * nvf_finals_flush_tail in ONE launch -- for steps whose queued final passes read nothing that reduction writes.
 * Only the final passes' workgroups wait for one another before the schedule hand-over, so the reduction must read
 * nothing from the step buffer: adam->coef_dev may not point into tail->sched_buf (NVF_EINVAL) -- use the copy that
 * nvf_wgrad_trunk_partial (coef_src, coef_live) staged earlier in the step, or host coefficients. */
int nvf_wgrad_reduce_finals_tail(const float* const* slabs, float* const* dws, const int* nslabs, const int* jtotals,
                                 int n, const float* const* addends, const NvfAdamFuse* adam, NvfStepCtx* ctx,
                                 const NvfStepTail* tail, const int64_t* ranges, int nranges, void* stream);
/* The same pairing without the optimiser, for steps whose gradients are not final yet (data parallelism: the all-reduce
 * and nvf_step_tail follow): nvf_wgrad_reduce_multi with addends + nvf_finals_flush in ONE launch.  Same condition: no
 * queued final pass may read what the reduction writes. */
int nvf_wgrad_reduce_finals(const float* const* slabs, float* const* dws, const int* nslabs, const int* jtotals, int n,
                            const float* const* addends, NvfStepCtx* ctx, void* stream);
int nvf_adam_coefficients(float lr, float beta1, float beta2, int step, float* coef_host);
/* ... of n consecutive steps step0, step0 + 1, ...: coef_host[2 k], coef_host[2 k + 1] (the rows of a schedule) */
int nvf_adam_coefficients_n(float lr, float beta1, float beta2, int step0, int n, float* coef_host);

/* rows: dst[r,:] = src[idx[r],:]  (emb[indices], NVFPCC.py:158) and its transpose
 * dst[idx[r],:] += src[r,:] (indices unique within a call) */
int nvf_gather_rows(const float* src, const int64_t* idx, float* dst, int rows, int width, void* stream);
int nvf_scatter_add_rows(const float* src, const int64_t* idx, float* dst, int rows, int width, void* stream);

/* up to 6 gathers sharing one index vector: dsts[t][r,:] = srcs[t][idx[r],:] */
int nvf_gather_rows_multi(const float* const* srcs, float* const* dsts, const int* widths, int n,
                          const int64_t* idx, int rows, void* stream);

/* The head of a training step (NVFPCC.py:149-160) in ONE launch: nvf_prepare_weights, nvf_pack_mfma_all and
 * nvf_gather_rows_multi.  Pack job j packs layout pack_bwd[j] (0: w_fwd, 1: w_bwd) of layer-table row pack_layers[j]
 * (kinds / c0s / c1s as in nvf_pack_mfma_all; npack may be 0); a packed element recomputes its effective weight from
 * the raw kernel, so nothing in the launch waits for anything else.  Same results as the three calls, bit for bit. */
int nvf_step_head(const void* table_dev, int nlayers, int q, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                  float* const* pack_dsts, const int* pack_kinds, const int* pack_c0s, const int* pack_c1s,
                  const int* pack_layers, const int* pack_bwd, int npack, const float* const* srcs,
                  float* const* dsts, const int* widths, int n, const int64_t* idx, int rows,
                  const NvfRateJob* rate /* may be NULL: see nvf_weight_rate_batch_final */, void* stream);

/* nvf_step_head AND nvf_stem_latent_fwd (latent generator + quantiser + up0 / IGDN / conv0 of the mini-batch) in ONE
 * launch, (c0, c1) = (8, 16) or (16, 32), ch <= 8, rows <= 32: the stem's workgroups derive their effective weights
 * from the raw parameters of layer-table rows lat_row / up0_row / conv0_row themselves (network.py:611-620, 735-740:
 * the arithmetic of nvf_prepare_weights, element by element) and fetch their latents as emb[idx[b]], so nothing in the
 * launch waits for anything else.  Same results as the two calls, bit for bit.  block ids of the latent noise = idx. */
typedef struct NvfStemHead {
  const float* emb;            /* latent table [N, ch, 2, 2, 2] */
  const float* lat_beta_hat;   /* GDN of the latent generator */
  const float* lat_gamma_hat;
  const float* sigma;          /* entropy coder [ch] */
  const float* mu;
  const float* beta_hat;       /* IGDN of the decoder */
  const float* gamma_hat;
  float* h;                    /* outputs of nvf_stem_latent_fwd */
  float* lat;
  float* x_rounded;
  float* bits;
  float* a0;
  float* h0;
  float* y1;
  int32_t lat_row, up0_row, conv0_row;
  int32_t mode, ch, c0, c1, reserved;
} NvfStemHead;
int nvf_step_head_stem(const void* table_dev, int nlayers, int q, uint64_t seed, uint64_t step,
                       const uint64_t* step_dev, float* const* pack_dsts, const int* pack_kinds, const int* pack_c0s,
                       const int* pack_c1s, const int* pack_layers, const int* pack_bwd, int npack,
                       const float* const* srcs, float* const* dsts, const int* widths, int n, const int64_t* idx,
                       int rows, const NvfRateJob* rate /* may be NULL */, const NvfStemHead* stem, void* stream);

/* U[0,1) floats, Philox4x32-10 keyed by (seed, stream_id), counter = element index */
int nvf_uniform(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);

/* ---- occupancy thresholding + compaction (NVFPCC.py:520,532-535,631-634) --------
 * For each block b, voxel (z,y,x) with p > thh: coords (origin[b] + (z,y,x)) appended in
 * raster order (b, z, y, x) -- the order torch.nonzero gives.  counts[b] = points of
 * block b.  Two-phase: call with coords == NULL to get counts, exclusive-scan them on
 * the host or device into offsets, then call again with coords/offsets. */
int nvf_threshold_count(const float* p, float thh, int32_t* counts, int batch, int voxels, void* stream);
int nvf_threshold_compact(const float* p, float thh, const int32_t* offsets, const int32_t* origins,
                          int32_t* coords, int batch, int dim, void* stream);

/* ---- pre-processing: exact squared distance of every voxel of every 32^3 leaf block to the nearest input
 * point (util_get_grids.py:19-46; gt_grid = (d2 == 0), dist = sqrt(d2)).  pts int32 [P,3] sorted by block,
 * blk_off [N+1] their ranges, origins int32 [N,3], (nb_off, nb_idx) a CSR list of candidate blocks per block
 * (the block itself first, then occupied blocks within +-2 block steps).  d2out int32 [N,32,32,32], axes (x,y,z). */
int nvf_nearest_dist2(const int32_t* pts, const int32_t* blk_off, const int32_t* origins, const int32_t* nb_off,
                      const int32_t* nb_idx, int32_t* d2out, int nblocks, void* stream);

/* ---- point-cloud metrics: exact 1-NN, k-NN + PCA normals, D1 / D2 error sums (nvfpcc_amd/pc_metrics.py) -----------
 * Geometry PSNR as pc_error defines it, for clouds of integer coordinates in [0, 1024) (the caller checks the range).
 *   nn_Y(p)      the point of Y with the least squared distance to p; ties go to the LOWEST input index of Y.
 *   D1(X->Y)     mean_i |x_i - nn_Y(x_i)|^2 (exact integers; equals pc_error's for clouds without duplicate points).
 *   D2(X->Y)     mean_i ((nn_Y(x_i) - x_i) . n_X[i])^2, pc_error's point-to-plane formula.
 * A SORTED CLOUD is int32 [n, 4] rows (x, y, z, input index) ordered by the cell key
 *   key = ((x >> 3) << 8 | (y >> 3) << 4 | (z >> 3)) << 9 | (x & 7) << 6 | (y & 7) << 3 | (z & 7)   of the cell
 *   (x, y, z) = (px >> 3, py >> 3, pz >> 3)  (edge 8 voxels; 64-voxel super-cells in the high bits), and cell_start
 *   int32 [NVF_PC_CELLS + 1] is the exclusive prefix sum of the per-key counts.  The order inside a cell is free.
 * nvf_pc_nearest: for every row of query_sorted, nn_idx / nn_d2 [n_query] at the row's input index receive the input
 *   index of its nearest target and the squared distance (int32, exact).  Exact however far the nearest target is.
 * nvf_pc_knn_normals: the k nearest points of every point of one cloud within itself (the point included, ordered by
 *   (squared distance, input index)), and normals [n, 3] = the unit eigenvector of the smallest eigenvalue of their
 *   covariance (integer sums, fp64 Jacobi), in input order; knn_idx [n, k] (may be NULL) gets the k-NN sets.
 *   cloud_xyz int32 [n, 3] is the same cloud in input order.  3 <= k <= 32 and n >= k, else NVF_EINVAL.
 * nvf_pc_error_sums: over i < n_query with e = target_xyz[nn_idx[i]] - query_xyz[i] (both [., 3], input order):
 *   sums[0] = sum |e|^2 (int64), sums[1] = max |e|^2, d2_sum[0] = sum (e . n)^2 in fp64 where n = normals[i], or
 *   normals[nn_idx[i]] when normals_of_target (normals == NULL: no D2 sum).  Fixed-order two-stage reduction:
 *   repeated calls give the same bits.  workspace >= nvf_pc_workspace_bytes(n_query, .) bytes, 8-byte aligned. */
#define NVF_PC_CELLS (128 * 128 * 128)
size_t nvf_pc_workspace_bytes(int n_query, int n_target);
int nvf_pc_nearest(const int32_t* query_sorted, int n_query, const int32_t* target_sorted, const int32_t* cell_start,
                   int n_target, int32_t* nn_idx, int32_t* nn_d2, void* stream);
int nvf_pc_knn_normals(const int32_t* cloud_sorted, const int32_t* cell_start, const int32_t* cloud_xyz, int n, int k,
                       float* normals, int32_t* knn_idx, void* stream);
int nvf_pc_error_sums(const int32_t* query_xyz, int n_query, const int32_t* target_xyz, const int32_t* nn_idx,
                      const float* normals, int normals_of_target, int64_t* sums, double* d2_sum, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- point-cloud metrics, sparse index: the same searches for clouds of 10, 11 and 12 bits per axis (csrc/pc_sparse.hip)
 * Coordinates lie in [0, 2^bits) (the caller checks the range).  Memory follows the points and the occupied cells, not
 * the volume.  Cells are 8 voxels, super-cells 64, hyper-cells 512; with c = p >> 3, s = p >> 6, h = p >> 9 per axis and
 * hb = bits - 9 the cell key nests the levels:
 *   key = (h.x << 2 hb | h.y << hb | h.z) << 18 | ((s.x & 7) << 6 | (s.y & 7) << 3 | (s.z & 7)) << 9
 *       | (c.x & 7) << 6 | (c.y & 7) << 3 | (c.z & 7)                                     (at most 27 bits)
 * so the points of a node of any level are one contiguous range of the SORTED CLOUD (int32 [n, 4] rows (x, y, z, input
 * index) ordered by key; the order inside a cell is free).  With M occupied cells and S occupied super-cells, both
 * numbered in key order:
 *   cell_start   int32 [M + 1]   exclusive prefix sum of the points per occupied cell.
 *   super_mask   uint64 [S, 8]   512-bit occupancy of the super-cell's cells: word = c.x & 7, bit = (c.y & 7) << 3 | c.z & 7.
 *   super_first  int32 [S]       number of the super-cell's first occupied cell; the cell of bit b of word w is number
 *                                super_first + popcount(words below w) + popcount(word w below bit b).
 *   super_table  int32 [NVF_PC_SPARSE_SUPERS(bits)]  at key >> 9: the super-cell's number, or -1 when it is empty.
 *   hyper_table  int32 [NVF_PC_SPARSE_HYPERS(bits)]  at key >> 18: 1 when the hyper-cell holds a point, else 0.
 * nvf_pc_sparse_build fills super_mask, super_first and both tables of `index` (whose sorted, cell_start, sizes and bits
 *   the caller has set) from cell_key int32 [M], the keys of the occupied cells ascending, and cell_super int32 [M],
 *   the number of each cell's super-cell.  Integer ORs and owner-written rows: the same bits on every call.
 * nvf_pc_nearest_sparse / nvf_pc_knn_normals_sparse: nvf_pc_nearest / nvf_pc_knn_normals on that index, the same
 *   definitions and the same answers (query_sorted is sorted by the same key).  d2 <= 3 * 4095^2 < 2^31.
 * A NULL pointer (knn_idx excepted), bits outside 10..12, sizes that contradict each other, k outside 3..32 or n < k give
 *   NVF_EINVAL before any device work.  nvf_pc_error_sums serves every bits unchanged. */
#define NVF_PC_SPARSE_SUPERS(bits) (1 << (3 * ((bits) - 6)))
#define NVF_PC_SPARSE_HYPERS(bits) (1 << (3 * ((bits) - 9)))
typedef struct NvfPcSparseIndex {
  int32_t* sorted;
  int32_t* cell_start;
  uint64_t* super_mask;
  int32_t* super_first;
  int32_t* super_table;
  int32_t* hyper_table;
  int32_t n, n_cells, n_supers, bits;
} NvfPcSparseIndex;
int nvf_pc_sparse_build(const NvfPcSparseIndex* index, const int32_t* cell_key, const int32_t* cell_super, void* stream);
int nvf_pc_nearest_sparse(const int32_t* query_sorted, int n_query, const NvfPcSparseIndex* target, int32_t* nn_idx,
                          int32_t* nn_d2, void* stream);
int nvf_pc_knn_normals_sparse(const NvfPcSparseIndex* cloud, const int32_t* cloud_xyz, int k, float* normals,
                              int32_t* knn_idx, void* stream);

/* ---- occupancy selection (nvfpcc_amd/thh_select.py, csrc/occ_select.hip) -------------------------------------------
 * The sort key of a probability is its bit pattern (monotone for floats >= 0; -0.0 counts as +0.0).  A key above the
 * bits of 1.0f (NaN, a negative value, a value over 1) is an input error: such voxels go into no bin and are counted
 * in bad[b] (uint32 [batch], always written); the caller raises on a non-zero total.  All sums are integers.
 * nvf_occ_hist: p [batch, voxels]; bin = (key >> shift) & (2^nbits - 1), 1 <= nbits <= 11, shift + nbits <= 32.
 *   prefix (may be NULL) uint32 [batch]: block b counts only voxels with key >> (shift + nbits) == prefix[b].
 *   count uint32 [batch, 2^nbits].  Riders, each pair NULL or not together: d2 int32 [batch, voxels] with values in
 *   [0, 2^25) -> sum_d2 uint64 [batch, 2^nbits]; gt uint8 [batch, voxels] (non-zero = occupied) -> count_gt uint32
 *   [batch, 2^nbits].  Three calls (shift, nbits) = (21, 11), (10, 11), (0, 10) walk the key from the top.
 * nvf_occ_hist_edges: the same with bin = number of edges e with p > e: edges float [nedges] ascending on the
 *   device, 1 <= nedges <= 2047, rows of nedges + 1 bins.  The voxels with p > edges[i] are the bins above i.
 * nvf_threshold_count_v / nvf_threshold_compact_v: nvf_threshold_count / nvf_threshold_compact with one threshold per
 *   block, thh float [batch] on the device. */
int nvf_occ_hist(const float* p, int batch, int voxels, int shift, int nbits, const uint32_t* prefix,
                 const int32_t* d2, const uint8_t* gt, uint32_t* count, uint64_t* sum_d2, uint32_t* count_gt,
                 uint32_t* bad, void* stream);
int nvf_occ_hist_edges(const float* p, int batch, int voxels, const float* edges, int nedges, const int32_t* d2,
                       const uint8_t* gt, uint32_t* count, uint64_t* sum_d2, uint32_t* count_gt, uint32_t* bad,
                       void* stream);
int nvf_threshold_count_v(const float* p, const float* thh, int32_t* counts, int batch, int voxels, void* stream);
int nvf_threshold_compact_v(const float* p, const float* thh, const int32_t* offsets, const int32_t* origins,
                            int32_t* coords, int batch, int dim, void* stream);

/* ---- level-of-detail decode (nvfpcc_amd/recon.py: reconstruct_points_lod, csrc/lod_points.hip) ----------------------
 * A coarse cloud comes from one of the two coarse classifier heads: level 1 = conv1_cls on the 16^3 grid, level 2 =
 * conv0_cls on the 8^3 grid.
 * nvf_head_occ_bits: x [batch, c, d^3] (the activation the head reads), w_fwd the head's forward-packed 3^3 weights
 *   (nvf_pack_conv_weight), bias [1] or NULL; the threshold is thh_v[b] when thh_v (float [batch] on the device) is
 *   given, else thh.  words uint64 [batch, d^3 / 64]: bit k of word w of a block is set when its voxel 64 w + k (raster
 *   order z, y, x) has p > t, with p the very float nvf_conv3d_gather (act = NVF_ACT_SIGMOID) stores for that voxel:
 *   the same fmaf chain and the same sigmoid, never written to memory.  counts int32 [batch] = set bits per block
 *   (cleared by the call, popcounts added in integers).  (c, d) is (8, 16), (16, 16), (16, 8) or (32, 8); anything
 *   else is NVF_EINVAL before any device work.
 * nvf_points_from_bits: words as above, d = 8, 16 or 32 (8, 64 or 512 words per block; 32 is the grid of the lossless
 *   coders' occupancy words, below); offsets int32 [batch] the exclusive prefix sum of counts; origins int32 [batch, 3]
 *   (NULL: zeros); points int32 [n, 3] receives (origin >> shift) + (z, y, x) per set bit in (block, z, y, x) order,
 *   the order of nvf_threshold_compact.  shift = 0..2.  A slot outside [0, n) is not written. */
int nvf_head_occ_bits(const float* x, const float* w_fwd, const float* bias, float thh, const float* thh_v,
                      uint64_t* words, int32_t* counts, int batch, int c, int d, void* stream);
int nvf_points_from_bits(const uint64_t* words, const int32_t* offsets, const int32_t* origins, int32_t* points, int n,
                         int batch, int d, int shift, void* stream);

/* ---- lossless geometry (nvfpcc_amd/lossless_pack.py, csrc/occ_rans.hip) ---------------------------------------------
 * The true occupancy of the 32^3 leaf blocks, entropy-coded under the probabilities p of the eval forward.  p and gt
 * are float [batch, 32768] in raster order (z, y, x); gt non-zero = occupied.
 * Context of a voxel, from the float32 bits of p alone: side = p > 0.5f; q = side ? 1.0f - p : p; key = bits(q) >> 21;
 *   idx = clamp((bits(0.5f) >> 21) - key, 0, 127); ctx = 2 idx + side, 256 contexts.  Every bit pattern has a context.
 * nvf_occ_ctx_hist: cnt[ctx] += voxels, occ[ctx] += occupied voxels (uint64 [256] each), bad[0] += voxels whose p is an
 *   input error as for nvf_occ_hist (NaN, negative, over 1; -0.0 counts as +0.0): they are in no context and the caller
 *   raises.  The three accumulate over calls (the caller clears them once); all sums are integers.  voxels <= 2^24.
 * The coder is binary rANS with 64-bit states in [2^31, 2^63), 32-bit words and 16-bit frequencies: f1 int32 [256] on the
 *   device is the frequency of "occupied" per context out of 65536 (an entry outside [1, 65535] is pulled inside);
 *   symbol 1 = (start 0, freq f1), symbol 0 = (start f1, freq 65536 - f1).  A GROUP is `group` consecutive blocks (the
 *   last one of a call may be shorter), 1 <= group <= NVF_OCC_RANS_MAX_GROUP, coded by one 64-lane wave with 64 states:
 *   symbol i = b_local * 32768 + raster voxel belongs to lane i % 64 at step i / 64.
 * nvf_occ_rans_encode: states uint64 [groups, 64] = the final states (the decoder's initial ones); words uint32
 *   [groups, group * 32768] is the worst-case region of each group, filled from the END of the region of its own blocks:
 *   group g's words are words[g][nb * 32768 - nwords[g] .. nb * 32768) with nb its number of blocks, in the order the
 *   decoder reads them; nwords uint32 [groups].  gt_words (may be NULL) uint64 [batch, 512]: the occupancy words of gt,
 *   bit k of word w = voxel 64 w + k, the format of nvf_head_occ_bits.
 * nvf_occ_rans_decode: words uint32 [total_words], group g's at words[word_off[g] .. word_off[g] + nwords[g]) (word_off
 *   int64 [groups], nwords uint32 [groups]).  occ_words uint64 [batch, 512] and counts int32 [batch] (set bits per block)
 *   are written for every block.  status int32 [groups] is always written: 0, or the OR of NVF_OCC_RANS_PAST_END (a word
 *   was wanted beyond the group's words, or its range leaves [0, total_words): such reads yield 0 and touch no memory),
 *   NVF_OCC_RANS_BAD_STATE (a final state is not 2^31) and NVF_OCC_RANS_WORDS_LEFT (words were left over).  No content
 *   of states, words, word_off or nwords makes the kernel read outside words[0 .. total_words).
 * nvf_points_from_bits (d = 32, shift 0) turns occ_words and counts into the points.
 * The coder's step, a group's word window and the status are csrc/occ_coder.h's, shared with the scalable coder below. */
#define NVF_OCC_RANS_MAX_GROUP 1024
#define NVF_OCC_RANS_PAST_END 1
#define NVF_OCC_RANS_BAD_STATE 2
#define NVF_OCC_RANS_WORDS_LEFT 4
int nvf_occ_ctx_hist(const float* p, const float* gt, int batch, int voxels, uint64_t* cnt, uint64_t* occ, uint64_t* bad,
                     void* stream);
int nvf_occ_rans_encode(const float* p, const float* gt, const int32_t* f1, int batch, int group, uint64_t* states,
                        uint32_t* words, uint32_t* nwords, uint64_t* gt_words, void* stream);
int nvf_occ_rans_decode(const float* p, const int32_t* f1, const uint64_t* states, const uint32_t* words,
                        const int64_t* word_off, const uint32_t* nwords, int64_t total_words, int batch, int group,
                        uint64_t* occ_words, int32_t* counts, int32_t* status, void* stream);

/* ---- scalable lossless geometry (nvfpcc_amd/lossless_lod_pack.py, csrc/occ_hier.hip) --------------------------------
 * The same occupancy coded coarse to fine in ONE stream per group: a decoder that stops after the first or the second
 * section holds the exact 8^3 or 16^3 max-pool of every block.  Levels: 0 = the 32^3 voxels, 1 = the 16^3 cells, 2 = the
 * 8^3 cells, all in raster order (z, y, x); the children of cell (Z, Y, X) are (2Z + dz, 2Y + dy, 2X + dx) one level
 * down, in order j = 4 dz + 2 dy + dx.
 * Pyramid of a block, from p with exact float comparisons only: P0 = p; P1[c] = the maximum of the 8 children of 16^3
 *   cell c, folded in child order as m = c0, m = (cj > m) ? cj : m (so the first of equal values, and of +0.0 / -0.0,
 *   stays); K1[c] = min(3, number of children with p > 0.5f); P2 and K2 likewise from P1 (children with P1 > 0.5f).  An
 *   input error (the rule of nvf_occ_ctx_hist) ANYWHERE in p is counted, and the encoder raises before it codes.
 * Contexts, NVF_OCC_HIER_CONTEXTS = 3 x 4 x 256: ctx = (level * 4 + k) * 256 + occ_ctx(P_level[cell]), with occ_ctx the
 *   context function above; k = K2[c] for an 8^3 cell c, K1[c] for a 16^3 cell c, K1[parent(v)] for a voxel v.
 * Symbols of a group of G consecutive blocks, three sections in this order: section 2 = block by block all 512 cells
 *   of the 8^3 grid; section 1 = block by block, for every OCCUPIED 8^3 cell in raster order, its 8 children in order j;
 *   section 0 = the same from the occupied 16^3 cells to the voxels.  Occupied = the max-pool of the ground truth.
 *   Everything under an empty parent is empty and costs no symbol.  Each section is padded to a multiple of 64 with idle
 *   slots; symbol i of a padded section belongs to lane i % 64 at that section's step i / 64; an idle lane neither
 *   codes nor renormalises.
 * Coder: the binary rANS coder above, unchanged (64-bit states from 2^31, 32-bit words, 16-bit frequencies, symbol 1 =
 *   (start 0, freq f1), the words of a step in ascending lane order for the decoder), ONE stream per group: the 64
 *   states run through sections 2, 1, 0 without a flush in between; the encoder walks section 0, then 1, then 2, each
 *   backwards.  A symbol emits at most one word, so a block's worst case is NVF_OCC_HIER_BLOCK_WORDS = 512 + 4096 +
 *   32768 words.  f1 is int32 [NVF_OCC_HIER_CONTEXTS] on the device (an entry outside [1, 65535] is pulled inside).
 * Occupancy words of a level: uint64 [batch, 512 >> 3 level], bit k of word w of a block = its cell 64 w + k, the
 *   format of nvf_head_occ_bits.  batch <= NVF_OCC_HIER_MAX_BATCH everywhere.
 * nvf_occ_hier_pyramid: p1 float [batch, 4096], k1 uint8 [batch, 4096], p2 float [batch, 512], k2 uint8 [batch, 512];
 *   bad[0] += input errors (uint64, the caller clears it once).  gt (float [batch, 32768], may be NULL) non-zero =
 *   occupied: gt_w0, gt_w1, gt_w2 receive its occupancy words at levels 0, 1 and 2 (untouched without gt).
 * nvf_occ_hier_cells: wpb = words per block, 8, 64 or 512.  counts int32 [batch] = set bits per block.  cells (NULL:
 *   counts only; must be NULL for wpb = 512) int32 [batch * wpb * 64], room for the all-full case: the occupied cells in
 *   (block, raster) order, entry = block * (wpb * 64) + cell; entries past the set bits of the call are not written.
 * nvf_occ_hier_hist: one level's coded symbols.  pv / kv are the level's values and child counts: (p2, k2) at level 2,
 *   (p1, k1) at level 1, (p, k1) at level 0; gt_words the ground truth's words of that level; cells / counts the
 *   nvf_occ_hier_cells list of the level above (unused at level 2).  cnt[ctx] += symbols, occ[ctx] += occupied ones
 *   (uint64 [NVF_OCC_HIER_CONTEXTS] each, accumulated over calls, integers).
 * nvf_occ_hier_encode: cells2 / counts2 and cells1 / counts1 are the lists of gt_w2 and gt_w1.  states, words, nwords
 *   as nvf_occ_rans_encode with a region of group * NVF_OCC_HIER_BLOCK_WORDS words per group, filled from the end of
 *   the region of its own blocks.
 * nvf_occ_hier_decode: ONE section (level) of every group per call, level 2 first.  states uint64 [groups, 64] (in: the
 *   pack's states or those the previous section left; out: the states after this section), pos int64 [groups] (words
 *   consumed so far: 0 before level 2) and status int32 [groups] (cleared by the caller before level 2; flags are ORed
 *   in) carry the coder from call to call.  pv / kv as nvf_occ_hier_hist; cells / counts the list of the words the
 *   previous call decoded (unused at level 2).  occ_words of the level: level 2 writes every word; levels 1 and 0 OR
 *   the occupied cells into words the caller has cleared.  words, word_off, nwords, total_words as
 *   nvf_occ_rans_decode, and the same guarantee: no content of them makes the kernel read outside words[0 ..
 *   total_words), and a damaged stream, which can decode ANY occupancy, writes inside occ_words and lists sized as
 *   above.  Levels 2 and 1 can only report NVF_OCC_RANS_PAST_END, and only for a word that was wanted beyond the
 *   group's words cut to the buffer: a stop there needs only a prefix of them.  Level 0 reports it as
 *   nvf_occ_rans_decode does, also for a range that leaves the buffer, and adds NVF_OCC_RANS_BAD_STATE and
 *   NVF_OCC_RANS_WORDS_LEFT. */
#define NVF_OCC_HIER_CONTEXTS 3072
#define NVF_OCC_HIER_BLOCK_WORDS 37376
#define NVF_OCC_HIER_MAX_BATCH 32768
int nvf_occ_hier_pyramid(const float* p, const float* gt, int batch, float* p1, uint8_t* k1, float* p2, uint8_t* k2,
                         uint64_t* bad, uint64_t* gt_w0, uint64_t* gt_w1, uint64_t* gt_w2, void* stream);
int nvf_occ_hier_cells(const uint64_t* words, int batch, int wpb, int32_t* counts, int32_t* cells, void* stream);
int nvf_occ_hier_hist(int level, const float* pv, const uint8_t* kv, const uint64_t* gt_words, const int32_t* cells,
                      const int32_t* counts, int batch, uint64_t* cnt, uint64_t* occ, void* stream);
int nvf_occ_hier_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                        const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2, const int32_t* cells2,
                        const int32_t* counts2, const int32_t* cells1, const int32_t* counts1, const int32_t* f1,
                        int batch, int group, uint64_t* states, uint32_t* words, uint32_t* nwords, void* stream);
int nvf_occ_hier_decode(int level, const float* pv, const uint8_t* kv, const int32_t* cells, const int32_t* counts,
                        const int32_t* f1, uint64_t* states, int64_t* pos, const uint32_t* words, const int64_t* word_off,
                        const uint32_t* nwords, int64_t total_words, int batch, int group, uint64_t* occ_words,
                        int32_t* status, void* stream);

/* ---- scalable lossless geometry, neighbour contexts (nvfpcc_amd/lossless_nbr_pack.py, csrc/occ_hier.hip) -------------
 * A second context model for the same stream: pyramid, sections, symbol order, idle slots, coder, regions and status
 * rules are those above, and so are the contexts of sections 2 and 1, (level * 4 + k) * 256 + occ_ctx(P): 1024..3071.
 * A voxel v = (z, y, x) of section 0 is coded under the level-1 occupancy around its parent P = (z >> 1, y >> 1, x >> 1)
 * as well.  With s_a = +1 where v's coordinate on axis a is odd, else -1, and O(q) the level-1 occupancy of cell q of
 * the SAME block, 0 outside [0, 16)^3 (blocks do not see each other):
 *   F = O(P + s_z e_z) + O(P + s_y e_y) + O(P + s_x e_x), E = the same sum over the three two-axis offsets, C = O at the
 *   three-axis offset, n = (F * 4 + E) * 2 + C in [0, 32), and
 *   ctx = 3072 + (n * 4 + k) * 256 + occ_ctx(p[v]), k = K1[P] as above.
 * O is the ground truth's max-pool (gt_w1) at the encoder and what section 1 decoded at the decoder: known before the
 * first voxel, and no part of the serial chain.  NVF_OCC_NBR_CONTEXTS = 3072 + 32 * 1024; contexts 0..1023 are never
 * used.  f1 is int32 [NVF_OCC_NBR_CONTEXTS] on the device, 16-byte aligned, entries pulled into [1, 65535].
 * nvf_occ_nbr_hist: the level-0 symbols, cnt / occ uint64 [NVF_OCC_NBR_CONTEXTS] as nvf_occ_hier_hist (which adds levels
 *   1 and 2 to entries 1024..3071 of the same arrays); cells1 / counts1 the list of gt_w1.
 * nvf_occ_nbr_encode: the arguments and results of nvf_occ_hier_encode, with the longer f1.
 * nvf_occ_nbr_decode: section 0 of every group, as nvf_occ_hier_decode at level 0 (states, pos, status in and out, every
 *   guarantee about damaged streams), plus w1 uint64 [batch, 64]: the level-1 words the previous call decoded, of which
 *   cells1 / counts1 are the list.  Sections 2 and 1 are decoded by nvf_occ_hier_decode under the first
 *   NVF_OCC_HIER_CONTEXTS entries of f1. */
#define NVF_OCC_NBR_CONTEXTS 35840
int nvf_occ_nbr_hist(const float* p, const uint8_t* k1, const uint64_t* gt_w0, const uint64_t* gt_w1, const int32_t* cells1,
                     const int32_t* counts1, int batch, uint64_t* cnt, uint64_t* occ, void* stream);
int nvf_occ_nbr_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                       const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2, const int32_t* cells2,
                       const int32_t* counts2, const int32_t* cells1, const int32_t* counts1, const int32_t* f1,
                       int batch, int group, uint64_t* states, uint32_t* words, uint32_t* nwords, void* stream);
int nvf_occ_nbr_decode(const float* p, const uint8_t* k1, const int32_t* cells1, const int32_t* counts1, const uint64_t* w1,
                       const int32_t* f1, uint64_t* states, int64_t* pos, const uint32_t* words, const int64_t* word_off,
                       const uint32_t* nwords, int64_t total_words, int batch, int group, uint64_t* occ_words,
                       int32_t* status, void* stream);

/* ---- scalable lossless geometry, inter contexts (nvfpcc_amd/lossless_inter_pack.py, csrc/occ_hier.hip) --------------
 * A third context model for the same stream: a voxel is coded under a REFERENCE cloud that encoder and decoder both
 * hold (the previous frame's decoded output, say) as well.  Everything but the context of a level-0 symbol is as above.
 * R, the reference words: uint64 [batch, 512] in the format of gt_w0, the reference rasterised onto THIS frame's blocks.
 * R(q) is the reference occupancy of voxel q of the SAME block, 0 outside [0, 32)^3.  For a voxel v = (z, y, x):
 *   a = R(v), f = the sum of R over the six face neighbours of v, r = a ? 2 : (f > 0 ? 1 : 0)   the temporal class
 *   F, E, C as for the neighbour contexts, s = (F * 2 + (E > 0)) * 2 + C in [0, 16)               the spatial class
 *   t = r * 16 + s in [0, 48), ctx = 3072 + (t * 4 + k) * 256 + occ_ctx(p[v]), k = K1[parent]
 * NVF_OCC_INTER_CONTEXTS = 3072 + 48 * 1024; contexts 0..1023 are never used.  f1 is int32 [NVF_OCC_INTER_CONTEXTS] on
 * the device, 16-byte aligned, entries pulled into [1, 65535].
 * nvf_occ_ref_words: points int32 [npts, 3] -> words uint64 [nblocks, 512], which the caller has cleared (bits are ORed
 *   in, so calls accumulate).  A point q belongs to the block whose origin is q & ~31 and sets the bit of voxel
 *   ((q[0] & 31) * 32 + (q[1] & 31)) * 32 + (q[2] & 31) there.  keys int64 [nblocks]: the blocks' origin keys
 *   (o[0] >> 5) << 42 | (o[1] >> 5) << 21 | (o[2] >> 5), origins in [0, 2^NVF_OCC_REF_COORD_BITS), sorted ascending and
 *   distinct; perm int32 [nblocks]: perm[i] = the block whose key is keys[i].  dropped[0] += the points under no block,
 *   a point with a coordinate outside [0, 2^NVF_OCC_REF_COORD_BITS) among them (uint64, cleared by the caller).
 *   Duplicate points are harmless; no content of points, keys or perm makes the kernel write outside words.
 * nvf_occ_inter_hist: the level-0 symbols, as nvf_occ_nbr_hist with ref_words; cnt / occ uint64 [NVF_OCC_INTER_CONTEXTS].
 * nvf_occ_inter_encode: the arguments and results of nvf_occ_nbr_encode, with ref_words and the longer f1.
 * nvf_occ_inter_decode: section 0 of every group, as nvf_occ_nbr_decode with ref_words (every guarantee about damaged
 *   streams holds).  Sections 2 and 1 are decoded by nvf_occ_hier_decode under the first NVF_OCC_HIER_CONTEXTS entries. */
#define NVF_OCC_INTER_CONTEXTS 52224
#define NVF_OCC_REF_COORD_BITS 26
int nvf_occ_ref_words(const int32_t* points, int64_t npts, const int64_t* keys, const int32_t* perm, int nblocks,
                      uint64_t* words, uint64_t* dropped, void* stream);
int nvf_occ_inter_hist(const float* p, const uint8_t* k1, const uint64_t* gt_w0, const uint64_t* gt_w1,
                       const uint64_t* ref_words, const int32_t* cells1, const int32_t* counts1, int batch, uint64_t* cnt,
                       uint64_t* occ, void* stream);
int nvf_occ_inter_encode(const float* p, const float* p1, const uint8_t* k1, const float* p2, const uint8_t* k2,
                         const uint64_t* gt_w0, const uint64_t* gt_w1, const uint64_t* gt_w2, const uint64_t* ref_words,
                         const int32_t* cells2, const int32_t* counts2, const int32_t* cells1, const int32_t* counts1,
                         const int32_t* f1, int batch, int group, uint64_t* states, uint32_t* words, uint32_t* nwords,
                         void* stream);
int nvf_occ_inter_decode(const float* p, const uint8_t* k1, const int32_t* cells1, const int32_t* counts1, const uint64_t* w1,
                         const uint64_t* ref_words, const int32_t* f1, uint64_t* states, int64_t* pos, const uint32_t* words,
                         const int64_t* word_off, const uint32_t* nwords, int64_t total_words, int batch, int group,
                         uint64_t* occ_words, int32_t* status, void* stream);

/* ---- scalable lossless geometry, motion-compensated reference (nvfpcc_amd/lossless_mv_pack.py, csrc/occ_motion.hip) --
 * A layer in FRONT of the inter contexts: the coder above only ever sees R, so R may be built block by block from the
 * reference displaced by that block's own integer vector.  Nothing in the version-4 stream changes.
 * Ref(q) = 1 when the reference cloud holds the point q, q in [0, 2^NVF_OCC_REF_COORD_BITS)^3, and 0 everywhere else.
 * A block with origin o_b and vector d_b = (d0, d1, d2), every |component| <= r <= NVF_OCC_MV_MAX_RADIUS, has the
 *   compensated reference R'_b(v) = Ref(o_b + v - d_b), v in [0, 32)^3, axes in the order of the points' columns, in the
 *   word format of gt_w0 and nvf_occ_ref_words: one uint32 per (v0, v1) row with bit v2, two rows to a uint64 word.
 *   With every d_b = 0, R' is what nvf_occ_ref_words writes whenever the reference's points all lie under the blocks.
 * The reference is held on its OWN blocks: ref_keys int64 [nref] = the distinct keys (as in nvf_occ_ref_words) of q & ~31
 *   over its in-range points, sorted ascending; ref_own uint64 [nref, 512] = their words, filled by nvf_occ_ref_words
 *   (in chunks of at most NVF_OCC_HIER_MAX_BATCH blocks when there are more; nref itself is not bounded).  A block's
 *   window reaches at most 2 x 2 x 2 reference blocks; a block that is absent reads as 0, and so does a window coordinate
 *   outside [0, 2^NVF_OCC_REF_COORD_BITS).  nref == 0 is valid (ref_own and ref_keys are then not read and may be NULL):
 *   words are all 0 and vectors are all 0.
 * nvf_occ_mv_words: origins int32 [nblocks, 3], mv int32 [nblocks, 3] -> words uint64 [nblocks, 512], EVERY word
 *   written.  A vector with a component outside +-NVF_OCC_MV_MAX_RADIUS zeroes that block's words and adds 1 to
 *   status[0] (int32, cleared by the caller).  No content of mv, origins or ref_keys makes the kernel read or write
 *   outside its arrays (origins need not be multiples of 32 for that; the window arithmetic is 64-bit).
 * nvf_occ_mv_search: gt_w0 uint64 [nblocks, 512], the blocks' own words.  For each block the exact Hamming distance
 *   sum popcount(G_b ^ R'_{b,d}) over all (2 radius + 1)^3 vectors d; mv int32 [nblocks, 3] = the vector of the smallest
 *   distance, ties broken by the smaller d0^2 + d1^2 + d2^2, then by the lexicographically smaller (d0, d1, d2): the zero
 *   vector wins every tie it takes part in, and a block whose window is empty gets 0.  cost uint32 [nblocks, 2] = (the
 *   winner's distance, the distance at d = 0).  All sums are integer: every call gives the same bits.
 * Both return NVF_EINVAL on a null pointer, nblocks <= 0 or > NVF_OCC_HIER_MAX_BATCH, nref < 0, and the search on a
 *   radius outside [1, NVF_OCC_MV_MAX_RADIUS]. */
#define NVF_OCC_MV_MAX_RADIUS 8
int nvf_occ_mv_words(const uint64_t* ref_own, const int64_t* ref_keys, int nref, const int32_t* origins, const int32_t* mv,
                     int nblocks, uint64_t* words, int32_t* status, void* stream);
int nvf_occ_mv_search(const uint64_t* gt_w0, const uint64_t* ref_own, const int64_t* ref_keys, int nref,
                      const int32_t* origins, int nblocks, int radius, int32_t* mv, uint32_t* cost, void* stream);

/* ---- pre-processing on the device (nvfpcc_amd/preprocess.py: preprocess_device, csrc/pp_device.hip) ----------------
 * From int32 [P,3] points with coordinates of `bits` bits (10, 11 or 12; anything else is NVF_EINVAL) to everything
 * nvf_nearest_dist2 and the trainer take, without a host pass.  D = bits - 5 is the level of the 32^3 leaves.  A CELL
 * CODE is the 3 D-bit Morton code of a level-D cell (x >> 5, y >> 5, z >> 5), x in the lowest bit of each level: the
 * reference's traversal order of the leaves is ascending cell code.  W = 8^D / 32 is the number of words of the level-D
 * bitmap and cap(L) = min(8^L, npts) bounds the nodes of level L.  Every result is an OR or an integer count, so
 * repeated calls give the same bits.  Call order: keys, (sort the keys ascending), tree, blocks, neighbours, each with
 * the same bits and npts.
 * nvf_pp_keys: clears bitmap and meta, then per point keys[i] = cell code << 15 | (x & 31) << 10 | (y & 31) << 5 |
 *   (z & 31) -- keys is int32 [P] at 10 bits (30-bit keys) and int64 [P] at 11 and 12 (up to 36 bits) --, the point's
 *   bit in bitmap (uint32 [8 W], the level-(D + 1) bitmap: bit = cell code << 3 | child index of the 16^3 cell, so byte
 *   c holds the eight children of cell c), and meta[1] += 1 for a point with a coordinate outside [0, 2^bits) (its key
 *   is the type's largest value, 0x7fffffff or 0x7fffffffffffffff; the caller raises on a non-zero count).
 * nvf_pp_tree: origins int32 [N,3] (room for cap(D) rows) in traversal order; rank_tab uint32 [2 W] = the level-D
 *   bitmap and the number of set bits before each of its words (block id of a cell = a prefix popcount);
 *   octree_bytes uint8 [sum of cap(L), L <= D]: the child-occupancy bytes of level L (bit i = child i), breadth first,
 *   start at byte sum of cap(l) over l < L; nb_off int32 [N+1] (room for cap(D) + 1) the row offsets of the candidate
 *   lists; work uint32 [NVF_PP_WORK_WORDS] is scratch.  A grid-wide prefix sum is three launches (sums per workgroup,
 *   one workgroup scans them, emit); no workgroup waits for another.
 *   meta int32 [NVF_PP_META_INTS]: [0] N, [1] rejected points, [2..9] bytes of level 0..7 (D + 1 of them are written),
 *   [10] nb_off[N], [11] occupied voxels (distinct points; written by nvf_pp_blocks).
 * nvf_pp_blocks: sorted_keys (the type nvf_pp_keys wrote) -> pts int32 [P,3] sorted by block and blk_off int32 [N+1]
 *   (room for cap(D) + 1); N is read from meta on the device.
 * nvf_pp_neighbours: nb_idx int32 [nb_off[N]]: per block the occupied blocks within +-2 block steps of the 2^D grid (an
 *   octant boundary is no boundary), the block itself first, then by squared block distance ((dx, dy, dz)
 *   lexicographic among equals).
 * nvf_pp_grids: dist[i] = sqrtf(d2[i]) correctly rounded, gt[i] = (d2[i] == 0) as 1.0f / 0.0f, i < n; d2 in [0, 2^24);
 *   pointers 16-byte aligned; dist may be the buffer of d2 itself. */
#define NVF_PP_META_INTS 16
#define NVF_PP_WORK_WORDS 11264
int nvf_pp_keys(const int32_t* pts, int npts, int bits, void* keys, uint32_t* bitmap, int32_t* meta, void* stream);
int nvf_pp_tree(const uint32_t* bitmap, int bits, int npts, int32_t* origins, uint32_t* rank_tab, uint8_t* octree_bytes,
                int32_t* nb_off, uint32_t* work, int32_t* meta, void* stream);
int nvf_pp_blocks(const void* sorted_keys, int npts, int bits, const uint32_t* rank_tab, int32_t* meta, int32_t* pts,
                  int32_t* blk_off, void* stream);
int nvf_pp_neighbours(const int32_t* origins, int bits, const uint32_t* rank_tab, const int32_t* nb_off, int32_t* nb_idx,
                      int nblocks, void* stream);
int nvf_pp_grids(const int32_t* d2, float* dist, float* gt, int64_t n, void* stream);

/* ---- PLY text (nvfpcc_amd/ply_io.py, csrc/ply_io.hip) ---------------------------------------------------------------
 * The body of an ASCII PLY, on the device in both directions.  `text` is uint8 [nbytes]; every offset is int64.  A line
 * ends at '\n' or at the end of the text; line k is the k-th of them, blank lines included.  No call reads or writes
 * at or beyond text + nbytes, whatever the bytes, `starts` or `offsets` hold.  Every call refuses null pointers and
 * negative sizes with NVF_EINVAL before any HIP call and returns NVF_OK without a launch when there is nothing to do
 * (nbytes == 0, n == 0, nlines == 0).
 * nvf_ply_count_lines: counts int64 [ceil(nbytes / chunk)], the '\n' in each chunk of `chunk` >= 1 bytes.
 * nvf_ply_line_starts: chunk_first int64 [as counts] = the exclusive prefix sum of counts; starts int64 [nlines]:
 *   starts[k] = the byte offset of the start of line k, for every line k < nlines that the text has (the line after a
 *   final '\n' starts at nbytes and is empty).  Entries of lines the text does not have are left as they were: the
 *   caller fills starts with -1 first.
 * nvf_ply_parse_xyz: one vertex per line first_line + i, i < n; starts holds at least first_line + n entries.  A token
 *   is a maximal run of bytes other than space, tab, CR, LF.  The tokens of columns cx, cy, cz (distinct, < nprops)
 *   must match [+-]?[0-9]{1,10}(\.0*)? with a magnitude <= 2147483647; xyz int32 [n, 3] receives their values (-0 is 0;
 *   0 for a token outside the grammar).  Other tokens are skipped, never interpreted.
 *   status int64 [4], written by the call: [0] lines with fewer than nprops tokens (a line with a negative start or one
 *   >= nbytes has none), [1] lines with a coordinate token outside the grammar or with a byte a host reader may split
 *   at where this one does not (below 0x20 other than tab, LF and a CR right before LF or the end; 0x7f and above),
 *   [2] and [3] the lowest i of either kind, -1 when there is none.
 * nvf_ply_format_sizes: sizes int32 [n] = strlen of "%d %d %d\n" for xyz int32 [n, 3] (INT32_MIN included).
 * nvf_ply_format_xyz: offsets int64 [n + 1], offsets[0] = 0 and offsets[i + 1] = offsets[i] + sizes[i]; writes the
 *   lines to text[offsets[i] ..).  A line that inconsistent offsets would put outside its workgroup's range or outside
 *   [0, nbytes) is not written. */
int nvf_ply_count_lines(const uint8_t* text, int64_t nbytes, int64_t chunk, int64_t* counts, void* stream);
int nvf_ply_line_starts(const uint8_t* text, int64_t nbytes, int64_t chunk, const int64_t* chunk_first, int64_t* starts,
                        int64_t nlines, void* stream);
int nvf_ply_parse_xyz(const uint8_t* text, int64_t nbytes, const int64_t* starts, int64_t first_line, int64_t n, int nprops,
                      int cx, int cy, int cz, int32_t* xyz, int64_t* status, void* stream);
int nvf_ply_format_sizes(const int32_t* xyz, int64_t n, int32_t* sizes, void* stream);
int nvf_ply_format_xyz(const int32_t* xyz, const int64_t* offsets, int64_t n, uint8_t* text, int64_t nbytes, void* stream);

/* ---- voxelisation of a float cloud (nvfpcc_amd/voxelize.py, csrc/voxelize.hip) ---------------------------------------
 * float64 [n, 3] points under the lattice (bits, o, s) -> the distinct lattice points, their counts and the error.  The
 * arithmetic is the format: t = x - o, u = t * inv, q = floor(u + 0.5) forward and x = o + q * s back,
 * every operation rounded to float64 on its own (the file is compiled with contraction off).  inv is 1.0 / s, divided
 * once by the caller.  A point is NON-FINITE if a coordinate is a NaN or an infinity, else OUTSIDE if some u + 0.5 is
 * below 0 or at least 2^bits (decided in float64), else INSIDE.  Call order: (bounds, when the lattice is to be fitted,)
 * quantize, (sort the keys ascending), unique.  Every call returns NVF_EINVAL before any HIP call on a null pointer, n
 * outside [1, 2^30), bits outside 10..12, s or inv not finite and above 0, or a non-finite origin, where it takes them.
 * A lowest-index word is -1 when there is no such point.
 * nvf_vox_bounds: bounds, 8-byte words [NVF_VOX_BOUNDS_WORDS]: [0..2] the minimum and [3..5] the maximum of each axis
 *   over the finite points as doubles (+inf / -inf when there is none), [6] the count of non-finite points, [7] the
 *   lowest index of one.  work [NVF_VOX_BOUNDS_WORK_WORDS] is scratch: one partial record per workgroup, folded by a
 *   final one-workgroup launch.  min and max are exact in any order; no atomics.
 * nvf_vox_quantize: q int32 [n, 3] and keys int64 [n]: for a point inside, its q and key = q0 << 2 bits | q1 << bits |
 *   q2 (30, 33 or 36 bits); for any other, q = -1 and key = INT64_MAX, which sorts last.  status, 8-byte words
 *   [NVF_VOX_STATUS_WORDS], cleared and written by the call: [0] non-finite points, [1] outside points, [2] and [3] the
 *   lowest index of either kind, [4] the maximum as a double and [8 + g], g < [6], the sum per workgroup, also doubles,
 *   of e2 = sum over axes 0, 1, 2 of (x - (o + q s))^2 over the points inside (each partial summed in a fixed order:
 *   the same call gives the same bits), [5] written by nvf_vox_unique, [6] the number of partial sums, [7] zero.
 * nvf_vox_unique: sorted_keys int64 [n] ascending -> pts int32 [M, 3] (room for n rows), the distinct points inside in
 *   ascending key order, counts int32 [M] (room for n) how many keys each had, and M in status[5].  Keys of INT64_MAX
 *   belong to no point.  work int32 [NVF_VOX_MAX_GROUPS] is scratch.  Three launches: sums per workgroup, one workgroup
 *   scans them, emit; no workgroup waits for another.  A run of equal keys may be longer than a workgroup's span and may
 *   straddle two: its count is the difference of two indices, each added by the workgroup that holds that end.
 * nvf_vox_dequantize: xyz float64 [n, 3] = o + q * s for q int32 [n, 3], any integers. */
#define NVF_VOX_MAX_GROUPS 1024
#define NVF_VOX_STATUS_WORDS (8 + NVF_VOX_MAX_GROUPS)
#define NVF_VOX_BOUNDS_WORDS 8
#define NVF_VOX_BOUNDS_WORK_WORDS (NVF_VOX_BOUNDS_WORDS * NVF_VOX_MAX_GROUPS)
int nvf_vox_bounds(const double* xyz, int n, int64_t* bounds, int64_t* work, void* stream);
int nvf_vox_quantize(const double* xyz, int n, int bits, double ox, double oy, double oz, double s, double inv, int32_t* q,
                     int64_t* keys, int64_t* status, void* stream);
int nvf_vox_unique(const int64_t* sorted_keys, int n, int bits, int32_t* pts, int32_t* counts, int64_t* status,
                   int32_t* work, void* stream);
int nvf_vox_dequantize(const int32_t* q, int n, double ox, double oy, double oz, double s, double* xyz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NVF_HIP_H */
