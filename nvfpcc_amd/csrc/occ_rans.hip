// Lossless geometry: the true occupancy of every leaf block, entropy-coded under the decoder's own field
// (nvfpcc_amd/lossless_pack.py).  The eval forward gives a probability p for every voxel on both sides of the pack; a
// voxel's CONTEXT is a function of the float32 bits of p alone (occ_ctx below), a calibration table sends the measured
// occupancy rate of each of the 256 contexts as a 16-bit frequency f1, and a binary rANS coder spends about
// -log2(f / 65536) bits per voxel.
//
//   nvf_occ_ctx_hist        per context the voxels and the occupied voxels, exact integers, accumulated over calls
//   nvf_occ_rans_encode     one 64-lane wave per GROUP of up to G consecutive blocks; symbol i = b_local * 32768 + raster
//                           voxel belongs to lane i % 64 at step i / 64, so a step reads 64 consecutive voxels.  64
//                           interleaved 64-bit states (start 2^31, 32-bit words, 16-bit frequencies).  The steps are
//                           walked BACKWARDS and the words of a step are written downwards from the end of the group's
//                           region, highest lane first: read forwards they come in the decoder's order.
//   nvf_occ_rans_decode     the same wave walks forwards; the lanes whose state fell below 2^31 take consecutive words in
//                           ascending lane order (a ballot and a prefix popcount).  The ballot of the decoded symbols of
//                           step t IS occupancy word t % 512 of block t / 512, the word format of nvf_head_occ_bits.
//                           Every word index is checked against the group's word count: a damaged stream sets the group's
//                           status and reads zeros, it cannot make the kernel read outside its words.
//
// Only the state recurrence is serial: contexts and frequencies depend on p alone, so each wave fetches OCC_AHEAD steps
// of p (and of the ground truth) at once and looks their frequencies up in LDS before it enters the chain.  The chain
// itself -- the step, the word window, the status -- is occ_coder.h's, shared with occ_hier.hip; no lane is ever idle here.
#include "occ_coder.h"

#define OCC_VOX 32768                                  // voxels of a 32^3 block
#define OCC_WPB 512                                    // occupancy words of a block
#define OCC_AHEAD 8                                    // steps fetched together; divides OCC_WPB
#define OCC_HIST_THREADS 1024
#define OCC_PEEL 4

namespace {

// same-address LDS adds serialise and trained decoders saturate, so a wave peels equal contexts before it adds, as
// occ_select.hip does for its bins
__global__ __launch_bounds__(OCC_HIST_THREADS) void occ_ctx_hist_kernel(const float* __restrict__ p,
                                                                        const float* __restrict__ gt, int voxels,
                                                                        unsigned long long* __restrict__ cnt,
                                                                        unsigned long long* __restrict__ occ,
                                                                        unsigned long long* __restrict__ bad) {
  __shared__ uint32_t h_cnt[OCC_CTX];
  __shared__ uint32_t h_occ[OCC_CTX];
  __shared__ uint32_t h_bad;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < OCC_CTX) { h_cnt[tid] = 0; h_occ[tid] = 0; }
  if (tid == 0) h_bad = 0;
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * voxels;
  uint32_t nbad = 0;
  // every lane of a wave runs the same number of rounds: the ballots below need the whole wave
  for (int base = 0; base < voxels; base += OCC_HIST_THREADS) {
    const int i = base + tid;
    bool live = i < voxels;
    const float v = live ? p[row + i] : 0.f;
    const bool hit = live && gt[row + i] != 0.f;
    if (live && occ_bad(v)) { ++nbad; live = false; }
    const int c = occ_ctx(v);
#pragma unroll 1
    for (int round = 0; round < OCC_PEEL; ++round) {
      const unsigned long long alive = __ballot(live);
      if (alive == 0ull) break;
      const int first = __ffsll((long long)alive) - 1;
      const int lead = __shfl(c, first, 64);
      const bool mine = live && c == lead;
      const int n = __popcll(__ballot(mine));
      if (n == 1) break;                               // nothing to aggregate: leave it to the plain adds
      const int nocc = __popcll(__ballot(mine && hit));
      if (lane == first) {
        atomicAdd(&h_cnt[lead], (uint32_t)n);
        if (nocc) atomicAdd(&h_occ[lead], (uint32_t)nocc);
      }
      if (mine) live = false;
    }
    if (live) {
      atomicAdd(&h_cnt[c], 1u);
      if (hit) atomicAdd(&h_occ[c], 1u);
    }
  }
  if (nbad) atomicAdd(&h_bad, nbad);
  __syncthreads();
  // integers: any order of these adds gives the same totals
  if (tid < OCC_CTX) {
    if (h_cnt[tid]) atomicAdd(cnt + tid, (unsigned long long)h_cnt[tid]);
    if (h_occ[tid]) atomicAdd(occ + tid, (unsigned long long)h_occ[tid]);
  }
  if (tid == 0 && h_bad) atomicAdd(bad, (unsigned long long)h_bad);
}

// one wave per group
__global__ __launch_bounds__(64) void occ_rans_encode_kernel(const float* __restrict__ p, const float* __restrict__ gt,
                                                             const int32_t* __restrict__ f1, int batch, int G,
                                                             unsigned long long* __restrict__ states,
                                                             uint32_t* __restrict__ words, uint32_t* __restrict__ nwords,
                                                             unsigned long long* __restrict__ gt_words) {
  __shared__ uint32_t tab[OCC_CTX];
  const int lane = threadIdx.x, g = blockIdx.x;
  occ_load_table<OCC_CTX>(f1, tab, lane);
  const int b0 = g * G, nb = min(G, batch - b0);
  const int steps = nb * OCC_WPB;
  const int region = nb * OCC_VOX;                     // a symbol emits one word at the most
  const float* pg = p + (size_t)b0 * OCC_VOX;
  const float* gg = gt + (size_t)b0 * OCC_VOX;
  uint32_t* wg = words + (size_t)g * G * OCC_VOX;
  unsigned long long x = OCC_RANS_L;
  int ptr = region;                                    // the words written so far are wg[ptr .. region)
  for (int t0 = steps - OCC_AHEAD; t0 >= 0; t0 -= OCC_AHEAD) {
    float pv[OCC_AHEAD], gv[OCC_AHEAD];
#pragma unroll
    for (int k = 0; k < OCC_AHEAD; ++k) {
      pv[k] = pg[(size_t)(t0 + k) * 64 + lane];
      gv[k] = gg[(size_t)(t0 + k) * 64 + lane];
    }
    uint32_t fr[OCC_AHEAD], st[OCC_AHEAD];
#pragma unroll
    for (int k = 0; k < OCC_AHEAD; ++k) {
      const uint32_t one = tab[occ_ctx(pv[k])];
      const bool s = gv[k] != 0.f;
      fr[k] = s ? one : 65536u - one;
      st[k] = s ? 0u : one;
      const unsigned long long word = __ballot(s);
      if (gt_words && lane == 0) gt_words[(size_t)b0 * OCC_WPB + t0 + k] = word;
    }
#pragma unroll
    for (int k = OCC_AHEAD - 1; k >= 0; --k)
      occ_encode_step<false>(x, fr[k], st[k], ptr, wg, lane);
  }
  states[(size_t)g * 64 + lane] = x;
  if (lane == 0) nwords[g] = (uint32_t)(region - ptr);
}

__global__ __launch_bounds__(64) void occ_rans_decode_kernel(const float* __restrict__ p, const int32_t* __restrict__ f1,
                                                             const unsigned long long* __restrict__ states,
                                                             const uint32_t* __restrict__ words,
                                                             const long long* __restrict__ word_off,
                                                             const uint32_t* __restrict__ nwords, long long total_words,
                                                             int batch, int G, unsigned long long* __restrict__ occ_words,
                                                             int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ uint32_t tab[OCC_CTX];
  const int lane = threadIdx.x, g = blockIdx.x;
  occ_load_table<OCC_CTX>(f1, tab, lane);
  const int b0 = g * G, nb = min(G, batch - b0);
  const float* pg = p + (size_t)b0 * OCC_VOX;
  OccWindow w = occ_window_open(words, word_off[g], (long long)nwords[g], total_words, true);
  unsigned long long x = states[(size_t)g * 64 + lane];
  for (int bl = 0; bl < nb; ++bl) {
    int cnt = 0;
    for (int t0 = 0; t0 < OCC_WPB; t0 += OCC_AHEAD) {
      uint32_t one[OCC_AHEAD];
#pragma unroll
      for (int k = 0; k < OCC_AHEAD; ++k) one[k] = tab[occ_ctx(pg[((size_t)bl * OCC_WPB + t0 + k) * 64 + lane])];
#pragma unroll
      for (int k = 0; k < OCC_AHEAD; ++k) {
        const bool s = occ_decode_step<false>(x, one[k], true, w, lane);
        const unsigned long long word = __ballot(s);
        cnt += __popcll(word);
        if (lane == 0) occ_words[((size_t)b0 + bl) * OCC_WPB + t0 + k] = word;
      }
    }
    if (lane == 0) counts[b0 + bl] = cnt;
  }
  const int st = occ_window_status(w, x, (long long)nwords[g]);
  if (lane == 0) status[g] = st;
}

}  // namespace

extern "C" int nvf_occ_ctx_hist(const float* p, const float* gt, int batch, int voxels, uint64_t* cnt, uint64_t* occ,
                                uint64_t* bad, void* stream) {
  if (!p || !gt || !cnt || !occ || !bad || batch <= 0 || voxels <= 0 || voxels > (1 << 24)) return NVF_EINVAL;
  occ_ctx_hist_kernel<<<batch, OCC_HIST_THREADS, 0, nvf_stream(stream)>>>(
      p, gt, voxels, (unsigned long long*)cnt, (unsigned long long*)occ, (unsigned long long*)bad);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_rans_encode(const float* p, const float* gt, const int32_t* f1, int batch, int group,
                                   uint64_t* states, uint32_t* words, uint32_t* nwords, uint64_t* gt_words,
                                   void* stream) {
  if (!p || !gt || !f1 || !states || !words || !nwords || batch <= 0 || group < 1 || group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  occ_rans_encode_kernel<<<groups, 64, 0, nvf_stream(stream)>>>(p, gt, f1, batch, group, (unsigned long long*)states,
                                                                words, nwords, (unsigned long long*)gt_words);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}

extern "C" int nvf_occ_rans_decode(const float* p, const int32_t* f1, const uint64_t* states, const uint32_t* words,
                                   const int64_t* word_off, const uint32_t* nwords, int64_t total_words, int batch,
                                   int group, uint64_t* occ_words, int32_t* counts, int32_t* status, void* stream) {
  if (!p || !f1 || !states || !words || !word_off || !nwords || !occ_words || !counts || !status || total_words < 0 ||
      batch <= 0 || group < 1 || group > NVF_OCC_RANS_MAX_GROUP)
    return NVF_EINVAL;
  const int groups = (batch + group - 1) / group;
  occ_rans_decode_kernel<<<groups, 64, 0, nvf_stream(stream)>>>(
      p, f1, (const unsigned long long*)states, words, (const long long*)word_off, nwords, (long long)total_words, batch,
      group, (unsigned long long*)occ_words, counts, status);
  NVF_LAUNCH_CHECK();
  return NVF_OK;
}
