// The lossless occupancy coder, once: the context of a probability, the input error rule, the table in LDS, the
// interleaved rANS step of the encoder and of the decoder, a group's checked word window with its status bits, and the
// walk over the set bits of a block's occupancy words.  occ_rans.hip and occ_hier.hip own their symbol ORDER (which
// cell a lane codes at which step, and the look-ahead that fetches its frequency); everything that touches a state or
// a word is here.  include/nvf_hip.h, "lossless geometry", is the contract.
//
// The bit walk lives here too, not in a header of its own: lod_points.hip (points of a level) and occ_hier.hip (cell
// lists) are its two users, both walk the occupancy words this coder decodes, and a sibling header would hold one
// function.  lod_points.hip includes this file for it.
#pragma once
#include "nvf_common.h"

#define OCC_CTX 256
#define OCC_KEY_ONE 0x3F800000u
#define OCC_RANS_L (1ull << 31)

namespace {

// the context of a probability, from its bits alone: which side of 0.5, and the exponent + 2 mantissa bits of the
// distance to the nearer end.  Any bit pattern (NaN, negative, > 1) lands inside [0, 256).
__device__ __forceinline__ int occ_ctx(float p) {
  const int side = p > 0.5f ? 1 : 0;
  const float q = side ? 1.0f - p : p;
  const int key = (int)(__float_as_uint(q) >> 21);
  int idx = (int)(0x3F000000u >> 21) - key;
  idx = idx < 0 ? 0 : (idx > 127 ? 127 : idx);
  return 2 * idx + side;
}

__device__ __forceinline__ bool occ_bad(float p) {
  uint32_t key = __float_as_uint(p);
  if (key == 0x80000000u) key = 0u;
  return key > OCC_KEY_ONE;
}

// x / f and x % f for x < 2^63 and 1 <= f < 2^16, in three 32-bit divisions (long division in base 2^16 below the top)
__device__ __forceinline__ void occ_divmod(unsigned long long x, uint32_t f, unsigned long long& quot, uint32_t& rem) {
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  const uint32_t q1 = hi / f, r1 = hi - q1 * f;
  const uint32_t n2 = (r1 << 16) | (lo >> 16);         // r1 < f < 2^16
  const uint32_t q2 = n2 / f, r2 = n2 - q2 * f;        // q2 < 2^16
  const uint32_t n3 = (r2 << 16) | (lo & 0xFFFFu);
  const uint32_t q3 = n3 / f;
  rem = n3 - q3 * f;
  quot = ((unsigned long long)q1 << 32) | ((unsigned long long)q2 << 16) | q3;
}

// the table of N frequencies in LDS, an entry outside [1, 65535] pulled inside: no frequency is ever 0.  One wave.
template <int N>
__device__ __forceinline__ void occ_load_table(const int32_t* __restrict__ f1, uint32_t* tab, int lane) {
#pragma unroll 4
  for (int i = lane; i < N; i += 64) {
    const int v = f1[i];
    tab[i] = (uint32_t)(v < 1 ? 1 : (v > 65535 ? 65535 : v));
  }
  __syncthreads();
}

// One encoder step of the 64 interleaved states: a lane whose state would overflow under frequency fr first writes
// its low word, then x = (x / fr << 16) + x % fr + st.  The words of a step go downwards from wg[ptr), the highest
// lane first, so that read forwards they come in ascending lane order; the words written so far are wg[ptr .. end).
// With MAY_IDLE, fr == 0 is an idle lane: it neither writes nor changes its state.  The ballot needs the WHOLE wave:
// all 64 lanes call this unconditionally, every step, never under `if (live)`.
template <bool MAY_IDLE>
__device__ __forceinline__ void occ_encode_step(unsigned long long& x, uint32_t fr, uint32_t st, int& ptr,
                                                uint32_t* __restrict__ wg, int lane) {
  const bool live = !MAY_IDLE || fr != 0u;
  const bool emit = live && x >= ((unsigned long long)fr << 47);
  const unsigned long long m = __ballot(emit);
  if (emit) {
    const int at = ptr - 1 - __popcll((m >> lane) >> 1);   // the lanes above write first
    if (at >= 0) wg[at] = (uint32_t)x;
    x >>= 32;
  }
  ptr -= __popcll(m);
  unsigned long long quot;
  uint32_t rem;
  occ_divmod(x, live ? fr : 1u, quot, rem);
  if (live) x = (quot << 16) + rem + st;
}

// A group's words, words[off .. off + nw) cut to the buffer: nothing outside is ever read.  strict: the cut itself is
// damage (the whole stream is wanted); otherwise only a word wanted beyond the cut is (a prefix is enough).
struct OccWindow {
  const uint32_t* wg;
  long long nw, pos;
  bool damaged;
};

__device__ __forceinline__ OccWindow occ_window_open(const uint32_t* __restrict__ words, long long off, long long nw,
                                                     long long total_words, bool strict) {
  bool cut = false;
  if (off < 0 || off > total_words) { off = 0; nw = 0; cut = true; }
  if (nw > total_words - off) { nw = total_words - off; cut = true; }
  return OccWindow{words + off, nw, 0, cut && strict};
}

// One decoder step: the symbol under `one` (the frequency of a 1), the state update, and the lanes whose state fell
// below 2^31 take consecutive words in ascending lane order -- past the end: a zero, and the status says so.  With
// MAY_IDLE a lane that is not live decodes 0 and keeps its state.  Two ballots: called by all 64 lanes, as above.
template <bool MAY_IDLE>
__device__ __forceinline__ bool occ_decode_step(unsigned long long& x, uint32_t one, bool live, OccWindow& w, int lane) {
  if (!MAY_IDLE) live = true;
  const uint32_t slot = (uint32_t)x & 0xFFFFu;
  const bool s = live && slot < one;
  if (live) {
    const uint32_t f = s ? one : 65536u - one;
    const uint32_t start = s ? 0u : one;
    x = (unsigned long long)f * (x >> 16) + slot - start;
  }
  const bool need = live && x < OCC_RANS_L;
  const unsigned long long m = __ballot(need);
  if (need) {
    const long long at = w.pos + __popcll(m & ((1ull << lane) - 1ull));
    uint32_t v = 0u;
    if (at < w.nw) v = w.wg[at]; else w.damaged = true;
    x = (x << 32) | v;
  }
  w.pos += __popcll(m);
  return s;
}

// all three NVF_OCC_RANS_* bits of a group whose header claims `claimed` words; the caller masks the ones that apply
// (a decoder that stops early has neither its final states nor all its words behind it).  Whole wave.
__device__ __forceinline__ int occ_window_status(const OccWindow& w, unsigned long long x, long long claimed) {
  int st = 0;
  if (__ballot(w.damaged) != 0ull) st |= NVF_OCC_RANS_PAST_END;
  if (__ballot(x != OCC_RANS_L) != 0ull) st |= NVF_OCC_RANS_BAD_STATE;
  if (w.pos < claimed) st |= NVF_OCC_RANS_WORDS_LEFT;
  return st;
}

// For each set bit of block b's wpb occupancy words in raster order: sink(slot, cell), cell = 64 * word + bit and
// slot = run + the set bits before it.  One wave: a lane holds one word of a chunk of 64, lane k owns bit k of the word
// in turn.  Empty chunks and empty words are skipped, wave-uniformly.
template <class Sink>
__device__ __forceinline__ void occ_walk_bits(const unsigned long long* __restrict__ words, int b, int wpb, int run,
                                              int lane, Sink sink) {
  for (int w0 = 0; w0 < wpb; w0 += 64) {
    const unsigned long long mine = w0 + lane < wpb ? words[(size_t)b * wpb + w0 + lane] : 0ull;
    if (__ballot(mine != 0ull) == 0ull) continue;
    const int nw = min(64, wpb - w0);
    for (int wi = 0; wi < nw; ++wi) {
      const unsigned long long word = __shfl(mine, wi, 64);
      if (word == 0ull) continue;
      if ((word >> lane) & 1ull) sink(run + __popcll(word & ((1ull << lane) - 1ull)), 64 * (w0 + wi) + lane);
      run += __popcll(word);
    }
  }
}

}  // namespace
