// grind.hpp — proof-of-work grinding (ms_grind, include/ministark.h; build-defined, no reference counterpart): the smallest nonce of a range whose digest
// D(seed || nonce) starts with `bits` zero bits, for every digest of digest.hpp.  Pure hashing: no loads but the found word, no LDS, no scratch.
//
//   * GrindPolicy<DG>::head(seed words, nonce) is the first 8 digest bytes of the 40-byte message as a big-endian integer, on the compression / permutation the
//     family's tree kernels use: ONE SHA-256 block (0x80 behind byte 40, bit length 320), one final BLAKE2s block of 40 bytes, the BLAKE3 single-block chunk
//     (CHUNK_START | CHUNK_END | ROOT, length 40), one Keccak rate block (suffix at byte 40, 0x80 at byte 135).  The digest itself is never stored: everything
//     of the last rounds that feeds words 2 .. 7 only is dead code to the compiler.
//   * The seed is the same for every lane: it travels in the kernel arguments (uniform values), as the 8 words the bytes are when loaded little-endian.
//   * Thread t of a grid of T threads walks start + t + j T for ascending j, so a launch tests its nonces in near-ascending order.  On a hit it raises the found
//     word to ~nonce with an atomic maximum (the word rests at 0, like the other result words: the largest ~nonce is the smallest nonce); before each nonce it
//     reads the word and stops once it shows a hit below its next nonce.  A STALE read of the word is safe: every value the word has ever held is a real hit, so
//     an old value can only make a thread hash nonces it could have skipped, never skip one below the smallest hit - the thread that owns the smallest hit of
//     the range stops early only for a smaller one, which does not exist.  The result does not depend on grid, launch split or scheduling.
#pragma once
#include "digest.hpp"

namespace msmerkle {

struct GrindParams {
  u32 seed[8];                 // seed bytes 4 i .. 4 i + 3 as a little-endian word
  u64 start, n;                // the launch tests start .. start + n - 1 (start + n <= 2^64 - 1: ~nonce is never 0)
  u64 mask;                    // a hit: (head & mask) == 0; mask = the top `bits` bits
  unsigned long long* found;   // 0, or ~(the smallest hit so far)
};

template <class DG> struct GrindPolicy;
template <> struct GrindPolicy<Sha256Kernels> {
  static constexpr int WGS_PER_CU = 5;   // workgroups (= waves per SIMD) a CU holds at the listing's 95 VGPRs
  static MS_HD u64 head(const u32 (&s)[8], u64 nonce) {
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = bswap32(s[i]);
    w[8] = bswap32((u32)nonce); w[9] = bswap32((u32)(nonce >> 32));
    w[10] = 0x80000000u; w[11] = 0u; w[12] = 0u; w[13] = 0u; w[14] = 0u; w[15] = 320u;
    Sha256 h; h.init(); h.compress(w);
    return ((u64)h.st[0] << 32) | h.st[1];
  }
};
// the little-endian families: message words are the seed words as they are, the nonce's halves behind them; the head is digest words 0 and 1 byte-swapped
MS_HD void grind_block16(const u32 (&s)[8], u64 nonce, u32 (&m)[16]) {
#pragma unroll
  for (int i = 0; i < 8; i++) m[i] = s[i];
  m[8] = (u32)nonce; m[9] = (u32)(nonce >> 32);
#pragma unroll
  for (int i = 10; i < 16; i++) m[i] = 0u;
}
MS_HD u64 grind_head_le(u32 w0, u32 w1) { return ((u64)bswap32(w0) << 32) | bswap32(w1); }
template <> struct GrindPolicy<Blake2sKernels> {
  static constexpr int WGS_PER_CU = 5;   // (95 VGPRs)
  static MS_HD u64 head(const u32 (&s)[8], u64 nonce) {
    u32 m[16];
    grind_block16(s, nonce, m);
    Blake2s h; h.init(); h.compress(m, 40u, true);
    return grind_head_le(h.st[0], h.st[1]);
  }
};
template <> struct GrindPolicy<Blake3Kernels> {
  static constexpr int WGS_PER_CU = 7;   // (70 VGPRs)
  static MS_HD u64 head(const u32 (&s)[8], u64 nonce) {
    u32 m[16];
    grind_block16(s, nonce, m);
    Blake3 h; h.init(); h.compress(m, 0u, 40u, B3_CHUNK_START | B3_CHUNK_END | B3_ROOT);
    return grind_head_le(h.st[0], h.st[1]);
  }
};
template <u32 SUFFIX> struct GrindPolicy<KeccakKernels<SUFFIX>> {
  static constexpr int WGS_PER_CU = 5;   // (81 VGPRs)
  static MS_HD u64 head(const u32 (&s)[8], u64 nonce) {
    Keccak1600 h; h.init();
#pragma unroll
    for (int i = 0; i < 4; i++) { h.lo[i] = s[2 * i]; h.hi[i] = s[2 * i + 1]; }
    h.lo[4] = (u32)nonce; h.hi[4] = (u32)(nonce >> 32);
    h.lo[5] = SUFFIX; h.hi[16] = 0x80000000u;
    h.permute();
    return grind_head_le(h.lo[0], h.hi[0]);
  }
};

template <class DG> struct GrindKernel {
  static constexpr int THREADS = msmerkle::THREADS;
  typedef GrindParams Params;
  static MS_HD size_t lds_bytes() { return 0; }
  static MS_DEV void run(const Params& p, int bx, int, int nbx, int tid, unsigned char*) {
    const u64 T = (u64)nbx * THREADS;
    const volatile unsigned long long* seen = p.found;
    for (u64 i = (u64)bx * THREADS + tid; i < p.n; i += T) {
      const u64 nonce = p.start + i;
      if (~*seen < nonce) break;   // (0 reads as 2^64 - 1: no hit yet)
      if ((GrindPolicy<DG>::head(p.seed, nonce) & p.mask) == 0) {
        if (~*seen > nonce) msrt::atomic_max_u64(p.found, ~nonce);   // (only a hit that improves on what the word shows: where hits are dense, atomics on the one word would queue)
        break;
      }
    }
  }
};

}  // namespace msmerkle
