// keccak.hpp — Keccak-256 (the original Keccak padding, Ethereum's hash: `sha3::Keccak256`) and SHA3-256 (FIPS 202: `sha3::Sha3_256`) Merkle commitment kernels: the
// fourth and fifth value of `D` beside the SHA-256 family of merkle.hpp and the BLAKE families of blake2s.hpp / blake3.hpp (MS_FLAG_DIGEST_KECCAK256,
// MS_FLAG_DIGEST_SHA3_256).  Same trees, same leaf messages, same node layout; only the hash differs.  The two functions are ONE sponge - Keccak-f[1600], rate
// 136 bytes, capacity 512 bits, 32 bytes squeezed - and differ in the domain suffix byte of the padding alone (0x01 / 0x06): a compile-time parameter of
// everything below (SUFFIX), so that no kernel argument of the existing families moves.
//
//   * The state is 25 lanes of 64 bits on a 32-bit VALU: 50 registers, lane i = (lo[i], hi[i]).  A 64-bit rotate by a compile-time offset is two
//     v_alignbit_b32 over the two halves (offsets above 32 swap the halves first; no rho offset is 32, lane 0 is not rotated), the theta parities and the
//     theta application are 3-input xors and chi's a ^ (~b & c) is one bit function: all v_bitop3_b32.  pi is register renaming inside a round.
//   * The 24 rounds are a ROLLED loop: a round is the same instruction sequence but for the round constant (KECCAK_RC, read with the uniform round index), so
//     a permutation site is one round's code (about 200 instructions), not 24 (about 4300).  Nothing of the state is indexed at run time: no scratch.
//   * Lanes are little-endian.  The leaf packer (merkle.hpp) produces big-endian ASCII words and is reused as it is: the 34 words of a rate block are
//     byte-swapped at the absorb site, as B2Stream does for its 16.  The digest is the first four lanes stored as little-endian words = memory order, so
//     inner nodes load their children and store their digest without any byte swap, in global memory and in LDS.
//   * A sponge pads EVERY message (pad10*1: the suffix byte behind the message, 0x80 into the block's last byte; one byte 0x81 / 0x86 when both meet), so
//     there is no hold-back rule as for the BLAKE families: a block is absorbed whenever 136 bytes are pending, and the final drain absorbs what is left - 0
//     to 135 bytes - with the padding written by position.  A message whose length is a multiple of 136 (the empty message included) ends in a block of
//     padding only, absorbed right there: no deferred blocks, no lists, one launch per commitment.  No message-length limit.
//   * One node per lane on every level, as for the BLAKE families: the inner kernels are the shared pair of merkle.hpp, LaneInnerHashKernelT<IC, ND>
//     and LaneSubtreeKernel<ND>, with ND = KeccakNode<SUFFIX> below.
#pragma once
#include "merkle.hpp"

namespace msmerkle {

constexpr u32 KECCAK_RATE_WORDS = 34, KECCAK_RATE_BYTES = 136;
constexpr u32 KECCAK_SUFFIX_KECCAK256 = 0x01u, KECCAK_SUFFIX_SHA3_256 = 0x06u;
struct KeccakRC { u32 w[48]; };   // round constant of round r: low half w[2r], high half w[2r + 1]
constexpr KeccakRC KECCAK_RC = {{
    0x00000001u, 0x00000000u, 0x00008082u, 0x00000000u, 0x0000808Au, 0x80000000u, 0x80008000u, 0x80000000u, 0x0000808Bu, 0x00000000u, 0x80000001u, 0x00000000u,
    0x80008081u, 0x80000000u, 0x00008009u, 0x80000000u, 0x0000008Au, 0x00000000u, 0x00000088u, 0x00000000u, 0x80008009u, 0x00000000u, 0x8000000Au, 0x00000000u,
    0x8000808Bu, 0x00000000u, 0x0000008Bu, 0x80000000u, 0x00008089u, 0x80000000u, 0x00008003u, 0x80000000u, 0x00008002u, 0x80000000u, 0x00000080u, 0x80000000u,
    0x0000800Au, 0x00000000u, 0x8000000Au, 0x80000000u, 0x80008081u, 0x80000000u, 0x00008080u, 0x80000000u, 0x80000001u, 0x00000000u, 0x80008008u, 0x80000000u}};
// rho offsets, lane x + 5 y
constexpr unsigned char KECCAK_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// a ^ (~b & c) in one instruction on gfx950 (v_bitop3_b32, truth table 0xD2)
MS_HD u32 chi3(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xD2);
#else
  return a ^ (~b & c);
#endif
}
// the high word of ({a, b} << n), 0 < n < 32: one v_alignbit_b32
MS_HD u32 funnel_l(u32 a, u32 b, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(a, b, 32 - n);
#else
  return (a << n) | (b >> (32 - n));
#endif
}

struct Keccak1600 {
  u32 lo[25], hi[25];
  MS_HD void init() {
#pragma unroll
    for (int i = 0; i < 25; i++) { lo[i] = 0u; hi[i] = 0u; }
  }
  // (l, h) = rol64((l, h), N), N a compile-time constant once the round's loops are unrolled
  static MS_HD void rol(u32 l, u32 h, int n, u32& ol, u32& oh) {
    if (n == 0) { ol = l; oh = h; }
    else if (n < 32) { oh = funnel_l(h, l, n); ol = funnel_l(l, h, n); }
    else { oh = funnel_l(l, h, n - 32); ol = funnel_l(h, l, n - 32); }
  }
  MS_HD void permute() {
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
      // theta: column parities, D[x] = C[x - 1] ^ rol(C[x + 1], 1) applied as a ^ C[x - 1] ^ rol(C[x + 1], 1)
      u32 cl[5], chh[5], rl[5], rh[5];
#pragma unroll
      for (int x = 0; x < 5; x++) {
        cl[x] = xor3(xor3(lo[x], lo[x + 5], lo[x + 10]), lo[x + 15], lo[x + 20]);
        chh[x] = xor3(xor3(hi[x], hi[x + 5], hi[x + 10]), hi[x + 15], hi[x + 20]);
      }
#pragma unroll
      for (int x = 0; x < 5; x++) rol(cl[x], chh[x], 1, rl[x], rh[x]);
      // rho and pi: B[y, 2x + 3y] = rol(A[x, y], RHO[x, y])
      u32 bl[25], bh[25];
#pragma unroll
      for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) {
          const u32 tl = xor3(lo[x + 5 * y], cl[(x + 4) % 5], rl[(x + 1) % 5]);
          const u32 th = xor3(hi[x + 5 * y], chh[(x + 4) % 5], rh[(x + 1) % 5]);
          const int d = y + 5 * ((2 * x + 3 * y) % 5);
          rol(tl, th, KECCAK_RHO[x + 5 * y], bl[d], bh[d]);
        }
      // chi
#pragma unroll
      for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) {
          lo[x + 5 * y] = chi3(bl[x + 5 * y], bl[(x + 1) % 5 + 5 * y], bl[(x + 2) % 5 + 5 * y]);
          hi[x + 5 * y] = chi3(bh[x + 5 * y], bh[(x + 1) % 5 + 5 * y], bh[(x + 2) % 5 + 5 * y]);
        }
      // iota
      lo[0] ^= KECCAK_RC.w[2 * r]; hi[0] ^= KECCAK_RC.w[2 * r + 1];
    }
  }
  // one rate block of 34 little-endian words into the state, and the permutation
  MS_HD void absorb(const u32 (&w)[34]) {
#pragma unroll
    for (int i = 0; i < 17; i++) { lo[i] ^= w[2 * i]; hi[i] ^= w[2 * i + 1]; }
    permute();
  }
  // the digest of the 64-byte message w (two child digests): one block, the padding at fixed places (suffix at byte 64, 0x80 at byte 135)
  template <u32 SUFFIX> MS_HD void node64(const u32 (&w)[16]) {
#pragma unroll
    for (int i = 0; i < 8; i++) { lo[i] = w[2 * i]; hi[i] = w[2 * i + 1]; }
#pragma unroll
    for (int i = 8; i < 25; i++) { lo[i] = 0u; hi[i] = 0u; }
    lo[8] = SUFFIX; hi[16] = 0x80000000u;
    permute();
  }
  // the digest is the first four lanes as little-endian words: memory order on this machine
  MS_HD void store(u32* dst) const {
    uint4_t* out = reinterpret_cast<uint4_t*>(dst);
    uint4_t o0, o1;
    o0.x = lo[0]; o0.y = hi[0]; o0.z = lo[1]; o0.w = hi[1]; o1.x = lo[2]; o1.y = hi[2]; o1.z = lo[3]; o1.w = hi[3];
    out[0] = o0; out[1] = o1;
  }
};

// byte stream -> Keccak over the buffer of PackStream.  `drain` holds the ONE permutation site of the kernel.  Before the final drain a block is absorbed once 34
// full words are pending (LAZY: and some lane of the wave is out of room), so fewer than 136 bytes are pending behind a non-LAZY drain and its final drain is
// one block.  The buffer is one rate block + room for one element for both forms (LeafHashKernel::NWORDS with LAZY_BLOCKS = 1): two rate blocks per thread
// would not leave LDS for two workgroups per CU.
// Final drain: called until it stops returning MORE; the words past the message's end read as zero, the last block (0 .. 135 message bytes) takes the padding by
// position.  DEFER is never returned.
template <int NWORDS, int NT, int MAXW, bool LAZY, u32 SUFFIX> struct KeccakStream : PackStream<NWORDS, NT> {
  static constexpr int RW = (int)KECCAK_RATE_WORDS;
  static_assert(NWORDS >= RW + MAXW + 1 && NWORDS <= 60, "buffer = one rate block + room for one element behind it");
  static_assert(MAXW <= RW, "an iteration appends less than a block");
  typedef PackStream<NWORDS, NT> Base;
  using Base::buf; using Base::total; using Base::done; using Base::fbase;
  Keccak1600 h;
  MS_HD void init(u32* lds_words, int tid_) { h.init(); Base::init_buf(lds_words, tid_); }
  MS_HD u32 end_message() { Base::begin_final(); return total; }
  MS_HD void store_digest(u32* dst) const { h.store(dst); }
  enum { DONE = 0, MORE = 1, DEFER = 2 };
  MS_HD int drain(bool final, u32 msg_bytes) {
    bool go, last = false;
    u32 rem = 0;
    if (!final) {
      const u32 pending = (total >> 2) - done;
      const bool room = LAZY ? msrt::wave_any(pending + (u32)MAXW + 1u > (u32)NWORDS) : true;
      go = room && pending >= (u32)RW;
    } else {
      go = true;
      rem = msg_bytes - 4u * done;            // message bytes from this block on
      last = rem < KECCAK_RATE_BYTES;
    }
    if (!go) return DONE;
    const u32 valid_end = final ? (msg_bytes + 3) >> 2 : ~0u;
    const u32* blk = buf + (final ? done - fbase : 0u) * NT;
    u32 w[RW];
#pragma unroll
    for (int i = 0; i < RW; i++) w[i] = (done + i < valid_end) ? bswap32(blk[i * NT]) : 0u;
    // pad10*1 by position: the suffix byte at offset rem, 0x80 at offset 135 (the same byte when rem = 135)
    const u32 pos = last ? rem >> 2 : ~0u, sfx = SUFFIX << (8u * (rem & 3u));
#pragma unroll
    for (int i = 0; i < RW; i++) w[i] ^= ((u32)i == pos) ? sfx : 0u;
    w[RW - 1] ^= last ? 0x80000000u : 0u;
    h.absorb(w);
    done += RW;
    if (final) return last ? DONE : MORE;
    u32 t[NWORDS - RW];
#pragma unroll
    for (int k = 0; k < NWORDS - RW; k++) t[k] = buf[(k + RW) * NT];
#pragma unroll
    for (int k = 0; k < NWORDS - RW; k++) buf[k * NT] = t[k];
    return DONE;
  }
};

// The node policy of the shared one-node-per-lane kernels (merkle.hpp: LaneInnerHashKernelT, LaneSubtreeKernel).  IC = 2: one permutation over the 64 bytes, the
// padding constant.  IC = 0 (inner_children from Params): the ic * 32 bytes of the contiguous children absorbed 136 at a time, ic * 32 / 136 + 1 blocks - when 136
// divides the length the last one holds the padding only.
template <u32 SUFFIX> struct KeccakNode {
  typedef Keccak1600 State;
  static MS_HD Keccak1600 node(const u32 (&w)[16]) { Keccak1600 h; h.template node64<SUFFIX>(w); return h; }
  // message words ic * 8 (digests are whole words: the suffix byte starts a word)
  template <int IC> static MS_HD u32 nblocks(u32 ic) {
    static_assert(IC == 0 || IC == 2, "the binary tree's instance, or the general one");
    return IC == 2 ? 1u : ic * 8u / KECCAK_RATE_WORDS + 1u;
  }
  template <int IC> static MS_HD void block(Keccak1600& h, const u32* ch, u32 b, u32 ic) {
    if constexpr (IC == 2) {
      u32 w[16];
      load_node64(ch, w);
      h.template node64<SUFFIX>(w);
    } else {
      const u32 nw = ic * 8u, w0 = b * KECCAK_RATE_WORDS;
      u32 w[34];
#pragma unroll
      for (int i = 0; i < 34; i++) w[i] = (w0 + i < nw) ? ch[w0 + i] : ((w0 + i == nw) ? SUFFIX : 0u);
      if (b + 1 == nblocks<IC>(ic)) w[33] ^= 0x80000000u;
      h.absorb(w);
    }
  }
};

// The Keccak kernel family (DG of LeafHashKernel and msfri::FriTailKernel), by the padding's domain suffix.
template <u32 SUFFIX> struct KeccakKernels {
  template <int NWORDS, int NT, int MAXW, bool LAZY> using Stream = KeccakStream<NWORDS, NT, MAXW, LAZY, SUFFIX>;
  static constexpr int BLOCK_WORDS = (int)KECCAK_RATE_WORDS;
  static constexpr int LAZY_BLOCKS = 1;
  static constexpr int EXTRA_WORDS = 0;
  static constexpr bool DEFERS = false;
  typedef LaneInnerHashKernelT<0, KeccakNode<SUFFIX>> Inner;
  typedef LaneInnerHashKernelT<2, KeccakNode<SUFFIX>> Inner2;
  typedef LaneSubtreeKernel<KeccakNode<SUFFIX>> Subtree;
};
typedef KeccakKernels<KECCAK_SUFFIX_KECCAK256> Keccak256Kernels;
typedef KeccakKernels<KECCAK_SUFFIX_SHA3_256> Sha3_256Kernels;

}  // namespace msmerkle
