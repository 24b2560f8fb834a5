// blake2s.hpp — BLAKE2s-256 (RFC 7693, unkeyed, 32-byte output) Merkle commitment kernels: the D = Blake2s256 counterpart of the SHA-256 family of merkle.hpp
// (MS_FLAG_DIGEST_BLAKE2S).  Same trees, same leaf messages, same node layout; only the compression differs.
//
//   * An inner node of the binary tree (64 bytes) is ONE compression with the final flag - SHA-256 needs the message block and a padding block.
//   * BLAKE2s has no padding block, but it must know that a block is the LAST one when it compresses it: a full block of the leaf stream is held back until a
//     65th byte arrives or the message ends ("compress once a 17th word is pending"), so a message of exactly 64 or 128 bytes ends in a full final block and the
//     empty message (a leaf group of zeros printed as "") is one all-zero block with t = 0.  No block without message bytes exists, so the leaf launch has no
//     deferred-block lists and no follow-up kernel.
//   * Message words are little-endian.  The leaf packer (merkle.hpp: put_dec, Affix, PackStream) produces big-endian ASCII words and is reused as it is: the 16
//     words of a block are byte-swapped at the compression site (16 v_perm_b32 against ~1000 instructions of the compression).  Packing little-endian instead
//     would save those 16 but needs a second copy of the whole assembler (funnel shifts the other way round, mirrored BCD packing and affix literals).  Digest
//     words are little-endian too, so inner nodes load their children and store their state without any byte swap.
//   * Instructions by the measured issue rates (profiles/r04_valu_issue_rate.txt): a + b + m is one v_add3_u32, every rotate one v_alignbit_b32 (a v_perm_b32
//     for 16 and 8 issues no faster), the closing h ^= v[i] ^ v[i + 8] one v_bitop3_b32.
//   * One node per lane on every level: the pair-of-lanes node of the SHA-256 subtree kernel (Sha256Pair) has no counterpart here (open latency item).
//     The inner kernels are therefore the shared pair of merkle.hpp, LaneInnerHashKernelT<IC, ND> and LaneSubtreeKernel<ND>, with ND = Blake2sNode below: this file
//     holds the compression, the stream, the node policy and the family.
#pragma once
#include "merkle.hpp"

namespace msmerkle {

constexpr u32 B2S_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr unsigned char B2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

struct Blake2s {
  u32 st[8];
  // parameter block of the unkeyed 32-byte digest: digest_length 32, key_length 0, fanout 1, depth 1
  MS_HD void init() {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = B2S_IV[i];
    st[0] ^= 0x01010020u;
  }
  static MS_HD void G(u32& a, u32& b, u32& c, u32& d, u32 x, u32 y) {
    a = a + b + x; d = rotr32(d ^ a, 16);
    c = c + d;     b = rotr32(b ^ c, 12);
    a = a + b + y; d = rotr32(d ^ a, 8);
    c = c + d;     b = rotr32(b ^ c, 7);
  }
  // one compression of the 16 little-endian words m; t = message bytes up to and including this block (messages are far below 2^32 bytes), last: the final block
  MS_HD void compress(const u32 (&m)[16], u32 t, bool last) {
    u32 v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { v[i] = st[i]; v[i + 8] = B2S_IV[i]; }
    v[12] ^= t;
    v[14] = last ? ~B2S_IV[6] : B2S_IV[6];
#pragma unroll
    for (int r = 0; r < 10; r++) {
      G(v[0], v[4], v[8], v[12], m[B2S_SIGMA[r][0]], m[B2S_SIGMA[r][1]]);
      G(v[1], v[5], v[9], v[13], m[B2S_SIGMA[r][2]], m[B2S_SIGMA[r][3]]);
      G(v[2], v[6], v[10], v[14], m[B2S_SIGMA[r][4]], m[B2S_SIGMA[r][5]]);
      G(v[3], v[7], v[11], v[15], m[B2S_SIGMA[r][6]], m[B2S_SIGMA[r][7]]);
      G(v[0], v[5], v[10], v[15], m[B2S_SIGMA[r][8]], m[B2S_SIGMA[r][9]]);
      G(v[1], v[6], v[11], v[12], m[B2S_SIGMA[r][10]], m[B2S_SIGMA[r][11]]);
      G(v[2], v[7], v[8], v[13], m[B2S_SIGMA[r][12]], m[B2S_SIGMA[r][13]]);
      G(v[3], v[4], v[9], v[14], m[B2S_SIGMA[r][14]], m[B2S_SIGMA[r][15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = xor3(st[i], v[i], v[i + 8]);
  }
  // the digest is the state as little-endian words: memory order on this machine
  MS_HD void store(u32* dst) const {
    uint4_t* out = reinterpret_cast<uint4_t*>(dst);
    uint4_t o0, o1;
    o0.x = st[0]; o0.y = st[1]; o0.z = st[2]; o0.w = st[3]; o1.x = st[4]; o1.y = st[5]; o1.z = st[6]; o1.w = st[7];
    out[0] = o0; out[1] = o1;
  }
};

// byte stream -> BLAKE2s-256 over the buffer of PackStream.  `drain` holds the ONE compression site of the kernel, for inner and final blocks alike (t and the final
// flag are run-time values).  Before the final drain a block is compressed once MORE than 64 bytes are pending (LAZY: and some lane of the wave is out of room), so
// at most 64 bytes are pending behind a non-LAZY drain - which is why the buffer is one word longer than ShaStream's (EXTRA_WORDS): an append may start at word 16.
// Final drain: called until it stops returning MORE; the words past the message's end read as zero.  DEFER is never returned.
template <int NWORDS, int NT, int MAXW, bool LAZY> struct B2Stream : PackStream<NWORDS, NT> {
  static_assert(NWORDS >= 16 + MAXW + 2 && NWORDS <= 49, "buffer = one or two blocks + room for one element behind a full block");
  static_assert(MAXW <= 16, "an iteration appends less than a block");
  typedef PackStream<NWORDS, NT> Base;
  using Base::buf; using Base::total; using Base::done; using Base::fbase;
  Blake2s h;
  MS_HD void init(u32* lds_words, int tid_) { h.init(); Base::init_buf(lds_words, tid_); }
  MS_HD u32 end_message() { Base::begin_final(); return total; }
  MS_HD void store_digest(u32* dst) const { h.store(dst); }
  enum { DONE = 0, MORE = 1, DEFER = 2 };
  MS_HD int drain(bool final, u32 msg_bytes) {
    bool go, last = false;
    if (!final) {
      const u32 pending = (total >> 2) - done;
      const bool room = LAZY ? msrt::wave_any(pending + (u32)MAXW + 1u > (u32)NWORDS) : true;
      go = room && total > 4u * done + 64u;
    } else {
      go = true;
      last = 4u * (done + 16u) >= msg_bytes;
    }
    if (!go) return DONE;
    const u32 valid_end = final ? (msg_bytes + 3) >> 2 : ~0u;
    const u32* blk = buf + (final ? done - fbase : 0u) * NT;
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = (done + i < valid_end) ? bswap32(blk[i * NT]) : 0u;
    h.compress(w, last ? msg_bytes : 4u * (done + 16u), last);
    done += 16;
    if (final) return last ? DONE : MORE;
    u32 t[NWORDS - 16];
#pragma unroll
    for (int k = 0; k < NWORDS - 16; k++) t[k] = buf[(k + 16) * NT];
#pragma unroll
    for (int k = 0; k < NWORDS - 16; k++) buf[k * NT] = t[k];
    return DONE;
  }
};

// The node policy of the shared one-node-per-lane kernels (merkle.hpp: LaneInnerHashKernelT, LaneSubtreeKernel): ic * 32 bytes = ic / 2 blocks, the last one final.
struct Blake2sNode {
  typedef Blake2s State;
  static MS_HD Blake2s node(const u32 (&w)[16]) { Blake2s h; h.init(); h.compress(w, 64u, true); return h; }
  template <int IC> static MS_HD u32 nblocks(u32 ic) { return ic / 2; }
  template <int IC> static MS_HD void block(Blake2s& st, const u32* ch, u32 b, u32 ic) {
    Blake2s h = st;   // (a local copy: compressing through the reference swaps the operands of some of G's xors)
    u32 w[16];
    load_node64(ch + b * 16, w);
    h.compress(w, 64u * (b + 1), b + 1 == ic / 2);
    st = h;
  }
};

// The BLAKE2s-256 kernel family (DG of LeafHashKernel and msfri::FriTailKernel).
struct Blake2sKernels {
  template <int NWORDS, int NT, int MAXW, bool LAZY> using Stream = B2Stream<NWORDS, NT, MAXW, LAZY>;
  static constexpr int BLOCK_WORDS = 16, LAZY_BLOCKS = 2;
  static constexpr int EXTRA_WORDS = 1;
  static constexpr bool DEFERS = false;
  typedef LaneInnerHashKernelT<0, Blake2sNode> Inner;
  typedef LaneInnerHashKernelT<2, Blake2sNode> Inner2;
  typedef LaneSubtreeKernel<Blake2sNode> Subtree;
};

}  // namespace msmerkle
