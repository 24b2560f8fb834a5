// blake3.hpp — BLAKE3 (unkeyed hash mode, 32-byte output) Merkle commitment kernels: the D = blake3::Hasher counterpart of the SHA-256 family of merkle.hpp and the
// BLAKE2s-256 family of blake2s.hpp (MS_FLAG_DIGEST_BLAKE3).  Same trees, same leaf messages, same node layout; only the hash differs.
//
//   * The compression is BLAKE2s's G on the same 4 x 4 state (rotations 16 / 12 / 8 / 7, 32-bit words), 7 rounds instead of 10.  The message schedule is ONE fixed
//     permutation applied between rounds: with the rounds unrolled every m[...] index is a compile-time constant (B3_SCHED), so the permutation is register
//     renaming and costs no instruction and no table in memory.  a + b + m is one v_add3_u32, every rotate one v_alignbit_b32 (blake2s.hpp).
//   * A message of up to 1024 bytes is ONE chunk: a chain of compressions whose first block carries CHUNK_START and whose last block carries CHUNK_END | ROOT, the
//     block length in bytes (64 but for the last block) and the chunk counter 0.  An inner node of the binary tree (64 bytes) is one compression with flags
//     START | END | ROOT = 11.  Every leaf message of the prover's default shapes and of the fused FRI round is a single chunk.
//   * Like BLAKE2s, BLAKE3 must know that a block is the chunk's LAST one when it compresses it, and there is no padding block: B3Stream uses B2Stream's hold-back
//     rule ("compress once more than 64 bytes are pending"), one compression site, one launch, no deferred blocks.  The packer's big-endian words are byte-swapped at
//     the compression site, as for BLAKE2s; digest words are little-endian = memory order.
//   * Messages of more than 1024 bytes (leaf groups such as the wide AIR's lpn = 128; inner nodes with 64 or more children) need BLAKE3's chunk tree: chunk c is
//     hashed with counter c, the chaining values of finished chunks wait on a stack and are merged by PARENT compressions (left subtree = the largest power of two
//     of chunks that leaves the right one non-empty), ROOT goes on the top parent.  These are SEPARATE instantiations (B3Stream<..., MULTI = true>,
//     B3InnerHashMultiKernel), picked by the host from an upper bound of the message length, so that the single-chunk kernels pay nothing and carry no stack.
//     LIMIT: B3_MAX_BYTES = 16 KiB per message = 16 chunks = a stack of B3_STACK = 4 chaining values, which lives in LDS (word-interleaved like the message
//     buffer), never in scratch.  Above the limit the host returns MS_ERR_ARG (merkle_tree.cpp); no kernel is launched.
//   * One node per lane on every level: no pair-of-lanes variant, as for BLAKE2s.  The single-chunk inner kernels are the shared pair of merkle.hpp,
//     LaneInnerHashKernelT<IC, ND> and LaneSubtreeKernel<ND>, with ND = Blake3Node below; B3InnerHashMultiKernel (LDS for its stack) is a kernel of its own.  The
//     family Blake3Kernels names the bounds and the multi-chunk instances the host chooses by.
#pragma once
#include "merkle.hpp"

namespace msmerkle {

constexpr u32 B3_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr u32 B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8;
constexpr u32 B3_CHUNK_BYTES = 1024;
constexpr int B3_STACK = 4;                                     // chaining values that can wait: popcount(chunks - 1) <= 4 for up to 16 chunks
constexpr u32 B3_MAX_BYTES = B3_CHUNK_BYTES << B3_STACK;        // 16 KiB: the longest message the multi-chunk kernels hash
constexpr unsigned char B3_PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
// B3_SCHED.s[r][i]: the index into the ORIGINAL message words of the i-th word round r takes (round 0: identity; m'[i] = m[PERM[i]] between rounds)
struct B3Sched { unsigned char s[7][16]; };
constexpr B3Sched make_b3_sched() {
  B3Sched t{};
  for (int i = 0; i < 16; i++) t.s[0][i] = (unsigned char)i;
  for (int r = 1; r < 7; r++)
    for (int i = 0; i < 16; i++) t.s[r][i] = t.s[r - 1][B3_PERM[i]];
  return t;
}
constexpr B3Sched B3_SCHED = make_b3_sched();

struct Blake3 {
  u32 st[8];   // the chaining value
  MS_HD void init() {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = B3_IV[i];
  }
  static MS_HD void G(u32& a, u32& b, u32& c, u32& d, u32 x, u32 y) {
    a = a + b + x; d = rotr32(d ^ a, 16);
    c = c + d;     b = rotr32(b ^ c, 12);
    a = a + b + y; d = rotr32(d ^ a, 8);
    c = c + d;     b = rotr32(b ^ c, 7);
  }
  // one compression of the 16 little-endian words m: st = the first 8 words of the output.  counter: the chunk index (0 for parents; messages are far below
  // 2^32 chunks: the high word is the constant 0), len: message bytes in the block, flags: B3_*
  MS_HD void compress(const u32 (&m)[16], u32 counter, u32 len, u32 flags) {
    u32 v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = st[i];
    v[8] = B3_IV[0]; v[9] = B3_IV[1]; v[10] = B3_IV[2]; v[11] = B3_IV[3];
    v[12] = counter; v[13] = 0u; v[14] = len; v[15] = flags;
#pragma unroll
    for (int r = 0; r < 7; r++) {
      G(v[0], v[4], v[8], v[12], m[B3_SCHED.s[r][0]], m[B3_SCHED.s[r][1]]);
      G(v[1], v[5], v[9], v[13], m[B3_SCHED.s[r][2]], m[B3_SCHED.s[r][3]]);
      G(v[2], v[6], v[10], v[14], m[B3_SCHED.s[r][4]], m[B3_SCHED.s[r][5]]);
      G(v[3], v[7], v[11], v[15], m[B3_SCHED.s[r][6]], m[B3_SCHED.s[r][7]]);
      G(v[0], v[5], v[10], v[15], m[B3_SCHED.s[r][8]], m[B3_SCHED.s[r][9]]);
      G(v[1], v[6], v[11], v[12], m[B3_SCHED.s[r][10]], m[B3_SCHED.s[r][11]]);
      G(v[2], v[7], v[8], v[13], m[B3_SCHED.s[r][12]], m[B3_SCHED.s[r][13]]);
      G(v[3], v[4], v[9], v[14], m[B3_SCHED.s[r][14]], m[B3_SCHED.s[r][15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = v[i] ^ v[i + 8];
  }
  // the digest is the chaining value of the ROOT compression as little-endian words: memory order on this machine
  MS_HD void store(u32* dst) const {
    uint4_t* out = reinterpret_cast<uint4_t*>(dst);
    uint4_t o0, o1;
    o0.x = st[0]; o0.y = st[1]; o0.z = st[2]; o0.w = st[3]; o1.x = st[4]; o1.y = st[5]; o1.z = st[6]; o1.w = st[7];
    out[0] = o0; out[1] = o1;
  }
};

// The chaining values of the finished chunks of ONE message that wait for their right siblings: B3_STACK entries of 8 words in LDS, word-interleaved over the NT
// threads of the workgroup (word i of entry s at base[(8 * s + i) * NT]: conflict free, and no dynamically indexed registers).  `merge` holds the one PARENT
// compression site.
template <int NT> struct B3CvStack {
  static constexpr int WORDS = 8 * B3_STACK;   // LDS words per thread
  u32* base;   // this thread's word 0
  u32 sp;      // entries waiting
  MS_HD void init(u32* lds_words_of_thread) { base = lds_words_of_thread; sp = 0; }
  // h.st = the chaining value of a right subtree: `n` times, h.st = PARENT(pop(), h.st); the last one carries ROOT if `root`
  MS_HD void merge(Blake3& h, u32 n, bool root) {
    for (u32 k = 0; k < n; k++) {
      sp--;
      const u32* e = base + (size_t)(8u * (sp & (u32)(B3_STACK - 1))) * NT;
      u32 w[16];
#pragma unroll
      for (int i = 0; i < 8; i++) { w[i] = e[i * NT]; w[i + 8] = h.st[i]; }
      h.init();
      h.compress(w, 0u, 64u, B3_PARENT | ((root && k + 1 == n) ? B3_ROOT : 0u));
    }
  }
  // chunk number `total_chunks` - 1 has just ended with chaining value h.st and more input follows: its completed subtrees are merged (one per trailing zero bit of
  // total_chunks), the result waits, h starts the next chunk
  MS_HD void push_chunk(Blake3& h, u32 total_chunks) {
    u32 nz = 0;
    while (((total_chunks >> nz) & 1u) == 0u) nz++;
    merge(h, nz, false);
    u32* e = base + (size_t)(8u * (sp & (u32)(B3_STACK - 1))) * NT;
#pragma unroll
    for (int i = 0; i < 8; i++) e[i * NT] = h.st[i];
    sp++;
    h.init();
  }
  // the message's last chunk has ended (without ROOT) with chaining value h.st: everything that waits is merged, right to left; h.st = the digest
  MS_HD void finish(Blake3& h) { merge(h, sp, true); }
};

// byte stream -> BLAKE3 over the buffer of PackStream.  `drain` holds the ONE block compression site of the kernel, for inner and final blocks alike (length and flags
// are run-time values).  Before the final drain a block is compressed once MORE than 64 bytes are pending (LAZY: and some lane of the wave is out of room), so at
// most 64 bytes are pending behind a non-LAZY drain and the buffer is one word longer than ShaStream's (EXTRA_WORDS), as B2Stream's.
// Final drain: called until it stops returning MORE; the words past the message's end read as zero.  DEFER is never returned.
// MULTI = false: the message is at most one chunk (1024 bytes; the host guarantees it).  MULTI = true: up to B3_MAX_BYTES; the last 8 * B3_STACK of the NWORDS
// LDS words of a thread are its chaining-value stack.
template <int NWORDS, int NT, int MAXW, bool LAZY, bool MULTI> struct B3StreamT : PackStream<NWORDS, NT> {
  static constexpr int BW = NWORDS - (MULTI ? B3CvStack<NT>::WORDS : 0);   // words of the message buffer
  static_assert(BW >= 16 + MAXW + 2 && BW <= 49, "buffer = one or two blocks + room for one element behind a full block");
  static_assert(MAXW <= 16, "an iteration appends less than a block");
  typedef PackStream<NWORDS, NT> Base;
  using Base::buf; using Base::total; using Base::done; using Base::fbase;
  Blake3 h;
  B3CvStack<NT> stack;   // (MULTI only)
  MS_HD void init(u32* lds_words, int tid_) { h.init(); Base::init_buf(lds_words, tid_); if constexpr (MULTI) stack.init(buf + (size_t)BW * NT); }
  MS_HD u32 end_message() { Base::begin_final(); return total; }
  MS_HD void store_digest(u32* dst) const { h.store(dst); }
  enum { DONE = 0, MORE = 1, DEFER = 2 };
  MS_HD int drain(bool final, u32 msg_bytes) {
    bool go, last = false;
    if (!final) {
      const u32 pending = (total >> 2) - done;
      const bool room = LAZY ? msrt::wave_any(pending + (u32)MAXW + 1u > (u32)BW) : true;
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
    const u32 len = last ? msg_bytes - 4u * done : 64u;
    if constexpr (!MULTI) {
      h.compress(w, 0u, len, (done == 0u ? B3_CHUNK_START : 0u) | (last ? (B3_CHUNK_END | B3_ROOT) : 0u));
      done += 16;
    } else {
      const u32 bic = (done >> 4) & 15u, chunk = done >> 8;   // block in its chunk, chunk in the message
      const bool chunk_end = last || bic == 15u;
      h.compress(w, chunk, len, (bic == 0u ? B3_CHUNK_START : 0u) | (chunk_end ? B3_CHUNK_END : 0u) | ((last && chunk == 0u) ? B3_ROOT : 0u));
      done += 16;
      if (chunk_end) {
        if (!last) stack.push_chunk(h, chunk + 1u);   // (a chunk's 16th block is compressed before the message's end only when more bytes are pending)
        else if (chunk) stack.finish(h);
      }
    }
    if (final) return last ? DONE : MORE;
    u32 t[BW - 16];
#pragma unroll
    for (int k = 0; k < BW - 16; k++) t[k] = buf[(k + 16) * NT];
#pragma unroll
    for (int k = 0; k < BW - 16; k++) buf[k * NT] = t[k];
    return DONE;
  }
};

// The node policy of the shared one-node-per-lane kernels (merkle.hpp: LaneInnerHashKernelT, LaneSubtreeKernel): ic * 32 bytes = ic / 2 blocks of ONE chunk
// (ic <= MAX_IC = 32; more children: B3InnerHashMultiKernel).  A node of the binary tree is one compression with flags START | END | ROOT = 11.
struct Blake3Node {
  typedef Blake3 State;
  static constexpr u32 MAX_IC = B3_CHUNK_BYTES / 32;
  static MS_HD Blake3 node(const u32 (&w)[16]) { Blake3 h; h.init(); h.compress(w, 0u, 64u, B3_CHUNK_START | B3_CHUNK_END | B3_ROOT); return h; }
  template <int IC> static MS_HD u32 nblocks(u32 ic) { static_assert(IC <= (int)MAX_IC, "one chunk"); return ic / 2; }
  template <int IC> static MS_HD void block(Blake3& st, const u32* ch, u32 b, u32 ic) {
    Blake3 h = st;   // (a local copy, as Blake2sNode's)
    u32 w[16];
    load_node64(ch + b * 16, w);
    h.compress(w, 0u, 64u, (b == 0 ? B3_CHUNK_START : 0u) | (b + 1 == ic / 2 ? (B3_CHUNK_END | B3_ROOT) : 0u));
    st = h;
  }
};

// Inner levels whose nodes have more than 32 children (ic * 32 bytes > one chunk), up to B3_MAX_BYTES / 32 = 512: ic / 32 whole chunks (ic is a power of two) and
// the parents above them, the waiting chaining values in LDS.  Launched with lds_bytes() of dynamic LDS.  (The stack needs the workgroup's LDS and the thread's
// index, which a node policy does not see: a kernel of its own, on the shared loader and root forwarder.)
struct B3InnerHashMultiKernel {
  static constexpr int THREADS = msmerkle::THREADS;
  static constexpr u32 MAX_IC = B3_MAX_BYTES / 32;
  typedef InnerHashParams Params;
  static MS_HD int nphases(const Params& p) { return (int)p.nlevels; }
  static MS_HD size_t lds_bytes() { return (size_t)B3CvStack<THREADS>::WORDS * THREADS * sizeof(u32); }
  static MS_DEV void phase(int ph, const Params& p, int bx, int, int tid, int nthreads, unsigned char* lds) {
    const u32 ic = p.ic;
    size_t child_off = p.child_off, nchildren = p.nchildren;
    for (int l = 0; l < ph; l++) { child_off += nchildren; nchildren /= ic; }
    const size_t nparents = nchildren / ic;
    const size_t stride = (p.nlevels > 1) ? (size_t)nthreads : 0;
    const u32 nblocks = ic / 2, nchunks = (nblocks + 15u) / 16u;
    for (size_t g = (size_t)bx * nthreads + tid; g < nparents; g += stride) {
      const u32* ch = p.nodes + (child_off + g * ic) * 8;
      Blake3 h; h.init();
      B3CvStack<THREADS> stack; stack.init(reinterpret_cast<u32*>(lds) + tid);
      for (u32 b = 0; b < nblocks; b++) {
        u32 w[16];
        load_node64(ch + b * 16, w);
        const u32 bic = b & 15u, chunk = b >> 4;
        const bool last = b + 1 == nblocks, chunk_end = last || bic == 15u;
        h.compress(w, chunk, 64u, (bic == 0 ? B3_CHUNK_START : 0u) | (chunk_end ? B3_CHUNK_END : 0u) | ((last && nchunks == 1) ? B3_ROOT : 0u));
        if (chunk_end) {
          if (!last) stack.push_chunk(h, chunk + 1u);
          else if (chunk) stack.finish(h);
        }
      }
      h.store(p.nodes + (child_off + nchildren + g) * 8);
      if (p.host_root && nparents == 1) forward_root(p, h);
      if (stride == 0) break;
    }
  }
};

// The BLAKE3 kernel families (DG of LeafHashKernel and msfri::FriTailKernel): messages of at most one chunk, and (leaf hashing only) of up to B3_MAX_BYTES.
struct Blake3MultiKernels {
  template <int NWORDS, int NT, int MAXW, bool LAZY> using Stream = B3StreamT<NWORDS, NT, MAXW, LAZY, true>;
  static constexpr int BLOCK_WORDS = 16, LAZY_BLOCKS = 2;
  static constexpr int EXTRA_WORDS = 1 + B3CvStack<THREADS>::WORDS;
  static constexpr bool DEFERS = false;
  typedef LaneInnerHashKernelT<0, Blake3Node> Inner;
  typedef LaneInnerHashKernelT<2, Blake3Node> Inner2;
  typedef LaneSubtreeKernel<Blake3Node> Subtree;
};
struct Blake3Kernels {
  template <int NWORDS, int NT, int MAXW, bool LAZY> using Stream = B3StreamT<NWORDS, NT, MAXW, LAZY, false>;
  static constexpr int BLOCK_WORDS = 16, LAZY_BLOCKS = 2;
  static constexpr int EXTRA_WORDS = 1;
  static constexpr bool DEFERS = false;
  typedef LaneInnerHashKernelT<0, Blake3Node> Inner;
  typedef LaneInnerHashKernelT<2, Blake3Node> Inner2;
  typedef LaneSubtreeKernel<Blake3Node> Subtree;
  // what the host picks an instance by: a message (a leaf group's upper bound, an inner node's ic * 32 bytes) of up to CHUNK_BYTES takes the kernels above,
  // up to MAX_BYTES the multi-chunk ones, a longer one is refused
  static constexpr u32 CHUNK_BYTES = B3_CHUNK_BYTES, MAX_BYTES = B3_MAX_BYTES;
  typedef Blake3MultiKernels Multi;            // DG of the multi-chunk leaf kernels
  typedef B3InnerHashMultiKernel InnerMulti;   // launched with its lds_bytes()
};

}  // namespace msmerkle
