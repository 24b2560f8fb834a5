// stark_host.cpp — C++ host-side mirror of the reference's prover API for the accelerated path,
// above the C ABI of include/ministark.h (the reference is compiled Rust; no Rust toolchain exists in
// this image, so the host layer is C++ — INTEGRATION.md has the Rust binding of the same calls).
//
//   ministark::StarkConfig   <- StarkConfig::new             src/starks.rs:268-310 (+312-332)
//   ministark::Stark::prove  <- Stark::prove                 src/starks.rs:59-169
//                               Fri::commit_phase/query_phase src/fri.rs:64-189 (inlined: same call order)
//   ministark::Stark::verify <- Stark::verify / Fri::verify / MerkleRoot::check_proof   src/starks.rs:171-235, src/fri.rs:191-290,
//                               src/merkle.rs:312-338 — on the CPU, as in the reference
//   ministark::Transcript    <- nimue Merlin                  BUILD-DEFINED stand-in: a hash chain over the context's digest (SHA-256 / BLAKE2s-256 / BLAKE3 / Keccak-256 / SHA3-256) with the
//                                                             message ORDER of src/fiatshamir.rs:48-64,100-116;
//                                                             not nimue's bytes (its source is unavailable).
// Every field operation of the PROVER happens on the GPU inside libministark.so; prove() only moves challenges and
// commitments between the transcript and the stage functions and calls nothing but ms_* symbols, which are resolved at
// load time from the already-loaded libministark.so.  verify() is host arithmetic (csrc/field.hpp), like the reference's.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ministark.h"
#include "../../include/ministark_host.h"
#define MS_HOST_ONLY 1
#include "../csrc/field.hpp"  // Goldilocks / BabyBear arithmetic for the CPU verifier (typedefs u64, u32, u8)

// (weak: a libministark build from before the symbol existed - MS_LIB_PATH naming an older library in an A/B run - commits with SHA-256 only)
extern "C" int ms_digest(const ms_ctx* ctx) __attribute__((weak));
// (weak for the same reason: such a library has no grinding; msh_stark_set_grinding then refuses any bits but 0)
extern "C" int ms_grind(ms_ctx* ctx, const uint8_t seed[32], uint32_t bits, uint64_t start, uint64_t limit, uint64_t* nonce) __attribute__((weak));
extern "C" int ms_num_queries_grind(ms_field f, uint64_t security_bits, uint64_t grinding_bits, uint64_t blowup, uint64_t steps, uint64_t* constrain_queries,
                                    uint64_t* fri_queries) __attribute__((weak));

namespace ministark {

// ---- SHA-256 for the transcript and check_proof (host, a few hundred bytes per proof) ------------------------
struct Sha256 {
  u32 st[8]; u8 buf[64]; size_t nb = 0; u64 total = 0;
  Sha256() { static const u32 iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19}; memcpy(st, iv, 32); }
  static u32 rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const u8* p) {
    static const u32 K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe,
        0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7,
        0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,
        0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    u32 w[64];
    for (int i = 0; i < 16; i++) w[i] = ((u32)p[4 * i] << 24) | ((u32)p[4 * i + 1] << 16) | ((u32)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; i++) {
      u32 t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      u32 t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
  }
  void update(const void* data, size_t n) {
    const u8* p = (const u8*)data; total += n;
    while (n) { size_t k = 64 - nb < n ? 64 - nb : n; memcpy(buf + nb, p, k); nb += k; p += k; n -= k; if (nb == 64) { block(buf); nb = 0; } }
  }
  void finish(u8 out[32]) {
    u64 bits = total * 8; u8 pad = 0x80; update(&pad, 1); u8 z = 0;
    while (nb != 56) update(&z, 1);
    u8 len[8]; for (int k = 0; k < 8; k++) len[k] = (u8)(bits >> (8 * (7 - k)));
    update(len, 8);
    for (int k = 0; k < 8; k++) { out[4 * k] = st[k] >> 24; out[4 * k + 1] = st[k] >> 16; out[4 * k + 2] = st[k] >> 8; out[4 * k + 3] = st[k]; }
  }
};

// ---- BLAKE2s-256 (RFC 7693, unkeyed, 32-byte output) ------------------------------------------
struct Blake2s {
  u32 st[8]; u8 buf[64]; size_t nb = 0; u64 total = 0;
  static const u32* iv() { static const u32 v[8] = {0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19}; return v; }
  Blake2s() { memcpy(st, iv(), 32); st[0] ^= 0x01010020u; memset(buf, 0, 64); }
  static u32 rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const u8* p, u64 t, bool last) {
    static const u8 S[10][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
                                 {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
                                 {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
                                 {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
                                 {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    u32 m[16], v[16];
    for (int i = 0; i < 16; i++) m[i] = (u32)p[4 * i] | ((u32)p[4 * i + 1] << 8) | ((u32)p[4 * i + 2] << 16) | ((u32)p[4 * i + 3] << 24);
    for (int i = 0; i < 8; i++) { v[i] = st[i]; v[i + 8] = iv()[i]; }
    v[12] ^= (u32)t; v[13] ^= (u32)(t >> 32); if (last) v[14] = ~v[14];
    auto G = [&](int a, int b, int c, int d, u32 x, u32 y) {
      v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 12);
      v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 8); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 7);
    };
    for (int r = 0; r < 10; r++) {
      const u8* s = S[r];
      G(0, 4, 8, 12, m[s[0]], m[s[1]]); G(1, 5, 9, 13, m[s[2]], m[s[3]]); G(2, 6, 10, 14, m[s[4]], m[s[5]]); G(3, 7, 11, 15, m[s[6]], m[s[7]]);
      G(0, 5, 10, 15, m[s[8]], m[s[9]]); G(1, 6, 11, 12, m[s[10]], m[s[11]]); G(2, 7, 8, 13, m[s[12]], m[s[13]]); G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; i++) st[i] ^= v[i] ^ v[i + 8];
  }
  // a full buffer is compressed only once more bytes arrive: the last block carries the final flag
  void update(const void* data, size_t n) {
    const u8* p = (const u8*)data;
    while (n) {
      if (nb == 64) { total += 64; block(buf, total, false); nb = 0; }
      size_t k = 64 - nb < n ? 64 - nb : n; memcpy(buf + nb, p, k); nb += k; p += k; n -= k;
    }
  }
  void finish(u8 out[32]) {
    total += nb; memset(buf + nb, 0, 64 - nb); block(buf, total, true);
    for (int k = 0; k < 8; k++) { out[4 * k] = st[k]; out[4 * k + 1] = st[k] >> 8; out[4 * k + 2] = st[k] >> 16; out[4 * k + 3] = st[k] >> 24; }
  }
};

// ---- BLAKE3 (unkeyed hash mode, 32-byte output), the whole specification: chunks of 1024 bytes, the binary tree of chunk chaining values -----------
struct Blake3 {
  enum { CHUNK_START = 1, CHUNK_END = 2, PARENT = 4, ROOT = 8 };
  u32 cv[8]; u8 buf[64]; size_t nb = 0; u32 blocks = 0 /* compressed in the current chunk */; u64 chunk = 0; u32 stack[64][8]; int sp = 0;
  Blake3() { memcpy(cv, Blake2s::iv(), 32); memset(buf, 0, 64); }
  static u32 rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
  // cv = the first 8 words of the compression of the 64-byte block p (little-endian words) under chaining value `in`
  static void compress(const u32 in[8], const u8* p, u64 counter, u32 len, u32 flags, u32 out[8]) {
    static const u8 PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    u32 m[16], v[16];
    for (int i = 0; i < 16; i++) m[i] = (u32)p[4 * i] | ((u32)p[4 * i + 1] << 8) | ((u32)p[4 * i + 2] << 16) | ((u32)p[4 * i + 3] << 24);
    for (int i = 0; i < 8; i++) v[i] = in[i];
    for (int i = 0; i < 4; i++) v[8 + i] = Blake2s::iv()[i];
    v[12] = (u32)counter; v[13] = (u32)(counter >> 32); v[14] = len; v[15] = flags;
    auto G = [&](int a, int b, int c, int d, u32 x, u32 y) {
      v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 12);
      v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 8); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 7);
    };
    for (int r = 0; r < 7; r++) {
      G(0, 4, 8, 12, m[0], m[1]); G(1, 5, 9, 13, m[2], m[3]); G(2, 6, 10, 14, m[4], m[5]); G(3, 7, 11, 15, m[6], m[7]);
      G(0, 5, 10, 15, m[8], m[9]); G(1, 6, 11, 12, m[10], m[11]); G(2, 7, 8, 13, m[12], m[13]); G(3, 4, 9, 14, m[14], m[15]);
      u32 t[16]; for (int i = 0; i < 16; i++) t[i] = m[PERM[i]];
      memcpy(m, t, 64);
    }
    for (int i = 0; i < 8; i++) out[i] = v[i] ^ v[i + 8];
  }
  void parent(const u32 left[8], u32 flags) {   // cv = PARENT(left, cv)
    u8 blk[64]; memcpy(blk, left, 32); memcpy(blk + 32, cv, 32);   // (little-endian host, as everywhere in this file)
    compress(Blake2s::iv(), blk, 0, 64, PARENT | flags, cv);
  }
  // a full buffer is compressed only once more bytes arrive: a chunk's (and the message's) last block carries its flags
  void update(const void* data, size_t n) {
    const u8* p = (const u8*)data;
    while (n) {
      if (nb == 64) {
        compress(cv, buf, chunk, 64, (blocks == 0 ? CHUNK_START : 0) | (blocks == 15 ? CHUNK_END : 0), cv);
        if (blocks == 15) {   // the chunk is complete and more follows: merge the subtrees it completes (one per trailing zero bit of the chunk count), wait
          u64 tot = ++chunk;
          while ((tot & 1) == 0) { parent(stack[--sp], 0); tot >>= 1; }
          memcpy(stack[sp++], cv, 32); memcpy(cv, Blake2s::iv(), 32); blocks = 0;
        } else blocks++;
        nb = 0;
      }
      size_t k = 64 - nb < n ? 64 - nb : n; memcpy(buf + nb, p, k); nb += k; p += k; n -= k;
    }
  }
  void finish(u8 out[32]) {
    memset(buf + nb, 0, 64 - nb);
    compress(cv, buf, chunk, (u32)nb, (blocks == 0 ? CHUNK_START : 0) | CHUNK_END | (sp == 0 ? ROOT : 0), cv);
    while (sp) { --sp; parent(stack[sp], sp == 0 ? ROOT : 0); }
    for (int k = 0; k < 8; k++) { out[4 * k] = cv[k]; out[4 * k + 1] = cv[k] >> 8; out[4 * k + 2] = cv[k] >> 16; out[4 * k + 3] = cv[k] >> 24; }
  }
};

// ---- Keccak-f[1600] sponge, rate 136 bytes, 32 bytes out: Keccak-256 (domain suffix 0x01, the original padding) and SHA3-256 (0x06, FIPS 202) ------------
struct Keccak {
  u64 a[25]; size_t nb = 0; u8 suffix;
  explicit Keccak(u8 suffix_ = 0x01) : suffix(suffix_) { memset(a, 0, sizeof a); }
  static u64 rol(u64 x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }
  void permute() {
    static const u64 RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
                               0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
                               0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
                               0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // lane x + 5 y
    for (int r = 0; r < 24; r++) {
      u64 c[5], b[25];
      for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
      for (int x = 0; x < 5; x++) { const u64 d = c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1); for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d; }
      for (int y = 0; y < 5; y++) for (int x = 0; x < 5; x++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol(a[x + 5 * y], RHO[x + 5 * y]);
      for (int y = 0; y < 5; y++) for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
      a[0] ^= RC[r];
    }
  }
  void xor_byte(size_t pos, u8 v) { a[pos >> 3] ^= (u64)v << (8 * (pos & 7)); }   // lanes are little-endian
  void update(const void* data, size_t n) {
    const u8* p = (const u8*)data;
    for (size_t i = 0; i < n; i++) { xor_byte(nb++, p[i]); if (nb == 136) { permute(); nb = 0; } }
  }
  void finish(u8 out[32]) {   // pad10*1: the suffix behind the message, 0x80 into the block's last byte
    xor_byte(nb, suffix); xor_byte(135, 0x80); permute();
    for (int k = 0; k < 32; k++) out[k] = (u8)(a[k >> 3] >> (8 * (k & 7)));
  }
};

// the `D` of the handle's context (ms_digest): one streaming hash by ms_digest_id
struct Hasher {
  int id; Sha256 s; Blake2s b; Blake3 b3; Keccak k;
  explicit Hasher(int digest) : id(digest), k(digest == MS_DIGEST_SHA3_256 ? 0x06 : 0x01) {}
  bool keccak() const { return id == MS_DIGEST_KECCAK256 || id == MS_DIGEST_SHA3_256; }
  void update(const void* d, size_t n) { if (keccak()) k.update(d, n); else if (id == MS_DIGEST_BLAKE3) b3.update(d, n); else if (id == MS_DIGEST_BLAKE2S256) b.update(d, n); else s.update(d, n); }
  void finish(u8 out[32]) { if (keccak()) k.finish(out); else if (id == MS_DIGEST_BLAKE3) b3.finish(out); else if (id == MS_DIGEST_BLAKE2S256) b.finish(out); else s.finish(out); }
};

// pow_ok of include/ministark.h: D(seed || nonce as 8 little-endian bytes) starts with `bits` zero bits (most significant bit of byte 0 first)
static bool pow_ok(int digest, const u8 seed[32], u64 nonce, u32 bits) {
  u8 d[32], le[8];
  for (int k = 0; k < 8; k++) le[k] = (u8)(nonce >> (8 * k));
  Hasher h(digest); h.update(seed, 32); h.update(le, 8); h.finish(d);
  u64 head = 0;
  for (int k = 0; k < 8; k++) head = (head << 8) | d[k];
  return bits == 0 || (head >> (64 - bits)) == 0;
}

// Build-defined Fiat–Shamir hash chain (byte-identical to mini-stark_amd/stark.py::Transcript): the stand-in for `DigestBridge<D>`, over the context's digest.
struct Transcript {
  u8 state[32]; std::vector<u8> prover_bytes; int digest;
  Transcript(const std::string& domsep, int digest_) : digest(digest_) {
    Hasher h(digest); const char* tag = "mini-stark_amd/transcript/v0"; h.update(tag, strlen(tag)); h.update(domsep.data(), domsep.size()); h.finish(state);
  }
  void add_bytes(const u8* d, size_t n) {  // fiatshamir.rs add_digest / add_scalars
    prover_bytes.insert(prover_bytes.end(), d, d + n);
    Hasher h(digest); h.update(state, 32); h.update("A", 1); h.update(d, n); h.finish(state);
  }
  void add_scalars(const u64* limbs, size_t n) { add_bytes((const u8*)limbs, n * 8); }  // little-endian host
  void challenge_bytes(u8* out, size_t n) {
    u32 ctr = 0; size_t got = 0;
    while (got < n) {
      u8 blk[32]; Hasher h(digest); h.update(state, 32); h.update("C", 1); h.update(&ctr, 4); h.finish(blk);
      size_t k = n - got < 32 ? n - got : 32; memcpy(out + got, blk, k); got += k; ctr++;
    }
    Hasher h(digest); h.update(state, 32); h.update("R", 1); h.finish(state);
  }
  void challenge_scalars(u64* out, size_t count, u64 p) {
    std::vector<u8> raw(16 * count); challenge_bytes(raw.data(), raw.size());
    for (size_t i = 0; i < count; i++) { unsigned __int128 v; memcpy(&v, raw.data() + 16 * i, 16); out[i] = (u64)(v % p); }
  }
};

// src/air.rs:63-161 — what crosses the boundary of a TraceTable: the padded N x w matrix (host or HBM)
// and the transition closures as linear combinations of trace polynomials (tests/e2e_goldilocks.rs:48-59).
struct Lincomb { std::vector<u64> scalars; std::vector<int> idx; };
struct TraceTable {
  size_t length = 0, width = 0;
  const u64* host = nullptr; const void* device = nullptr;
  std::vector<Lincomb> transitions;
  size_t constrain_number() const { return width + transitions.size(); }  // air.rs:123-125
};

// byte buffer in page-locked host memory (ms_pinned_alloc: hipHostMalloc): the device copies the ~64 MiB FRI proof into it by DMA
struct PinnedBuf {
  u8* p = nullptr; size_t n = 0, cap = 0; bool pinned = false;   // plain malloc when page-locking is not available (no GPU in the process)
  void drop() { if (p) { if (pinned) ms_pinned_free(p); else free(p); } p = nullptr; cap = 0; }
  PinnedBuf() {}
  PinnedBuf(const PinnedBuf& o) { assign(o.p, o.p + o.n); }
  PinnedBuf& operator=(const PinnedBuf& o) { if (this != &o) assign(o.p, o.p + o.n); return *this; }
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.n = o.cap = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { drop(); p = o.p; n = o.n; cap = o.cap; pinned = o.pinned; o.p = nullptr; o.n = o.cap = 0; } return *this; }
  ~PinnedBuf() { drop(); }
  void reserve(size_t m) {
    if (m <= cap) return;
    drop();
    p = (u8*)ms_pinned_alloc(m); pinned = p != nullptr;
    if (!p) p = (u8*)malloc(m);
    cap = p ? m : 0;
  }
  void assign(size_t m, u8 v) { reserve(m); n = p ? m : 0; if (n) memset(p, v, n); }
  void resize_uninit(size_t m) { reserve(m); n = p ? m : 0; }
  void assign(const u8* a, const u8* b) { const size_t m = (size_t)(b - a); reserve(m); n = p ? m : 0; if (n) memcpy(p, a, n); }
  u8* data() { return p; } const u8* data() const { return p; }
  size_t size() const { return n; } bool empty() const { return n == 0; }
};

struct StarkProof {  // src/starks.rs:21-28 (+ the per-round roots and drawn challenges, for inspection)
  std::vector<u8> arthur; u8 trace_commit[32], constrain_trace_commit[32];
  std::vector<u64> evals;        // [q][c+1][E]: constrain_queries then validity_query per point
  std::vector<u8> fri_roots;     // rounds * 32 (round 0 first; round 0 is not in the transcript, as in the reference)
  PinnedBuf fri_blob;            // FriProof, MSFP layout (empty if left resident in HBM); page-locked: read back by DMA
  std::vector<u64> challenges;   // shift, r, z[q*E], then per round z[E], alpha[E], finally betas
  size_t c = 0;
  u64 pow_nonce = 0; bool has_pow = false;   // the proof of work's nonce (grinding_bits > 0: its 8 bytes are the last of arthur)
};

struct StarkConfig {  // src/starks.rs:238-333
  ms_ctx* ctx; ms_field field; u64 p; int e; int digest;   // digest: ms_digest(ctx), the D of commitments, transcript and check_proof
  u64 security_bits, blowup_factor, steps, rounds, constrain_queries, fri_queries, degree, trace_columns;
  u32 grinding_bits = 0;   // build-defined (msh_stark_set_grinding): bits of the security that a proof of work in front of the query phase gives
  std::string domsep;
  static int create(ms_ctx* ctx, ms_field field, u64 security_bits, u64 blowup, u64 steps, u64 trace_columns, StarkConfig* out) {
    u64 cq, fq;
    int rc = ms_num_queries(field, security_bits, blowup, steps, &cq, &fq);  // starks.rs:274-275
    if (rc) return rc;                                                       // < 20 bits panics in the reference (starks.rs:317-320)
    out->ctx = ctx; out->field = field; out->p = field == MS_FIELD_GOLDILOCKS ? 0xFFFFFFFF00000001ULL : 2013265921ULL; out->e = ms_ext_degree(ctx); out->digest = ms_digest ? ms_digest(ctx) : (int)MS_DIGEST_SHA256;
    out->security_bits = security_bits; out->blowup_factor = blowup; out->steps = steps;
    out->constrain_queries = cq; out->fri_queries = fq;
    out->degree = steps - 1;                                    // starks.rs:276
    out->rounds = ms_ceil_log2_k(steps * blowup + 1, 2);        // starks.rs:277
    out->trace_columns = trace_columns;                         // merkle_config.leafs_per_node, starks.rs:297-302
    out->domsep = "\xF0\x9F\x90\xBA";                           // starks.rs:307
    return MS_OK;
  }
};

struct Stark {
  // TWO proof slots: prove() k + 1 fills the slot proof k - 1 lived in, so that proof k - transcript, values, and its page-locked
  // FRI blob, possibly still arriving on the copy stream - stays whole and readable (`prev`, msh_prev_proof_*) while proof k + 1 is computed.
  StarkConfig cfg; StarkProof proof, prev;
  std::vector<u8> linked;   // the MSLP bytes of the last linked proof (msh_stark_prove_linked): a slot of its own, the two MSFP slots are untouched
  // src/starks.rs:59-169
  // read_fri_proof: 0 the FRI proof stays in HBM; 1 read back before returning; 2 read back ASYNCHRONOUSLY (ms_fri_proof_read_async: the bytes
  // land in the slot's page-locked buffer while the caller goes on - e.g. into the next prove; wait_proof() / any accessor of the blob completes
  // it); 3 the query-phase kernels write the blob straight INTO the slot's page-locked buffer (ms_fri_query_into: no copy at all)
  int wait_proof() const { return cfg.ctx ? ms_fri_proof_wait(cfg.ctx) : 0; }
  const u64* next_host = nullptr; size_t next_N = 0, next_w = 0;
  int prove(const TraceTable& trace, int read_fri_proof) {
    const StarkConfig& c = cfg; ms_ctx* ctx = c.ctx; const int e = c.e; const u64 p = c.p;
    std::swap(proof, prev);   // (PinnedBuf moves by pointer swap below: the buffers stay where the device writes them)
    StarkProof& pr = proof;
    pr.arthur.clear(); pr.evals.clear(); pr.fri_roots.clear(); pr.challenges.clear(); pr.c = 0; pr.fri_blob.n = 0; pr.pow_nonce = 0; pr.has_pow = false;   // the page-locked proof buffers are kept across proofs
    Transcript t(c.domsep, c.digest);
    int rc;
    // 1.1 commit to the raw trace (starks.rs:68-73)
    if (trace.device) rc = ms_trace_commit_device(ctx, trace.device, trace.length, trace.width, c.trace_columns, pr.trace_commit);
    else rc = ms_trace_commit(ctx, trace.host, trace.length, trace.width, c.trace_columns, pr.trace_commit);
    if (rc) return rc;
    // the NEXT proof's trace (msh_stark_next_trace), if the caller named one: its upload travels on an SDMA engine while this proof computes (ms_trace_upload_async)
    if (next_host) { const u64* nh = next_host; next_host = nullptr; if ((rc = ms_trace_upload_async(ctx, nh, next_N, next_w))) return rc; }
    t.add_bytes(pr.trace_commit, 32);
    // 1.2 coset LDE of the constraint polynomials + commit (starks.rs:80-95)
    u64 shift; t.challenge_scalars(&shift, 1, p); if (!shift) shift = 1;
    pr.challenges.push_back(shift);
    if ((rc = ms_interpolate(ctx))) return rc;                                  // air.rs:147-160
    for (const Lincomb& l : trace.transitions)                                  // air.rs:130-134
      if ((rc = ms_polys_lincomb(ctx, l.scalars.data(), l.idx.data(), (int)l.idx.size()))) return rc;
    if ((rc = ms_lde_commit(ctx, c.blowup_factor, shift, c.trace_columns, pr.constrain_trace_commit))) return rc;
    t.add_bytes(pr.constrain_trace_commit, 32);
    // 1.3 mix (starks.rs:108-119)
    u64 r; t.challenge_scalars(&r, 1, p); pr.challenges.push_back(r);
    if ((rc = ms_mix(ctx, r))) return rc;
    // 2. DEEP-ALI (starks.rs:124-151)
    const size_t q = c.constrain_queries; pr.c = (size_t)ms_polys_count(ctx);
    std::vector<u64> z(q * e); t.challenge_scalars(z.data(), z.size(), p);
    pr.challenges.insert(pr.challenges.end(), z.begin(), z.end());
    pr.evals.assign(q * (pr.c + 1) * e, 0);
    if ((rc = ms_eval_ext(ctx, z.data(), (int)q, pr.evals.data()))) return rc;
    // 3. FRI commit phase (fri.rs:64-113)
    pr.fri_roots.assign(c.rounds * 32, 0);
    if ((rc = ms_fri_begin(ctx, c.blowup_factor, c.rounds, pr.fri_roots.data()))) return rc;  // fri.rs:73-82
    std::vector<u64> zq(e), B(2 * e), alpha(e);
    for (u64 i = 1; i < c.rounds; i++) {                                        // fri.rs:85-110
      t.challenge_scalars(zq.data(), e, p);
      if ((rc = ms_fri_deep(ctx, zq.data(), B.data()))) return rc;              // fri.rs:89-93
      t.add_scalars(B.data(), 2 * e);                                           // fri.rs:94
      t.challenge_scalars(alpha.data(), e, p);                                  // fri.rs:96
      if ((rc = ms_fri_fold_commit(ctx, alpha.data(), pr.fri_roots.data() + i * 32))) return rc;  // fri.rs:97-107
      t.add_bytes(pr.fri_roots.data() + i * 32, 32);                            // fri.rs:108
      pr.challenges.insert(pr.challenges.end(), zq.begin(), zq.end());
      pr.challenges.insert(pr.challenges.end(), alpha.begin(), alpha.end());
    }
    // build-defined: the proof of work, behind the last commitment and in front of the query positions; the nonce travels in arthur
    if (c.grinding_bits) {
      u8 seed[32]; t.challenge_bytes(seed, 32);
      if (!ms_grind) return MS_ERR_ARG;
      if ((rc = ms_grind(ctx, seed, c.grinding_bits, 0, ~(u64)0, &pr.pow_nonce))) return rc;
      u8 le[8]; for (int k = 0; k < 8; k++) le[k] = (u8)(pr.pow_nonce >> (8 * k));
      t.add_bytes(le, 8);
      pr.has_pow = true;
    }
    // FRI query phase (fri.rs:115-189)
    std::vector<u8> raw(8 * c.fri_queries); t.challenge_bytes(raw.data(), raw.size());        // fri.rs:121-122
    std::vector<u64> betas(c.fri_queries);
    for (size_t i = 0; i < betas.size(); i++) memcpy(&betas[i], raw.data() + 8 * i, 8);        // usize::from_le_bytes, fri.rs:123-126
    if (read_fri_proof == 3) {
      size_t need = 0;
      if ((rc = ms_fri_proof_wait(ctx))) return rc;          // this slot's buffer may still be the target of proof k - 2's asynchronous read-back
      if ((rc = ms_fri_query_into(ctx, betas.data(), (int)betas.size(), nullptr, 0, &need))) return rc;
      pr.fri_blob.resize_uninit(need ? need : 1);
      if ((rc = ms_fri_query_into(ctx, betas.data(), (int)betas.size(), pr.fri_blob.data(), pr.fri_blob.size(), &need))) return rc;
      pr.fri_blob.n = need;
    } else if ((rc = ms_fri_query(ctx, betas.data(), (int)betas.size()))) return rc;
    pr.challenges.insert(pr.challenges.end(), betas.begin(), betas.end());
    if (read_fri_proof == 1 || read_fri_proof == 2) {
      if ((rc = ms_fri_proof_wait(ctx))) return rc;          // an earlier asynchronous read-back (proof k - 1's: one copy in flight per context)
      pr.fri_blob.resize_uninit(ms_fri_proof_size(ctx));
      if (!pr.fri_blob.empty() && (rc = (read_fri_proof == 2 ? ms_fri_proof_read_async(ctx, pr.fri_blob.data()) : ms_fri_proof_read(ctx, pr.fri_blob.data())))) return rc;
    }
    pr.arthur = t.prover_bytes;                                                 // starks.rs:160
    return MS_OK;
  }
};

// ------------------------------------------------------------------------------------------------
// Verifier (CPU).  src/starks.rs:171-235, src/fri.rs:191-290, src/merkle.rs:312-338.
// A PARITY MIRROR of the reference's verifier, NOT a sound verifier: like the reference it takes round 0's Merkle root from the proof
// (it never enters the transcript), does not tie y3 of a window to y1 / the opening of the next window, does not check the last round
// polynomial and only degree-bounds the shipped quotients.  "accepted" means "the reference's verifier would accept" (INTEGRATION.md 8).
// ------------------------------------------------------------------------------------------------
// nimue's Arthur: replays the prover's messages out of `arthur` into the same hash chain
struct Arthur {
  Transcript t; const u8* data; size_t len, pos = 0;
  Arthur(const std::string& domsep, int digest, const u8* d, size_t n) : t(domsep, digest), data(d), len(n) {}
  bool next_bytes(u8* out, size_t n) { if (pos + n > len) return false; memcpy(out, data + pos, n); t.add_bytes(data + pos, n); pos += n; return true; }
  bool next_scalars(u64* out, size_t n) { return next_bytes((u8*)out, n * 8); }
};

// arkworks Display (see csrc/merkle.hpp): decimal, ZERO -> "" when zae, "QuadExtField(c0 + c1 * u)" nested
template <class F> static void display(std::string& s, const u64* c, int E, int zae) {
  if (E == 1) { if (c[0] != 0 || !zae) s += std::to_string((unsigned long long)c[0]); return; }
  s += "QuadExtField("; display<F>(s, c, E / 2, zae); s += " + "; display<F>(s, c + E / 2, E / 2, zae); s += " * u)";
}
// MerkleRoot::check_proof (merkle.rs:312-338) on a serialised MerklePath (include/ministark.h); y must be one of the leaf_neighbours
template <class F, int E> static bool check_path(int digest, const u8 root[32], const u8* p, size_t avail, size_t* used, const u64* y, int zae, std::string* why) {
  const size_t lpn = 2;
  if (avail < 8 + lpn * E * 8 + 8) { *why = "truncated Merkle path"; return false; }
  const u64* q = (const u64*)p;
  const u64* leafs = q + 1;
  const u64 nlev = q[1 + lpn * E];
  const size_t total = 8 + lpn * E * 8 + 8 + (size_t)nlev * 64;
  if (nlev > 64 || avail < total) { *why = "truncated Merkle path"; return false; }
  *used = total;
  bool has = false;
  for (size_t i = 0; i < lpn; i++) { bool eq = true; for (int k = 0; k < E; k++) eq = eq && leafs[i * E + k] == y[k]; has = has || eq; }
  if (!has) { *why = "opened value is not among the leaf_neighbours (fri.rs:236-238)"; return false; }
  std::string msg;
  for (size_t i = 0; i < lpn; i++) display<F>(msg, leafs + i * E, E, zae);          // calculate_from_leafs, merkle.rs:162-168
  u8 prev[32]; { Hasher h(digest); h.update(msg.data(), msg.size()); h.finish(prev); }
  const u8* lv = p + 8 + lpn * E * 8 + 8;
  for (u64 l = 0; l < nlev; l++, lv += 64) {
    if (memcmp(lv, prev, 32) != 0 && memcmp(lv + 32, prev, 32) != 0) { *why = "Merkle path does not contain the running digest"; return false; }
    Hasher h(digest); h.update(lv, 64); h.finish(prev);                                     // calculate_from_nodes, merkle.rs:171-177
  }
  if (memcmp(prev, root, 32) != 0) { *why = "Merkle path does not end at the round's root"; return false; }
  return true;
}

template <class F, int E> struct Verifier {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  static X load(const u64* v) { X r; for (int k = 0; k < E; k++) r.c[k] = F::from_u64(v[k]); return r; }
  static bool canon(const u64* v, size_t n) { for (size_t i = 0; i < n; i++) if (v[i] >= F::P) return false; return true; }
  static bool eq(const X& a, const u64* v) { for (int k = 0; k < E; k++) if (F::to_u64(a.c[k]) != v[k]) return false; return true; }
  // base-coefficient polynomial at an extension point (field.rs:23-32 extend_poly + evaluate)
  static X horner_base(const u64* coef, size_t n, const X& z) {
    X acc = e_zero<F, E>();
    for (size_t i = n; i-- > 0;) { acc = e_mul<F>(acc, z); acc.c[0] = F::add(acc.c[0], F::from_u64(coef[i])); }
    return acc;
  }
  // 1 accepted, 0 rejected (reason in *why), < 0 malformed input
  static int run(const StarkConfig& c, const u64* constrains, size_t nc, size_t N, const StarkProof& pr, int zae, std::string* why) {
    const int e = E; const u64 p = c.p;
    if (!canon(constrains, nc * N) || !canon(pr.evals.data(), pr.evals.size())) { *why = "non-canonical element"; return MS_ERR_ARG; }
    // 1. commits match the transcript (starks.rs:186-193)
    Arthur ar(c.domsep, c.digest, pr.arthur.data(), pr.arthur.size());
    u8 d[32];
    if (!ar.next_bytes(d, 32) || memcmp(d, pr.trace_commit, 32)) { *why = "trace commit does not match the transcript"; return 0; }
    u64 shift; ar.t.challenge_scalars(&shift, 1, p);
    if (!ar.next_bytes(d, 32) || memcmp(d, pr.constrain_trace_commit, 32)) { *why = "constraint-trace commit does not match the transcript"; return 0; }
    u64 r; ar.t.challenge_scalars(&r, 1, p);
    // 2. DEEP-ALI linking (starks.rs:195-225)
    const size_t q = c.constrain_queries;
    if (pr.evals.size() != q * (nc + 1) * e) { *why = "wrong number of out-of-domain values"; return 0; }
    std::vector<u64> z(q * e); ar.t.challenge_scalars(z.data(), z.size(), p);
    // c_x = sum_i r^i f_i, then divide_by_vanishing_poly over Radix2(degree + 1): the FIRST returned polynomial must be zero and
    // the SECOND is evaluated (starks.rs:220-224; the reference binds (quotient, remainder) to the names (rest, quotient): quirk Q1)
    size_t nd = 1; while (nd < c.degree + 1) nd <<= 1;
    std::vector<u64> cx(N, 0);
    { T rp = F::from_u64(1);
      for (size_t i = 0; i < nc; i++) { for (size_t k = 0; k < N; k++) cx[k] = F::to_u64(F::add(F::from_u64(cx[k]), F::mul(rp, F::from_u64(constrains[i * N + k])))); rp = F::mul(rp, F::from_u64(r)); } }
    std::vector<u64> rem(nd < N ? nd : N, 0);
    for (size_t k = 0; k < N; k++) {
      if (k >= nd && cx[k] != 0) { *why = "mixed constraint polynomial has degree >= |trace domain|: first output of divide_by_vanishing_poly is not zero (starks.rs:221)"; return 0; }
      if (k < rem.size()) rem[k] = cx[k];
    }
    for (size_t t = 0; t < q; t++) {
      const X zz = load(&z[t * e]);
      const u64* ev = &pr.evals[t * (nc + 1) * e];
      for (size_t i = 0; i < nc; i++)
        if (!eq(horner_base(constrains + i * N, N, zz), ev + i * e)) { *why = "constraint polynomial evaluation does not match the proof (starks.rs:215)"; return 0; }
      if (!eq(horner_base(rem.data(), rem.size(), zz), ev + nc * e)) { *why = "validity evaluation does not match the proof (starks.rs:224)"; return 0; }
    }
    // 3. FRI (fri.rs:191-290)
    const size_t R = c.rounds, nq = c.fri_queries;
    if (R < 1 || pr.fri_roots.size() != R * 32) { *why = "wrong number of FRI roots"; return 0; }
    std::vector<X> zs, alphas, B0, B1;
    for (size_t i = 1; i < R; i++) {                                              // read_proof_transcript, fri.rs:247-279
      std::vector<u64> v(e), b(2 * e), a(e);
      ar.t.challenge_scalars(v.data(), e, p);
      if (!ar.next_scalars(b.data(), 2 * e) || !canon(b.data(), 2 * e)) { *why = "transcript too short / DEEP coefficients not canonical"; return 0; }
      ar.t.challenge_scalars(a.data(), e, p);
      if (!ar.next_bytes(d, 32)) { *why = "transcript too short"; return 0; }
      // round i's commitment is in the transcript; round 0's never is (fri.rs:73-82: as in the reference) and is taken from the proof
      if (memcmp(d, pr.fri_roots.data() + i * 32, 32)) { *why = "FRI round root does not match the transcript"; return 0; }
      zs.push_back(load(v.data())); alphas.push_back(load(a.data())); B0.push_back(load(b.data())); B1.push_back(load(b.data() + e));
    }
    if (c.grinding_bits) {   // the prover's step at the same place: seed drawn, nonce read (and absorbed), predicate checked
      u8 seed[32], le[8]; ar.t.challenge_bytes(seed, 32);
      if (!ar.next_bytes(le, 8)) { *why = "transcript too short: no proof of work nonce"; return 0; }
      u64 nonce = 0; for (int k = 0; k < 8; k++) nonce |= (u64)le[k] << (8 * k);
      if (!pow_ok(c.digest, seed, nonce, c.grinding_bits)) { *why = "proof of work: the nonce's digest has fewer leading zero bits than the configured grinding bits"; return 0; }
    }
    if (ar.pos != ar.len) { *why = "trailing bytes in the transcript"; return 0; }
    std::vector<u8> raw(8 * nq); ar.t.challenge_bytes(raw.data(), raw.size());
    if (R > 63) { *why = "too many rounds"; return MS_ERR_ARG; }
    const u64 dsize = (u64)1 << R;
    const T g = f_root_of_unity<F>((int)R);
    std::vector<T> prev(nq);
    for (size_t j = 0; j < nq; j++) { u64 b; memcpy(&b, raw.data() + 8 * j, 8); if (b > dsize) b %= dsize; prev[j] = f_pow<F>(g, b); }  // fri.rs:271-277 (quirk Q6: `>`)
    const u8* bp = pr.fri_blob.data(); size_t left = pr.fri_blob.size();
    for (size_t i = 0; i + 1 < R; i++) {
      for (size_t j = 0; j < nq; j++) {
        if (left < (size_t)(6 * e + 1) * 8) { *why = "FRI proof truncated"; return 0; }
        const u64* pts = (const u64*)bp;
        if (!canon(pts, 6 * e)) { *why = "FRI point not canonical"; return 0; }
        const X x1 = load(pts), y1 = load(pts + e), x2 = load(pts + 2 * e), y2 = load(pts + 3 * e), x3 = load(pts + 4 * e), y3 = load(pts + 5 * e);
        const u64 qlen = pts[6 * e];
        if (qlen > ((u64)1 << 40) || left < (size_t)(6 * e + 1) * 8 + (size_t)qlen * e * 8) { *why = "FRI proof truncated"; return 0; }
        const u64* quo = pts + 6 * e + 1;
        if (!canon(quo, (size_t)qlen * e)) { *why = "quotient coefficient not canonical"; return 0; }
        bp += (6 * e + 1) * 8 + qlen * e * 8; left -= (6 * e + 1) * 8 + qlen * e * 8;
        const X X1 = e_from_base<F, E>(prev[j]);
        if (!e_eq<F, E>(x1, X1)) { *why = "x1 is not the previous round's x3 (fri.rs:215)"; return 0; }
        if (!e_eq<F, E>(e_from_base<F, E>(F::neg(prev[j])), x2)) { *why = "x2 != -x1 (fri.rs:216)"; return 0; }
        const T x3b = F::mul(prev[j], prev[j]);
        if (!e_eq<F, E>(e_from_base<F, E>(x3b), x3)) { *why = "x3 != x1^2 (fri.rs:217)"; return 0; }
        // degree bound of the shipped quotient (fri.rs:219-224): trimmed degree + deg((x-x1)(x-x2)(x-x3))
        size_t deg = 0;
        for (size_t k = qlen; k-- > 0;) { bool nz = false; for (int l = 0; l < e; l++) nz = nz || quo[k * e + l] != 0; if (nz) { deg = k; break; } }
        const u64 total = deg + 3;
        if (total < 2 || total > ((u64)1 << (R - i))) { *why = "quotient degree out of bounds (fri.rs:222-223)"; return 0; }
        // linearity against the DEEP-adjusted next-round value (fri.rs:226-234): the line through (x1,y1), (x2,y2) at alpha
        const T dxi = f_inv<F>(F::sub(F::neg(prev[j]), prev[j]));               // 1 / (x2 - x1), base field
        const X a = e_mul_base<F, E>(e_sub<F, E>(y2, y1), dxi);
        const X b = e_sub<F, E>(y1, e_mul_base<F, E>(a, prev[j]));
        const X lhs = e_add<F, E>(b, e_mul<F>(a, alphas[i]));
        const X deep = e_add<F, E>(e_mul<F>(y3, e_sub<F, E>(x3, zs[i])), e_add<F, E>(B0[i], e_mul<F>(B1[i], alphas[i])));
        if (!e_eq<F, E>(lhs, deep)) { *why = "DEEP-adjusted linearity check failed (fri.rs:234)"; return 0; }
        // Merkle openings of y1, y2 in round i's tree (fri.rs:236-239; checked against round i's root and enforced — the reference
        // discards check_proof's result and names the next round's root: DESIGN.md quirk Q13)
        for (int s2 = 0; s2 < 2; s2++) {
          size_t used = 0;
          if (!check_path<F, E>(c.digest, pr.fri_roots.data() + i * 32, bp, left, &used, s2 ? pts + 3 * e : pts + e, zae, why)) return 0;
          bp += used; left -= used;
        }
        prev[j] = x3b;
      }
    }
    if (left != 0) { *why = "trailing bytes in the FRI proof"; return 0; }
    return 1;
  }
};

// ---- the verifying side of the openings by index (ministark.h: ms_tree_open, ms_fri_query_index; build-defined) ----------------------------------------------
// check_path made POSITIONAL: the path's leaf_index word must be `expect_index` (an element index: its group is expect_index / lpn), the leaf_neighbours (lpn
// elements of E limbs) canonical; at level l the running digest must sit in slot (group >> l) & 1 - not in either half -, the path must be exactly as high as the
// position needs (group >> nlevels == 0) and end at `root`.  true, or false with the reason in *why; *used: the bytes of the path
template <class F> static bool check_path_at(int digest, int E, size_t lpn, int zae, const u8 root[32], const u8* p, size_t avail, u64 expect_index, size_t* used, std::string* why) {
  const size_t head = 8 + lpn * E * 8 + 8;
  if (avail < head) { *why = "truncated Merkle path"; return false; }
  u64 leaf_index, nlev;
  memcpy(&leaf_index, p, 8); memcpy(&nlev, p + head - 8, 8);
  if (nlev > 64 || avail - head < (size_t)nlev * 64) { *why = "truncated Merkle path"; return false; }
  *used = head + (size_t)nlev * 64;
  if (leaf_index != expect_index) { *why = "the path's leaf_index is not the position asked for"; return false; }
  std::vector<u64> leafs(lpn * E);
  memcpy(leafs.data(), p + 8, lpn * E * 8);
  for (u64 v : leafs) if (v >= F::P) { *why = "leaf neighbour not canonical"; return false; }
  const u64 group = expect_index / lpn;
  if (nlev < 64 && (group >> nlev) != 0) { *why = "the path is too short for its position"; return false; }
  std::string msg;
  for (size_t i = 0; i < lpn; i++) display<F>(msg, leafs.data() + i * E, E, zae);
  u8 prev[32]; { Hasher h(digest); h.update(msg.data(), msg.size()); h.finish(prev); }
  const u8* lv = p + head;
  for (u64 l = 0; l < nlev; l++, lv += 64) {
    if (memcmp(lv + 32 * ((group >> l) & 1), prev, 32) != 0) { *why = "the running digest is not in the slot its position names"; return false; }
    Hasher h(digest); h.update(lv, 64); h.finish(prev);
  }
  if (memcmp(prev, root, 32) != 0) { *why = "Merkle path does not end at the root"; return false; }
  return true;
}

// the MSFI blob (ministark.h) against the rounds' roots and the round challenges: 1 accepted, 0 rejected (reason in *why)
template <class F, int E> static int fri_index_verify(int digest, int zae, u64 blowup, const u8* roots, size_t R, const u64* z, const u64* B, const u64* alpha,
                                                      const u64* betas, size_t nq, const u8* blob, size_t len, std::string* why) {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  const size_t W = R - 1;
  if (!V::canon(z, W * E) || !V::canon(B, W * 2 * E) || !V::canon(alpha, W * E)) { *why = "round challenge not canonical"; return 0; }
  if (len < 48) { *why = "MSFI blob shorter than its header"; return 0; }
  u64 hd[6]; memcpy(hd, blob, 48);
  if (hd[0] != 0x4946534DULL) { *why = "not an MSFI blob (magic)"; return 0; }
  if (hd[1] != (u64)E || hd[2] != (u64)R || hd[3] != (u64)nq) { *why = "MSFI header: E, rounds or queries are not the verifier's"; return 0; }
  const u64 D0 = hd[4], nfinal = hd[5];
  if (D0 < 2 || (D0 & (D0 - 1)) || D0 > ((u64)1 << F::TWO_ADICITY) || (D0 >> W) < 2) { *why = "MSFI header: D_0 is no domain size that R rounds can halve"; return 0; }
  const u64 Dlast = D0 >> W, bound = Dlast / blowup > 1 ? Dlast / blowup : 1;
  if (nfinal > bound) { *why = "the final polynomial is longer than D_(R-1) / blowup"; return 0; }
  const u8* bp = blob + 48; size_t left = len - 48;
  if (left / 8 < nfinal * E) { *why = "MSFI blob truncated in the final polynomial"; return 0; }
  const u64* fin = (const u64*)bp;
  if (!V::canon(fin, (size_t)nfinal * E)) { *why = "final polynomial coefficient not canonical"; return 0; }
  bp += nfinal * E * 8; left -= nfinal * E * 8;
  // the openings: y[(i * nq + j) * 2 + s], every path checked at its position under round i's root
  std::vector<X> y(W * nq * 2);
  std::vector<u64> b(betas, betas + nq);
  for (size_t i = 0; i < W; i++) {
    const u64 D = D0 >> i;
    u64 want_lev = 0; while (((u64)2 << want_lev) < D) want_lev++;   // log2(D / 2)
    for (size_t j = 0; j < nq; j++) {
      b[j] %= D;
      for (int s = 0; s < 2; s++) {
        const u64 pos = s ? (b[j] + D / 2) % D : b[j];
        size_t used = 0;
        if (!check_path_at<F>(digest, E, 2, zae, roots + i * 32, bp, left, pos, &used, why)) return 0;
        u64 nlev; memcpy(&nlev, bp + 8 + 2 * E * 8, 8);
        if (nlev != want_lev) { *why = "a path's height is not its round's"; return 0; }
        y[(i * nq + j) * 2 + s] = V::load((const u64*)(bp + 8) + (pos & 1) * E);
        bp += used; left -= used;
      }
    }
  }
  if (left != 0) { *why = "trailing bytes in the MSFI blob"; return 0; }
  // the folds: the line through (x1, y1), (x2, y2) at alpha_i against the DEEP-adjusted next value (Verifier::run step 3), y3 = the next window's y1 / the final polynomial at x3
  b.assign(betas, betas + nq);
  for (size_t i = 0; i < W; i++) {
    const u64 D = D0 >> i;
    int lg = 0; while (((u64)1 << lg) < D) lg++;
    const T g = f_root_of_unity<F>(lg);
    const X zi = V::load(z + i * E), ai = V::load(alpha + i * E), B0 = V::load(B + i * 2 * E), B1 = V::load(B + i * 2 * E + E);
    for (size_t j = 0; j < nq; j++) {
      b[j] %= D;
      const T x1 = f_pow<F>(g, b[j]), x3b = F::mul(x1, x1);
      const X y1 = y[(i * nq + j) * 2], y2 = y[(i * nq + j) * 2 + 1], x3 = e_from_base<F, E>(x3b);
      X y3;
      if (i + 1 < W) y3 = y[((i + 1) * nq + j) * 2];
      else { y3 = e_zero<F, E>(); for (size_t k = nfinal; k-- > 0;) y3 = e_add<F, E>(e_mul<F>(y3, x3), V::load(fin + k * E)); }
      const T dxi = f_inv<F>(F::sub(F::neg(x1), x1));
      const X a = e_mul_base<F, E>(e_sub<F, E>(y2, y1), dxi);
      const X c0 = e_sub<F, E>(y1, e_mul_base<F, E>(a, x1));
      const X lhs = e_add<F, E>(c0, e_mul<F>(a, ai));
      const X deep = e_add<F, E>(e_mul<F>(y3, e_sub<F, E>(x3, zi)), e_add<F, E>(B0, e_mul<F>(B1, ai)));
      if (!e_eq<F, E>(lhs, deep)) { *why = i + 1 < W ? "DEEP-adjusted linearity check failed against the next round's opening" : "DEEP-adjusted linearity check failed against the final polynomial"; return 0; }
    }
  }
  return 1;
}

// ---- the verifying side of the folded FRI (ministark.h: ms_fri_begin_folded .. ms_fri_query_folded; build-defined) ------------------------------------------------
// The MSFF blob against the rounds' roots and the fold challenges: 1 accepted, 0 rejected (*why names the step).  Order: header, the length the header fixes, the
// final polynomial's limbs, every opening round by round, every fold, the final polynomial.  Round 0's values are bound to nothing here
template <class F, int E> static int fri_folded_verify(int digest, int zae, u64 blowup, int k, const u8* roots, size_t R, const u64* alpha, const u64* betas, size_t nq,
                                                       const u8* blob, size_t len, std::string* why) {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  const size_t a = (size_t)1 << k;
  if (len < 56) { *why = "header: MSFF blob shorter than its header"; return 0; }
  u64 hd[7]; memcpy(hd, blob, 56);
  if (hd[0] != 0x4646534DULL) { *why = "header: not an MSFF blob (magic)"; return 0; }
  if (hd[1] != (u64)E || hd[2] != (u64)k || hd[3] != (u64)R || hd[4] != (u64)nq) { *why = "header: E, log_arity, rounds or queries are not the verifier's"; return 0; }
  const u64 D0 = hd[5], nfinal = hd[6];
  const unsigned sh = (unsigned)k * (unsigned)R;   // (R <= 64: no overflow; above the two-adicity no domain is that large)
  if (sh > (unsigned)F::TWO_ADICITY || D0 < 1 || (D0 & (D0 - 1)) || D0 > ((u64)1 << F::TWO_ADICITY) || (D0 >> sh) < blowup) { *why = "header: D_0 is no domain size with arity^R * blowup <= D_0"; return 0; }
  const u64 DR = D0 >> sh;
  if (nfinal != DR / blowup) { *why = "header: nfinal is not D_R / blowup"; return 0; }
  std::vector<u64> height(R), psize(R);
  size_t want = 56 + (size_t)nfinal * E * 8;
  for (size_t i = 0; i < R; i++) {
    u64 groups = D0 >> ((unsigned)k * (unsigned)(i + 1)), h = 0;
    while (((u64)1 << h) < groups) h++;
    height[i] = h; psize[i] = 16 + a * E * 8 + 64 * h;
    want += nq * (size_t)psize[i];
  }
  if (len != want) { *why = "header: the blob's length is not the one its header fixes (truncated, or trailing bytes)"; return 0; }
  const u64* fin = (const u64*)(blob + 56);
  if (!V::canon(fin, (size_t)nfinal * E)) { *why = "final polynomial: coefficient not canonical"; return 0; }
  const u8* bp = blob + 56 + (size_t)nfinal * E * 8;
  // positions b[i * nq + j], i = 0 .. R
  std::vector<u64> b((R + 1) * nq);
  for (size_t j = 0; j < nq; j++) b[j] = betas[j] % D0;
  for (size_t i = 0; i < R; i++) for (size_t j = 0; j < nq; j++) b[(i + 1) * nq + j] = b[i * nq + j] % (D0 >> ((unsigned)k * (unsigned)(i + 1)));
  std::vector<X> cos(R * nq * a);
  for (size_t i = 0; i < R; i++)
    for (size_t j = 0; j < nq; j++) {
      const std::string at = "round " + std::to_string(i) + " opening: ";
      const u64 grp = b[(i + 1) * nq + j];
      u64 nlev; memcpy(&nlev, bp + 8 + a * E * 8, 8);
      if (nlev != height[i]) { *why = at + "a path's height is not its round's"; return 0; }
      size_t used = 0; std::string w;
      if (!check_path_at<F>(digest, E, a, zae, roots + i * 32, bp, (size_t)psize[i], grp * a, &used, &w) || used != psize[i]) { *why = at + w; return 0; }
      for (size_t t = 0; t < a; t++) cos[(i * nq + j) * a + t] = V::load((const u64*)(bp + 8) + t * E);
      bp += used;
    }
  // the fold of round i's opened coset at alpha_i, by Lagrange interpolation on the coset of x = g_i^(b_(i+1,j)): the value at position b_(i+1,j) of round i + 1
  auto folded = [&](size_t i, size_t j) {
    const u64 D = D0 >> ((unsigned)k * (unsigned)i), m = D / a;
    int lg = 0; while (((u64)1 << lg) < D) lg++;
    const T g = f_root_of_unity<F>(lg), w = f_pow<F>(g, m);
    const X al = V::load(alpha + i * E);
    T xs[8];
    xs[0] = f_pow<F>(g, b[(i + 1) * nq + j]);
    for (size_t t = 1; t < a; t++) xs[t] = F::mul(xs[t - 1], w);
    X acc = e_zero<F, E>();
    for (size_t t = 0; t < a; t++) {
      X num = e_one<F, E>(); T den = F::from_u64(1);
      for (size_t u = 0; u < a; u++) if (u != t) { num = e_mul<F>(num, e_sub<F, E>(al, e_from_base<F, E>(xs[u]))); den = F::mul(den, F::sub(xs[t], xs[u])); }
      acc = e_add<F, E>(acc, e_mul_base<F, E>(e_mul<F>(cos[(i * nq + j) * a + t], num), f_inv<F>(den)));
    }
    return acc;
  };
  for (size_t i = 1; i < R; i++) {
    const u64 Dn = D0 >> ((unsigned)k * (unsigned)(i + 1));
    for (size_t j = 0; j < nq; j++)
      if (!e_eq<F, E>(cos[(i * nq + j) * a + b[i * nq + j] / Dn], folded(i - 1, j))) {
        *why = "round " + std::to_string(i) + " fold: the opened value is not the fold of the previous round's coset"; return 0;
      }
  }
  int lgR = 0; while (((u64)1 << lgR) < DR) lgR++;
  const T gR = f_root_of_unity<F>(lgR);
  for (size_t j = 0; j < nq; j++) {
    const X x = e_from_base<F, E>(f_pow<F>(gR, b[R * nq + j]));
    X y = e_zero<F, E>();
    for (size_t n = nfinal; n-- > 0;) y = e_add<F, E>(e_mul<F>(y, x), V::load(fin + n * E));
    if (!e_eq<F, E>(y, folded(R - 1, j))) { *why = "final polynomial: its value is not the fold of the last round's coset"; return 0; }
  }
  return 1;
}

// ---- the verifying side of the DEEP stage (ministark.h: ms_validity_commit, ms_deep_compose; build-defined) -------------------------------------------------------
// V(z) = sum_k z^(kN) sum_l u_l V_(k,l)(z) from the m = ve * nchunks chunk evaluations (chunk column k * ve + l, E limbs each); u_l = the l-th basis element of K
template <class F, int E> static void validity_from_chunks(u32 ve, u32 nchunks, u64 N, const u64* z, const u64* ev, u64* out) {
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  const X zz = V::load(z), zN = e_pow<F, E>(zz, N);
  X acc = e_zero<F, E>();
  for (u32 k = nchunks; k-- > 0;) {   // Horner in z^N
    X inner = e_zero<F, E>();
    for (u32 l = 0; l < ve; l++) { X u = e_zero<F, E>(); u.c[l] = F::from_u64(1); inner = e_add<F, E>(inner, e_mul<F>(u, V::load(ev + ((size_t)k * ve + l) * E))); }
    acc = e_add<F, E>(e_mul<F>(acc, zN), inner);
  }
  for (int l = 0; l < E; l++) out[l] = F::to_u64(acc.c[l]);
}

// ---- what the two link verifiers share: the validation of their arguments, the tables over the claimed evaluations, D(x) from opened leaf groups
template <class F, int E> struct LinkTables {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  const ms_deep& d; u32 c0, c; size_t ne = 0; u64 L = 0; T sh, gL;
  std::vector<X> z, gpow, ev, inv; std::vector<u32> pt_of;
  LinkTables(const ms_deep& d_, u32 c0_, u32 c1) : d(d_), c0(c0_), c(c0_ + c1) {}
  // 1: go on; otherwise the verdict (0 rejected, < 0 malformed arguments) with the reason in *why.  min_L: the smallest LDE domain the caller's leaf groups need;
  // `step` stands in front of the two rejections (the folded verifier names the step there, the plain one does not)
  int init(u64 N, u64 blowup, u64 shift, u64 min_L, u32 m, const u64* evals, const u64* gamma, const std::string& step, std::string* why) {
    L = N * blowup;
    if (shift == 0 || shift >= F::P || L > ((u64)1 << F::TWO_ADICITY) || L < min_L) { *why = "shift or domain size out of range"; return MS_ERR_ARG; }
    if (d.npts < 1 || d.npts > 8 || d.pt_begin[0] != 0) { *why = "malformed ms_deep"; return MS_ERR_ARG; }
    for (u32 t = 0; t < d.npts; t++) if (d.pt_begin[t + 1] <= d.pt_begin[t] || d.pt_begin[t + 1] > 8192) { *why = "malformed ms_deep"; return MS_ERR_ARG; }
    ne = d.pt_begin[d.npts];
    for (size_t n = 0; n < ne; n++) if (d.pt_poly[n] >= c + m) { *why = "malformed ms_deep: an index at or above c + m"; return MS_ERR_ARG; }
    if (!V::canon(d.z, (size_t)d.npts * E) || !V::canon(gamma, E)) { *why = "a point or gamma is not canonical"; return MS_ERR_ARG; }
    if (!V::canon(evals, ne * E)) { *why = step + "claimed evaluation not canonical"; return 0; }
    int lgL = 0; while (((u64)1 << lgL) < L) lgL++;
    sh = F::from_u64(shift); gL = f_root_of_unity<F>(lgL);
    const T shL = f_pow<F>(sh, L);
    z.resize(d.npts); inv.resize(d.npts);
    for (u32 t = 0; t < d.npts; t++) {
      z[t] = V::load(d.z + (size_t)t * E);
      if (e_eq<F, E>(e_pow<F, E>(z[t], L), e_from_base<F, E>(shL))) { *why = step + "a point lies in the LDE coset: the quotient by (x - z) is undefined at one of its rows"; return 0; }
    }
    X gp = e_one<F, E>();
    const X g = V::load(gamma);
    gpow.resize(ne); ev.resize(ne); pt_of.resize(ne);
    for (u32 t = 0; t < d.npts; t++) for (u32 n = d.pt_begin[t]; n < d.pt_begin[t + 1]; n++) pt_of[n] = t;
    for (size_t n = 0; n < ne; n++, gp = e_mul<F>(gp, g)) { gpow[n] = gp; ev[n] = V::load(evals + n * E); }
    return 1;
  }
  // D(x) = sum_n gamma^n (f_n(x) - ev_n) / (x - z_t) from the opened leaf groups and the claimed evaluations: word col * a + t of a group is column col at
  // slot t (a plain row: a = 1, t = 0)
  X compose_at(T x, const u64* lrow, const u64* srow, const u64* vrow, u64 a, u64 t) {
    for (u32 p = 0; p < d.npts; p++) inv[p] = e_inv<F>(e_sub<F, E>(e_from_base<F, E>(x), z[p]));
    X Dx = e_zero<F, E>();
    for (size_t n = 0; n < ne; n++) {
      const u32 fi = d.pt_poly[n];
      const T fx = F::from_u64(fi < c0 ? lrow[(u64)fi * a + t] : fi < c ? srow[(u64)(fi - c0) * a + t] : vrow[(u64)(fi - c) * a + t]);
      Dx = e_add<F, E>(Dx, e_mul<F>(gpow[n], e_mul<F>(e_sub<F, E>(e_from_base<F, E>(fx), ev[n]), inv[pt_of[n]])));
    }
    return Dx;
  }
};
// a cursor over one tree's opening section: open() checks the next path at its element index under the root and yields the leaf group's lpn words
template <class F> struct OpenCursor {
  const char* name; int digest, zae; const u8* root; size_t lpn; const u8* p; size_t left;
  const u64* open(u64 index, std::string* why) {
    size_t used = 0; std::string w;
    if (!check_path_at<F>(digest, 1, lpn, zae, root, p, left, index, &used, &w)) { *why = std::string(name) + " opening: " + w; return nullptr; }
    const u64* words = (const u64*)(p + 8);
    p += used; left -= used;
    return words;
  }
  bool done(std::string* why) const { if (left) *why = std::string(name) + " opening: trailing bytes"; return left == 0; }
};

// the link between FRI's round 0 and the two committed trees: 1 accepted, 0 rejected (reason in *why), < 0 malformed arguments
// c1 > 0 (msh_deep_link_verify_staged): the columns c0 .. c0 + c1 - 1 come from rows of a second tree under stg_root, opened at the same rows
template <class F, int E> static int deep_link_verify(int digest, int zae, u64 N, u64 blowup, u64 shift, u32 c0, u32 c1, u32 m, const u8* lde_root, const u8* stg_root, const u8* val_root,
                                                      const ms_deep& d, const u64* evals, const u64* gamma, const u64* betas, size_t nq, const u8* msfi, size_t msfi_len,
                                                      const u8* lde_open, size_t lde_len, const u8* stg_open, size_t stg_len, const u8* val_open, size_t val_len, std::string* why) {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  LinkTables<F, E> lt(d, c0, c1);
  const int ok = lt.init(N, blowup, shift, 0, m, evals, gamma, "", why);
  if (ok != 1) return ok;
  const u64 L = lt.L;
  // the MSFI header, the final polynomial, and window 0's openings (the whole blob is msh_fri_index_verify's to check)
  if (msfi_len < 48) { *why = "MSFI blob shorter than its header"; return 0; }
  u64 hd[6]; memcpy(hd, msfi, 48);
  if (hd[0] != 0x4946534DULL) { *why = "not an MSFI blob (magic)"; return 0; }
  if (hd[1] != (u64)E || hd[3] != (u64)nq || hd[2] < 1 || hd[2] > 64) { *why = "MSFI header: E, rounds or queries are not the verifier's"; return 0; }
  const u64 R = hd[2], D0 = hd[4], nfinal = hd[5];
  if (D0 < 1 || (D0 & (D0 - 1)) || D0 > L || L % D0) { *why = "MSFI header: D_0 does not divide the LDE domain"; return 0; }
  if (R > 1 && D0 < 2) { *why = "MSFI header: D_0 cannot be halved"; return 0; }
  const u8* bp = msfi + 48; size_t left = msfi_len - 48;
  if (left / 8 < nfinal * E || nfinal > D0) { *why = "MSFI blob truncated in the final polynomial"; return 0; }
  const u64* fin = (const u64*)bp;
  if (!V::canon(fin, (size_t)nfinal * E)) { *why = "final polynomial coefficient not canonical"; return 0; }
  bp += nfinal * E * 8; left -= nfinal * E * 8;
  const u64 step = L / D0;
  int lg0 = 0; while (((u64)1 << lg0) < D0) lg0++;
  const T g0 = f_root_of_unity<F>(lg0);
  OpenCursor<F> lde{"LDE", digest, zae, lde_root, c0, lde_open, lde_len}, stg{"staged", digest, zae, stg_root, c1, stg_open, stg_len},
      val{"validity", digest, zae, val_root, m, val_open, val_len};
  for (size_t j = 0; j < nq; j++) {
    const u64 b = betas[j] % D0;
    for (int s = 0; s < 2; s++) {
      const u64 pos = s ? (b + D0 / 2) % D0 : b, row = pos * step;
      const u64* lrow = lde.open(row * c0, why);
      const u64* srow = lrow && c1 ? stg.open(row * c1, why) : nullptr;
      if (!lrow || (c1 && !srow)) return 0;
      const u64* vrow = val.open(row * m, why);
      if (!vrow) return 0;
      // D(x) at x = shift * g_L^row from the opened rows and the claimed evaluations
      const X Dx = lt.compose_at(F::mul(lt.sh, f_pow<F>(lt.gL, row)), lrow, srow, vrow, 1, 0);
      X y;
      if (R > 1) {   // what window 0 opened at this position
        const size_t head = 8 + 2 * (size_t)E * 8 + 8;
        if (left < head) { *why = "MSFI blob truncated in window 0"; return 0; }
        u64 li, nlev; memcpy(&li, bp, 8); memcpy(&nlev, bp + head - 8, 8);
        if (nlev > 64 || left - head < (size_t)nlev * 64) { *why = "MSFI blob truncated in window 0"; return 0; }
        if (li != pos) { *why = "MSFI: a window-0 path is not at the query's position"; return 0; }
        if (!V::canon((const u64*)(bp + 8), 2 * E)) { *why = "MSFI: opened value not canonical"; return 0; }
        y = V::load((const u64*)(bp + 8) + (pos & 1) * E);
        bp += head + (size_t)nlev * 64; left -= head + (size_t)nlev * 64;
      } else {       // no window: the final polynomial IS round 0's, in the clear
        const X xb = e_from_base<F, E>(f_pow<F>(g0, pos));
        y = e_zero<F, E>();
        for (size_t k = nfinal; k-- > 0;) y = e_add<F, E>(e_mul<F>(y, xb), V::load(fin + k * E));
      }
      if (!e_eq<F, E>(Dx, y)) { *why = R > 1 ? "DEEP link: the composition recomputed from the opened rows and the claimed evaluations is not the value round 0 opened" : "DEEP link: the composition recomputed from the opened rows and the claimed evaluations is not the final polynomial's value"; return 0; }
    }
  }
  if (!lde.done(why) || (c1 && !stg.done(why)) || !val.done(why)) return 0;
  return 1;
}

// the link between a FOLDED FRI's round 0 and the coset-grouped row trees (ministark.h: ms_lde_commit_coset .., ms_query_linked_folded): 1 accepted, 0 rejected (the
// reason in *why, beginning with the step's name), < 0 malformed arguments.  Query j opens ONE leaf group of every tree, group q_j s with q_j = (beta mod D_0) mod D_1
// and s = L / D_0: slot col * a + t of it is column col of the LDE row q_j s + t L / a, which lies under position q_j + t D_1 of round 0 - slot t of round 0's opened
// coset.  ALL a slots are recomputed and compared: all of them feed the fold.  The MSFF itself is msh_fri_folded_verify's to check
template <class F, int E> static int deep_link_verify_folded(int digest, int zae, u64 N, u64 blowup, u64 shift, int k, u32 c0, u32 c1, u32 m, const u8* lde_root, const u8* stg_root,
                                                             const u8* val_root, const ms_deep& d, const u64* evals, const u64* gamma, const u64* betas, size_t nq, const u8* msff,
                                                             size_t msff_len, const u8* lde_open, size_t lde_len, const u8* stg_open, size_t stg_len, const u8* val_open, size_t val_len,
                                                             std::string* why) {
  typedef typename F::T T;
  typedef Verifier<F, E> V;
  const u64 a = (u64)1 << k;
  LinkTables<F, E> lt(d, c0, c1);
  const int ok = lt.init(N, blowup, shift, 2 * a, m, evals, gamma, "DEEP link: ", why);
  if (ok != 1) return ok;
  const u64 L = lt.L;
  // the MSFF header and round 0's paths: D_0 is the blob's own
  if (msff_len < 56) { *why = "MSFF blob shorter than its header"; return 0; }
  u64 hd[7]; memcpy(hd, msff, 56);
  if (hd[0] != 0x4646534DULL) { *why = "MSFF: not an MSFF blob (magic)"; return 0; }
  if (hd[1] != (u64)E || hd[2] != (u64)k || hd[4] != (u64)nq || hd[3] < 1 || hd[3] > 64) { *why = "MSFF header: E, log_arity, rounds or queries are not the verifier's"; return 0; }
  const u64 D0 = hd[5], nfinal = hd[6];
  if (D0 < a || (D0 & (D0 - 1)) || D0 > L || L % D0) { *why = "MSFF header: D_0 is no power of two that divides the LDE domain and holds a coset"; return 0; }
  const u64 s = L / D0, D1 = D0 >> k;
  u64 h0 = 0; while (((u64)1 << h0) < D1) h0++;
  const size_t psize = 16 + (size_t)a * E * 8 + 64 * (size_t)h0;
  if (nfinal > D0 || (msff_len - 56) / 8 < nfinal * E) { *why = "MSFF blob truncated in the final polynomial"; return 0; }
  const u8* r0 = msff + 56 + (size_t)nfinal * E * 8;
  if ((msff_len - 56 - (size_t)nfinal * E * 8) / psize < nq) { *why = "MSFF blob truncated in round 0's openings"; return 0; }
  OpenCursor<F> lde{"LDE", digest, zae, lde_root, (size_t)a * c0, lde_open, lde_len}, stg{"staged", digest, zae, stg_root, (size_t)a * c1, stg_open, stg_len},
      val{"validity", digest, zae, val_root, (size_t)a * m, val_open, val_len};
  const T wa = f_pow<F>(lt.gL, L / a);   // the step between the coset's rows
  for (size_t j = 0; j < nq; j++) {
    const u64 q = betas[j] % D0 % D1, grp = q * s;
    const u64* lrow = lde.open(grp * a * c0, why);
    const u64* srow = lrow && c1 ? stg.open(grp * a * c1, why) : nullptr;
    if (!lrow || (c1 && !srow)) return 0;
    const u64* vrow = val.open(grp * a * m, why);
    if (!vrow) return 0;
    const u64* slots = (const u64*)(r0 + j * psize + 8);
    u64 li; memcpy(&li, r0 + j * psize, 8);
    if (li != q * a) { *why = "MSFF: a round-0 path is not at the query's leaf group"; return 0; }
    if (!V::canon(slots, (size_t)a * E)) { *why = "MSFF: opened value not canonical"; return 0; }
    T x = F::mul(lt.sh, f_pow<F>(lt.gL, grp));
    for (u64 t = 0; t < a; t++, x = F::mul(x, wa)) {   // x = shift * g_L^(q s + t L / a)
      if (!e_eq<F, E>(lt.compose_at(x, lrow, srow, vrow, a, t), V::load(slots + t * E))) { *why = "DEEP link: the composition recomputed from the opened leaf groups and the claimed evaluations is not the value in slot " + std::to_string(t) + " of round 0's coset"; return 0; }
    }
  }
  if (!lde.done(why) || (c1 && !stg.done(why)) || !val.done(why)) return 0;
  return 1;
}

}  // namespace ministark

// ---- C entry points for the Python test / bench harness ---------------------------------------
using namespace ministark;
struct msh_stark { Stark s; };
// What ms_mix_terms and ms_mix_air ask of the CSR term arrays (the stages' own limits): the most factors of any term, or -1 for a program they refuse
template <class F> static int term_program_degree(u32 ncons, const u32* tb, const u64* coef, const u32* fb) {
  if (tb[0] != 0 || fb[0] != 0) return -1;
  for (u32 t = 0; t < ncons; t++) if (tb[t + 1] < tb[t] || tb[t + 1] > 65536) return -1;
  u32 d = 0;
  for (u32 m = 0; m < tb[ncons]; m++) { if (fb[m + 1] < fb[m] || fb[m + 1] - fb[m] > 8 || coef[m] >= F::P) return -1; d = std::max(d, fb[m + 1] - fb[m]); }
  return (int)d;
}
static int slot_of(const u32* rows, int nrows, u32 row) { for (int k = 0; k < nrows; k++) if (rows[k] == row) return k; return -1; }   // the opening at w^row z; -1: not opened
template <class F> static typename F::T trace_root(u64 N) { int lg = 0; while (((u64)1 << lg) < N) lg++; return f_root_of_unity<F>(lg); }
// The verifying side of ms_mix_terms: the value validity(z) must have, from the opened values opened[k][j] = P_j(w^rows[k] z) - the same program in the extension field,
//   (sum_t r^t C_t(z)) prod_{k=1..nexempt} (z - w^(N-k)) / (z^N - 1),   C_t(z) = sum_m coef_m prod_f opened[row_f][poly_f]
template <class F, int E> static int terms_expected(u64 r, int ncons, const u32* tb, const u64* coef, const u32* fb, const u32* fp, const u32* fr, int nexempt, u64 N,
                                                    const u64* z, int nrows, const u32* rows, const u64* opened, size_t row_stride, u32 npolys, u64* out) {
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  if (r >= F::P || !V::canon(z, E) || term_program_degree<F>((u32)ncons, tb, coef, fb) < 0) return MS_ERR_ARG;   // (d = 0, which the stage refuses, evaluates here)
  const u32 nterms = tb[ncons];
  std::vector<int> slot(fb[nterms], -1);
  for (u32 f = 0; f < fb[nterms]; f++) {
    if (fp[f] >= npolys || (u64)fr[f] >= N) return MS_ERR_ARG;
    slot[f] = slot_of(rows, nrows, fr[f]);
    if (slot[f] < 0) return MS_ERR_OUT_OF_RANGE;
    if (!V::canon(opened + (size_t)slot[f] * row_stride + (size_t)fp[f] * E, E)) return MS_ERR_ARG;
  }
  const X zz = V::load(z);
  X acc = e_zero<F, E>();
  typename F::T rp = F::from_u64(1);
  for (int t = 0; t < ncons; t++) {
    X ct = e_zero<F, E>();
    for (u32 m = tb[t]; m < tb[t + 1]; m++) {
      X v = e_from_base<F, E>(F::from_u64(coef[m]));
      for (u32 f = fb[m]; f < fb[m + 1]; f++) v = e_mul<F>(v, V::load(opened + (size_t)slot[f] * row_stride + (size_t)fp[f] * E));
      ct = e_add<F, E>(ct, v);
    }
    acc = e_add<F, E>(acc, e_mul_base<F, E>(ct, rp));
    rp = F::mul(rp, F::from_u64(r));
  }
  const typename F::T wi = f_inv<F>(trace_root<F>(N));
  typename F::T wk = wi;                                                // w^(N-k) = w^-k
  for (int k = 0; k < nexempt; k++) { acc = e_mul<F>(acc, e_sub<F, E>(zz, e_from_base<F, E>(wk))); wk = F::mul(wk, wi); }
  const X den = e_sub<F, E>(e_pow<F, E>(zz, N), e_one<F, E>());
  if (e_is_zero<F, E>(den)) return MS_ERR_SHAPE;                       // z lies in the trace domain
  acc = e_mul<F>(acc, e_inv<F>(den));
  for (int l = 0; l < E; l++) out[l] = F::to_u64(acc.c[l]);
  return MS_OK;
}
// The verifying side of ms_mix_air: the same program in the extension field from the opened values, the periodic columns evaluated here, the boundary quotients
// from the row-0 opening:  sum_t r^t C_t(z) Z_t(z) / (z^N - 1)  +  sum_b r^(ncons+b) (opened[row 0][j_b] - v_b) / (z - w^rho_b)
// r: E limbs, the powers taken in the extension (ms_mix_air_ext); ms_mix_air's base-field r is (r, 0, ..)
template <class F, int E> static int air_expected(const u64* r, const ms_air& a, u64 N, const u64* z, int nrows, const u32* rows, const u64* opened, size_t row_stride, u32 npolys, u64* out) {
  typedef Ext<F, E> X;
  typedef Verifier<F, E> V;
  typedef typename F::T T;
  const u32 ncons = a.ncons;
  if (!V::canon(r, E) || !V::canon(z, E) || term_program_degree<F>(ncons, a.term_begin, a.coef, a.fac_begin) <= 0 || a.ex_begin[0] != 0) return MS_ERR_ARG;   // (d = 0 too)
  for (u32 t = 0; t < ncons; t++) if (a.ex_begin[t + 1] < a.ex_begin[t] || a.ex_begin[t + 1] - a.ex_begin[t] > 16) return MS_ERR_ARG;
  const u32 nterms = a.term_begin[ncons];
  if (a.ex_begin[ncons] && !a.ex_row) return MS_ERR_ARG;
  const T wN = trace_root<F>(N), wi = f_inv<F>(wN), one = F::from_u64(1);
  // periodic columns: Q_k by the inverse DFT of the q_k values
  std::vector<std::vector<T>> Q(a.nperiodic);
  if (a.nperiodic && a.per_begin[0] != 0) return MS_ERR_ARG;
  for (u32 k = 0; k < a.nperiodic; k++) {
    if (a.per_begin[k + 1] <= a.per_begin[k] || a.per_begin[k + 1] > 4096) return MS_ERR_ARG;
    const u64 q = a.per_begin[k + 1] - a.per_begin[k];
    if ((q & (q - 1)) || q > N || q > 256 || !V::canon(a.per_val + a.per_begin[k], q)) return MS_ERR_ARG;
    const u64* val = a.per_val + a.per_begin[k];
    const T eta_inv = f_pow<F>(wi, N / q), qinv = f_inv<F>(F::from_u64(q));
    Q[k].resize(q);
    T em = one;
    for (u64 m = 0; m < q; m++) { T s = 0, e = one; for (u64 i = 0; i < q; i++) { s = F::add(s, F::mul(F::from_u64(val[i]), e)); e = F::mul(e, em); } Q[k][m] = F::mul(s, qinv); em = F::mul(em, eta_inv); }
  }
  { std::vector<std::vector<u32>> sets;            // the stage's limits on the exemption sets
    for (u32 t = 0; t < ncons; t++) {
      std::vector<u32> s(a.ex_row ? a.ex_row + a.ex_begin[t] : nullptr, a.ex_row ? a.ex_row + a.ex_begin[t + 1] : nullptr);
      std::sort(s.begin(), s.end());
      for (size_t k = 0; k < s.size(); k++) if ((u64)s[k] >= N || (k && s[k] == s[k - 1])) return MS_ERR_ARG;
      if (std::find(sets.begin(), sets.end(), s) == sets.end()) { if (sets.size() == 32) return MS_ERR_ARG; sets.push_back(s); }
    }
    std::vector<u32> brows;
    for (u32 b = 0; b < a.nbound; b++) {
      if (a.bnd_poly[b] >= npolys || (u64)a.bnd_row[b] >= N || a.bnd_val[b] >= F::P) return MS_ERR_ARG;
      if (std::find(brows.begin(), brows.end(), a.bnd_row[b]) == brows.end()) { if (brows.size() == 16) return MS_ERR_ARG; brows.push_back(a.bnd_row[b]); }
    } }
  const u32 nfacs = a.fac_begin[nterms];
  for (u32 f = 0; f < nfacs; f++) {
    const u32 fp = a.fac_poly[f];
    if ((fp & MS_AIR_PERIODIC) ? (fp & ~MS_AIR_PERIODIC) >= a.nperiodic : fp >= npolys) return MS_ERR_ARG;
    if ((u64)a.fac_row[f] >= N) return MS_ERR_ARG;
  }
  std::vector<int> slot(nfacs, -1);
  for (u32 f = 0; f < nfacs; f++) {
    if (a.fac_poly[f] & MS_AIR_PERIODIC) continue;   // (a periodic factor needs no opening)
    slot[f] = slot_of(rows, nrows, a.fac_row[f]);
    if (slot[f] < 0) return MS_ERR_OUT_OF_RANGE;
    if (!V::canon(opened + (size_t)slot[f] * row_stride + (size_t)a.fac_poly[f] * E, E)) return MS_ERR_ARG;
  }
  const int slot0 = a.nbound ? slot_of(rows, nrows, 0) : 0;
  if (slot0 < 0) return MS_ERR_OUT_OF_RANGE;                           // the boundary quotients are evaluated from P_j(z)
  for (u32 b = 0; b < a.nbound; b++) if (!V::canon(opened + (size_t)slot0 * row_stride + (size_t)a.bnd_poly[b] * E, E)) return MS_ERR_ARG;
  const X zz = V::load(z);
  const X den = e_sub<F, E>(e_pow<F, E>(zz, N), e_one<F, E>());
  if (e_is_zero<F, E>(den)) return MS_ERR_SHAPE;                       // z lies in the trace domain
  X acc = e_zero<F, E>();
  const X rr = V::load(r);
  X rp = e_one<F, E>();
  for (u32 t = 0; t < ncons; t++) {
    X ct = e_zero<F, E>();
    for (u32 m = a.term_begin[t]; m < a.term_begin[t + 1]; m++) {
      X v = e_from_base<F, E>(F::from_u64(a.coef[m]));
      for (u32 f = a.fac_begin[m]; f < a.fac_begin[m + 1]; f++) {
        if (a.fac_poly[f] & MS_AIR_PERIODIC) {                           // K_k(w^row z) = Q_k((w^row z)^(N/q))
          const std::vector<T>& q = Q[a.fac_poly[f] & ~MS_AIR_PERIODIC];
          const u64 step = N / q.size();
          const X y = e_mul_base<F, E>(e_pow<F, E>(zz, step), f_pow<F>(wN, (u64)a.fac_row[f] * step % N));
          X kv = e_zero<F, E>();
          for (size_t i = q.size(); i-- > 0;) kv = e_add<F, E>(e_mul<F>(kv, y), e_from_base<F, E>(q[i]));
          v = e_mul<F>(v, kv);
        } else v = e_mul<F>(v, V::load(opened + (size_t)slot[f] * row_stride + (size_t)a.fac_poly[f] * E));
      }
      ct = e_add<F, E>(ct, v);
    }
    for (u32 k = a.ex_begin[t]; k < a.ex_begin[t + 1]; k++) ct = e_mul<F>(ct, e_sub<F, E>(zz, e_from_base<F, E>(f_pow<F>(wN, (u64)a.ex_row[k]))));
    acc = e_add<F, E>(acc, e_mul<F>(ct, rp));
    rp = e_mul<F>(rp, rr);
  }
  acc = e_mul<F>(acc, e_inv<F>(den));
  for (u32 b = 0; b < a.nbound; b++) {
    const X num = e_sub<F, E>(V::load(opened + (size_t)slot0 * row_stride + (size_t)a.bnd_poly[b] * E), e_from_base<F, E>(F::from_u64(a.bnd_val[b])));
    const X dn = e_sub<F, E>(zz, e_from_base<F, E>(f_pow<F>(wN, (u64)a.bnd_row[b])));   // (non-zero: z^N != 1)
    acc = e_add<F, E>(acc, e_mul<F>(e_mul<F>(num, e_inv<F>(dn)), rp));
    rp = e_mul<F>(rp, rr);
  }
  for (int l = 0; l < E; l++) out[l] = F::to_u64(acc.c[l]);
  return MS_OK;
}

// ---- linked proofs, MSLP v1, v2 and v3 (ministark_host.h): the program's encoding, the redraw rules, the shape a statement fixes ------------------------------------
// The shape of an ms_air: every array that is needed is there, the CSR offsets start at 0 and do not decrease, the stages' own limits hold.  The counts the encoding carries
struct AirShape { u32 ncons, nterms, nfacs, nex, nperiodic, nperval, nbound; };
static bool air_shape(const ms_air* a, AirShape* s) {
  if (!a || a->ncons < 1 || a->ncons > 4096 || a->nperiodic > 64 || a->nbound > 4096 || !a->term_begin || !a->coef || !a->fac_begin || !a->ex_begin) return false;
  if (a->term_begin[0] != 0 || a->fac_begin[0] != 0 || a->ex_begin[0] != 0) return false;
  for (u32 t = 0; t < a->ncons; t++) {
    if (a->term_begin[t + 1] < a->term_begin[t] || a->term_begin[t + 1] > 65536) return false;
    if (a->ex_begin[t + 1] < a->ex_begin[t] || a->ex_begin[t + 1] - a->ex_begin[t] > 16) return false;
  }
  const u32 nterms = a->term_begin[a->ncons];
  for (u32 m = 0; m < nterms; m++) if (a->fac_begin[m + 1] < a->fac_begin[m] || a->fac_begin[m + 1] - a->fac_begin[m] > 8) return false;
  const u32 nfacs = a->fac_begin[nterms], nex = a->ex_begin[a->ncons];
  if ((nfacs && (!a->fac_poly || !a->fac_row)) || (nex && !a->ex_row)) return false;
  u32 nperval = 0;
  if (a->nperiodic) {
    if (!a->per_begin || !a->per_val || a->per_begin[0] != 0) return false;
    for (u32 k = 0; k < a->nperiodic; k++) if (a->per_begin[k + 1] <= a->per_begin[k] || a->per_begin[k + 1] > 4096) return false;
    nperval = a->per_begin[a->nperiodic];
  }
  if (a->nbound && (!a->bnd_poly || !a->bnd_row || !a->bnd_val)) return false;
  *s = AirShape{a->ncons, nterms, nfacs, nex, a->nperiodic, nperval, a->nbound};
  return true;
}
// msh_air_encode: 'MSAR' | version 1 | ncons nterms nfacs nexempt nperiodic nperval nbound array_bytes (u32 each), then the arrays in the order of the struct
static const u32 AIR_MAGIC = 0x5241534Du;   // 'MSAR'
static bool air_encode(const ms_air* a, std::vector<u8>* out) {
  AirShape sh;
  if (!air_shape(a, &sh)) return false;
  out->clear();
  auto put = [&](const void* src, size_t n) { const u8* b = (const u8*)src; out->insert(out->end(), b, b + n); };   // little-endian host
  const u32 zero = 0;
  const size_t arrays = 4 * ((size_t)sh.ncons + 1) * 2 + 8 * (size_t)sh.nterms + 4 * ((size_t)sh.nterms + 1) + 8 * (size_t)sh.nfacs + 4 * (size_t)sh.nex + 4 * ((size_t)sh.nperiodic + 1) +
                        8 * (size_t)sh.nperval + 16 * (size_t)sh.nbound;
  const u32 head[10] = {AIR_MAGIC, 1, sh.ncons, sh.nterms, sh.nfacs, sh.nex, sh.nperiodic, sh.nperval, sh.nbound, (u32)arrays};
  put(head, sizeof head);
  put(a->term_begin, 4 * ((size_t)sh.ncons + 1)); put(a->coef, 8 * (size_t)sh.nterms); put(a->fac_begin, 4 * ((size_t)sh.nterms + 1));
  put(a->fac_poly, 4 * (size_t)sh.nfacs); put(a->fac_row, 4 * (size_t)sh.nfacs);
  put(a->ex_begin, 4 * ((size_t)sh.ncons + 1)); put(a->ex_row, 4 * (size_t)sh.nex);
  if (sh.nperiodic) { put(a->per_begin, 4 * ((size_t)sh.nperiodic + 1)); put(a->per_val, 8 * (size_t)sh.nperval); } else put(&zero, 4);
  put(a->bnd_poly, 4 * (size_t)sh.nbound); put(a->bnd_row, 4 * (size_t)sh.nbound); put(a->bnd_val, 8 * (size_t)sh.nbound);
  return out->size() == sizeof head + arrays;
}
// msh_air_rows: the row offsets of the program's factors, and row 0 when there are boundary constraints, ascending (mini_stark_amd.air_rows)
static bool air_rows(const ms_air* a, std::vector<u32>* rows) {
  AirShape sh;
  if (!air_shape(a, &sh)) return false;
  rows->assign(a->fac_row, a->fac_row + sh.nfacs);
  if (sh.nbound) rows->push_back(0);
  std::sort(rows->begin(), rows->end());
  rows->erase(std::unique(rows->begin(), rows->end()), rows->end());
  return true;
}
// the redraw rules of the linked transcript (ministark_host.h: msh_linked_shift_ok, msh_linked_z_ok)
template <class F> static bool linked_shift_ok(u64 shift, u64 L) { return shift != 0 && shift < F::P && F::to_u64(f_pow<F>(F::from_u64(shift), L)) != 1; }
static bool linked_z_ok(const u64* z, int e) { for (int l = 1; l < e; l++) if (z[l]) return true; return false; }
template <class F> static u64 draw_shift(Transcript& t, u64 L) { u64 s; do t.challenge_scalars(&s, 1, F::P); while (!linked_shift_ok<F>(s, L)); return s; }
static void draw_z(Transcript& t, u64* z, int e, u64 p) { do t.challenge_scalars(z, e, p); while (!linked_z_ok(z, e)); }

// What prover and verifier derive from the configuration, the AIR, the arguments, N, w and the rounds alone: the statement they absorb and every count of the MSLP header
struct LinkedShape {
  u32 c = 0, m = 0, npts = 0, R = 0, nq = 0, gb = 0; u64 N = 0, blowup = 0, L = 0;
  std::vector<u32> rows;          // the points are z * w^rows[t]; row 0 first
  std::vector<u32> pt_begin, pt_poly; size_t ne = 0;   // every point opens the c columns, the point of row 0 the m chunk columns too
  std::vector<u8> statement; size_t words_bytes = 0, air_bytes = 0;   // the statement's words | msh_air_encode(air) | msh_aux_encode(args), when there are arguments
};
// what the program fixes, for c columns: m, the points and what they open (o->c, o->N set by the caller)
static int linked_program_shape(const ms_air* air, const AirShape& sh, int e, LinkedShape* o) {
  const u64 N = o->N;
  // m = E * VL / N, VL by ms_mix_air's rule (ministark.h): nq = max(max_t (d_t (N - 1) + e_t - N + 1), N - 1 if nbound > 0, 1), VL = N * next_pow2(ceil(nq / N))
  u64 nqv = sh.nbound ? N - 1 : 1;
  if (nqv < 1) nqv = 1;
  for (u32 t = 0; t < sh.ncons; t++) {
    u64 d = 0;
    for (u32 k = air->term_begin[t]; k < air->term_begin[t + 1]; k++) d = std::max<u64>(d, air->fac_begin[k + 1] - air->fac_begin[k]);
    const u64 et = air->ex_begin[t + 1] - air->ex_begin[t], deg = d * (N - 1) + et;
    if (air->term_begin[t + 1] > air->term_begin[t] && deg + 1 > N && deg - N + 1 > nqv) nqv = deg - N + 1;
  }
  u64 slots = 1; while (slots * N < nqv) slots *= 2;
  o->m = (u32)(slots * e);
  if (!air_rows(air, &o->rows)) return MS_ERR_ARG;
  if (o->rows.empty() || o->rows[0] != 0) o->rows.insert(o->rows.begin(), 0);
  for (u32 r : o->rows) if (r >= N) return MS_ERR_ARG;
  if (o->rows.size() > 8) return MS_ERR_ARG;   // ms_deep_compose takes at most 8 points
  o->npts = (u32)o->rows.size();
  o->pt_begin.assign(1, 0); o->pt_poly.clear();
  for (u32 t = 0; t < o->npts; t++) {
    for (u32 j = 0; j < o->c + (t == 0 ? o->m : 0); j++) o->pt_poly.push_back(j);
    o->pt_begin.push_back((u32)o->pt_poly.size());
  }
  o->ne = o->pt_poly.size();
  if (o->ne > 8192) return MS_ERR_ARG;
  return MS_OK;
}
// what the configuration fixes: field sizes, queries, grinding bits
template <class F> static int linked_config_shape(const StarkConfig& c, size_t N, size_t w, LinkedShape* o) {
  if (N < 2 || (N & (N - 1)) || w < 1 || w > (1u << 16) || !c.blowup_factor || (c.blowup_factor & (c.blowup_factor - 1))) return MS_ERR_ARG;
  if (N > ((u64)1 << F::TWO_ADICITY) / c.blowup_factor) return MS_ERR_ARG;
  o->N = N; o->blowup = c.blowup_factor; o->L = N * c.blowup_factor; o->gb = c.grinding_bits; o->nq = (u32)c.fri_queries;
  return o->nq < 1 || o->nq > 4096 ? MS_ERR_ARG : MS_OK;
}
// z * w^row for every point, E limbs each (an element of K times a base-field scalar: limb by limb)
template <class F> static std::vector<u64> linked_points(const LinkedShape& sh, const u64* z, int e) {
  const typename F::T w = trace_root<F>(sh.N);
  std::vector<u64> pts((size_t)sh.npts * e);
  for (u32 t = 0; t < sh.npts; t++) {
    const typename F::T s = f_pow<F>(w, (u64)sh.rows[t]);
    for (int l = 0; l < e; l++) pts[(size_t)t * e + l] = F::to_u64(F::mul(F::from_u64(z[l]), s));
  }
  return pts;
}
// ---- the running columns of linked proofs (MSLP v2, v3; ministark_host.h): the arguments' encoding, their instances, the combined program ---------------------------
// msh_aux_arg: what ms_aux_running's limits and the selectors ask of a descriptor; nterms out
static bool aux_arg_shape(const msh_aux_arg& a, u32 nch, u64 p, u32* nterms_out) {
  if (a.op > 1 || a.nfrac < 1 || a.nfrac > 4 || !a.form_begin || !a.form_const || !a.form_ch || a.form_begin[0] != 0) return false;
  const u32 nforms = 2 * a.nfrac;
  for (u32 f = 0; f < nforms; f++) if (a.form_begin[f + 1] < a.form_begin[f] || a.form_begin[f + 1] - a.form_begin[f] > 16) return false;
  const u32 nterms = a.form_begin[nforms];
  if (nterms && (!a.term_col || !a.term_coef || !a.term_ch)) return false;
  for (u32 m = 0; m < nterms; m++) if (a.term_ch[m] > nch || a.term_coef[m] >= p) return false;
  for (u32 f = 0; f < nforms; f++) if (a.form_ch[f] > nch || a.form_const[f] >= p) return false;
  *nterms_out = nterms;
  return true;
}
static const u32 AUX_MAGIC = 0x5841534Du;   // 'MSAX'
// msh_aux_encode: 'MSAX' | version 1 | nargs | nch, then per argument op, nfrac, nterms | form_begin | term_col | term_ch | form_ch | term_coef | form_const.  w: the
// columns a term may name (0: not checked)
static bool aux_encode(const msh_aux_arg* args, u32 nargs, u32 nch, u64 p, int e, u64 w, std::vector<u8>* out) {
  if (!args || nargs < 1 || nch < 1 || nch > 8 || (u64)nargs * e > 16) return false;
  out->clear();
  auto put = [&](const void* src, size_t n) { const u8* b = (const u8*)src; out->insert(out->end(), b, b + n); };
  const u32 head[4] = {AUX_MAGIC, 1, nargs, nch};
  put(head, sizeof head);
  for (u32 k = 0; k < nargs; k++) {
    const msh_aux_arg& a = args[k];
    u32 nterms;
    if (!aux_arg_shape(a, nch, p, &nterms)) return false;
    if (w) for (u32 m = 0; m < nterms; m++) if (a.term_col[m] >= w) return false;
    const u32 nforms = 2 * a.nfrac, h3[3] = {a.op, a.nfrac, nterms};
    put(h3, sizeof h3);
    put(a.form_begin, 4 * ((size_t)nforms + 1)); put(a.term_col, 4 * (size_t)nterms); put(a.term_ch, 4 * (size_t)nterms); put(a.form_ch, 4 * (size_t)nforms);
    put(a.term_coef, 8 * (size_t)nterms); put(a.form_const, 8 * (size_t)nforms);
  }
  return true;
}
// a descriptor with the drawn challenges in place: the ms_aux of ms_aux_running_staged (ext = E).  A selector k > 0 multiplies the base-field value by ch[k - 1]
struct AuxInstance { std::vector<u64> term_coef, form_const; ms_aux aux; };
template <class F> static void aux_instantiate(const msh_aux_arg& a, const u64* ch, int e, AuxInstance* o) {
  const u32 nforms = 2 * a.nfrac, nterms = a.form_begin[nforms];
  auto value = [&](u64 base, u32 sel, u64* dst) {
    for (int l = 0; l < e; l++) dst[l] = sel ? F::to_u64(F::mul(F::from_u64(base), F::from_u64(ch[(size_t)(sel - 1) * e + l]))) : (l == 0 ? base : 0);
  };
  o->term_coef.assign((size_t)nterms * e, 0); o->form_const.assign((size_t)nforms * e, 0);
  for (u32 m = 0; m < nterms; m++) value(a.term_coef[m], a.term_ch[m], o->term_coef.data() + (size_t)m * e);
  for (u32 f = 0; f < nforms; f++) value(a.form_const[f], a.form_ch[f], o->form_const.data() + (size_t)f * e);
  o->aux = ms_aux{a.op, (u32)e, a.nfrac, a.form_begin, a.term_col, o->term_coef.data(), o->form_const.data()};
}
// a growable copy of an ms_air program
struct AirProg {
  std::vector<u32> tb{0}, fb{0}, fp, fr, eb{0}, er, pb{0}, bp, br;
  std::vector<u64> coef, pv, bv;
  ms_air air{};
  bool load(const ms_air* a) {
    AirShape sh;
    if (!air_shape(a, &sh)) return false;
    tb.assign(a->term_begin, a->term_begin + sh.ncons + 1); coef.assign(a->coef, a->coef + sh.nterms); fb.assign(a->fac_begin, a->fac_begin + sh.nterms + 1);
    fp.assign(a->fac_poly, a->fac_poly + sh.nfacs); fr.assign(a->fac_row, a->fac_row + sh.nfacs);
    eb.assign(a->ex_begin, a->ex_begin + sh.ncons + 1); er.assign(a->ex_row, a->ex_row + sh.nex);
    if (sh.nperiodic) { pb.assign(a->per_begin, a->per_begin + sh.nperiodic + 1); pv.assign(a->per_val, a->per_val + sh.nperval); }
    bp.assign(a->bnd_poly, a->bnd_poly + sh.nbound); br.assign(a->bnd_row, a->bnd_row + sh.nbound); bv.assign(a->bnd_val, a->bnd_val + sh.nbound);
    return true;
  }
  const ms_air* view() {
    air.ncons = (u32)tb.size() - 1; air.term_begin = tb.data(); air.coef = coef.data(); air.fac_begin = fb.data(); air.fac_poly = fp.data(); air.fac_row = fr.data();
    air.ex_begin = eb.data(); air.ex_row = er.data(); air.nperiodic = (u32)pb.size() - 1; air.per_begin = pb.data(); air.per_val = pv.data();
    air.nbound = (u32)bp.size(); air.bnd_poly = bp.data(); air.bnd_row = br.data(); air.bnd_val = bv.data();
    return &air;
  }
};
// msh_aux_constraints: mini_stark_amd.aux_constraints in C++ - the transition constraint cleared of denominators as a polynomial in the (polynomial, row) variables
// with coefficients in K (monomial: its sorted factors), one base-field constraint per limb, terms in the monomials' order; no exemption; z(w^0) = identity
template <class F, int E> static int aux_constraints(AirProg& pg, const ms_aux& a, u32 first_poly) {
  typedef Ext<F, E> X;
  typedef std::vector<std::pair<u32, u32>> Mono;
  typedef std::map<Mono, X> Poly;
  if (a.ext != (u32)E || a.op > 1 || a.nfrac < 1 || a.nfrac > 4) return MS_ERR_ARG;
  bool over = false;
  auto padd = [&](Poly& acc, const Poly& b, bool minus) { for (auto& kv : b) { auto it = acc.find(kv.first); const X v = it == acc.end() ? e_zero<F, E>() : it->second; acc[kv.first] = minus ? e_sub<F, E>(v, kv.second) : e_add<F, E>(v, kv.second); } };
  auto pmul = [&](const Poly& x, const Poly& y) {
    Poly out;
    for (auto& ka : x) {
      for (auto& kb : y) {
        Mono mo(ka.first); mo.insert(mo.end(), kb.first.begin(), kb.first.end());
        std::sort(mo.begin(), mo.end());
        if (mo.size() > 8) { over = true; return out; }
        const X c = e_mul<F>(ka.second, kb.second);
        auto it = out.find(mo);
        if (it == out.end()) out[mo] = c; else it->second = e_add<F, E>(it->second, c);
      }
      if (out.size() * E > 65536) { over = true; return out; }
    }
    return out;
  };
  auto load = [&](const u64* v) { X x; for (int l = 0; l < E; l++) x.c[l] = F::from_u64(v[l]); return x; };
  auto form = [&](u32 f) {
    Poly out; out[Mono()] = load(a.form_const + (size_t)f * E);
    for (u32 m = a.form_begin[f]; m < a.form_begin[f + 1]; m++) { Poly t; t[Mono{{a.term_col[m], 0}}] = load(a.term_coef + (size_t)m * E); padd(out, t, false); }
    return out;
  };
  auto unit = [&](int l) { X x = e_zero<F, E>(); x.c[l] = F::from_u64(1); return x; };
  Poly z, zn, one; one[Mono()] = unit(0);
  for (int l = 0; l < E; l++) { z[Mono{{first_poly + l, 0}}] = unit(l); zn[Mono{{first_poly + l, 1}}] = unit(l); }
  std::vector<Poly> nums, dens;
  for (u32 k = 0; k < a.nfrac; k++) { nums.push_back(form(2 * k)); dens.push_back(form(2 * k + 1)); }
  Poly den_all = one, expr;
  for (auto& d : dens) den_all = pmul(den_all, d);
  if (a.op == MS_AUX_PRODUCT) {
    Poly num_all = one;
    for (auto& n : nums) num_all = pmul(num_all, n);
    expr = pmul(zn, den_all);
    padd(expr, pmul(z, num_all), true);
  } else {
    Poly dz = zn; padd(dz, z, true);
    expr = pmul(dz, den_all);
    for (u32 k = 0; k < a.nfrac; k++) {
      Poly t = nums[k];
      for (u32 j = 0; j < a.nfrac; j++) if (j != k) t = pmul(t, dens[j]);
      padd(expr, t, true);
    }
  }
  if (over) return MS_ERR_ARG;
  size_t total = pg.coef.size();
  for (int l = 0; l < E; l++) {
    bool any_factor = false; size_t n = 0;
    for (auto& kv : expr) if (kv.second.c[l] != 0) { n++; any_factor = any_factor || !kv.first.empty(); }
    if (!any_factor) return MS_ERR_ARG;
    total += n;
  }
  if (total > 65536 || pg.tb.size() - 1 + E > 4096 || pg.bp.size() + E > 4096) return MS_ERR_ARG;
  for (int l = 0; l < E; l++) {
    for (auto& kv : expr) if (kv.second.c[l] != 0) {
      pg.coef.push_back(F::to_u64(kv.second.c[l]));
      for (auto& fc : kv.first) { pg.fp.push_back(fc.first); pg.fr.push_back(fc.second); }
      pg.fb.push_back((u32)pg.fp.size());
    }
    pg.tb.push_back((u32)pg.coef.size());
    pg.eb.push_back((u32)pg.er.size());
  }
  for (int l = 0; l < E; l++) { pg.bp.push_back(first_poly + l); pg.br.push_back(0); pg.bv.push_back((a.op == MS_AUX_PRODUCT && l == 0) ? 1 : 0); }
  return MS_OK;
}
// the combined program - air plus msh_aux_constraints of every instantiated argument, argument k at first_poly = w + k E - and the shape it fixes
template <class F, int E> static int linked_combined(const ms_air* air, const msh_aux_arg* args, u32 nargs, const u64* ch, size_t w, AirProg* pg, std::vector<AuxInstance>* inst, LinkedShape* o) {
  if (!pg->load(air)) return MS_ERR_ARG;
  inst->resize(nargs);
  for (u32 k = 0; k < nargs; k++) {
    aux_instantiate<F>(args[k], ch, E, &(*inst)[k]);
    const int rc = aux_constraints<F, E>(*pg, (*inst)[k].aux, (u32)w + k * E);
    if (rc) return rc;
  }
  AirShape sh;
  if (!air_shape(pg->view(), &sh)) return MS_ERR_ARG;
  return linked_program_shape(pg->view(), sh, E, o);
}

// ---- the one prover driver and the one verifier of linked proofs: MSLP v1, v2 and v3 (ministark_host.h) ------------------------------------------------------------
// The kind of a linked proof.  Everything in which the versions differ follows from these fields, at the places this table names; the rest is shared:
//   point                          v1                          v2                              v3
//   domain separator suffix        /linked/v1                  /linked/v2                      /linked/v3
//   statement words                8                           10 (+ nargs, nch)               11 (+ k in front of R)
//   aux encoding absorbed          no                          always                          when nargs > 0
//   program shape fixed            before any device call      after the challenge draw        after the LDE root (challenges drawn when nargs > 0)
//   LDE / staged / validity root   plain                       plain, staged root always       the _coset calls, staged root when nargs > 0
//   FRI commit phase               ms_fri_begin, R - 1 x (z, B, alpha, root)       (as v1)     ms_fri_begin_folded, R - 1 x (alpha, root), alpha, final polynomial
//   query call / blob              ms_query_linked, MSLQ (3)   ms_query_linked, MSLS (4)       ms_query_linked_folded, MSLF (4 sections)
//   header                         9 x u32 + 4 x u64           12 x u32 + 4 x u64              13 x u32 + 5 x u64 (D_0)
//   arthur length                  plain FRI, three roots      + 32 (the staged root)          folded FRI, + 32 when nargs > 0
// (v2 has at least one argument - msh_aux_encode refuses none -, so "when nargs > 0" is v2's "always" and v1's "never")
struct LinkedKind {
  u32 version;                              // 1, 2 or 3
  int k;                                    // log_arity of the folded FRI (v3); 0: the plain FRI
  const msh_aux_arg* args; u32 nargs, nch;  // the arguments of the running columns and the challenges their selectors name
  u32 rounds;                               // fri_rounds (plain) or fri_folds (folded); 0: the configuration's rounds, or floor(log2 N / k)
};
// what the verifier words per version: the header's and the query blob's name, its magic and sections, the two refusals of malformed arguments
struct LinkedText { const char* head; const char* blob; u64 magic; int nsec; const char* bad_args; const char* bad_program; };
static const LinkedText LINKED_TEXT[3] = {
    {"MSLP", "MSLQ", 0x514C534DULL, 3, "malformed arguments: the AIR program, N, w, the rounds or the configuration", ""},
    {"MSLP v2", "MSLS", 0x534C534DULL, 4, "malformed arguments: the AIR program, the arguments, N, w, the rounds or the configuration",
     "malformed arguments: the combined program exceeds ms_mix_air's limits"},
    {"MSLP v3", "MSLF", 0x464C534DULL, 4, "malformed arguments: the AIR program, the arguments, N, w, log_arity, the folds or the configuration",
     "malformed arguments: the program exceeds ms_mix_air's limits"}};

// the statement and what the configuration fixes; the program's part of the shape is linked_combined's (v1: at once; v2, v3: once the challenges are drawn)
template <class F> static int linked_shape(const StarkConfig& c, const ms_air* air, size_t N, size_t w, const LinkedKind& kd, LinkedShape* o) {
  AirShape sh;
  if ((kd.version == 3 && (kd.k < 1 || kd.k > 3)) || !air_shape(air, &sh) || linked_config_shape<F>(c, N, w, o)) return MS_ERR_ARG;
  if ((kd.nargs == 0) != (kd.args == nullptr) || (kd.nargs == 0 && kd.nch != 0)) return MS_ERR_ARG;
  int lgN = 0; while (((u64)1 << lgN) < N) lgN++;
  o->R = kd.rounds ? kd.rounds : kd.k ? (u32)(lgN / kd.k) : (u32)c.rounds;
  if (o->R < 1 || o->R > 64 || (kd.k && o->L < ((u64)2 << kd.k))) return MS_ERR_ARG;
  if (kd.version > 1)   // the main program is over the w trace columns (v1 leaves a column at or above w to the mix stage and to the evaluation at z)
    for (u32 j = 0; j < sh.nfacs; j++) if (!(air->fac_poly[j] & 0x80000000u) && air->fac_poly[j] >= w) return MS_ERR_ARG;
  std::vector<u64> words = {(u64)c.field, (u64)c.digest, (u64)N, (u64)w, c.blowup_factor};
  if (kd.k) words.push_back((u64)kd.k);
  words.insert(words.end(), {(u64)o->R, (u64)o->nq, (u64)o->gb});
  if (kd.version > 1) words.insert(words.end(), {(u64)kd.nargs, (u64)kd.nch});
  std::vector<u8> enc, enx;
  if (!air_encode(air, &enc) || ((kd.version == 2 || kd.nargs) && !aux_encode(kd.args, kd.nargs, kd.nch, c.p, c.e, w, &enx))) return MS_ERR_ARG;
  o->words_bytes = 8 * words.size(); o->air_bytes = enc.size();
  o->statement.assign((const u8*)words.data(), (const u8*)words.data() + o->words_bytes);
  o->statement.insert(o->statement.end(), enc.begin(), enc.end());
  o->statement.insert(o->statement.end(), enx.begin(), enx.end());
  o->c = (u32)w + kd.nargs * (u32)c.e;
  return MS_OK;
}
static Transcript linked_transcript(const StarkConfig& c, const LinkedShape& sh, const LinkedKind& kd) {
  Transcript t(c.domsep + "/linked/v" + std::to_string(kd.version), c.digest);
  const u8* s = sh.statement.data(); const size_t aux_at = sh.words_bytes + sh.air_bytes;
  t.add_bytes(s, sh.words_bytes);                                            // field, digest, N, w, blowup, (k,) R, nq, grinding bits (, nargs, nch)
  t.add_bytes(s + sh.words_bytes, sh.air_bytes);                             // msh_air_encode(air)
  if (sh.statement.size() > aux_at) t.add_bytes(s + aux_at, sh.statement.size() - aux_at);   // msh_aux_encode(args), where it is part of the statement
  t.prover_bytes.clear();                                                    // the statement is the verifier's own: it does not travel
  return t;
}
// plain: trace, LDE, (staged,) validity root, evaluations, round 0's root, R - 1 x (B, root), nonce; folded: .. evaluations, R round roots, final polynomial, nonce
static size_t linked_arthur_len(const LinkedShape& sh, const LinkedKind& kd, int e, u64 nfinal) {
  const size_t fri = kd.k ? (size_t)sh.R * 32 + (size_t)nfinal * e * 8 : 32 + (size_t)(sh.R - 1) * (2 * e * 8 + 32);
  return (size_t)(3 + (kd.nargs ? 1 : 0)) * 32 + sh.ne * e * 8 + fri + (sh.gb ? 8 : 0);
}
// The u32 words of a version's MSLP header, by name; behind them N, blowup, (D_0,) len(arthur), len(blob) as u64.  The prover writes the header from this table, the
// verifier compares against it.  late: fixed by the program, which v2 and v3 know only once the challenges are drawn
static const u32 MSLP_MAGIC = 0x504C534Du;   // 'MSLP'
struct HeadWord { const char* name; u32 v; bool late; };
template <int E> static std::vector<HeadWord> linked_header(const LinkedShape& sh, const LinkedKind& kd, size_t w) {
  const bool late = kd.version > 1;
  std::vector<HeadWord> h = {{"magic", MSLP_MAGIC, false}, {"version", kd.version, false}, {"E", (u32)E, false}};
  if (kd.k) h.push_back({"log_arity", (u32)kd.k, false});
  if (kd.version == 1) h.push_back({"c", sh.c, false});
  else h.insert(h.end(), {{"c0", (u32)w, false}, {"c1", kd.nargs * (u32)E, false}});
  h.insert(h.end(), {{"m", sh.m, late}, {"npts", sh.npts, late}, {"R", sh.R, false}, {"nq", sh.nq, false}, {"grinding bits", sh.gb, false}});
  if (kd.version > 1) h.insert(h.end(), {{"nargs", kd.nargs, false}, {"nch", kd.nch, false}});
  return h;
}
static size_t linked_head_bytes(const std::vector<HeadWord>& h, const LinkedKind& kd) { return 4 * h.size() + 8 * (size_t)(kd.k ? 5 : 4); }
// the proof's u32 words against the verifier's own: the rows the statement fixes (late = false), or those the program fixes
static bool linked_header_ok(const std::vector<HeadWord>& h, const u8* data, bool late, std::string* why) {
  for (size_t j = 0; j < h.size(); j++) {
    u32 got; memcpy(&got, data + 4 * j, 4);
    if (h[j].late != late || got == h[j].v) continue;
    if (j == 1 && h[1].v > 1) *why = "header: version is not " + std::to_string(h[1].v);   // (v1 words it like the other rows; both texts are pinned by callers)
    else *why = std::string("header: ") + h[j].name + " is not the verifier's";
    return false;
  }
  return true;
}

// the prover's driver: transcript order and redraw rules of ministark_host.h; it branches at the rows of the table above and nowhere else
template <class F, int E> static int prove_linked(Stark& s, const u64* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const LinkedKind& kd) {
  const StarkConfig& c = s.cfg; ms_ctx* ctx = c.ctx; const int e = E; const u64 p = c.p;
  s.linked.clear();
  if (!ctx || c.e != E || (!trace_host && !trace_dev)) return MS_ERR_ARG;
  // the statement
  LinkedShape sh;
  int rc = linked_shape<F>(c, air, N, w, kd, &sh);
  if (rc) return rc;
  AirProg pg; std::vector<AuxInstance> inst;
  std::vector<u64> ch((size_t)kd.nch * e);
  if (kd.version == 1 && (rc = linked_combined<F, E>(air, nullptr, 0, nullptr, w, &pg, &inst, &sh))) return rc;   // v1 refuses a bad program before it touches the context
  Transcript t = linked_transcript(c, sh, kd);
  u8 root[32];
  // the raw-trace root: ms_trace_commit is how the trace gets in.  It is absorbed first and binds nothing
  rc = trace_dev ? ms_trace_commit_device(ctx, trace_dev, N, w, w, root) : ms_trace_commit(ctx, trace_host, N, w, w, root);
  if (rc) return rc;
  t.add_bytes(root, 32);
  // the shift (redrawn while the coset would meet the trace domain), the LDE root
  const u64 shift = draw_shift<F>(t, sh.L);
  if ((rc = ms_interpolate(ctx))) return rc;
  if ((rc = kd.k ? ms_lde_commit_coset(ctx, sh.blowup, shift, kd.k, root) : ms_lde_commit(ctx, sh.blowup, shift, w, root))) return rc;
  t.add_bytes(root, 32);
  // the arguments' challenges follow the commitment to the main columns; the program they fix; the running columns and the staged root
  if (kd.nargs) t.challenge_scalars(ch.data(), ch.size(), p);
  if (kd.version > 1 && (rc = linked_combined<F, E>(air, kd.args, kd.nargs, ch.data(), w, &pg, &inst, &sh))) return rc;
  for (u32 j = 0; j < kd.nargs; j++) {
    u64 fin[E];
    if ((rc = ms_aux_running_staged(ctx, &inst[j].aux, fin, nullptr))) return rc;          // MS_ERR_SHAPE: a zero denominator (probability about N / |K|)
    for (int l = 0; l < e; l++) if (fin[l] != ((kd.args[j].op == MS_AUX_PRODUCT && l == 0) ? 1u : 0u)) return MS_ERR_SHAPE;   // the argument does not hold
  }
  if (kd.nargs) {
    if ((rc = kd.k ? ms_lde_commit_stage_coset(ctx, kd.k, root) : ms_lde_commit_stage(ctx, kd.nargs * (u32)e, root))) return rc;
    t.add_bytes(root, 32);
  }
  // r, the mix stage, the validity root
  std::vector<u64> r(e), z(e), gamma(e);
  t.challenge_scalars(r.data(), e, p);
  if ((rc = ms_mix_air_ext(ctx, r.data(), pg.view()))) return rc;            // MS_ERR_SHAPE: the trace violates the AIR
  if ((u64)ms_validity_len(ctx) / N * e != sh.m) return MS_ERR_STATE;        // (the stage's VL is the header's rule)
  if ((rc = kd.k ? ms_validity_commit_coset(ctx, kd.k, root) : ms_validity_commit(ctx, sh.m, root))) return rc;
  t.add_bytes(root, 32);
  // z (redrawn while it lies in the base field), the DEEP evaluations, gamma, the composition
  draw_z(t, z.data(), e, p);
  const std::vector<u64> pts = linked_points<F>(sh, z.data(), e);
  const ms_deep deep{sh.npts, pts.data(), sh.pt_begin.data(), sh.pt_poly.data()};
  std::vector<u64> evals(sh.ne * e);
  if ((rc = ms_deep_evals(ctx, &deep, evals.data()))) return rc;
  t.add_scalars(evals.data(), evals.size());
  t.challenge_scalars(gamma.data(), e, p);
  if ((rc = ms_deep_compose(ctx, &deep, gamma.data()))) return rc;
  // the FRI commit phase; round 0's root is in the transcript
  std::vector<u64> zq(e), B(2 * e), alpha(e);
  u64 nc = 0, D0 = 0; size_t nfinal = 0;
  if ((rc = kd.k ? ms_fri_begin_folded(ctx, sh.blowup, kd.k, root) : ms_fri_begin(ctx, sh.blowup, sh.R, root))) return rc;
  t.add_bytes(root, 32);
  if (!kd.k) {
    for (u32 i = 1; i < sh.R; i++) {
      t.challenge_scalars(zq.data(), e, p);
      if ((rc = ms_fri_deep(ctx, zq.data(), B.data()))) return rc;
      t.add_scalars(B.data(), 2 * e);
      t.challenge_scalars(alpha.data(), e, p);
      if ((rc = ms_fri_fold_commit(ctx, alpha.data(), root))) return rc;
      t.add_bytes(root, 32);
    }
  } else {
    if ((rc = ms_fri_round_info(ctx, 0, &nc, &D0))) return rc;
    for (u32 i = 0; i + 1 < sh.R; i++) {
      t.challenge_scalars(alpha.data(), e, p);
      if ((rc = ms_fri_fold_folded(ctx, alpha.data(), root))) return rc;     // MS_ERR_SHAPE: the DEEP polynomial is so short that R folds do not fit
      t.add_bytes(root, 32);
    }
    t.challenge_scalars(alpha.data(), e, p);
    if ((rc = ms_fri_fold_final(ctx, alpha.data(), nullptr, 0, &nfinal))) return rc;
    std::vector<u64> fin(nfinal * e + 1);
    if ((rc = ms_fri_fold_final(ctx, alpha.data(), fin.data(), nfinal * e, &nfinal))) return rc;
    t.add_scalars(fin.data(), nfinal * e);
  }
  // the proof of work, exactly as Stark::prove
  if (sh.gb) {
    u8 seed[32]; t.challenge_bytes(seed, 32);
    u64 nonce = 0;
    if (!ms_grind) return MS_ERR_ARG;
    if ((rc = ms_grind(ctx, seed, sh.gb, 0, ~(u64)0, &nonce))) return rc;
    u8 le[8]; for (int b = 0; b < 8; b++) le[b] = (u8)(nonce >> (8 * b));
    t.add_bytes(le, 8);
  }
  // the betas, the query phase in one call (asked for its size first), the header
  std::vector<u8> raw(8 * (size_t)sh.nq); t.challenge_bytes(raw.data(), raw.size());
  std::vector<u64> betas(sh.nq);
  memcpy(betas.data(), raw.data(), raw.size());
  const auto query = kd.k ? ms_query_linked_folded : ms_query_linked;
  size_t lq = 0;
  if ((rc = query(ctx, betas.data(), (int)sh.nq, nullptr, 0, &lq))) return rc;
  const size_t la = t.prover_bytes.size();
  if (la != linked_arthur_len(sh, kd, e, nfinal)) return MS_ERR_STATE;
  const std::vector<HeadWord> head = linked_header<E>(sh, kd, w);
  std::vector<u64> h64 = {sh.N, sh.blowup};
  if (kd.k) h64.push_back(D0);
  h64.insert(h64.end(), {(u64)la, (u64)lq});
  const size_t hb = linked_head_bytes(head, kd);
  std::vector<u8> out(hb + la + lq);
  for (size_t j = 0; j < head.size(); j++) memcpy(out.data() + 4 * j, &head[j].v, 4);
  memcpy(out.data() + 4 * head.size(), h64.data(), 8 * h64.size());
  memcpy(out.data() + hb, t.prover_bytes.data(), la);
  if ((rc = query(ctx, betas.data(), (int)sh.nq, out.data() + hb + la, lq, &lq))) return rc;
  s.linked.swap(out);
  return MS_OK;
}

// the replay of arthur: Arthur, with the rejection of a transcript that ends early written once
struct Replay : Arthur {
  std::string* why;
  Replay(const Transcript& t0, const u8* d, size_t n, std::string* why_) : Arthur("", t0.digest, d, n), why(why_) { t = t0; }
  bool bytes(u8* out, size_t n) { if (next_bytes(out, n)) return true; *why = "transcript: arthur ends early"; return false; }
  bool scalars(u64* out, size_t n) { return bytes((u8*)out, n * 8); }
};
// the verifier: 1 accepted, 0 rejected (*why names the step), < 0 malformed arguments.  Nothing of the proof is trusted: every header field is the verifier's own.
// Order: header, transcript replay (both redraw rules, the challenge draw), proof of work, AIR identity, FRI, round 0 against the row trees
template <class F, int E> static int verify_linked(const StarkConfig& c, const ms_air* air, size_t N, size_t w, const LinkedKind& kd, const u8* data, size_t len, int zae, std::string* why) {
  typedef Verifier<F, E> V;
  const u64 p = c.p;
  const LinkedText& tx = LINKED_TEXT[kd.version - 1];
  LinkedShape sh;
  AirProg pg; std::vector<AuxInstance> inst;
  if (c.e != E || linked_shape<F>(c, air, N, w, kd, &sh) || (kd.version == 1 && linked_combined<F, E>(air, nullptr, 0, nullptr, w, &pg, &inst, &sh))) {
    *why = tx.bad_args; return MS_ERR_ARG;
  }
  const u32 c0 = (u32)w, c1 = kd.nargs * (u32)E;
  // ---- header, first part: what the statement fixes without the challenges (v1: all of it); lengths exact
  std::vector<HeadWord> head = linked_header<E>(sh, kd, w);
  const size_t n64 = kd.k ? 5 : 4, hb = linked_head_bytes(head, kd);
  if (len < hb) { *why = std::string("header: the proof is shorter than the ") + tx.head + " header"; return 0; }
  if (!linked_header_ok(head, data, false, why)) return 0;
  u64 h64[5]; memcpy(h64, data + 4 * head.size(), 8 * n64);
  if (h64[0] != sh.N) { *why = "header: N is not the verifier's"; return 0; }
  if (h64[1] != sh.blowup) { *why = "header: blowup is not the verifier's"; return 0; }
  u64 D0 = 0, nfinal = 0;
  if (kd.k) {
    D0 = h64[2];
    const unsigned kr = (unsigned)kd.k * sh.R;
    if (D0 < 1 || (D0 & (D0 - 1)) || D0 > sh.L || sh.L % D0 || kr >= 64 || (D0 >> kr) < sh.blowup) { *why = "header: D_0 is no power of two that divides L with arity^R * blowup <= D_0"; return 0; }
    nfinal = (D0 >> kr) / sh.blowup;
  }
  const char* const bad_la = "header: len(arthur) is not what the statement fixes";
  const u64 h_la = h64[n64 - 2], h_lq = h64[n64 - 1];
  if (kd.version == 1 && h_la != (u64)linked_arthur_len(sh, kd, E, 0)) { *why = bad_la; return 0; }   // (v1 knows it here, and says so before it looks at the fit)
  if (h_la > len - hb || h_lq != (u64)(len - hb) - h_la) { *why = "header: the lengths do not fit the proof exactly"; return 0; }
  const size_t la = (size_t)h_la, lq = len - hb - la;
  if (la < 64) { *why = bad_la; return 0; }
  // ---- transcript up to the challenges of the arguments (la >= 64: the two roots are there); then the program and the rest of the header
  Replay a(linked_transcript(c, sh, kd), data + hb, la, why);
  u8 troot[32], lroot[32], sroot[32], vroot[32];
  if (!a.bytes(troot, 32)) return 0;
  const u64 shift = draw_shift<F>(a.t, sh.L);
  if (!a.bytes(lroot, 32)) return 0;
  std::vector<u64> ch((size_t)kd.nch * E);
  if (kd.nargs) a.t.challenge_scalars(ch.data(), ch.size(), p);
  if (kd.version > 1 && linked_combined<F, E>(air, kd.args, kd.nargs, ch.data(), w, &pg, &inst, &sh)) { *why = tx.bad_program; return MS_ERR_ARG; }
  head = linked_header<E>(sh, kd, w);
  if (!linked_header_ok(head, data, true, why)) return 0;
  if (la != linked_arthur_len(sh, kd, E, nfinal)) { *why = kd.k ? "header: len(arthur) is not what the statement and D_0 fix" : bad_la; return 0; }
  // ---- the query blob behind arthur: its magic, its section lengths exact.  Sections: FRI, LDE, (staged,) validity
  const std::string blob = tx.blob;
  const size_t qh = 8 * (size_t)(1 + tx.nsec);
  std::vector<u64> q((lq + 7) / 8 + 5, 0);            // aligned for the section verifiers
  memcpy(q.data(), data + hb + la, lq);
  if (lq < qh || q[0] != tx.magic) { *why = "header: no " + blob + " blob behind arthur"; return 0; }
  const u64 l_fri = q[1], l_lde = q[2], l_stg = tx.nsec == 4 ? q[3] : 0, l_val = q[tx.nsec];
  if (l_fri > lq - qh || l_lde > lq - qh - l_fri || l_stg > lq - qh - l_fri - l_lde || l_val != lq - qh - l_fri - l_lde - l_stg) {
    *why = "header: the " + blob + " section lengths do not fit the blob exactly"; return 0;
  }
  if ((l_fri | l_lde | l_stg | l_val) & 7) { *why = "header: an " + blob + " section length is no multiple of 8"; return 0; }
  if (!c1 && l_stg) { *why = "header: a staged section in a proof without running columns"; return 0; }
  const u8* fri = (const u8*)q.data() + qh; const u8* lde_open = fri + l_fri; const u8* stg_open = lde_open + l_lde; const u8* val_open = stg_open + l_stg;
  if (kd.k && (l_fri < 56 + nfinal * E * 8 || q[qh / 8 + 5] != D0)) { *why = "header: D_0 is not the MSFF's own"; return 0; }
  // ---- transcript, the rest: replayed from arthur, the redraw of z included
  const size_t W = kd.k ? 0 : sh.R - 1;               // the windows of the plain FRI
  std::vector<u8> roots((size_t)sh.R * 32);
  std::vector<u64> r(E), z(E), gamma(E), evals(sh.ne * E), zs(W * E), Bs(W * 2 * E), alphas((kd.k ? sh.R : W) * E), fin((size_t)nfinal * E + 1), betas(sh.nq);
  if (kd.nargs && !a.bytes(sroot, 32)) return 0;
  a.t.challenge_scalars(r.data(), E, p);
  if (!a.bytes(vroot, 32)) return 0;
  draw_z(a.t, z.data(), E, p);
  if (!a.scalars(evals.data(), evals.size())) return 0;
  if (!V::canon(evals.data(), evals.size())) { *why = "transcript: a claimed evaluation is not canonical"; return 0; }
  a.t.challenge_scalars(gamma.data(), E, p);
  if (!a.bytes(roots.data(), 32)) return 0;
  if (!kd.k) {
    for (u32 i = 1; i < sh.R; i++) {
      a.t.challenge_scalars(zs.data() + (size_t)(i - 1) * E, E, p);
      if (!a.scalars(Bs.data() + (size_t)(i - 1) * 2 * E, 2 * E)) return 0;
      a.t.challenge_scalars(alphas.data() + (size_t)(i - 1) * E, E, p);
      if (!a.bytes(roots.data() + (size_t)i * 32, 32)) return 0;
    }
    if (!V::canon(Bs.data(), Bs.size())) { *why = "transcript: a round's B is not canonical"; return 0; }
  } else {
    for (u32 i = 0; i + 1 < sh.R; i++) {
      a.t.challenge_scalars(alphas.data() + (size_t)i * E, E, p);
      if (!a.bytes(roots.data() + (size_t)(i + 1) * 32, 32)) return 0;
    }
    a.t.challenge_scalars(alphas.data() + (size_t)(sh.R - 1) * E, E, p);
    if (!a.scalars(fin.data(), (size_t)nfinal * E)) return 0;
    if (!V::canon(fin.data(), (size_t)nfinal * E)) { *why = "transcript: a coefficient of the final polynomial is not canonical"; return 0; }
    if (memcmp(fin.data(), fri + 56, (size_t)nfinal * E * 8)) { *why = "transcript: the final polynomial in arthur is not the MSFF's"; return 0; }
  }
  u8 seed[32] = {0}; u64 nonce = 0;
  if (sh.gb) {
    a.t.challenge_bytes(seed, 32);
    u8 le[8];
    if (!a.bytes(le, 8)) return 0;
    for (int b = 0; b < 8; b++) nonce |= (u64)le[b] << (8 * b);
  }
  if (a.pos != la) { *why = "transcript: bytes left in arthur"; return 0; }
  { std::vector<u8> raw(8 * (size_t)sh.nq); a.t.challenge_bytes(raw.data(), raw.size()); memcpy(betas.data(), raw.data(), raw.size()); }
  // ---- 1. the proof of work
  if (sh.gb && !pow_ok(c.digest, seed, nonce, sh.gb)) { *why = "proof of work: the nonce does not give the digest its leading zero bits"; return 0; }
  // ---- 2. the AIR identity at z: the program on the opened evaluations against V(z) from the chunk evaluations
  {
    std::vector<u64> opened((size_t)sh.npts * sh.c * E);
    for (u32 t = 0; t < sh.npts; t++) memcpy(opened.data() + (size_t)t * sh.c * E, evals.data() + (size_t)sh.pt_begin[t] * E, (size_t)sh.c * E * 8);
    u64 want[E], got[E];
    const int rc = air_expected<F, E>(r.data(), *pg.view(), N, z.data(), (int)sh.npts, sh.rows.data(), opened.data(), (size_t)sh.c * E, sh.c, want);
    if (rc) { *why = "malformed arguments: the AIR program cannot be evaluated at z"; return rc < 0 ? rc : MS_ERR_ARG; }
    validity_from_chunks<F, E>((u32)E, sh.m / E, N, z.data(), evals.data() + (size_t)sh.c * E, got);
    if (memcmp(want, got, sizeof want)) { *why = "AIR identity: the program on the opened evaluations is not V(z) of the chunk evaluations"; return 0; }
  }
  // ---- 3. FRI on the blob's first section (MSFI, or MSFF for the folded FRI), with the roots and challenges of the replay
  std::string sub;
  int rc = kd.k ? fri_folded_verify<F, E>(c.digest, zae, sh.blowup, kd.k, roots.data(), sh.R, alphas.data(), betas.data(), sh.nq, fri, l_fri, &sub)
                : fri_index_verify<F, E>(c.digest, zae, sh.blowup, roots.data(), sh.R, zs.data(), Bs.data(), alphas.data(), betas.data(), sh.nq, fri, l_fri, &sub);
  if (rc != 1) { *why = "FRI: " + sub; return rc; }
  // ---- 4. round 0 against the row trees (every slot of its cosets against the coset-grouped trees)
  const std::vector<u64> pts = linked_points<F>(sh, z.data(), E);
  const ms_deep deep{sh.npts, pts.data(), sh.pt_begin.data(), sh.pt_poly.data()};
  const u8* stg_root = c1 ? sroot : nullptr;
  rc = kd.k ? deep_link_verify_folded<F, E>(c.digest, zae, N, sh.blowup, shift, kd.k, c0, c1, sh.m, lroot, stg_root, vroot, deep, evals.data(), gamma.data(), betas.data(), sh.nq, fri, l_fri,
                                            lde_open, l_lde, stg_open, l_stg, val_open, l_val, &sub)
            : deep_link_verify<F, E>(c.digest, zae, N, sh.blowup, shift, c0, c1, sh.m, lroot, stg_root, vroot, deep, evals.data(), gamma.data(), betas.data(), sh.nq, fri, l_fri, lde_open, l_lde,
                                     stg_open, l_stg, val_open, l_val, &sub);
  if (rc != 1) { *why = sub; return rc; }
  return 1;
}
static size_t copy_out(const void* src, size_t n, void* dst, size_t cap) { if (dst && cap >= n && n) memcpy(dst, src, n); return n; }

extern "C" {
msh_stark* msh_stark_new(ms_ctx* ctx, int field, u64 security_bits, u64 blowup, u64 steps, u64 trace_columns, int* err) {
  msh_stark* h = new msh_stark();
  int rc = StarkConfig::create(ctx, (ms_field)field, security_bits, blowup, steps, trace_columns, &h->s.cfg);
  if (err) *err = rc;
  if (rc) { delete h; return nullptr; }
  return h;
}
void msh_stark_free(msh_stark* h) { delete h; }
int msh_stark_config(const msh_stark* h, u64* rounds, u64* constrain_queries, u64* fri_queries) {
  *rounds = h->s.cfg.rounds; *constrain_queries = h->s.cfg.constrain_queries; *fri_queries = h->s.cfg.fri_queries; return 0;
}
// trace: host pointer (trace_host) or device pointer (trace_dev); transitions: ntrans lincombs, the i-th with tr_k[i]
// terms taken consecutively from tr_scalars / tr_idx.
int msh_stark_prove(msh_stark* h, const u64* trace_host, const void* trace_dev, size_t N, size_t w, int ntrans, const int* tr_k,
                    const u64* tr_scalars, const int* tr_idx, int read_fri_proof) {
  TraceTable t; t.length = N; t.width = w; t.host = trace_host; t.device = trace_dev;
  size_t off = 0;
  for (int i = 0; i < ntrans; i++) {
    Lincomb l; l.scalars.assign(tr_scalars + off, tr_scalars + off + tr_k[i]); l.idx.assign(tr_idx + off, tr_idx + off + tr_k[i]);
    off += tr_k[i]; t.transitions.push_back(l);
  }
  return h->s.prove(t, read_fri_proof);
}
// names the page-locked host trace of the proof AFTER the next msh_stark_prove: that call prefetches it right behind its own trace commitment
void msh_stark_next_trace(msh_stark* h, const u64* trace_host, size_t N, size_t w) { h->s.next_host = trace_host; h->s.next_N = N; h->s.next_w = w; }
size_t msh_proof_arthur(const msh_stark* h, u8* out, size_t cap) { return copy_out(h->s.proof.arthur.data(), h->s.proof.arthur.size(), out, cap); }
int msh_proof_commits(const msh_stark* h, u8* trace_commit, u8* lde_commit) { memcpy(trace_commit, h->s.proof.trace_commit, 32); memcpy(lde_commit, h->s.proof.constrain_trace_commit, 32); return 0; }
size_t msh_proof_evals(const msh_stark* h, u64* out, size_t cap_elems) { return copy_out(h->s.proof.evals.data(), h->s.proof.evals.size() * 8, out, cap_elems * 8) / 8; }
size_t msh_proof_fri_roots(const msh_stark* h, u8* out, size_t cap) { return copy_out(h->s.proof.fri_roots.data(), h->s.proof.fri_roots.size(), out, cap); }
int msh_proof_wait(const msh_stark* h) { return h->s.wait_proof(); }
size_t msh_proof_fri_blob(const msh_stark* h, u8* out, size_t cap) { h->s.wait_proof(); return copy_out(h->s.proof.fri_blob.data(), h->s.proof.fri_blob.size(), out, cap); }
size_t msh_proof_challenges(const msh_stark* h, u64* out, size_t cap_elems) { return copy_out(h->s.proof.challenges.data(), h->s.proof.challenges.size() * 8, out, cap_elems * 8) / 8; }
size_t msh_proof_num_polys(const msh_stark* h) { return h->s.proof.c; }
// build-defined proof of work (ministark.h: pow_ok).  set_grinding: before msh_stark_prove / msh_stark_verify*; fri_queries follows ms_num_queries_grind
int msh_stark_set_grinding(msh_stark* h, uint32_t bits) {
  if (!h) return MS_ERR_ARG;
  StarkConfig& c = h->s.cfg;
  u64 cq = 0, fq = 0;
  int rc;
  if (bits == 0) rc = ms_num_queries(c.field, c.security_bits, c.blowup_factor, c.steps, &cq, &fq);
  else if (!ms_num_queries_grind || !ms_grind) return MS_ERR_ARG;
  else rc = ms_num_queries_grind(c.field, c.security_bits, bits, c.blowup_factor, c.steps, &cq, &fq);
  if (rc) return rc;
  c.grinding_bits = bits; c.constrain_queries = cq; c.fri_queries = fq;
  return MS_OK;
}
int msh_proof_pow_nonce(const msh_stark* h, uint64_t* nonce) {
  if (!h || !nonce) return MS_ERR_ARG;
  if (!h->s.proof.has_pow) return MS_ERR_STATE;
  *nonce = h->s.proof.pow_nonce;
  return MS_OK;
}
// the proof BEFORE the last one (the other slot): still whole while / after the next msh_stark_prove runs.  msh_prev_proof_fri_blob waits for an
// asynchronous read-back in flight on the context (mode 2: at most the copy of the last proof, issued after this one's had finished).
size_t msh_prev_proof_arthur(const msh_stark* h, u8* out, size_t cap) { return copy_out(h->s.prev.arthur.data(), h->s.prev.arthur.size(), out, cap); }
size_t msh_prev_proof_fri_roots(const msh_stark* h, u8* out, size_t cap) { return copy_out(h->s.prev.fri_roots.data(), h->s.prev.fri_roots.size(), out, cap); }
size_t msh_prev_proof_fri_blob(const msh_stark* h, u8* out, size_t cap) { return copy_out(h->s.prev.fri_blob.data(), h->s.prev.fri_blob.size(), out, cap); }
// FNV-1a over the FRI blob of the last (which = 0) or the previous (which = 1) proof, read IN PLACE from the page-locked slot: what a consumer
// that streams the proof out would touch (bench.py's I/O-inclusive leg reads every proof this way); 0 if there is none
static u64 blob_fnv(const msh_stark* h, int which, size_t stride_words) {
  if (which == 0) h->s.wait_proof();
  const PinnedBuf& b = which ? h->s.prev.fri_blob : h->s.proof.fri_blob;
  u64 x = 0xCBF29CE484222325ULL;
  const u64* w = (const u64*)b.data();
  const size_t nw = b.size() / 8;
  for (size_t i = 0; i < nw; i += stride_words) { x ^= w[i]; x *= 0x100000001B3ULL; }
  if (nw) { x ^= w[nw - 1]; x *= 0x100000001B3ULL; }
  return b.size() ? x : 0;
}
u64 msh_proof_blob_checksum(const msh_stark* h, int which) { return blob_fnv(h, which, 1); }
// the same over one word per `stride_bytes` (and the last word): touches every page of the blob without the cost of reading 64 MiB
u64 msh_proof_blob_sample(const msh_stark* h, int which, size_t stride_bytes) { return blob_fnv(h, which, stride_bytes >= 8 ? stride_bytes / 8 : 1); }
static int set_why(char* why, size_t why_cap, const char* msg, int rc);
// Stark::verify (src/starks.rs:171-235) of a proof given by its parts; `constrains` = the c constraint polynomials in coefficient
// form ([c][N] canonical u64: what trace.derive_constrains() hands the reference's verifier).  1 accepted, 0 rejected, < 0 malformed;
// the reason is copied to `why`.
int msh_stark_verify(const msh_stark* h, const u64* constrains, size_t c, size_t N, const u8* arthur, size_t arthur_len, const u8* trace_commit,
                     const u8* lde_commit, const u64* evals, size_t nevals, const u8* fri_roots, size_t nroots, const u8* blob, size_t blob_len,
                     int zero_display_empty, char* why, size_t why_cap) {
  if (!h || !constrains || !trace_commit || !lde_commit || (!arthur && arthur_len) || (!evals && nevals) || (!fri_roots && nroots) || (!blob && blob_len) ||
      arthur_len > ((size_t)1 << 32) || nroots > 64 || nevals > ((size_t)1 << 40) || blob_len > ((size_t)1 << 44))
    return set_why(why, why_cap, "malformed proof (null part or absurd length)", -1);
  try {
  StarkProof pr;
  pr.arthur.assign(arthur, arthur + arthur_len);
  memcpy(pr.trace_commit, trace_commit, 32); memcpy(pr.constrain_trace_commit, lde_commit, 32);
  pr.evals.assign(evals, evals + nevals);
  pr.fri_roots.assign(fri_roots, fri_roots + nroots * 32);
  pr.fri_blob.assign(blob, blob + blob_len);
  std::string reason;
  int rc;
  if (h->s.cfg.field == MS_FIELD_GOLDILOCKS) rc = Verifier<GL, 2>::run(h->s.cfg, constrains, c, N, pr, zero_display_empty, &reason);
  else rc = Verifier<BB, 4>::run(h->s.cfg, constrains, c, N, pr, zero_display_empty, &reason);
  if (why && why_cap) { size_t n = reason.size() < why_cap - 1 ? reason.size() : why_cap - 1; memcpy(why, reason.data(), n); why[n] = 0; }
  return rc;
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }   // nothing unwinds through the C boundary
}
// ---- whole-proof wire format "MSSP" v1 (layout in include/ministark_host.h) ----------------------------
static const size_t MSSP_HEAD = 4 + 5 * 4 + 2 * 8;
// bytes needed for the last proof of `h` (0: no proof, or its FRI proof was left in HBM); writes them when cap suffices
size_t msh_proof_serialize(const msh_stark* h, u8* out, size_t cap) {
  const StarkProof& pr = h->s.proof; const StarkConfig& c = h->s.cfg;
  h->s.wait_proof();   // an asynchronous read-back of the FRI proof
  if (pr.arthur.empty() || pr.fri_blob.empty()) return 0;
  const u32 e = (u32)c.e, cc = (u32)pr.c, q = (u32)c.constrain_queries, rounds = (u32)(pr.fri_roots.size() / 32);
  const size_t need = MSSP_HEAD + 64 + pr.evals.size() * 8 + pr.fri_roots.size() + pr.arthur.size() + pr.fri_blob.size();
  if (!out || cap < need) return need;
  u8* w = out;
  auto put = [&](const void* d, size_t n) { memcpy(w, d, n); w += n; };
  const u32 ver = 1; const u64 la = pr.arthur.size(), lb = pr.fri_blob.size();
  put("MSSP", 4); put(&ver, 4); put(&e, 4); put(&cc, 4); put(&q, 4); put(&rounds, 4); put(&la, 8); put(&lb, 8);
  put(pr.trace_commit, 32); put(pr.constrain_trace_commit, 32);
  // evals are stored [q][c+1][E] (constrain queries then the validity query per point); the wire order is all constrain queries, then all validity queries
  for (u32 i = 0; i < q; i++) put(pr.evals.data() + (size_t)i * (cc + 1) * e, (size_t)cc * e * 8);
  for (u32 i = 0; i < q; i++) put(pr.evals.data() + ((size_t)i * (cc + 1) + cc) * e, (size_t)e * 8);
  put(pr.fri_roots.data(), pr.fri_roots.size()); put(pr.arthur.data(), la); put(pr.fri_blob.data(), lb);
  return need;
}
// parses an MSSP blob: 0 on success (fields of `v` point INTO `data`), -1 malformed.  Every length is checked against the bytes that
// are LEFT, field by field, with comparisons that cannot wrap (a single wrapping sum let arthur_len = 2^64 - 1000 through).
int msh_proof_parse(const u8* data, size_t len, msh_proof_view* v) {
  if (!data || !v || len < MSSP_HEAD + 64 || memcmp(data, "MSSP", 4) != 0) return -1;
  u32 ver; memcpy(&ver, data + 4, 4); if (ver != 1) return -1;
  memcpy(&v->e, data + 8, 4); memcpy(&v->c, data + 12, 4); memcpy(&v->q, data + 16, 4); memcpy(&v->rounds, data + 20, 4);
  memcpy(&v->arthur_len, data + 24, 8); memcpy(&v->fri_blob_len, data + 32, 8);
  if ((v->e != 2 && v->e != 4) || v->c == 0 || v->c > (1u << 20) || v->q > (1u << 16) || v->rounds == 0 || v->rounds > 64) return -1;
  size_t left = len - (MSSP_HEAD + 64);
  const u64 ev = (u64)v->q * ((u64)v->c + 1) * v->e * 8;          // < 2^16 * 2^21 * 4 * 8 = 2^42: no wrap
  if (ev > left) return -1;
  left -= (size_t)ev;
  const size_t rb = (size_t)v->rounds * 32;
  if (rb > left) return -1;
  left -= rb;
  if (v->arthur_len > left) return -1;
  left -= (size_t)v->arthur_len;
  if (v->fri_blob_len != left) return -1;                          // the blob is the rest, exactly
  const u8* p = data + MSSP_HEAD;
  v->trace_commit = p; v->constrain_trace_commit = p + 32; p += 64;
  v->constrain_queries = (const u64*)p; p += (size_t)v->q * v->c * v->e * 8;
  v->validity_queries = (const u64*)p; p += (size_t)v->q * v->e * 8;
  v->fri_roots = p; p += rb;
  v->arthur = p; p += v->arthur_len;
  v->fri_blob = p;
  return 0;
}
static int set_why(char* why, size_t why_cap, const char* msg, int rc) { if (why && why_cap) { strncpy(why, msg, why_cap - 1); why[why_cap - 1] = 0; } return rc; }
// Stark::verify straight from the wire format: 1 accepted, 0 rejected, < 0 malformed
int msh_stark_verify_mssp(const msh_stark* h, const u64* constrains, size_t c, size_t N, const u8* data, size_t len, int zero_display_empty, char* why, size_t why_cap) {
  if (!h || !constrains) return set_why(why, why_cap, "null argument", -1);
  try {
    msh_proof_view v;
    if (msh_proof_parse(data, len, &v) || v.c != c || (int)v.e != h->s.cfg.e) return set_why(why, why_cap, "malformed MSSP proof", -1);
    // the sizes that feed allocations come from the HANDLE's configuration, never from the wire
    if (v.q != h->s.cfg.constrain_queries || v.rounds != h->s.cfg.rounds) return set_why(why, why_cap, "MSSP proof does not match this configuration (queries / rounds)", -1);
    std::vector<u64> evals((size_t)v.q * (v.c + 1) * v.e);
    for (u32 i = 0; i < v.q; i++) {
      memcpy(evals.data() + (size_t)i * (v.c + 1) * v.e, v.constrain_queries + (size_t)i * v.c * v.e, (size_t)v.c * v.e * 8);
      memcpy(evals.data() + ((size_t)i * (v.c + 1) + v.c) * v.e, v.validity_queries + (size_t)i * v.e, (size_t)v.e * 8);
    }
    return msh_stark_verify(h, constrains, c, N, v.arthur, v.arthur_len, v.trace_commit, v.constrain_trace_commit, evals.data(), evals.size(), v.fri_roots, v.rounds,
                            v.fri_blob, v.fri_blob_len, zero_display_empty, why, why_cap);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
// FriProof (src/fri.rs:17-22) out of its MSFP bytes (layout: ministark.h) - the compiled counterpart of the Rust shim's FriProof::from_msfp
// (examples/rust_shim/src/fri_proof.rs): `windows` = rounds - 1, `nq` queries per window, E limbs per element.  Fills up to `cap` records
// (views INTO `blob`), returns the number of records (windows * nq) or -1 if the bytes do not parse exactly.
int msh_fri_proof_parse(const u8* blob, size_t len, u32 e, u32 windows, u32 nq, msh_fri_query_view* out, size_t cap) {
  if ((!blob && len) || (e != 1 && e != 2 && e != 4) || windows > 64 || nq > (1u << 16)) return -1;
  const u8* p = blob; size_t left = len; size_t n = 0;
  auto path = [&](msh_merkle_path_view* mp) -> bool {
    const size_t head = 8 + (size_t)2 * e * 8 + 8;                   // leaf_index | lpn = 2 leaf_neighbours | nlevels
    if (left < head) return false;
    u64 nlev; memcpy(&mp->leaf_index, p, 8); memcpy(&nlev, p + 8 + (size_t)2 * e * 8, 8);
    if (nlev > 64 || left - head < (size_t)nlev * 64) return false;
    mp->leaf_neighbours = (const u64*)(p + 8); mp->nlevels = nlev; mp->levels = p + head;
    p += head + (size_t)nlev * 64; left -= head + (size_t)nlev * 64;
    return true;
  };
  for (u32 i = 0; i < windows; i++)
    for (u32 j = 0; j < nq; j++, n++) {
      msh_fri_query_view q;
      const size_t head = ((size_t)6 * e + 1) * 8;
      if (left < head) return -1;
      q.points = (const u64*)p;
      memcpy(&q.qlen, p + (size_t)6 * e * 8, 8);
      if (q.qlen > ((u64)1 << 40) || left - head < (size_t)q.qlen * e * 8) return -1;
      q.quotient = (const u64*)(p + head);
      p += head + (size_t)q.qlen * e * 8; left -= head + (size_t)q.qlen * e * 8;
      if (!path(&q.path[0]) || !path(&q.path[1])) return -1;
      if (out && n < cap) out[n] = q;
    }
  return left == 0 ? (int)n : -1;
}
int msh_terms_expected_validity(int field, u64 r, int ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, const u32* fac_poly, const u32* fac_row,
                                int nexempt, u64 N, const u64* z, int nrows, const u32* rows, const u64* opened, size_t row_stride, u32 npolys, u64* out) {
  if (!term_begin || !coef || !fac_begin || !fac_poly || !fac_row || !z || !opened || !out || (nrows && !rows)) return MS_ERR_ARG;
  if ((field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) || ncons < 1 || ncons > 4096 || nexempt < 0 || nexempt > 16 || nrows < 0 || !N || (N & (N - 1))) return MS_ERR_ARG;
  try {
    if (field == MS_FIELD_GOLDILOCKS) return N > ((u64)1 << GL::TWO_ADICITY) ? MS_ERR_ARG : terms_expected<GL, 2>(r, ncons, term_begin, coef, fac_begin, fac_poly, fac_row, nexempt, N, z, nrows, rows, opened, row_stride, npolys, out);
    return N > ((u64)1 << BB::TWO_ADICITY) ? MS_ERR_ARG : terms_expected<BB, 4>(r, ncons, term_begin, coef, fac_begin, fac_poly, fac_row, nexempt, N, z, nrows, rows, opened, row_stride, npolys, out);
  } catch (...) { return MS_ERR_NOMEM; }   // nothing unwinds through the C boundary
}
int msh_air_expected_validity(int field, u64 r, const ms_air* air, u64 N, const u64* z, int nrows, const u32* rows, const u64* opened, size_t row_stride, u32 npolys, u64* out) {
  const u64 rk[4] = {r, 0, 0, 0};
  return msh_air_expected_validity_ext(field, rk, air, N, z, nrows, rows, opened, row_stride, npolys, out);
}
int msh_air_expected_validity_ext(int field, const u64* r, const ms_air* air, u64 N, const u64* z, int nrows, const u32* rows, const u64* opened, size_t row_stride, u32 npolys, u64* out) {
  if (!r || !air || !z || !opened || !out || (nrows && !rows)) return MS_ERR_ARG;
  const ms_air& a = *air;
  if (!a.term_begin || !a.coef || !a.fac_begin || !a.fac_poly || !a.fac_row || !a.ex_begin || (a.nperiodic && (!a.per_begin || !a.per_val)) || (a.nbound && (!a.bnd_poly || !a.bnd_row || !a.bnd_val))) return MS_ERR_ARG;
  if ((field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) || a.ncons < 1 || a.ncons > 4096 || a.nperiodic > 64 || a.nbound > 4096 || nrows < 0 || !N || (N & (N - 1))) return MS_ERR_ARG;
  try {
    if (field == MS_FIELD_GOLDILOCKS) return N > ((u64)1 << GL::TWO_ADICITY) ? MS_ERR_ARG : air_expected<GL, 2>(r, a, N, z, nrows, rows, opened, row_stride, npolys, out);
    return N > ((u64)1 << BB::TWO_ADICITY) ? MS_ERR_ARG : air_expected<BB, 4>(r, a, N, z, nrows, rows, opened, row_stride, npolys, out);
  } catch (...) { return MS_ERR_NOMEM; }   // nothing unwinds through the C boundary
}
// synthetic trace of the build-defined degree-3 wide AIR (ms_mix_cubic; BASELINE configs[4]): row 0 and the w scalars from SplitMix64(seed), then
// col_j[i+1] = col_j[i] * col_{j+1}[i] * col_{j+2}[i] + s_j * col_{j+3}[i]  (column indices mod w) - the same values as tests/parity_cases.py:cubic_trace
int msh_cubic_rows(u64 p, size_t length, size_t w, u64 seed, u64* out, u64* scalars) {
  if (!out || !scalars || !length || w < 4 || p < 2) return -1;
  u64 sm = seed;
  auto next = [&]() { sm += 0x9E3779B97F4A7C15ULL; u64 z = sm; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); };
  auto mm = [&](u64 a, u64 b) { return (u64)(((unsigned __int128)a * b) % p); };
  for (size_t j = 0; j < w; j++) scalars[j] = next() % p;
  for (size_t j = 0; j < w; j++) out[j] = next() % p;
  for (size_t i = 1; i < length; i++) {
    const u64* a = out + (i - 1) * w; u64* b = out + i * w;
    for (size_t j = 0; j < w; j++) b[j] = (u64)(((unsigned __int128)mm(mm(a[j], a[(j + 1) % w]), a[(j + 2) % w]) + mm(scalars[j], a[(j + 3) % w])) % p);
  }
  return 0;
}
// D(data) for an ms_digest_id, by the hashes of this mirror (the Python mirror has no BLAKE3 of its own and calls this one): 0, or -1 for an unknown id
int msh_hash(int digest_id, const u8* data, size_t len, u8 out[32]) {
  const bool known = (digest_id >= MS_DIGEST_SHA256 && digest_id <= MS_DIGEST_BLAKE3) || digest_id == MS_DIGEST_KECCAK256 || digest_id == MS_DIGEST_SHA3_256;   // (3 is unassigned)
  if (!known || !out || (!data && len)) return -1;
  ministark::Hasher h(digest_id); if (len) h.update(data, len); h.finish(out);
  return 0;
}
int msh_pow_check(int digest_id, const u8 seed[32], u64 nonce, uint32_t bits) {
  const bool known = (digest_id >= MS_DIGEST_SHA256 && digest_id <= MS_DIGEST_BLAKE3) || digest_id == MS_DIGEST_KECCAK256 || digest_id == MS_DIGEST_SHA3_256;
  if (!known || !seed || bits > 64) return -1;
  return ministark::pow_ok(digest_id, seed, nonce, bits) ? 1 : 0;
}
static bool known_digest(int id) { return (id >= MS_DIGEST_SHA256 && id <= MS_DIGEST_BLAKE3) || id == MS_DIGEST_KECCAK256 || id == MS_DIGEST_SHA3_256; }
int msh_merkle_path_check_index(int digest_id, int field, int ext, size_t lpn, int zero_display_empty, const u8 root[32], const u8* path, size_t avail,
                                u64 expect_leaf_group, size_t* used) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) || !root || !path || !used) return MS_ERR_ARG;
  const int E = field == MS_FIELD_GOLDILOCKS ? 2 : 4;
  if ((ext != 1 && ext != E) || lpn < 1 || lpn > ((size_t)1 << 24) || expect_leaf_group > ~(u64)0 / lpn) return MS_ERR_ARG;
  try {
    std::string why;
    const u64 at = expect_leaf_group * lpn;
    const bool ok = field == MS_FIELD_GOLDILOCKS ? check_path_at<GL>(digest_id, ext, lpn, zero_display_empty, root, path, avail, at, used, &why)
                                                 : check_path_at<BB>(digest_id, ext, lpn, zero_display_empty, root, path, avail, at, used, &why);
    return ok ? 1 : 0;
  } catch (...) { return MS_ERR_NOMEM; }   // nothing unwinds through the C boundary
}
int msh_fri_index_verify(int digest_id, int field, int zero_display_empty, u64 blowup, const u8* roots, size_t rounds, const u64* z, const u64* B, const u64* alpha,
                         const u64* betas, size_t nq, const u8* blob, size_t len, char* why, size_t why_cap) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return set_why(why, why_cap, "unknown digest or field", MS_ERR_ARG);
  if (!roots || !betas || !blob || rounds < 1 || rounds > 64 || nq < 1 || nq > 4096 || !blowup || (blowup & (blowup - 1)) || (rounds > 1 && (!z || !B || !alpha)))
    return set_why(why, why_cap, "null argument, or rounds, queries or blowup out of range", MS_ERR_ARG);
  try {
    std::string w;
    const int rc = field == MS_FIELD_GOLDILOCKS ? fri_index_verify<GL, 2>(digest_id, zero_display_empty, blowup, roots, rounds, z, B, alpha, betas, nq, blob, len, &w)
                                                : fri_index_verify<BB, 4>(digest_id, zero_display_empty, blowup, roots, rounds, z, B, alpha, betas, nq, blob, len, &w);
    return set_why(why, why_cap, w.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
int msh_fri_folded_verify(int digest_id, int field, int zero_display_empty, u64 blowup, int log_arity, const u8* roots, size_t rounds, const u64* alpha, const u64* betas,
                          size_t nq, const u8* blob, size_t len, char* why, size_t why_cap) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return set_why(why, why_cap, "unknown digest or field", MS_ERR_ARG);
  if (!roots || !alpha || !betas || !blob || rounds < 1 || rounds > 64 || nq < 1 || nq > 4096 || !blowup || (blowup & (blowup - 1)) || log_arity < 1 || log_arity > 3)
    return set_why(why, why_cap, "null argument, or rounds, queries, blowup or log_arity out of range", MS_ERR_ARG);
  if (!(field == MS_FIELD_GOLDILOCKS ? Verifier<GL, 2>::canon(alpha, rounds * 2) : Verifier<BB, 4>::canon(alpha, rounds * 4)))
    return set_why(why, why_cap, "fold challenge not canonical", MS_ERR_ARG);
  try {
    std::string w;
    const int rc = field == MS_FIELD_GOLDILOCKS ? fri_folded_verify<GL, 2>(digest_id, zero_display_empty, blowup, log_arity, roots, rounds, alpha, betas, nq, blob, len, &w)
                                                : fri_folded_verify<BB, 4>(digest_id, zero_display_empty, blowup, log_arity, roots, rounds, alpha, betas, nq, blob, len, &w);
    return set_why(why, why_cap, w.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
int msh_validity_from_chunks(int field, uint32_t ve, uint32_t nchunks, u64 N, const u64* z, const u64* chunk_evals, u64* out) {
  if ((field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) || !z || !chunk_evals || !out || !nchunks || !N) return MS_ERR_ARG;
  const u32 E = field == MS_FIELD_GOLDILOCKS ? 2 : 4;
  if ((ve != 1 && ve != E) || nchunks > 4096) return MS_ERR_ARG;
  const bool ok = field == MS_FIELD_GOLDILOCKS ? Verifier<GL, 2>::canon(z, E) && Verifier<GL, 2>::canon(chunk_evals, (size_t)ve * nchunks * E)
                                               : Verifier<BB, 4>::canon(z, E) && Verifier<BB, 4>::canon(chunk_evals, (size_t)ve * nchunks * E);
  if (!ok) return MS_ERR_ARG;
  if (field == MS_FIELD_GOLDILOCKS) validity_from_chunks<GL, 2>(ve, nchunks, N, z, chunk_evals, out); else validity_from_chunks<BB, 4>(ve, nchunks, N, z, chunk_evals, out);
  return MS_OK;
}
int msh_deep_link_verify(int digest_id, int field, int zero_display_empty, u64 N, u64 blowup, u64 shift, uint32_t c, uint32_t m, const u8 lde_root[32], const u8 val_root[32],
                         const ms_deep* deep, const u64* evals, const u64* gamma, const u64* betas, size_t nq, const u8* msfi, size_t msfi_len,
                         const u8* lde_open, size_t lde_len, const u8* val_open, size_t val_len, char* why, size_t why_cap) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return set_why(why, why_cap, "unknown digest or field", MS_ERR_ARG);
  if (!lde_root || !val_root || !deep || !deep->z || !deep->pt_begin || !deep->pt_poly || !evals || !gamma || !betas || !msfi || !lde_open || !val_open || nq < 1 || nq > 4096 ||
      !N || (N & (N - 1)) || !blowup || (blowup & (blowup - 1)) || N > ((u64)1 << 32) || blowup > ((u64)1 << 16) || c < 1 || m < 1 || c > (1u << 24) || m > (1u << 24))
    return set_why(why, why_cap, "null argument, or N, blowup, c, m or queries out of range", MS_ERR_ARG);
  try {
    std::string w;
    const int rc = field == MS_FIELD_GOLDILOCKS
      ? deep_link_verify<GL, 2>(digest_id, zero_display_empty, N, blowup, shift, c, 0, m, lde_root, nullptr, val_root, *deep, evals, gamma, betas, nq, msfi, msfi_len, lde_open, lde_len, nullptr, 0, val_open, val_len, &w)
      : deep_link_verify<BB, 4>(digest_id, zero_display_empty, N, blowup, shift, c, 0, m, lde_root, nullptr, val_root, *deep, evals, gamma, betas, nq, msfi, msfi_len, lde_open, lde_len, nullptr, 0, val_open, val_len, &w);
    return set_why(why, why_cap, w.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
// ---- linked proofs (MSLP v1, v2, v3): every entry point checks its own arguments and names its kind; a proof that is refused or fails leaves an empty slot
static int prove_linked_kind(msh_stark* h, const u64* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const LinkedKind& kd) {
  if (!h) return MS_ERR_ARG;
  try {
    return h->s.cfg.field == MS_FIELD_GOLDILOCKS ? prove_linked<GL, 2>(h->s, trace_host, trace_dev, N, w, air, kd) : prove_linked<BB, 4>(h->s, trace_host, trace_dev, N, w, air, kd);
  } catch (...) { h->s.linked.clear(); return MS_ERR_NOMEM; }
}
static int verify_linked_kind(const msh_stark* h, const ms_air* air, size_t N, size_t w, const LinkedKind& kd, const u8* data, size_t len, int zae, char* why, size_t why_cap) {
  try {
    std::string msg;
    const StarkConfig& c = h->s.cfg;
    const int rc = c.field == MS_FIELD_GOLDILOCKS ? verify_linked<GL, 2>(c, air, N, w, kd, data, len, zae, &msg) : verify_linked<BB, 4>(c, air, N, w, kd, data, len, zae, &msg);
    return set_why(why, why_cap, msg.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
int msh_stark_prove_linked(msh_stark* h, const u64* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, uint32_t fri_rounds) {
  return prove_linked_kind(h, trace_host, trace_dev, N, w, air, LinkedKind{1, 0, nullptr, 0, 0, fri_rounds});
}
size_t msh_linked_proof(const msh_stark* h, u8* out, size_t cap) { return h ? copy_out(h->s.linked.data(), h->s.linked.size(), out, cap) : 0; }
int msh_stark_verify_linked(const msh_stark* h, const ms_air* air, size_t N, size_t w, uint32_t fri_rounds, const u8* data, size_t len, int zero_display_empty, char* why, size_t why_cap) {
  if (!h || !data || !air) return set_why(why, why_cap, "null argument", MS_ERR_ARG);
  return verify_linked_kind(h, air, N, w, LinkedKind{1, 0, nullptr, 0, 0, fri_rounds}, data, len, zero_display_empty, why, why_cap);
}
int msh_stark_prove_linked_aux(msh_stark* h, const u64* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const msh_aux_arg* args, uint32_t nargs,
                               uint32_t nch, uint32_t fri_rounds) {
  return prove_linked_kind(h, trace_host, trace_dev, N, w, air, LinkedKind{2, 0, args, nargs, nch, fri_rounds});
}
int msh_stark_verify_linked_aux(const msh_stark* h, const ms_air* air, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, size_t N, size_t w, uint32_t fri_rounds,
                                const u8* data, size_t len, int zero_display_empty, char* why, size_t why_cap) {
  if (!h || !data || !air || !args) return set_why(why, why_cap, "null argument", MS_ERR_ARG);
  return verify_linked_kind(h, air, N, w, LinkedKind{2, 0, args, nargs, nch, fri_rounds}, data, len, zero_display_empty, why, why_cap);
}
int msh_stark_prove_linked_folded(msh_stark* h, const u64* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const msh_aux_arg* args, uint32_t nargs,
                                  uint32_t nch, int log_arity, uint32_t fri_folds) {
  return prove_linked_kind(h, trace_host, trace_dev, N, w, air, LinkedKind{3, log_arity, args, nargs, nch, fri_folds});
}
int msh_stark_verify_linked_folded(const msh_stark* h, const ms_air* air, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, size_t N, size_t w, int log_arity, uint32_t fri_folds,
                                   const u8* data, size_t len, int zero_display_empty, char* why, size_t why_cap) {
  if (!h || !data || !air) return set_why(why, why_cap, "null argument", MS_ERR_ARG);
  return verify_linked_kind(h, air, N, w, LinkedKind{3, log_arity, args, nargs, nch, fri_folds}, data, len, zero_display_empty, why, why_cap);
}
// ---- running columns: the combined program and the encoding of the arguments
struct msh_air_prog { AirProg p; };
msh_air_prog* msh_air_prog_new(const ms_air* base) {
  try { std::unique_ptr<msh_air_prog> g(new msh_air_prog()); if (!g->p.load(base)) return nullptr; return g.release(); } catch (...) { return nullptr; }
}
void msh_air_prog_free(msh_air_prog* g) { delete g; }
const ms_air* msh_air_prog_air(msh_air_prog* g) { return g ? g->p.view() : nullptr; }
int msh_aux_constraints(msh_air_prog* g, int field, const ms_aux* aux, uint32_t first_poly) {
  if (!g || !aux || !aux->form_begin || !aux->form_const || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return MS_ERR_ARG;
  try {
    AirProg work = g->p;   // (a refused expansion leaves the program as it was)
    const int rc = field == MS_FIELD_GOLDILOCKS ? aux_constraints<GL, 2>(work, *aux, first_poly) : aux_constraints<BB, 4>(work, *aux, first_poly);
    if (!rc) g->p = std::move(work);
    return rc;
  } catch (...) { return MS_ERR_NOMEM; }
}
size_t msh_aux_encode(int field, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, u8* out, size_t cap) {
  if (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) return 0;
  try {
    std::vector<u8> enc;
    const bool gl = field == MS_FIELD_GOLDILOCKS;
    return aux_encode(args, nargs, nch, gl ? (u64)GL::P : (u64)BB::P, gl ? 2 : 4, 0, &enc) ? copy_out(enc.data(), enc.size(), out, cap) : 0;
  } catch (...) { return 0; }
}
int msh_deep_link_verify_staged(int digest_id, int field, int zero_display_empty, u64 N, u64 blowup, u64 shift, uint32_t c0, uint32_t c1, uint32_t m, const u8 lde_root[32],
                                const u8 stg_root[32], const u8 val_root[32], const ms_deep* deep, const u64* evals, const u64* gamma, const u64* betas, size_t nq,
                                const u8* msfi, size_t msfi_len, const u8* lde_open, size_t lde_len, const u8* stg_open, size_t stg_len, const u8* val_open, size_t val_len,
                                char* why, size_t why_cap) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return set_why(why, why_cap, "unknown digest or field", MS_ERR_ARG);
  if (!lde_root || !stg_root || !val_root || !deep || !deep->z || !deep->pt_begin || !deep->pt_poly || !evals || !gamma || !betas || !msfi || !lde_open || !stg_open || !val_open ||
      nq < 1 || nq > 4096 || !N || (N & (N - 1)) || !blowup || (blowup & (blowup - 1)) || N > ((u64)1 << 32) || blowup > ((u64)1 << 16) || c0 < 1 || c1 < 1 || m < 1 ||
      c0 > (1u << 24) || c1 > (1u << 24) || m > (1u << 24))
    return set_why(why, why_cap, "null argument, or N, blowup, c0, c1, m or queries out of range", MS_ERR_ARG);
  try {
    std::string w;
    const int rc = field == MS_FIELD_GOLDILOCKS
      ? deep_link_verify<GL, 2>(digest_id, zero_display_empty, N, blowup, shift, c0, c1, m, lde_root, stg_root, val_root, *deep, evals, gamma, betas, nq, msfi, msfi_len, lde_open, lde_len, stg_open, stg_len, val_open, val_len, &w)
      : deep_link_verify<BB, 4>(digest_id, zero_display_empty, N, blowup, shift, c0, c1, m, lde_root, stg_root, val_root, *deep, evals, gamma, betas, nq, msfi, msfi_len, lde_open, lde_len, stg_open, stg_len, val_open, val_len, &w);
    return set_why(why, why_cap, w.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
int msh_deep_link_verify_folded(int digest_id, int field, int zero_display_empty, u64 N, u64 blowup, u64 shift, int log_arity, uint32_t c0, uint32_t c1, uint32_t m,
                                const u8 lde_root[32], const u8 stg_root[32], const u8 val_root[32], const ms_deep* deep, const u64* evals, const u64* gamma, const u64* betas,
                                size_t nq, const u8* msff, size_t msff_len, const u8* lde_open, size_t lde_len, const u8* stg_open, size_t stg_len, const u8* val_open,
                                size_t val_len, char* why, size_t why_cap) {
  if (!known_digest(digest_id) || (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR)) return set_why(why, why_cap, "unknown digest or field", MS_ERR_ARG);
  if (!lde_root || !val_root || (c1 == 0) != (stg_root == nullptr) || (c1 != 0 && !stg_open) || !deep || !deep->z || !deep->pt_begin || !deep->pt_poly || !evals || !gamma || !betas ||
      !msff || !lde_open || !val_open || nq < 1 || nq > 4096 || !N || (N & (N - 1)) || !blowup || (blowup & (blowup - 1)) || N > ((u64)1 << 32) || blowup > ((u64)1 << 16) ||
      log_arity < 1 || log_arity > 3 || c0 < 1 || m < 1 || c0 > (1u << 21) || c1 > (1u << 21) || m > (1u << 21))
    return set_why(why, why_cap, "null argument (stg_root is NULL iff c1 = 0), or N, blowup, log_arity, c0, c1, m or queries out of range", MS_ERR_ARG);
  try {
    std::string w;
    const int rc = field == MS_FIELD_GOLDILOCKS
      ? deep_link_verify_folded<GL, 2>(digest_id, zero_display_empty, N, blowup, shift, log_arity, c0, c1, m, lde_root, stg_root, val_root, *deep, evals, gamma, betas, nq, msff, msff_len, lde_open, lde_len, stg_open, c1 ? stg_len : 0, val_open, val_len, &w)
      : deep_link_verify_folded<BB, 4>(digest_id, zero_display_empty, N, blowup, shift, log_arity, c0, c1, m, lde_root, stg_root, val_root, *deep, evals, gamma, betas, nq, msff, msff_len, lde_open, lde_len, stg_open, c1 ? stg_len : 0, val_open, val_len, &w);
    return set_why(why, why_cap, w.c_str(), rc);
  } catch (...) { return set_why(why, why_cap, "out of memory / internal error while verifying", -1); }
}
size_t msh_air_encode(const ms_air* air, u8* out, size_t cap) {
  try {
    std::vector<u8> enc;
    return air_encode(air, &enc) ? copy_out(enc.data(), enc.size(), out, cap) : 0;
  } catch (...) { return 0; }
}
int msh_air_rows(const ms_air* air, uint32_t* rows, int cap) {
  try {
    std::vector<u32> r;
    if (!air_rows(air, &r) || (cap > 0 && !rows)) return MS_ERR_ARG;
    for (int k = 0; k < cap && k < (int)r.size(); k++) rows[k] = r[k];
    return (int)r.size();
  } catch (...) { return MS_ERR_NOMEM; }
}
int msh_linked_shift_ok(int field, uint64_t L, uint64_t shift) {
  if (field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) return MS_ERR_ARG;
  return (field == MS_FIELD_GOLDILOCKS ? linked_shift_ok<GL>(shift, L) : linked_shift_ok<BB>(shift, L)) ? 1 : 0;
}
int msh_linked_z_ok(int field, const uint64_t* z) {
  if ((field != MS_FIELD_GOLDILOCKS && field != MS_FIELD_BABYBEAR) || !z) return MS_ERR_ARG;
  return linked_z_ok(z, field == MS_FIELD_GOLDILOCKS ? 2 : 4) ? 1 : 0;
}
// the synthetic Fibonacci-AIR trace of the benchmark workload (tests/e2e_goldilocks.rs:20-63 rows + SplitMix64 padding; = mini_stark_amd.synthetic.fibonacci_rows)
int msh_fibonacci_rows(u64 p, size_t length, size_t steps, u64 secret_b, u64 pad_seed, u64* out) {
  if (!out || steps > length || p < 2) return -1;
  u64 a = 1 % p, b = secret_b % p;
  for (size_t i = 0; i < steps; i++) {
    const u64 cc = (u64)(((unsigned __int128)a + b) % p);
    out[3 * i] = a; out[3 * i + 1] = b; out[3 * i + 2] = cc;
    a = b; b = cc;
  }
  u64 sm = pad_seed;
  for (size_t i = 3 * steps; i < 3 * length; i++) {
    sm += 0x9E3779B97F4A7C15ULL; u64 z = sm;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
    out[i] = z % p;
  }
  return 0;
}
}
