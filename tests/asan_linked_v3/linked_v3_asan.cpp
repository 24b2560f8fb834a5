// Stand-alone sanitizer run of the host library's code that takes the least trusted bytes: msh_stark_verify_linked_folded, the parser and verifier of MSLP v3 proofs.
// Compiled together with mini-stark_amd/host/stark_host.cpp under -fsanitize=address,undefined (Makefile) and linked against the emulation build of the C ABI, which
// only configures the handle here (ms_create, ms_num_queries, ..): nothing is proved, no kernel code runs.  Reads tests/golden/linked_v3_tampered.bin
// (tests/golden/gen_linked_v3_tampered.py), gives every proof to the verifier in a heap block of exactly its size - a read past either end is a sanitizer report - and
// compares verdict and step with the recorded ones.  Exit status 0: every case as recorded and no report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ministark.h"
#include "../../include/ministark_host.h"

struct Reader {
  const std::vector<uint8_t>& b; size_t pos = 0;
  explicit Reader(const std::vector<uint8_t>& b_) : b(b_) {}
  uint32_t u32() { if (pos + 4 > b.size()) { fprintf(stderr, "fixture truncated\n"); exit(2); } uint32_t v; memcpy(&v, b.data() + pos, 4); pos += 4; return v; }
  std::vector<uint8_t> bytes() { const uint32_t n = u32(); if (pos + n > b.size()) { fprintf(stderr, "fixture truncated\n"); exit(2); } std::vector<uint8_t> v(b.begin() + pos, b.begin() + pos + n); pos += n; return v; }
};

// an ms_air over arrays decoded from msh_air_encode bytes (the arrays are copied out: the encoding does not align its u64 arrays)
struct Air {
  std::vector<uint32_t> term_begin, fac_begin, fac_poly, fac_row, ex_begin, ex_row, per_begin, bnd_poly, bnd_row;
  std::vector<uint64_t> coef, per_val, bnd_val;
  ms_air a;
  explicit Air(const std::vector<uint8_t>& enc) {
    uint32_t h[10];
    if (enc.size() < sizeof h) { fprintf(stderr, "AIR encoding truncated\n"); exit(2); }
    memcpy(h, enc.data(), sizeof h);
    size_t pos = sizeof h;
    auto take32 = [&](std::vector<uint32_t>& v, size_t n) { v.resize(n); if (pos + 4 * n > enc.size()) exit(2); if (n) memcpy(v.data(), enc.data() + pos, 4 * n); pos += 4 * n; };
    auto take64 = [&](std::vector<uint64_t>& v, size_t n) { v.resize(n); if (pos + 8 * n > enc.size()) exit(2); if (n) memcpy(v.data(), enc.data() + pos, 8 * n); pos += 8 * n; };
    const uint32_t ncons = h[2], nterms = h[3], nfacs = h[4], nex = h[5], nper = h[6], nperval = h[7], nbound = h[8];
    take32(term_begin, ncons + 1); take64(coef, nterms); take32(fac_begin, nterms + 1); take32(fac_poly, nfacs); take32(fac_row, nfacs);
    take32(ex_begin, ncons + 1); take32(ex_row, nex); take32(per_begin, nper + 1); take64(per_val, nperval);
    take32(bnd_poly, nbound); take32(bnd_row, nbound); take64(bnd_val, nbound);
    if (pos != enc.size()) { fprintf(stderr, "AIR encoding: trailing bytes\n"); exit(2); }
    a = ms_air{ncons, term_begin.data(), coef.data(), fac_begin.data(), fac_poly.data(), fac_row.data(), ex_begin.data(), ex_row.data(), nper, per_begin.data(), per_val.data(),
               nbound, bnd_poly.data(), bnd_row.data(), bnd_val.data()};
  }
};

// msh_aux_arg descriptors over arrays decoded from msh_aux_encode bytes
struct AuxArgs {
  struct One { std::vector<uint32_t> form_begin, term_col, term_ch, form_ch; std::vector<uint64_t> term_coef, form_const; };
  std::vector<One> own; std::vector<msh_aux_arg> args; uint32_t nch = 0;
  explicit AuxArgs(const std::vector<uint8_t>& enc) {
    if (enc.empty()) return;
    size_t pos = 0;
    auto u32 = [&]() { if (pos + 4 > enc.size()) exit(2); uint32_t v; memcpy(&v, enc.data() + pos, 4); pos += 4; return v; };
    auto take32 = [&](std::vector<uint32_t>& v, size_t n) { v.resize(n); if (pos + 4 * n > enc.size()) exit(2); if (n) memcpy(v.data(), enc.data() + pos, 4 * n); pos += 4 * n; };
    auto take64 = [&](std::vector<uint64_t>& v, size_t n) { v.resize(n); if (pos + 8 * n > enc.size()) exit(2); if (n) memcpy(v.data(), enc.data() + pos, 8 * n); pos += 8 * n; };
    if (u32() != 0x5841534Du || u32() != 1) { fprintf(stderr, "not an MSAX encoding\n"); exit(2); }
    const uint32_t nargs = u32(); nch = u32();
    own.resize(nargs);
    for (uint32_t k = 0; k < nargs; k++) {
      const uint32_t op = u32(), nfrac = u32(), nterms = u32();
      One& o = own[k];
      take32(o.form_begin, 2 * nfrac + 1); take32(o.term_col, nterms); take32(o.term_ch, nterms); take32(o.form_ch, 2 * nfrac); take64(o.term_coef, nterms); take64(o.form_const, 2 * nfrac);
      args.push_back(msh_aux_arg{op, nfrac, o.form_begin.data(), o.term_col.data(), o.term_coef.data(), o.term_ch.data(), o.form_const.data(), o.form_ch.data()});
    }
    if (pos != enc.size()) { fprintf(stderr, "MSAX encoding: trailing bytes\n"); exit(2); }
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s tests/golden/linked_v3_tampered.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t buf[65536]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
  fclose(f);
  Reader r(file);
  if (r.u32() != 0x334C534Du || r.u32() != 1) { fprintf(stderr, "not an MSL3 v1 fixture\n"); return 2; }
  const uint32_t field = r.u32(), digest = r.u32(), bits = r.u32(), blowup = r.u32(), steps = r.u32(), w = r.u32(), gb = r.u32(), N = r.u32(), k = r.u32(), folds = r.u32(), nargs = r.u32(), nch = r.u32();
  Air air(r.bytes());
  AuxArgs aux(r.bytes());
  if (digest != MS_DIGEST_SHA256 || aux.args.size() != nargs || (nargs && aux.nch != nch)) { fprintf(stderr, "the fixture's digest is not SHA-256, or its arguments do not decode\n"); return 2; }
  ms_ctx* ctx = nullptr;
  if (ms_create(&ctx, 0, (ms_field)field, MS_FLAG_ZERO_DISPLAY_EMPTY) != MS_OK) { fprintf(stderr, "ms_create failed\n"); return 2; }
  int err = 0;
  msh_stark* h = msh_stark_new(ctx, (int)field, bits, blowup, steps, w, &err);
  if (!h || (gb && msh_stark_set_grinding(h, gb) != MS_OK)) { fprintf(stderr, "msh_stark_new failed (%d)\n", err); return 2; }
  const msh_aux_arg* args = nargs ? aux.args.data() : nullptr;
  int bad = 0;
  const std::vector<uint8_t> base = r.bytes();
  const uint32_t ncases = r.u32();
  uint32_t accepted = 0;
  for (uint32_t cs = 0; cs < ncases; cs++) {
    const std::vector<uint8_t> name = r.bytes();
    const uint32_t cut = r.u32(), append = r.u32(), nedits = r.u32();
    if (cut > base.size()) { fprintf(stderr, "fixture: a cut beyond the proof\n"); return 2; }
    std::vector<uint8_t> proof(base.begin(), base.begin() + cut);
    proof.resize(cut + append, 0);
    for (uint32_t e = 0; e < nedits; e++) {
      const uint32_t at = r.u32();
      const std::vector<uint8_t> put = r.bytes();
      if ((size_t)at + put.size() > proof.size()) { fprintf(stderr, "fixture: an edit beyond the proof\n"); return 2; }
      if (!put.empty()) memcpy(proof.data() + at, put.data(), put.size());
    }
    const int want_rc = (int)r.u32();
    const std::vector<uint8_t> step = r.bytes();
    uint8_t* exact = (uint8_t*)malloc(proof.size() ? proof.size() : 1);   // exactly the proof's bytes: the redzones of the block are the sanitizer's
    if (!proof.empty()) memcpy(exact, proof.data(), proof.size());
    char why[512] = "";
    const int rc = msh_stark_verify_linked_folded(h, &air.a, args, nargs, nch, N, w, (int)k, folds, exact, proof.size(), 1, why, sizeof why);
    free(exact);
    accepted += rc == 1;
    const std::string got(why), want((const char*)step.data(), step.size());
    if (rc != want_rc || got.compare(0, want.size(), want) != 0) {
      fprintf(stderr, "case %.*s: rc %d (recorded %d), why \"%s\" (recorded step \"%s\")\n", (int)name.size(), (const char*)name.data(), rc, want_rc, why, want.c_str());
      bad++;
    }
    char tiny[4] = "";   // a tiny why buffer is respected
    msh_stark_verify_linked_folded(h, &air.a, args, nargs, nch, N, w, (int)k, folds, proof.empty() ? (const uint8_t*)"" : proof.data(), proof.size(), 1, tiny, sizeof tiny);
  }
  msh_stark_free(h);
  ms_destroy(ctx);
  printf("%u cases, %u accepted, %d differ from the fixture\n", ncases, accepted, bad);
  return bad ? 1 : 0;
}
