// Stand-alone sanitizer run of msh_deep_link_verify_folded (include/ministark_host.h), host code that takes untrusted bytes: the MSFF blob and the three opening
// sections of ms_query_linked_folded.  Compiled together with mini-stark_amd/host/stark_host.cpp under -fsanitize=address,undefined (Makefile) and linked against the
// emulation build of the C ABI only because the host library's drivers name it: nothing is proved, no kernel code runs, no context is made.  Reads
// tests/golden/link_folded_tampered.bin (tests/golden/gen_link_folded_tampered.py), gives every section to the verifier in a heap block of exactly its size - a read
// past either end is a sanitizer report - and compares verdict and step with the recorded ones.  Exit status 0: every case as recorded and no report.
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
  void need(size_t n) { if (pos + n > b.size()) { fprintf(stderr, "fixture truncated\n"); exit(2); } }
  uint32_t u32() { need(4); uint32_t v; memcpy(&v, b.data() + pos, 4); pos += 4; return v; }
  uint64_t u64() { need(8); uint64_t v; memcpy(&v, b.data() + pos, 8); pos += 8; return v; }
  std::vector<uint32_t> u32s(size_t n) { std::vector<uint32_t> v(n); for (auto& x : v) x = u32(); return v; }
  std::vector<uint64_t> u64s(size_t n) { std::vector<uint64_t> v(n); for (auto& x : v) x = u64(); return v; }
  std::vector<uint8_t> raw(size_t n) { need(n); std::vector<uint8_t> v(b.begin() + pos, b.begin() + pos + n); pos += n; return v; }
  std::vector<uint8_t> bytes() { const uint32_t n = u32(); return raw(n); }
};

// a heap block of exactly the bytes (one byte when there are none: the verifier is never given a null section)
struct Exact {
  uint8_t* p; size_t n;
  explicit Exact(const std::vector<uint8_t>& v) : p((uint8_t*)malloc(v.size() ? v.size() : 1)), n(v.size()) { if (n) memcpy(p, v.data(), n); }
  ~Exact() { free(p); }
};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s tests/golden/link_folded_tampered.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t buf[65536]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
  fclose(f);
  Reader r(file);
  if (r.u32() != 0x464B534Du || r.u32() != 1) { fprintf(stderr, "not an MSKF v1 fixture\n"); return 2; }
  const uint32_t field = r.u32(), digest = r.u32(), N = r.u32(), blowup = r.u32(), k = r.u32(), c0 = r.u32(), c1 = r.u32(), m = r.u32(), npts = r.u32(), ne = r.u32(), nq = r.u32();
  const uint64_t shift = r.u64();
  const int E = field == MS_FIELD_GOLDILOCKS ? 2 : 4;
  const std::vector<uint32_t> pt_begin = r.u32s(npts + 1), pt_poly = r.u32s(ne);
  const std::vector<uint64_t> z = r.u64s((size_t)npts * E), evals = r.u64s((size_t)ne * E), gamma = r.u64s(E), betas = r.u64s(nq);
  const std::vector<uint8_t> lde_root = r.raw(32), stg_root = r.raw(32), val_root = r.raw(32);
  std::vector<uint8_t> base[4];
  for (auto& s : base) s = r.bytes();
  ms_deep deep{npts, z.data(), pt_begin.data(), pt_poly.data()};
  const uint32_t ncases = r.u32();
  uint32_t accepted = 0; int bad = 0;
  for (uint32_t cs = 0; cs < ncases; cs++) {
    const std::vector<uint8_t> name = r.bytes();
    const uint32_t sec = r.u32(), cut = r.u32(), append = r.u32(), nedits = r.u32();
    if (sec > 3 || cut > base[sec].size()) { fprintf(stderr, "fixture: a section or a cut out of range\n"); return 2; }
    std::vector<uint8_t> t(base[sec].begin(), base[sec].begin() + cut);
    t.resize(cut + append, 0);
    for (uint32_t e = 0; e < nedits; e++) {
      const uint32_t at = r.u32();
      const std::vector<uint8_t> put = r.bytes();
      if ((size_t)at + put.size() > t.size()) { fprintf(stderr, "fixture: an edit beyond the section\n"); return 2; }
      if (!put.empty()) memcpy(t.data() + at, put.data(), put.size());
    }
    const int want_rc = (int)r.u32();
    const std::vector<uint8_t> step = r.bytes();
    const Exact s0(sec == 0 ? t : base[0]), s1(sec == 1 ? t : base[1]), s2(sec == 2 ? t : base[2]), s3(sec == 3 ? t : base[3]);
    char why[512] = "";
    const int rc = msh_deep_link_verify_folded((int)digest, (int)field, 1, N, blowup, shift, (int)k, c0, c1, m, lde_root.data(), c1 ? stg_root.data() : nullptr, val_root.data(), &deep,
                                               evals.data(), gamma.data(), betas.data(), nq, s0.p, s0.n, s1.p, s1.n, s2.p, s2.n, s3.p, s3.n, why, sizeof why);
    accepted += rc == 1;
    const std::string got(why), want((const char*)step.data(), step.size());
    if (rc != want_rc || got.compare(0, want.size(), want) != 0) {
      fprintf(stderr, "case %.*s: rc %d (recorded %d), why \"%s\" (recorded step \"%s\")\n", (int)name.size(), (const char*)name.data(), rc, want_rc, why, want.c_str());
      bad++;
    }
    char tiny[4] = "";   // a tiny why buffer is respected
    msh_deep_link_verify_folded((int)digest, (int)field, 1, N, blowup, shift, (int)k, c0, c1, m, lde_root.data(), c1 ? stg_root.data() : nullptr, val_root.data(), &deep, evals.data(),
                                gamma.data(), betas.data(), nq, s0.p, s0.n, s1.p, s1.n, s2.p, s2.n, s3.p, s3.n, tiny, sizeof tiny);
  }
  printf("%u cases, %u accepted, %d differ from the fixture\n", ncases, accepted, bad);
  return bad ? 1 : 0;
}
