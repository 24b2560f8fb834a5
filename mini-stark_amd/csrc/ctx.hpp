// ctx.hpp — the prover session behind the C ABI (include/ministark.h): one class template per field, Ctx<F>, declared here and DEFINED in
// the translation units below (r05: one 2547-line unit until then; every kernel experiment paid its 2.5-minute rebuild).  A kernel template is
// instantiated - and its device code generated - in the unit that launches it, so the units also partition the device code:
//   session.cpp      ms_create's init, pools, I/O staging, profile, trace_commit / aux_running[_staged] / interpolate / polys_*  (transpose, narrow / widen, running-column kernels)
//   io.cpp           the boundary's bulk transfers: trace in, FRI proof out, on SDMA engines or the HIP runtime; their failure handling
//   air_stages.cpp   constraint columns, LDE commit (and its second stage), mix, the build-defined mix stages (mix_cubic, mix_terms, mix_air:     (lincomb, mix, cubic, terms, air, eval kernels,
//                    one host pipeline, a compose kernel each), the trace-domain check of their program, DEEP-ALI evaluations     the check kernel of air_check.hpp)
//   ntt_plan.cpp     NTT plans (shape, instances, tables), coset evaluation, ms_ntt / ms_coset_lde                        (every NTT pass instance)
//   merkle_tree.cpp  MerkleTree::new, replicated and sharded, ms_merkle_commit; ms_grind                            (leaf / inner kernels of every digest, grind kernels)
//   fri_commit.cpp   FRI commit phase: round commitments, DEEP evaluations, fold, suffix-Horner planning             (fold, scan, degree kernels)
//   fri_query.cpp    FRI query phase, ms_merkle_prove, openings by index (ms_tree_open, ms_fri_query_index, ms_query_linked)   (find-first, path, open, copy kernels)
//   shard.cpp        one proof over several ranks: exchange (RCCL or callback), ms_set_shard*
//   abi.cpp          the extern "C" entry points and their never-unwind guard
// Built with hipcc for gfx950 into libministark.so (csrc/Makefile).  There is no CPU fallback.
#pragma once
#include "../../include/ministark.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "field.hpp"
#include "merkle.hpp"
#include "ntt.hpp"
#include "poly.hpp"

namespace msctx {

// ---- owners.  Whatever the runtime hands out is held by exactly one of these and goes back when its owner dies: they move, they do not copy.
// Memory: a pointer and its capacity, freed by Free.  release() is the deliberate early free.
template <int (*Free)(void*)> struct Owned {
  void* p = nullptr; size_t cap = 0;
  Owned() = default;
  Owned(Owned&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Owned& operator=(Owned&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~Owned() { release(); }
  void release() { if (p) Free(p); p = nullptr; cap = 0; }
  template <class U> U* as() const { return reinterpret_cast<U*>(p); }
};
struct DevBuf : Owned<msrt::free_dev> {
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    size_t want = bytes + bytes / 8 + 256;
    if (msrt::malloc_dev(&p, want)) { p = nullptr; return 1; }
    cap = want;
    return 0;
  }
};
// page-locked host memory, exactly `bytes` of it (coherent: msrt::malloc_host_coherent); what it held is freed first
struct HostBuf : Owned<msrt::free_host> {
  int alloc(size_t bytes, bool coherent = false) {
    release();
    if (coherent ? msrt::malloc_host_coherent(&p, bytes) : msrt::malloc_host(&p, bytes)) { p = nullptr; return 1; }
    cap = bytes;
    return 0;
  }
};
// Handles: a unique_ptr whose deleter is the runtime's destroy call.  make() creates into an EMPTY owner.  Handles that only work together (a stream and its
// events, the two signals of a context) are made into locals and moved into the context when the last one exists: a failure half-way leaves nothing behind
template <class H, int (*Destroy)(H*)> struct Destroyer { void operator()(H* h) const { Destroy(h); } };
typedef std::unique_ptr<msrt::Stream, Destroyer<msrt::Stream, msrt::stream_destroy>> StreamOwner;
typedef std::unique_ptr<msrt::Event, Destroyer<msrt::Event, msrt::event_destroy>> EventOwner;
inline int make(StreamOwner& o) { msrt::Stream* s = nullptr; const int e = msrt::stream_create(&s); if (!e) o.reset(s); return e; }
inline int make(EventOwner& o) { msrt::Event* v = nullptr; const int e = msrt::event_create(&v); if (!e) o.reset(v); return e; }
struct SdmaSignal {
  msrt::Sdma::Signal s{0};
  SdmaSignal() = default;
  SdmaSignal(SdmaSignal&& o) noexcept : s(o.s) { o.s.handle = 0; }
  SdmaSignal& operator=(SdmaSignal&& o) noexcept { if (this != &o) { reset(); s = o.s; o.s.handle = 0; } return *this; }
  ~SdmaSignal() { reset(); }
  void reset() { if (s.handle) msrt::Sdma::get().signal_destroy(s); s.handle = 0; }
  int create() { msrt::Sdma::Signal n{0}; if (msrt::Sdma::get().signal_create(&n)) return 1; reset(); s = n; return 0; }
};

// ---- src/util.rs:4-44 ------------------------------------------------------
inline bool is_pow2(u64 n) { return (n & (n - 1)) == 0; }
inline int ctz64(u64 x) { return x ? __builtin_ctzll(x) : 64; }
inline long log_two_k(u64 number, u64 base) {
  int log_n = ctz64(base);
  if (!is_pow2(number)) return -1;
  int p2 = ctz64(number);
  if (p2 % log_n != 0) return -2;
  return p2 / log_n;
}
inline u64 ceil_log2_k(u64 number, u64 base) {
  if (number == 1) return 1;
  u64 lb = ctz64(base), ln = ctz64(number);
  if (is_pow2(number) && ln % lb == 0) return ln;
  u64 np2 = 64 - __builtin_clzll(number);
  return ((np2 + lb - 1) / lb) * lb;
}

struct CtxBase {
  std::string err;
  // A copy engine did not finish a transfer within the time limit: it may still be reading or writing memory this context (or the caller) owns.  Every later
  // entry point returns MS_ERR_STATE; only ms_destroy is valid, and it waits for the transfer WITHOUT limit before it frees anything.
  bool poisoned = false;
  virtual ~CtxBase() {}
  int digest = MS_DIGEST_SHA256;   // ms_digest_id: the D of every commitment of this context (the MS_FLAG_DIGEST_* flag at ms_create)
  virtual int ext_degree() const = 0;
  virtual void bind_device() const = 0;  // HIP's current device is per host thread: every entry point binds the context's device
  virtual int set_stream(void* s) = 0;
  virtual void* current_stream() const = 0;
  virtual int synchronize() = 0;
  virtual int set_shard(int rank, int world, void* d_send, void* d_recv, size_t cap, ms_exchange_fn fn, void* user) = 0;
  virtual int set_shard_rccl(int rank, int world, const u8* unique_id, size_t cap) = 0;
  virtual int shard_stats(u64* out) = 0;
  virtual int shard_proof_on_root(int on) = 0;
  virtual int shard_round_is_distributed(int r) = 0;
  virtual int shard_proof_is_elsewhere() const = 0;
  virtual int shard_slice_layout(size_t* off, size_t* stride) = 0;
  virtual int rccl_selftest() = 0;
  virtual int trace_commit(const u64* trace, bool on_device, size_t N, size_t w, size_t lpn, u8* root) = 0;
  virtual int trace_upload_async(const u64* trace, size_t N, size_t w) = 0;
  virtual int aux_running(const ms_aux* aux, u64* final_out, u64* column_out) = 0;
  virtual int aux_count() const = 0;
  virtual int aux_running_staged(const ms_aux* aux, u64* final_out, u64* column_out) = 0;
  virtual int aux_staged_count() const = 0;
  virtual int lde_commit_stage(size_t lpn, u8* root) = 0;
  virtual int lde_commit_coset(size_t blowup, u64 shift, int log_arity, u8* root) = 0;
  virtual int lde_commit_stage_coset(int log_arity, u8* root) = 0;
  virtual int validity_commit_coset(int log_arity, u8* root) = 0;
  virtual int query_linked_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) = 0;
  virtual int interpolate() = 0;
  virtual int polys_lincomb(const u64* s, const int* idx, int k) = 0;
  virtual int polys_append(const u64* coeffs, size_t n) = 0;
  virtual int polys_count() const = 0;
  virtual int poly_read(int i, u64* out) = 0;
  virtual int lde_commit(size_t blowup, u64 shift, size_t lpn, u8* root) = 0;
  virtual int lde_read(u64* out) = 0;
  virtual int mix(u64 r) = 0;
  virtual int mix_cubic(u64 r, const int* spec, const u64* sc, int ncons) = 0;
  virtual int mix_terms(u64 r, int ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, const u32* fac_poly, const u32* fac_row, int nexempt) = 0;
  virtual int mix_air(u64 r, const ms_air* air) = 0;
  virtual int mix_air_ext(const u64* r, const ms_air* air) = 0;
  virtual int air_check(const ms_air* air, u64* nfail, u64* cons_count, u64* cons_first_row, u64* bnd_got) = 0;
  virtual int validity_ext_() const = 0;
  virtual size_t validity_len_() const = 0;
  virtual int validity_read(u64* out) = 0;
  virtual int eval_ext(const u64* z, int q, u64* out) = 0;
  virtual int fri_begin(size_t blowup, size_t rounds, u8* root0) = 0;
  virtual int fri_deep(const u64* z, u64* B) = 0;
  virtual int fri_fold_commit(const u64* alpha, u8* root) = 0;
  virtual int fri_round_info(int r, u64* ncoef, u64* D) = 0;
  virtual int fri_round_poly_read(int r, u64* out) = 0;
  virtual int fri_round_codeword_read(int r, u64* out) = 0;
  virtual int fri_query(const u64* betas, int nq, u8* ext_out, size_t ext_cap, size_t* ext_len) = 0;
  virtual size_t fri_proof_size() const = 0;
  virtual int fri_proof_read(u8* out) = 0;
  virtual int fri_proof_read_async(u8* out) = 0;
  virtual int fri_proof_wait() = 0;
  virtual int io_engine() const = 0;
  virtual int merkle_commit(const u64* leafs, size_t leaf_num, int ext, size_t lpn, size_t ic, u8* nodes_out, size_t cap, size_t* nn, u8* root) = 0;
  virtual int merkle_prove(const u64* leafs, size_t leaf_num, int ext, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len) = 0;
  virtual int tree_open(int tree, int round, const u64* index, size_t n, u8* out, size_t cap, size_t* len) = 0;
  virtual int fri_query_index(const u64* betas, int nq, u8* out, size_t cap, size_t* len) = 0;
  virtual int query_linked(const u64* betas, int nq, u8* out, size_t cap, size_t* len) = 0;
  virtual int fri_begin_folded(size_t blowup, int log_arity, u8* root0) = 0;
  virtual int fri_fold_folded(const u64* alpha, u8* root) = 0;
  virtual int fri_fold_final(const u64* alpha, u64* coeffs, size_t cap, size_t* n) = 0;
  virtual int fri_query_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) = 0;
  virtual int fri_folded_refusal(const char* who) = 0;
  virtual int validity_commit(size_t lpn, u8* root) = 0;
  virtual int deep_evals(const ms_deep* deep, u64* evals) = 0;
  virtual int deep_compose(const ms_deep* deep, const u64* gamma) = 0;
  virtual int deep_len_() const = 0;
  virtual int grind(const u8* seed, u32 bits, u64 start, u64 limit, u64* nonce) = 0;
  virtual int ntt(u64* data, size_t n, size_t batch, int inverse) = 0;
  virtual int coset_lde(const u64* coeffs, size_t ncoef, size_t batch, u64 shift, u64* out, size_t L) = 0;
  virtual int bench_lde(size_t blowup, u64 shift) = 0;
  virtual int arith_selftest(int op, const u64* a, const u64* b, u64* out, size_t n) = 0;
  virtual int profile_begin() = 0;
  virtual int profile_end(char* out, size_t cap) = 0;
};

// runs `fn` when the scope ends, however it ends (early return, exception): state the stage functions set around a call that can fail
template <class Fn> struct ScopeExit { Fn fn; ~ScopeExit() { fn(); } };
template <class Fn> inline ScopeExit<Fn> scope_exit(Fn fn) { return ScopeExit<Fn>{fn}; }

#define CK(...) do { int _e = (__VA_ARGS__); if (_e) return this->fail_rt(_e, #__VA_ARGS__); } while (0)
#define RQ(...) do { int _e = (__VA_ARGS__); if (_e) return _e; } while (0)

template <class F> struct Ctx : CtxBase {
  typedef typename F::T T;
  static constexpr int E = F::EXT;
  typedef Ext<F, E> XE;

  int device = 0, zae = 1, trace_mont = 0;
  int lde_linear = 1;  // MS_LDE_LINEAR=0 disables the linear-provenance shortcut of lde_compute (A/B measurements)
  int lde_multi = -1;  // MS_LDE_MULTI: the linear LDE columns in shared sweeps (LincombMultiKernel).  -1 (default): for AIRs of >= 16 polynomials (the wide AIR: 112
                       // launches become 16 and the LDE commit 108.7 -> 105.6 ms, r03); 0 / 1 force it.  Narrow AIRs keep the one-by-one kernel: measured (r02) 45 us less
                       // per Fibonacci proof alone, but 248 -> 240 proofs/s with 8 proofs in flight (five interleaved runs each)
  int tree_top_parents = msmerkle::THREADS;  // MS_TREE_TOP: levels of at most this many parents are walked by one workgroup in one launch (measured: 256 beats 1024 by 3 % in latency)
  int leaf_lazy_min = 16;  // MS_LEAF_LAZY_MIN: leaf groups of at least this many base limbs use the wave-synchronous two-block leaf kernel
  size_t fold_small_max = 131072;  // MS_FOLD_SMALL_MAX (16384 / 131072 / 2^20: within noise of each other with one proof and with eight in flight; 0 is 1.5 % slower with one)
  size_t eval_small_max = (size_t)1 << 19;   // MS_EVAL_SMALL_MAX: polynomials of at most this many coefficients are evaluated 4 coefficients per thread (latency), longer ones 16
  // MS_TREE_SUBTREE_PARENTS: binary-tree levels of at most this many parents run as subtree launches (msmerkle::InnerSubtreeKernel); 0: one launch per level + the fused top.
  // Same-box A/Bs (profiles/r04_small_round_kernels_ab.log), final build, 4 passes: 8 proofs in flight 4096 / 16384 / 65536 -> 258.9 / 260.5 / 254.2 proofs/s, one proof in
  // flight 127.0 / 129.6 / 130.3; against 0 (one launch per level): 4096 -> +0.8 % in flight, +1.2 % alone
  size_t subtree_parents = 16384;
  int fri_pointwise = 1;  // MS_FRI_POINTWISE=0: codewords of FRI rounds >= 1 by NTT of the round polynomial instead of the evaluation-domain fold
  // MEMBER ORDER, the one rule: the context's own stream and its page-locked memory stand in front of every device buffer, so they are destroyed behind them.
  // Freeing device memory waits for the device; until then a launch may still store to the result slots in `pinned` and a copy may still read `h_tabs`.
  StreamOwner own_stream;
  msrt::Stream* stream = nullptr;   // own_stream, or the caller's (ms_set_stream)
  HostBuf pinned; size_t pinned_cap = 0;   // pinned_cap: the staging area; the slots of the stage results lie behind it
  // page-locked staging for the per-proof job tables (r03): uploads out of it are plain DMA, not the runtime's pageable-memory path (which pins or stages the
  // caller's pages on the fly), and need no synchronisation of their own - the area is rewritten by the NEXT proof's same stage, behind that stage's final
  // stream synchronisation
  HostBuf h_tabs;
  int tabs_host(size_t bytes, u8** out);

  // ---- one proof sharded over `sh_world` ranks (ms_set_shard; include/ministark.h)
  int sh_rank = 0, sh_world = 1;
  // sh_on: the sharded code paths are active.  Normally that is world > 1; with MS_SHARD_WORLD1=1 (tests) a ONE-rank "world" runs them too - every exchange degenerates to a
  // transfer to itself, but every kernel, buffer offset, stream ordering and RCCL call of the sharded prover executes, through whole proofs, on one GPU
  bool sh_on = false; int allow_w1 = 0;
  int shard_stub = 0;   // MS_SHARD_STUB=1 (the rank probe): ms_set_shard without a callback = a world without peers, every exchange a device copy of the rank's own payload
  u8* xs = nullptr; u8* xr = nullptr; size_t xcap = 0;   // caller-owned exchange buffers (device)
  ms_exchange_fn xfn = nullptr; void* xuser = nullptr;
  size_t shard_min_leaves = 32768;                        // MS_SHARD_MIN_LEAVES: smaller commitments stay replicated
  void* rccl_comm = nullptr; DevBuf rccl_send, rccl_recv;   // ms_set_shard_rccl: the library owns the communicator and the exchange buffers
  size_t rccl_max_piece = (size_t)1 << 30;                  // MS_RCCL_MAX_PIECE: most bytes of one ncclSend / ncclRecv / ncclAllGather (see exchange)
  u64 xstat[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // calls per op [0..3], bytes sent per op [4..7] (ms_shard_stats)
  int exchange(int op, size_t bytes);
  // one slice of a sliced digest all-to-all: peer r's piece at offset `off + r * stride`, `bytes` long, in both exchange buffers
  int shard_slices = 4; bool shard_slices_set = false; size_t shard_slice_min = 1024;   // (RCCL path: 1 unless MS_SHARD_SLICES is set - ADVICE r3: the two-stream overlap has never run on more than one GPU)
  size_t xl_off = 0, xl_stride = 0;
  StreamOwner comm_stream; struct SliceEvents { EventOwner hashed, exchanged; }; std::vector<SliceEvents> ev_slice;   // (a slice's two events are made, and kept, together)
  int shard_slice_layout(size_t* off, size_t* stride) override { if (!off || !stride) return fail(MS_ERR_ARG, "shard_slice_layout"); *off = xl_off; *stride = xl_stride; return MS_OK; }
  int exchange_slice(size_t off, size_t stride, size_t bytes, int sl, int S);
  void drop_rccl();
  void unshard() { sh_on = false; sh_rank = 0; sh_world = 1; xs = xr = nullptr; xcap = 0; xfn = nullptr; xuser = nullptr; have_lde = false; nrounds_done = 0; blob_size = 0; }
  int set_shard_rccl(int rank, int world, const u8* unique_id, size_t cap) override;
  // The four collectives on a one-rank communicator (send/recv to self, all-gather, both all-reduces) with known payloads:
  // checks the run-time binding of librccl.so (symbols, calling convention of the by-value ncclUniqueId, datatype / op enums)
  // and the stream ordering on a box with a single GPU.
  int rccl_selftest() override;
  int shard_proof_on_root(int on) override { proof_root_only = on ? 1 : 0; return MS_OK; }
  int shard_proof_is_elsewhere() const override { return (proof_root_only && sh_world > 1 && sh_rank != 0 && nrounds_done == fri_rounds && fri_rounds) ? 1 : 0; }
  int shard_round_is_distributed(int r) override { return (r >= 0 && (size_t)r < nrounds_done && rounds[r]->dist) ? 1 : 0; }
  int shard_stats(u64* out) override { if (!out) return fail(MS_ERR_ARG, "shard_stats"); memcpy(out, xstat, sizeof xstat); return MS_OK; }
  bool shardable(size_t leaf_groups) const { return sh_on && leaf_groups >= shard_min_leaves && leaf_groups >= (size_t)sh_world * (size_t)sh_world; }
  int set_shard(int rank, int world, void* d_send, void* d_recv, size_t cap, ms_exchange_fn fn, void* user) override;

  int fail_rt(int e, const char* what) { err = std::string("runtime error ") + std::to_string(e) + " in " + what + ": " + msrt::last_error_string(); return MS_ERR_HIP; }
  int fail(int code, const char* msg) { err = msg; return code; }
  int fail(int code, const std::string& msg) { err = msg; return code; }   // (a shared step's message, prefixed with the entry point that ran it)

  // ---- optional per-kernel timing with HIP events on the launching stream (bench.py roofline leg)
  enum { K_NTT_PASS, K_SCALE_POW, K_LEAF_HASH, K_INNER_HASH, K_TRANSPOSE, K_IO, K_LINCOMB, K_MIX, K_EVAL, K_EVAL_REDUCE, K_FOLD,
         K_SUFFIX_HORNER, K_DEGREE, K_FIND_FIRST, K_PATH, K_QUERY_POINTS, K_FRI_TAIL, K_MIX_TERMS, K_MIX_AIR, K_AIR_INV, K_AUX, K_GRIND, K_MIX_AIR_EXT, K_AIR_CHECK, K_DEEP_COMBINE, K_DEEP_SCALE, K_COUNT };
  struct ProfRec { int kid, sub; EventOwner a, b; double bytes; bool part; };   // (the records of a profile never ended go with the context)
  // sharded proofs: launches inside a PartScope work on this rank's PART of the proof (1 / world of it); everything else is replicated on every rank.
  // ms_profile_end reports both sums: the replicated one bounds the strong scaling (bench.py: sharded.replicated_ms_estimate)
  int part_depth = 0;
  struct PartScope { Ctx* c; explicit PartScope(Ctx* c_) : c(c_) { c->part_depth++; } ~PartScope() { c->part_depth--; } };
  struct PartScopeIf { Ctx* c; bool on; PartScopeIf(Ctx* c_, bool on_) : c(c_), on(on_) { if (on) c->part_depth++; } ~PartScopeIf() { if (on) c->part_depth--; } };
  bool prof_on = false;
  std::vector<ProfRec> prof_recs;
  double next_bytes = 0;  // algorithmic bytes attributed to the next launch
  int next_sub = 0;       // NTT pass template instance of the next launch: index into ntt_names (the kernel names rocprofv3 reports)
  std::vector<std::string> ntt_names{std::string("?")};
  void name_next(const char* name) {
    if (!prof_on) return;
    for (size_t i = 0; i < ntt_names.size(); i++) if (ntt_names[i] == name) { next_sub = (int)i; return; }
    ntt_names.push_back(name); next_sub = (int)ntt_names.size() - 1;
  }
  // ------------------------------------------------------------------ stage results: ONE owner of what a stage brings home
  // Every stage that ends in a host round trip brings home a Merkle root, one 8-byte device word, or just the news that it is done.  The stage's LAST launch stores
  // them in page-locked memory (the host_root / aux_src -> aux_dst / flag fields of its Params) and, under MS_FLAG_LATENCY, raises a sequence number behind them
  // (msrt::HostFlag, rt.hpp) that the host polls instead of synchronising with the stream: 4-5 us less per round trip, 44 of them per proof.
  //   expect   the stage says what it wants; the guard it gets back abandons on every exit that is not a clean collect
  //   attach   called with the Params of the launch that is the stage's last: joins the side stream, fills root slot, word and flag
  //   collect  copies what no launch carried, waits (the polled flag if one is armed and nothing was enqueued behind it, the stream otherwise), hands back root and word
  //   abandon  nothing pending, flag disarmed, the context's stream behind the side stream, the owned word zero
  // The device words that must outlive a zero_alloc piece live here too: one 128-byte line each, zeroed once at ms_create; whoever forwards or copies one leaves it zero.
  int poll_sync = 0;   // MS_FLAG_LATENCY at ms_create (MS_SYNC_POLL=0/1 overrides: A/B)
  struct Results {
    Ctx& c;
    enum Word { FRI_LEN = 0, TAIL_DONE = 128, VALIDITY_LEN = 256, TRACE_BAD = 384, GRIND = 512, WORD_BYTES = 640 };   // round polynomial's length (+ the fused tail's completion counter: ms_fri_begin re-zeroes both lines) | validity polynomial's length | trace range-check flag | ms_grind's found word
    DevBuf words;
    unsigned long long* word(Word w) const { return reinterpret_cast<unsigned long long*>(words.as<u8>() + w); }
    bool owns(const void* p) const { return p >= words.p && p < words.as<u8>() + WORD_BYTES; }
    // page-locked slots behind the staging area, a 64-byte line each (the host spins on the first: the results land on lines of their own): sequence number | word | root
    static constexpr size_t SLOT_BYTES = 192;
    unsigned long long* seq_slot() const { return reinterpret_cast<unsigned long long*>(c.pinned.template as<u8>() + c.pinned_cap); }
    unsigned long long* word_slot() const { return seq_slot() + 8; }
    u32* root_slot() const { return reinterpret_cast<u32*>(seq_slot() + 16); }
    bool open = false, may_poll = false, attached = false, root_sent = false, word_sent = false;
    enum { SIDE_NONE, SIDE_FORKED, SIDE_DONE } side = SIDE_NONE;   // FORKED: launches on the side stream, its event not yet recorded
    unsigned long long* want = nullptr; bool over_ranks = false;
    unsigned long long seq_no = 0, seq_pending = 0, seq_armed = 0;
    int fail_rt(int e, const char* what) { return c.fail_rt(e, what); }
    struct Guard { Results& r; ~Guard() { if (r.open) r.abandon(); } };
    // w: a device word to bring home (over_ranks_: it also rides on a sharded tree's root all-gather and comes back as the maximum over the ranks); poll: the stage's end may be polled
    Guard expect(unsigned long long* w = nullptr, bool over_ranks_ = false, bool poll = true) {
      open = true; want = w; over_ranks = over_ranks_; may_poll = poll; attached = root_sent = word_sent = false; return Guard{*this};
    }
    unsigned long long* shard_word() const { return open && over_ranks ? want : nullptr; }
    // the coefficient side of a FRI round goes to the side stream: call BEHIND expect (the guard then orders the context's stream behind it on every exit)
    // side_done (behind the side stream's last launch) records the event early: it is long up when the join, in front of the stage's last launch, waits for it
    int fork_side() {
      if (!c.side_stream) { StreamOwner s; EventOwner e; CK(make(s)); CK(make(e)); c.side_stream = std::move(s); c.ev_side = std::move(e); }
      side = SIDE_FORKED; return 0;
    }
    int side_done() { if (side == SIDE_FORKED) { CK(msrt::event_record(c.ev_side.get(), c.side_stream.get())); side = SIDE_DONE; } return 0; }
    int join_side() { if (side == SIDE_NONE) return 0; RQ(side_done()); side = SIDE_NONE; CK(msrt::stream_wait_event(c.stream, c.ev_side.get())); return 0; }
    template <class P> int attach(P& p) {   // (outside a stage nobody reads the slots: nothing is attached)
      if (!open) return 0;
      RQ(join_side());
      if constexpr (std::is_same<P, msmerkle::InnerHashParams>::value) { p.host_root = root_slot(); root_sent = true; }
      if (want && !word_sent) { p.aux_src = want; p.aux_dst = word_slot(); word_sent = true; }
      if (may_poll && c.poll_sync && !c.prof_on) { seq_pending = ++seq_no; p.flag = msrt::HostFlag{seq_slot(), seq_pending}; }
      attached = true;
      return 0;
    }
    // every launch of the context reports here: the attached one arms the flag, any other (work enqueued behind the results) and a launch that never ran disarm it
    void launched(bool ran) { seq_armed = ran ? seq_pending : 0; seq_pending = 0; if (attached && !ran) root_sent = word_sent = false; attached = false; }
    int collect(const void* dev_root = nullptr, u8* root = nullptr, unsigned long long* word_out = nullptr) {
      if (!open) return c.fail(MS_ERR_STATE, "stage results collected outside a stage");
      bool behind = side != SIDE_NONE;   // something is enqueued behind the flagged launch: the stream synchronisation it is
      RQ(join_side());
      if (want && !word_sent) { CK(msrt::d2h(word_slot(), want, 8, c.stream)); if (owns(want)) CK(msrt::memset_dev(want, 0, 8, c.stream)); behind = true; }   // (a tree of one leaf group, a scan outside a tree)
      if (dev_root && !root_sent) { CK(msrt::d2h(root_slot(), dev_root, 32, c.stream)); behind = true; }
      const unsigned long long a = behind ? 0 : seq_armed; seq_armed = 0;
      CK(a ? msrt::sync_flag(c.stream, seq_slot(), a) : msrt::sync(c.stream));
      if (root) memcpy(root, root_slot(), 32);
      if (word_out) *word_out = *word_slot();
      open = false; want = nullptr;
      return 0;
    }
    void abandon() {   // (the stage is leaving with an error of its own, or never asked: failures of the calls below are not reported)
      if (side == SIDE_FORKED) msrt::event_record(c.ev_side.get(), c.side_stream.get());
      if (side != SIDE_NONE) msrt::stream_wait_event(c.stream, c.ev_side.get());
      side = SIDE_NONE;
      if (want && owns(want)) msrt::memset_dev(want, 0, 8, c.stream);
      open = attached = false; want = nullptr; seq_pending = seq_armed = 0;
    }
  } res{*this};
  // trimmed length of the validity polynomial: unknown (ms_fri_begin scans), in its device word since ms_mix, on the host once ms_eval_ext has brought it along
  enum { VLEN_RESCAN, VLEN_DEVICE, VLEN_HOST } validity_len_at = VLEN_RESCAN; size_t validity_ncoef = 0;
  // one launch: `go` enqueues it; an empty grid and a failed launch count as never run
  template <class Go> int run_as(int kid, unsigned gx, unsigned gy, const Go& go) {
    int e = 0; bool ran = false;
    if (gx == 0 || gy == 0) ;
    else if (!prof_on) { e = go(); ran = !e; }
    else {
      ProfRec r; r.kid = kid; r.sub = next_sub; r.bytes = next_bytes; r.part = part_depth > 0; next_bytes = 0; next_sub = 0;
      if (make(r.a) || make(r.b)) e = 1;
      else { msrt::event_record(r.a.get(), stream); e = go(); msrt::event_record(r.b.get(), stream); prof_recs.push_back(std::move(r)); ran = !e; }
    }
    res.launched(ran);
    return e;
  }
  template <class K> int run_coop(int kid, unsigned gx, int threads, size_t lds, const typename K::Params& p, unsigned gy = 1) {
    return run_as(kid, gx, gy, [&] { return msrt::launch_coop<K>(stream, gx, gy, threads, lds, p); });
  }
  template <class K> int run(int kid, unsigned gx, unsigned gy, int threads, size_t lds, const typename K::Params& p) {
    return run_as(kid, gx, gy, [&] { return msrt::launch<K>(stream, gx, gy, threads, lds, p); });
  }
  int profile_begin() override { prof_on = true; return 0; }
  int profile_end(char* out, size_t cap) override;

  // ------------------------------------------------------------------ NTT plans
  // A transform is decided ONCE, when its plan is built: the shape (passes, tile rows and columns, the virtual pass) and the kernel instance of every pass
  typedef msntt::PassParams<F> PassParams;
  // One instantiated pass kernel of ntt.hpp (ntt_plan.cpp, pass_instance: the one map from a pass's shape to its instance).  Empty: there is no such instance
  struct Instance {
    char name[96] = "";                                    // the kernel name a profiler reports, from the instance's own constants: the key of the profile's ntt_pass_variants
    bool coop = false; int per_cu = 0;                     // grid: cooperative -> coop_grid(tiles * batch, per_cu) x 1; else own_grid(pp) x batch where set (register pass), tiles x batch
    unsigned (*own_grid)(const PassParams&) = nullptr; bool (*applicable)(const PassParams&) = nullptr;   // applicable: the kernel's own precondition
    int (*launch)(Ctx&, unsigned gx, unsigned gy, const PassParams&) = nullptr;   // run / run_coop of the instance, with its threads and LDS bytes
    explicit operator bool() const { return launch != nullptr; }
  };
  enum Gen { GEN_TILE, GEN_FAST, GEN_COOP, GEN_REG };   // generic round-1 tiles (PassKernel) | compile-time specialised ones (PassKernelK) | PassKernel2 | RegPassKernel (last pass, radix <= 32, registers only)
  static Instance pass_instance(Gen gen, bool inverse, int K, int log_C, int mode);
  struct Pass {
    int K = 0, LC = msntt::TILE_LOG_C; Gen gen = GEN_TILE;   // log2 tile rows and tile columns; the kernel generation
    int log_Rp = 0, log_C = 0;           // log2 of the points done before the pass; the columns its tiles really have (LC, or all that is left outside the rows)
    Instance inst, shared;               // shared: the shared-table instance (MODE 3) a first pass behind the virtual pass may run as instead (pick)
    DevBuf w_r;
  };
  struct Plan {
    int log_n = 0, log_pad = 0, log_r0 = 0, log_rho = 0, npass = 0, lo_bits = 0;
    static constexpr int MAX_PASSES = 7; Pass pass[MAX_PASSES];   // (the smallest MS_NTT_KMAX, 5, at the largest two-adicity, 32)
    DevBuf tw_lo, tw_hi, vtw, w0;
    T n_inv = 0, root = 0;   // root: w_n the tables hold the powers of (host copy: the FRI fold's octet table is derived from it)
    size_t tiles(int k) const { return (size_t)1 << (log_n - pass[k].K - pass[k].log_C); }
    // what the plan alone says about the PassParams of pass k (the caller adds buffers, strides, n_in, batch and scale)
    PassParams params(int k) const {
      PassParams pp{}; pp.log_n = log_n; pp.log_r = pass[k].K; pp.log_Rp = pass[k].log_Rp; pp.log_C = pass[k].log_C; pp.lo_bits = lo_bits;
      pp.log_r0 = k == 0 ? log_r0 : 0; pp.log_rho = k == 0 ? log_rho : 0; pp.last = k == npass - 1; return pp;
    }
  };
  std::map<int, Plan> plans;  // key = (log_n*4 + log_pad)*2 + inverse; complete plans only (get_plan), and a map's elements stay where they are
  int power_table(DevBuf& tab, T w, size_t count, const char* what);   // w^0 .. w^(count-1) in twiddle form -> device
  DevBuf ntt_scratch;
  int ntt_kmax = 9;            // largest tile (log2 rows) of a multi-pass plan; MS_NTT_KMAX overrides (tuning)
  int ntt_v2 = 1, ntt_v2_regpass = 1;   // MS_NTT_V2=0: round-1 kernels only (tests, A/B); MS_NTT_V2_REGPASS: the register-only last pass of 2^21..2^25-point transforms (0: off; 2: tests, on 2^7-row tiles)
  int ntt_fast = 1;            // MS_NTT_FAST=0: no compile-time specialised round-1 tiles (tests)
  // persistent grid of the cooperative pass kernels: two workgroups per CU (their 72-80 KiB of LDS), a multiple of 8 (XCD-aware tile walk)
  int ntt_coop_wgs = 512, ntt_share = 1;   // MS_NTT_SHARE=0: never the shared-table instance (A/B)
  unsigned coop_grid(size_t work_items, int per_cu = 2) const { const size_t g = (size_t)ntt_coop_wgs * per_cu / 2; return (unsigned)(work_items < g ? work_items : g); }
  // log_pad: the input is zero beyond n >> log_pad.  plan_shape: everything but the tables - no device memory, no stream; get_plan: shape, then tables, then publish
  int plan_shape(int log_n, int log_pad, bool inverse, Plan* pl); int get_plan(int log_n, int log_pad, bool inverse, Plan** out);
  // the instance pass k launches for `batch` transforms.  Goldilocks, several columns, enough tiles to feed the persistent grid one tile at a time: the instance that
  // builds the per-tile twiddle tables once per tile for all columns (measured r03: six-column LDE 0.560 -> 0.555 ms; BabyBear 0.333 -> 0.375 ms, so it has none)
  const Instance& pick(const Plan& pl, int k, size_t batch) const {
    const Pass& ps = pl.pass[k]; const size_t tiles = pl.tiles(k);
    return (ps.shared && ntt_share && batch > 1 && tiles >= (size_t)coop_grid(tiles * batch) && (tiles & 7) == 0) ? ps.shared : ps.inst;
  }

  // batch transforms of size 2^log_n: src (n_in valid elements per entry, zero padded) -> dst
  int ntt_run(int log_n, bool inverse, const T* src, size_t src_bstride, size_t n_in, T* dst, size_t dst_bstride, size_t batch);
  int scale_pow(const T* src, size_t src_bstride, T* dst, size_t dst_bstride, size_t n, T s, size_t batch);

  // ------------------------------------------------------------------ pool of zeroed device words
  // Counters that kernels bump (deferred-block lists, the degree result) must start at zero.  One memset clears a 256 KiB
  // pool; zero_alloc hands out fresh pieces of it and clears it again only when it runs out (stream order keeps earlier
  // users ahead of the clear) — a proof needs ~50 such counters, i.e. one memset instead of ~50 four-microsecond fills.
  // CONTRACT: a piece is valid only until the next zero_alloc call on the context (that call may wipe the whole pool): its last reader must be enqueued before
  // then.  A word that has to live longer is one of res.word()'s.
  DevBuf d_zero; size_t zero_used = 0, zero_cap = 0;
  int zero_alloc(size_t bytes, void** out);

  // ------------------------------------------------------------------ Merkle
  // sharded (ms_set_shard): this rank holds the subtree over leaf groups [rank*Mloc, (rank+1)*Mloc) followed by the replicated top
  // (world subtree roots and the levels above); local_nodes = nodes held here, root last in both cases
  struct TreeShape { size_t leaf_num = 0, lpn = 0, ic = 0, levels = 0, nodes = 0, local_nodes = 0, Mloc = 0; bool sharded = false; };
  // src/merkle.rs:89-118 (shape checks and node count)
  int tree_shape(size_t leaf_num, size_t lpn, size_t ic, TreeShape* ts);
  // leaf-group digests of `ngroups` groups into `out`: LeafHashKernel + (a family that defers them: SHA-256) the compacted pad-only blocks; the family by the context's digest (msmerkle::with_digest)
  template <int EL>
  int leaf_hash(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, size_t lpn, size_t ngroups, u32* out,
                size_t g_first = 0, u32 run_len = 0, u32 run_stride = 0, const msmerkle::LinColSpec* lin = nullptr, size_t out_g0 = 0);
  template <int EL>
  int tree_build(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, const TreeShape& ts, DevBuf& nodes, const msmerkle::LinColSpec* lin = nullptr);
  // inner levels above `nchildren` digests at nodes[0..): level-major, root last (merkle.rs:131-140)
  // `final_levels`: these levels end in the tree's root: their last launch is the stage's last (res.attach)
  int inner_levels(u32* nodes, size_t nchildren, size_t ic, bool final_levels = true, u8* rec_out = nullptr);
  int inner_launch(unsigned grid, const msmerkle::InnerHashParams& ip);
  // Sharded MerkleTree::new over a binary tree of M = leaf_num/lpn leaf groups, of which this rank hashes the groups
  // j = rank + W*i found at local group index i of the view (base, strides): digest all-to-all, subtree, root all-gather, top.
  template <int EL>
  int tree_build_sharded(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, TreeShape& ts, DevBuf& nodes, const msmerkle::LinColSpec* lin = nullptr);
  // the subtree over this rank's Mloc contiguous leaf digests (at nodes[0..)), the all-gather of the W subtree roots, the replicated top.
  // res.shard_word() (a device word, optional): rides on the root all-gather; every rank gets the maximum over the ranks back in the same word.
  int finish_sharded_tree(TreeShape& ts, DevBuf& nodes, size_t Mloc);
  // MerkleTree::new over data EVERY rank holds (the raw trace): rank k hashes the contiguous leaf groups [k*M/W, (k+1)*M/W) - no digest exchange at all -
  // builds that subtree, and the ranks all-gather the W subtree roots
  template <int EL>
  int tree_build_sharded_contiguous(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, TreeShape& ts, DevBuf& nodes);
  // root of the tree built LAST on this context (every caller reads it right behind the build): the stage's collect
  int read_root(const DevBuf& nodes, const TreeShape& ts, u8* root, unsigned long long* word_out = nullptr) { return res.collect(nodes.as<u8>() + (ts.local_nodes - 1) * 32, root, word_out); }

  // ------------------------------------------------------------------ session state
  size_t N = 0, w = 0, L = 0, blowup = 0;
  int npolys = 0; size_t polys_cap = 0;
  struct Lin { std::vector<u64> s; std::vector<int> idx; };   // provenance of polynomial i: a linear combination of earlier ones (empty: none)
  std::vector<Lin> poly_lin;
  // r04, linear provenance carried through the coefficient domain: a polynomial ms_polys_lincomb defined is not computed when it is defined.  Its LDE column is the
  // combination of the computed LDE columns (as before), the mix is ONE linear combination of the polynomials without provenance with the scalars
  // sum_i r^i * (coefficient of that polynomial in f_i), and its DEEP-ALI value is the same combination of the opened values - exact field arithmetic, so every
  // output is bit-identical.  The coefficient vector is materialised on demand only (ms_poly_read, MS_LDE_LINEAR=0).  MS_LAZY_LINCOMB=0: computed at definition (r03).
  std::vector<char> poly_mat; int lazy_lin = 1;
  void expand(int i, T scale, std::map<int, T>& acc) const {   // f_i as a combination of the polynomials without provenance
    const Lin& li = poly_lin[i];
    if (li.idx.empty()) { auto it = acc.find(i); if (it == acc.end()) acc[i] = scale; else it->second = F::add(it->second, scale); return; }
    for (size_t t = 0; t < li.idx.size(); t++) expand(li.idx[t], F::mul(scale, F::from_u64(li.s[t] % F::P)), acc);
  }
  int materialize(int i);
  bool have_trace = false, have_polys = false, have_lde = false, have_validity = false;
  DevBuf d_trace[2], d_polys, d_coef, d_lde, d_trace_nodes, d_lde_nodes, d_io, d_partials, d_small;
  TreeShape trace_ts, lde_ts;
  size_t lde_c = 0;

  // dist (one proof over several ranks, r04): the round polynomial is worked on BY COEFFICIENT RANGE - rank k owns the coefficients [k*S, (k+1)*S), S = D / (blowup * world).
  // Round 0 keeps the whole (replicated) validity polynomial in `poly` and every rank uses its range of it; later rounds hold only their own S coefficients
  // (local_store: limb l of coefficient k*S + i at poly[l*S + i]).
  struct Round { DevBuf poly, cw, nodes; size_t cap = 0, ncoef = 0, D = 0; TreeShape ts; size_t m = 0; /* sharded: local codeword = limbs x 2 cosets x m */
                 bool dist = false, local_store = false; size_t S = 0;
                 bool base_cw = false; /* the codeword's limbs >= 1 are identically zero (round 0: transform of a base-field polynomial) */ };
  size_t shard_gather_chunk = 0;
  int shard_dist = 1;          // MS_SHARD_DIST=0: the coefficient-domain work of a sharded proof stays replicated on every rank (r03 behaviour; A/B and tests)
  int proof_root_only = 0;     // ms_shard_proof_on_root: the FRI proof blob is assembled on rank 0 only
  const T* lpoly(const Round* r) const { return r->local_store ? r->poly.template as<T>() : r->poly.template as<T>() + (size_t)sh_rank * r->S; }
  size_t lstride(const Round* r) const { return r->local_store ? r->S : r->cap; }
  size_t lcount(const Round* r, size_t n) const { const size_t lo = (size_t)sh_rank * r->S; return n <= lo ? 0 : (n - lo < r->S ? n - lo : r->S); }
  // chunk of a distributed round polynomial on a domain of D points (0: the round stays replicated): the commitment must be sharded and the chunk even
  size_t dist_chunk(size_t D) const {
    if (!sh_on || !shard_dist || !fri_blowup || !shardable(D / 2)) return 0;
    const size_t den = fri_blowup * (size_t)sh_world;
    if (D % den) return 0;
    const size_t S = D / den;
    return (S >= 2 && !(S & 1)) ? S : 0;
  }
  DevBuf d_carry, d_lq, d_pack, d_fullpoly;
  std::vector<std::unique_ptr<Round>> rounds; size_t nrounds_done = 0, fri_rounds = 0, fri_blowup = 0;
  bool have_deep = false; XE cur_z; XE cur_B[2];
  DevBuf d_folded, d_sh, d_blob, d_tabs, d_targets, d_idx, d_ovf;
  size_t blob_size = 0;

  int ensure_polys(size_t count);

  int init(int dev, u32 flags);
  // Only what needs an order, in front of every member's own destructor: the communicator goes while its streams exist, and transfers still in flight read or write
  // memory the members free - wait for them, however long it takes (a poisoned context got here exactly because one did not finish in time)
  ~Ctx() {
    drop_rccl();
    if (sdma_pending) msrt::Sdma::get().wait(sdma_sig.s, -1.0);
    else if (copy_pending) msrt::event_sync(ev_copy.get());
    if (up.pending) msrt::Sdma::get().wait(sdma_up_sig.s, -1.0);
    if (side_stream) msrt::sync(side_stream.get());
  }
  int ext_degree() const override { return E; }
  void bind_device() const override { msrt::set_device(device); }
  // A HAND-OVER POINT: everything enqueued before the switch happens before everything enqueued after it.  ms_interpolate, ms_mix, ms_polys_lincomb (MS_LAZY_LINCOMB=0)
  // and ms_bench_lde return with launches in flight that write d_polys, d_lde or the validity-length word, which the next stage reads on whatever stream it finds: the
  // stream being left is drained here, and with it the side stream (every stage joins it back before it returns; an error exit may not have) and a sharded context's
  // communication stream.  No handle is needed, and naming the stream the context is on already costs nothing.  The switch happens even when the drain fails (the
  // caller destroyed the stream it had lent): the error is reported, and the context is not left on a dead stream.
  int set_stream(void* s) override {
    msrt::Stream* next = s ? reinterpret_cast<msrt::Stream*>(s) : own_stream.get();
    int e = 0;
    if (next != stream) {
      e = msrt::sync(stream);
      if (side_stream) { const int e2 = msrt::sync(side_stream.get()); if (!e) e = e2; }
      if (comm_stream) { const int e2 = msrt::sync(comm_stream.get()); if (!e) e = e2; }
    }
    stream = next; zero_used = zero_cap;
    if (e) return fail_rt(e, "ms_set_stream: draining the stream being left (the context is on the new stream)");
    return 0;
  }
  void* current_stream() const override { return stream; }
  int synchronize() override { CK(msrt::sync(stream)); return 0; }

  static unsigned grid1(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

  // staged copies between the u64 ABI and device storage
  int upload_narrow(const u64* host, size_t n, T* dst);
  int transpose_in(const u64* src, T* dst, size_t rows, size_t cols, T rinv, int mont, u32* bad);
  int download_widen(const T* src, size_t n, size_t limb_stride, u32 e, u64* host);
  static bool canonical(const u64* v, size_t n) { for (size_t i = 0; i < n; i++) if (v[i] >= F::P) return false; return true; }

  // ------------------------------------------------------------------ starks.rs:68-73
  int trace_commit(const u64* trace, bool on_device, size_t N_, size_t w_, size_t lpn, u8* root) override;
  // ------------------------------------------------------------------ build-defined: running columns of permutation / lookup arguments (include/ministark.h; kernels: running.hpp)
  // naux limb columns sit behind the w trace columns of d_polys until ms_interpolate transforms them with the trace.  d_aux: [flag word | final, E u64 | tile
  // aggregates | carries]; the flag is a word of its own (not the zero pool, which may be wiped between the launch that sets it and the copy that reads it)
  int naux = 0;
  static constexpr int AUX_TILE_DEFAULT = 2048;
  int aux_tile = AUX_TILE_DEFAULT;   // MS_AUX_TILE: rows per workgroup of the tile launch, a power of two from 256 up to the default (each value its own kernel instance)
  DevBuf d_aux;
  int aux_running(const ms_aux* aux, u64* final_out, u64* column_out) override;
  int aux_count() const override { return naux; }
  template <int EA> int aux_running_t(const ms_aux& a, u64* final_out, u64* column_out);
  template <int EA, int SEG> int aux_tile_launch(const T* cols, const void* prog, T* out, T* agg, size_t ntiles, u64* fin, u32* flag);
  // what both entry points ask of a descriptor (`used`: the limb columns there are already), and the launches they share: the program with `term_col` as its column
  // indices over `cols` (N apart), the column into `out` (limb l at + l * N), final into fin[0..EA) - or MS_ERR_SHAPE for a zero denominator - behind one synchronisation
  int aux_args_check(const char* who, const ms_aux& a, size_t used);
  template <int EA> int aux_columns(const char* who, const ms_aux& a, const u32* term_col, const T* cols, size_t ncols, T* out, u64* fin);
  // ------------------------------------------------------------------ build-defined: the staged LDE commitment (include/ministark.h).  Running columns built AFTER ms_lde_commit
  // - their challenges may depend on the LDE root - become polynomials behind the c0 = lde_c0 committed ones (ms_aux_running_staged: stg_pending of them, not in any tree yet);
  // ms_lde_commit_stage evaluates them into the columns c0 .. of d_lde and builds a second tree (d_stg_nodes) over that L x c1 view.  From then on lde_c = c0 + c1: the mix
  // stages, the DEEP stage and ms_lde_read see all columns, MS_TREE_LDE still opens rows of c0.  The staged tree lives and dies with the LDE tree (stg_live); one stage per
  // ms_lde_commit.  d_stg: the forward transform of the trace polynomials a descriptor names, and the column before its inverse transform
  int stg_pending = 0, stg_total = 0;   // limb columns staged and not committed | staged since ms_trace_commit (the limit of 16 counts them with naux)
  size_t lde_c0 = 0; bool have_stg = false;
  DevBuf d_stg, d_stg_nodes; TreeShape stg_ts;
  bool stg_live() const { return have_stg && have_lde; }
  int aux_running_staged(const ms_aux* aux, u64* final_out, u64* column_out) override;
  int aux_staged_count() const override { return stg_pending; }
  template <int EA> int aux_running_staged_t(const ms_aux& a, u64* final_out, u64* column_out);
  int lde_commit_stage(size_t lpn, u8* root) override;
  // ------------------------------------------------------------------ build-defined: coset-grouped row trees (include/ministark.h).  The `_coset` twins of ms_lde_commit,
  // ms_lde_commit_stage and ms_validity_commit differ in the tree alone: L / a leaf groups, a = 2^k, group j = the a rows j + t L / a of the folded FRI's round-0 coset,
  // column-major (element col * a + t) - the leaf kernels' own view with width = lpn = a * c and col_stride = L / a.  *_ck: the k of the live tree, 0 for a plain one
  int lde_ck = 0, stg_ck = 0, val_ck = 0;
  int lde_commit_k(size_t blowup_, u64 shift, size_t lpn, int k, u8* root);
  int lde_commit_stage_k(size_t lpn, int k, u8* root);
  int validity_commit_k(size_t lpn, int k, u8* root);
  int coset_arity_check(const char* who, int k, size_t L_);   // MS_ERR_ARG: k outside 1..3; MS_ERR_STATE: sharding on; MS_ERR_SHAPE: L < 2a
  int coset_leaf_check(const char* who, size_t lpn);          // MS_ERR_ARG: BLAKE3 and a leaf message that may exceed 16 KiB (leaf_hash's rule, asked before anything changes)
  bool linear_columns_would_be_virtual() const;               // finish_linear_columns' decision, without its effects
  int lde_commit_coset(size_t blowup_, u64 shift, int log_arity, u8* root) override;
  int lde_commit_stage_coset(int log_arity, u8* root) override;
  int validity_commit_coset(int log_arity, u8* root) override;
  // ------------------------------------------------------------------ air.rs:147-160
  int interpolate() override;
  int polys_lincomb(const u64* s, const int* idx, int k) override;
  int polys_append(const u64* coeffs, size_t n) override;
  int polys_count() const override { return npolys; }
  int poly_read(int i, u64* out) override;

  // ------------------------------------------------------------------ starks.rs:80-95
  // one lincomb launch chain: dst = sum_t s[t] * base[idx[t]] over n elements (columns `stride` apart)
  int lincomb_into(const T* base, size_t stride, size_t n, const u64* sc, const int* idx, int k, int self_index, T* dst);
  // The LDE columns of all polynomials with linear provenance (columns `stride` apart, n elements each).  Consecutive ones whose sources
  // are all transformed columns (no linear column among them) and fit LincombMultiKernel (<= 4 outputs over <= 8 distinct sources) share
  // one sweep; anything else goes through lincomb_into one by one.
  int lincomb_linear_columns(T* base, size_t stride, size_t n);
  // starks.rs:80-91.  The coset evaluation is linear, so a polynomial that ms_polys_lincomb defined as
  // sum_t s_t * P_idx[t] has LDE column sum_t s_t * LDE(P_idx[t]): only polynomials without such provenance
  // (the trace columns, ms_polys_append uploads) go through the NTT.
  int lde_compute(size_t blowup_, u64 shift);
  // The linear LDE columns: VIRTUAL when every one of them is a combination of at most LIN_MAXT stored (transformed) columns - the leaf-hash kernel
  // then evaluates them row by row while it hashes (they are never read again: the query phase opens FRI codewords only) and ms_lde_read materialises
  // them on demand; otherwise written out by the lincomb kernels.  MS_LDE_VIRTUAL: -1 (default) for AIRs of >= 16 polynomials, 0 never, 1 always.
  // Measured r03: wide AIR (64 linear columns of 2^25 rows) LDE commit 105.5 -> 103.6 ms - the 20 ms of lincomb launches go away, but the leaf kernel reads
  // its source columns again (out of L2 by then) and multiplies; Fibonacci AIR with 8 proofs in flight 239 -> 233 proofs/s (the prover is bound by its VALU
  // instruction count, and the leaf kernel's grew): so narrow AIRs keep the lincomb kernels.
  int lde_virtual = -1; bool lde_cols_virtual = false; size_t lde_col_stride = 0, lde_col_len = 0;
  DevBuf d_lin;
  int finish_linear_columns(size_t stride, size_t n);
  const msmerkle::LinColSpec* lde_lin() const { return lde_cols_virtual ? d_lin.as<msmerkle::LinColSpec>() : nullptr; }
  // Evaluations of `batch` polynomials (ncoef coefficients each) on this rank's share of the size-2^log_D domain shift*<w_D>:
  // the rows g*(rank + W*i) + t (t < g, i < m = D/(g*W)) — g cosets of <w_m> — land at dst[b*dst_bstride + t*m + i].
  int coset_eval(const T* coef, size_t coef_bstride, size_t ncoef, int log_D, T shift, size_t g, T* dst, size_t dst_bstride, size_t batch);
  // lde_compute for a sharded proof: column i of the local LDE (rows rank + W*j) at d_lde + i*m, m = L/W
  int lde_compute_sharded(size_t blowup_, u64 shift);
  int lde_commit(size_t blowup_, u64 shift, size_t lpn, u8* root) override;
  int bench_lde(size_t blowup_, u64 shift) override;
  int arith_selftest(int op, const u64* a, const u64* b, u64* out, size_t n) override;
  template <class A> int arith_launch(int op, u64* buf, size_t n);   // one operation of class A on buf = a | b | out, n words each
  int lde_read(u64* out) override;
  // ------------------------------------------------------------------ starks.rs:108-119
  int mix(u64 r) override;
  // build-defined degree-3 composition with the true quotient (include/ministark.h; kernel: mspoly::CubicComposeKernel)
  size_t validity_len = 0; u64 lde_shift = 0; DevBuf d_cubic;
  size_t validity_len_() const override { return have_validity ? validity_len : 0; }
  // limbs per coefficient of the validity polynomial: 1 (base field: every mix stage but ms_mix_air_ext) or E, limb l of the coefficients at + l * validity_len
  int validity_ext = 1;
  int validity_ext_() const override { return have_validity ? validity_ext : 0; }
  int mix_cubic(u64 r, const int* spec, const u64* sc, int ncons) override;
  // build-defined composition of any degree: constraints as sums of monomials over the polynomials, in CSR arrays (include/ministark.h; kernel: mspoly::ComposeTermsKernel)
  int mix_terms(u64 r, int ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, const u32* fac_poly, const u32* fac_row, int nexempt) override;
  // build-defined AIR composition: ms_mix_terms plus per-constraint exemption sets, periodic columns and boundary constraints (include/ministark.h; kernels:
  // mspoly::ComposeAirKernel, mspoly::CosetInvKernel).  d_air_inv holds D[i] = 1 / (x_i - 1) over the LDE domain, built for the first program with boundary
  // constraints and kept while (N, blowup, shift) stay what it was built for
  DevBuf d_air_inv; bool air_inv_valid = false; size_t air_inv_N = 0, air_inv_blowup = 0; u64 air_inv_shift = 0;
  int mix_air(u64 r, const ms_air* air) override;
  // ms_mix_air with r in the extension (kernel: mspoly::ComposeAirExtKernel): the same gate, checks, sizes and tables, the program as segments with K weights
  int mix_air_ext(const u64* r, const ms_air* air) override;
  // ms_mix_air's program regrouped for ComposeAirKernel: filled by air_validate, read by air_layout and air_table
  struct AirProgram {
    u32 nterms = 0, nfacs = 0;
    std::vector<u32> deg;                    // per constraint: the most factors of any of its terms
    std::vector<u32> per_off;                // offsets of the periodic columns' tables in the device table, in elements: column k has blowup * q_k entries
    std::vector<std::vector<u32>> sets;      // the distinct exemption sets, sorted: one transition group each
    std::vector<u32> set_of;                 // per constraint: its set
    std::vector<u32> brows, brow_of;         // the distinct boundary rows (one boundary group each); per boundary constraint: its row's index
  };
  struct AirLayout { size_t VL, ngroups, tterms, tfacs, off_t, off_f, off_x, off_p, off_d, bytes; };   // [groups | terms | factors | exemption roots | periodic tables | den_inv]
  int air_validate(const ms_air& a, AirProgram& pg, size_t c);   // c: the polynomials (columns) an index may name
  int air_layout(const ms_air& a, const AirProgram& pg, AirLayout& lay);
  void air_table(u64 r, const ms_air& a, const AirProgram& pg, const AirLayout& lay, const std::vector<T>& dinv, u8* tab);
  // the table of ComposeAirExtKernel: [groups | segments | terms | factors | exemption roots | periodic tables | den_inv]; the last three as air_table writes them
  struct AirLayoutExt { size_t nsegs, tterms, tfacs, off_s, off_t, off_f, off_x, off_p, off_d, bytes; };
  AirLayoutExt air_layout_ext(const ms_air& a, const AirProgram& pg, const AirLayout& lay) const;
  void air_table_ext(const XE& r, const ms_air& a, const AirProgram& pg, const AirLayoutExt& lx, const std::vector<T>& dinv, u8* tab);
  void air_periodic_tables(const ms_air& a, const AirProgram& pg, T* hp);   // periodic column k on the domain, at hp + pg.per_off[k] (both tables)
  int air_inv_table(T gL_step);
  // build-defined, diagnostic: the same program on the ROWS of the trace domain (include/ministark.h; kernel: mspoly::AirCheckKernel, air_check.hpp) - per constraint the
  // number of violating rows and the first one, per boundary constraint the value the trace has.  Before ms_interpolate the kernel reads the columns of d_polys as
  // they stand; afterwards one forward transform of all polynomials into d_chk_eval first.  Buffers of its own: nothing another stage reads is written
  DevBuf d_chk_eval, d_chk_tab;
  int air_check(const ms_air* air, u64* nfail, u64* cons_count, u64* cons_first_row, u64* bnd_got) override;
  // ---- the pipeline the three build-defined mix stages share (air_stages.cpp): gate, [the stage's own checks and host table], upload, [its compose launch], finish.
  // `who` is the entry point, for the messages
  int mix_gate(const char* who, u64 r);
  // 1 / (x^N - 1) on the LDE coset, blowup values: x^N - 1 is shift^N * zeta^(i mod blowup) - 1 there, zeta = g_L^N.  Refuses a coset that meets the trace domain
  int coset_vanishing_inv(const char* who, std::vector<T>& dinv);
  // what ms_mix_terms and ms_mix_air ask of the CSR term arrays; *d = the most factors of any term (deg_per_constraint, when given and zeroed: the same per constraint)
  int check_term_program(const char* who, u32 ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, u32* deg_per_constraint, u32* d);
  // virtual LDE columns written out, d_cubic / d_tabs sized, the host table staged and copied to d_tabs
  int upload_mix_table(const char* who, const u8* tab, size_t bytes, size_t ne = 1);
  // d_cubic's evaluations (ne limb planes of L) -> the validity polynomial of VL coefficients behind the constraint polynomials (limb l at + l * VL), or MS_ERR_SHAPE
  // with `refusal` when the division was not exact
  int finish_mix(const char* refusal, size_t VL, int ne = 1);
  // trimmed length of a base-field coefficient vector
  int degree_launch1(const T* poly, size_t n, unsigned long long** dres_out);
  int validity_read(u64* out) override;

  // evaluate `npoly` polynomials (views) at ext point z into dst as [npoly][E] T.  stage_end: the caller's LAST evaluation - its final launch is the stage's (res.attach)
  template <int EC>
  int eval_views(const T* base, size_t poly_stride, size_t limb_stride, size_t kstride, const size_t* off, const size_t* count, int npoly, const XE& z, T* dst, bool stage_end = false);
  template <int EC, int ITEMS>
  int eval_views_i(const T* base, size_t poly_stride, size_t limb_stride, size_t kstride, const size_t* off, const size_t* count, int npoly, const XE& z, T* dst, size_t maxc, bool stage_end);
  static bool load_ext(const u64* v, XE* out) { for (int l = 0; l < E; l++) { if (v[l] >= F::P) return false; out->c[l] = F::from_u64(v[l]); } return true; }

  // sharded proof: out[i] = sum_r part_r[i] * zstep^r for n extension elements of the all-gathered partials (rank r's payload rank_stride limbs apart, the elements from `off` on)
  int shard_combine_launch(size_t off, size_t rank_stride, u32 n, const XE& zstep, T* out);
  // DEEP-ALI evaluations by coefficient range (r04): rank k evaluates the coefficients [k*Sx, (k+1)*Sx) of every polynomial at every point, ONE all-gather of the partial
  // sums, and every rank combines them with z^Sx
  bool dist_eval() const { return sh_on && shard_dist && N >= shard_min_leaves && N >= (size_t)sh_world * 2; }
  // the polynomials the DEEP-ALI kernels evaluate: those whose coefficients exist, then the validity polynomial (index npolys); the lazily defined ones get their
  // values on the host as the combination their provenance names (eval_finish)
  std::vector<int> eval_set() const { std::vector<int> ev; for (int i = 0; i < npolys; i++) if (poly_mat[i]) ev.push_back(i); ev.push_back(npolys); return ev; }
  // page-locked results [q][ev.size()][E] -> out [q][npolys + 1][E] (u64)
  int eval_finish(int q, const std::vector<int>& ev, u64* out);
  int eval_ext_sharded(const u64* z, int q, u64* out);

  // ------------------------------------------------------------------ starks.rs:124-151
  int eval_ext(const u64* z, int q, u64* out) override;

  // ------------------------------------------------------------------ FRI rounds (fri.rs:314-352)
  Round* round_slot(size_t i) { while (rounds.size() <= i) rounds.push_back(std::make_unique<Round>()); return rounds[i].get(); }
  // codeword + tree of rounds[i] from its coefficient limbs (ncoef_in valid coefficients)
  // `nonzero_limbs`: limbs >= this are identically zero (round 0: extend_poly embeds base coefficients), so their
  // transform is all zeros and is not computed
  // `prev` != nullptr: the codeword is folded out of prev's codeword in the evaluation domain (FriFoldEvalKernel / FriFoldWgKernel) instead of
  // transforming the round polynomial — same values, a quarter of the arithmetic
  int round_commit(Round* r, size_t ncoef_in, int nonzero_limbs = E, const Round* prev = nullptr, const XE* alpha = nullptr);
  // trimmed length of a round polynomial (DegreeKernel) into a zeroed device word
  int degree_launch(const T* poly, size_t limb_stride, size_t n, unsigned long long** dres_out);
  // fri.rs:73-82
  int fri_begin(size_t blowup_, size_t nrounds, u8* root0) override;
  // fri.rs:89-94
  int fri_deep(const u64* z, u64* B) override;

  // ---- suffix Horner job planning (shared by the DEEP quotient and the query quotients).
  // A logical job (view, m, z, out, h0) expands into one kernel job per level; level buffers
  // (aggregates = input of the level above, carries = output of the level above) come from d_sh.
  typedef mspoly::SHJob<F, E> SHJ;
  typedef mspoly::SuffixHornerKernel<F, E> SHK;
  struct SHPlan { int nl; std::vector<SHJ> agg; std::vector<SHJ> fin; bool has_top_agg = false; SHJ top_agg; size_t P = 0; bool dist = false; };  // agg[l] for l < nl-1, fin[l] for l < nl
  // (P = BS^nl: where the kernel places a carry-in of the top level, in elements of the job)
  static size_t sh_scratch_elems(size_t m) {
    const size_t BS = mspoly::SH_BS;
    size_t tot = 0, cur = m;
    for (;;) { size_t nb = cur ? (cur + BS - 1) / BS : 1; tot += 2 * nb * E; if (nb <= 1) break; cur = nb; }
    return tot;
  }
  // `scratch` must hold sh_scratch_elems(m) elements of T
  // ext_carry (E limbs, device): carry-in of the top level (a rank of a sharded proof: the suffix sum over the higher ranks, scaled - ShardCarryKernel);
  // top_agg (E limbs, device): the job's aggregate over all its elements, stored by one extra AGG launch of the top level; out_h0: see SHJob
  SHPlan sh_plan(const T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const XE& z,
                 void* out, bool out_u64, size_t out_limb_stride, size_t out_off, size_t out_stride, T* h0, T* scratch,
                 const T* ext_carry = nullptr, T* top_agg = nullptr, bool out_h0 = false);
  // z^(m - P) = (1/z)^(P - m): moves a top-level carry-in from the padded position P to the job's end m (0 for z = 0: nothing then carries over)
  static XE carry_scale(const XE& z, size_t m, size_t P) { return e_pow<F, E>(e_inv<F>(z), (u64)(P - m)); }
  int sh_launch_inline(const SHJ& j, int final_mode);
  int sh_launch_table(const SHJ* d_jobs, size_t njobs, size_t maxnb, int final_mode);
  int shard_carry_table(const mspoly::CarryJob<F, E>* d_jobs, size_t njobs);
  // one logical job, launched level by level with the job inline in the kernel arguments
  int suffix_horner(const T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const XE& z,
                    T* out, size_t out_limb_stride, size_t out_off, size_t out_stride, T* h0);

  // all-gather of a distributed round polynomial's parts into one replicated vector (dst: E limbs, dst_stride apart, `count` coefficients)
  int gather_poly(const T* local, size_t S, size_t count, T* dst, size_t dst_stride);
  // fri.rs:96-101 on a DISTRIBUTED round polynomial (r04): rank k folds its own coefficient pairs, runs the suffix Horner of (folded - B(alpha)) / (x - z) over its
  // own range with the sum over the higher ranks as carry-in (one all-gather of [first folded element | aggregate] per rank, ShardCarryKernel), and ends up with
  // its range [k*S', (k+1)*S') of the quotient = the next round polynomial, S' = S/2.  If the next round is too small to stay distributed the parts are
  // all-gathered into a replicated polynomial.  H_j for j in (lo, hi) comes from the rank's own job over f[lo+1 .. hi); H_hi = q_(hi-1) IS the carry-in.
  int fold_dist(Round* pr, Round* nr, const XE& a, size_t* nq_coef_out);
  // fri.rs:96-109
  int fri_fold_commit(const u64* alpha, u8* root) override;
  // MS_FRI_TAIL_MAX: rounds folding a domain of at most this many points run as ONE launch (fri_tail.hpp; 0: never).  Same-box A/B: DESIGN.md
  size_t fri_tail_max = (size_t)1 << 15;   // (8192 / 32768 / 131072: within noise of each other alone and with eight in flight, profiles/r05_fri_tail_ab.log; 2^15 = every replicated round of a sharded proof at the default MS_SHARD_MIN_LEAVES)
  // MS_FLAG_LATENCY (r05): the coefficient side of a round's ms_fri_fold_commit (fold, DEEP quotient scan, trimmed length: ~55 us of small launches) on a SIDE stream
  // while the evaluation side (pointwise codeword, leaf hashing, tree) runs on the context's stream - the two are independent (the codeword never reads the
  // quotient); the launch that forwards root and length word to the host waits for the side stream's event.  The fused tail rounds do the same inside one kernel.
  int fri_overlap = 0;   // MS_FLAG_LATENCY at ms_create (MS_FRI_OVERLAP=0/1 overrides: A/B)
  StreamOwner side_stream; EventOwner ev_side;   // (made together, forked and joined by `res`)
  struct StreamScope { Ctx* c; msrt::Stream* keep; StreamScope(Ctx* c_, msrt::Stream* s) : c(c_), keep(c_->stream) { c->stream = s; } ~StreamScope() { c->stream = keep; } };
  int fri_tail_round(Round* pr, Round* nr, const XE& a, bool* done);
  template <class DG> int fri_tail_round_t(Round* pr, Round* nr, const XE& a, bool* done);   // DG: the kernel family of `digest` (msmerkle::with_digest, digest.hpp)
  int fri_round_info(int r, u64* ncoef, u64* D) override;
  int fri_round_poly_read(int r, u64* out) override;
  int fri_round_codeword_read(int r, u64* out) override;
  // ------------------------------------------------------------------ build-defined: folded FRI (include/ministark.h; kernel: mspoly::FriFoldArityKernel, host side: fri_commit.cpp,
  // the query phase: fri_query.cpp).  fri_k = log2 of the arity while the FRI state is in folded mode: rounds[i] then holds codeword and tree of round i only (no
  // polynomial), its tree over the coset view (width = lpn = a, col_stride = D_i / a), ncoef the bound D_i / blowup.  The mode lives as long as the rounds do: whatever
  // zeroes nrounds_done ends it.  fold_fin: the final polynomial (cap = its limb stride D_R, ncoef = nfinal) once ms_fri_fold_final has run
  int fri_k = 0; bool fold_final_done = false; Round fold_fin; DevBuf d_fold_cw;
  bool folded() const { return fri_k != 0 && nrounds_done != 0; }
  int fri_folded_refusal(const char* who) override { return folded() ? fail(MS_ERR_STATE, std::string(who) + ": the FRI state is in folded mode (ms_fri_begin_folded)") : 0; }
  int fold_arity_launch(const Round* pr, const XE& a, T* dst);   // ONE launch: pr's codeword folded by 2^fri_k at `a` into dst (limbs pr->D >> fri_k apart)
  int coset_tree(Round* r);                                      // the tree over r's codeword, one coset of the next fold per leaf group
  int fri_begin_folded(size_t blowup_, int log_arity, u8* root0) override;
  int fri_fold_folded(const u64* alpha, u8* root) override;
  int fri_fold_final(const u64* alpha, u64* coeffs, size_t cap, size_t* n) override;
  int fri_query_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) override;

  // ------------------------------------------------------------------ fri.rs:115-189
  // The whole query phase is a fixed handful of batched launches, whatever the number of
  // rounds and queries: every per-(window, query) step is a job in a device-side table.
  // ext_out != nullptr (ms_fri_query_into): the query-phase kernels write the MSFP blob straight into the caller's buffer - page-locked host
  // memory (ms_pinned_alloc; hipHostMalloc memory is mapped into the device's address space) or device memory - instead of d_blob:
  // no read-back copy afterwards (r02: the runtime executed most of the 64 MiB read-back as shader copies, -15 % on the I/O-inclusive rate)
  bool blob_external = false;
  int fri_query(const u64* betas, int nq, u8* ext_out, size_t ext_cap, size_t* ext_len) override;
  // what the steps of one query phase share (fri_query.cpp): blob layout, host-side job tables, their offsets in the one uploaded table area
  struct QueryPlan {
    typedef mspoly::CarryJob<F, E> CJ; typedef mspoly::FindJob<F, E> FJ; typedef msmerkle::PathJob<F, E> PJ; typedef msmerkle::ShardPathJob<F, E> SPJ;
    size_t W = 0; int nq = 0; size_t pos = 0; u8* blob = nullptr;
    T* d_h0 = nullptr; T* d_tg = nullptr; unsigned long long* d_ix = nullptr;          // H_0 outputs of the scans | find-first targets | found leaf indices
    std::vector<size_t> rec_off, path_off; std::vector<u64> qlen; std::vector<T> x1h;
    std::vector<std::vector<SHJ>> tables; std::vector<int> table_mode, table_part; size_t n_agg_tables = 0;   // launch order: every aggregate launch, then - behind the carry exchange - every final launch
    std::vector<CJ> carry_jobs; bool any_dist = false;                                 // sharded proofs: carry-ins of the ranks' scan jobs
    std::vector<msmerkle::CopyJob> unp; std::vector<size_t> unp_first, unp_cnt, chunk_c0, chunk_len;   // ... and the slices' way into the blob, chunk by chunk
    std::vector<FJ> fjobs; std::vector<PJ> pjobs; std::vector<SPJ> sjobs; std::vector<msmerkle::CopyJob> cjobs; size_t stage_bytes = 0;
    std::vector<size_t> toff; size_t off_f = 0, off_p = 0, off_sp = 0, off_cj = 0, off_rec = 0, off_ql = 0, off_x1 = 0, off_cr = 0, off_un = 0; const u8* dt = nullptr;
  };
  int query_layout(QueryPlan& q, int nq);
  int query_build(QueryPlan& q, const u64* betas);
  int query_scans(QueryPlan& q);
  int query_shard_assembly(QueryPlan& q);
  int query_openings(QueryPlan& q);
  size_t fri_proof_size() const override { return blob_size; }
  int fri_proof_read(u8* out) override;
  // The same copy on the context's COPY stream, ordered behind the query phase by an event: the call returns at once and the next proof's
  // stages run while the ~64 MiB travel; the next ms_fri_query waits (on the device, not on the host) for the copy before it rewrites the blob.
  StreamOwner copy_stream; EventOwner ev_blob, ev_copy; bool copy_pending = false;   // (the three are made together: all or none)
  // r04: the read-back as an explicit SDMA copy through the HSA runtime (rt.hpp, msrt::Sdma) - queued on a copy engine whatever the engines' load, never a
  // blit kernel; completion is an HSA signal the host waits on (ms_fri_proof_wait, or the next ms_fri_query before it rewrites the blob).  MS_READBACK=hip keeps
  // hipMemcpyAsync on the copy stream (A/B); io_engine() reports which path the last read-back took.
  int readback_sdma = 2, sdma_gpu = -1, sdma_state = 0 /* 0 untried, 1 bound, 2 unavailable */, last_io_engine = 0;
  SdmaSignal sdma_sig, sdma_up_sig; bool sdma_pending = false; int upload_sdma = 1;   // (both or neither: sdma_state == 1 means both)
  u8* readback_dst = nullptr; size_t readback_bytes = 0;   // destination and size of the read-back in flight (a FAILED engine copy is redone through the HIP runtime)
  double sdma_timeout_s = 20.0;        // MS_SDMA_TIMEOUT_S: how long a stage waits for a copy engine before it poisons the context
  bool sdma_ready();
  int poison(const char* what);        // -> MS_ERR_HIP now, MS_ERR_STATE from every later entry point
  int io_engine() const override { return last_io_engine; }
  int fri_proof_read_async(u8* out) override;
  int fri_proof_wait() override;
  // ---- the trace's way in (r05): two device buffers; ms_trace_upload_async queues the SDMA copy of the NEXT proof's trace into the one the current proof does not
  // use, ms_trace_commit of that trace finds it there (it waits for the signal - long since 0 - instead of for the whole transfer)
  struct Upload { const u64* src = nullptr; size_t N = 0, w = 0; int slot = 0; bool pending = false; } up;
  int trace_slot = 0;                  // the buffer the last ms_trace_commit read
  int trace_upload_async(const u64* trace, size_t N_, size_t w_) override;
  int trace_to_device(const u64* trace, const u64** dsrc);
  int upload_wait(const char* what);   // completes the upload in flight: 0 arrived, MS_ERR_HIP poisoned (timeout), 1 = the engine reported failure (the caller copies again)

  // ------------------------------------------------------------------ standalone entry points
  int merkle_commit(const u64* leafs, size_t leaf_num, int ext, size_t lpn, size_t ic, u8* nodes_out, size_t cap, size_t* nn, u8* root) override;
  // src/merkle.rs:272-288 on a standalone binary tree: leaves de-interleaved to SoA limbs, then the same
  // LeafHash / InnerHash / FindFirst / MerklePath kernels the FRI query phase uses
  template <int EL>
  int merkle_prove_t(const u64* leafs, size_t leaf_num, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len);
  int merkle_prove(const u64* leafs, size_t leaf_num, int ext, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len) override;
  // ------------------------------------------------------------------ build-defined: Merkle openings by index (include/ministark.h; kernel: msmerkle::OpenKernel, host side: fri_query.cpp)
  // ms_tree_open, ms_fri_query_index and ms_query_linked: a host-built job table through the page-locked staging area, ONE launch, the bytes copied to the caller.  Buffers of their own
  // (d_open: job table | output), nothing another stage reads is written.  `view`: the leaf view and the nodes of a tree this context holds, or why there is none
  DevBuf d_open;
  struct OpenView { const T* base = nullptr; size_t col_stride = 0, row_stride = 0, limb_stride = 0; const msmerkle::LinColSpec* lin = nullptr; const u32* nodes = nullptr;
                    size_t ngroups = 0; u32 width = 1, lpn = 1, nlevels = 0; int el = 1;
                    size_t path_bytes() const { return 8 + (size_t)lpn * el * 8 + 8 + (size_t)nlevels * 64; } };
  int open_view(int tree, int round, OpenView* v);
  void open_jobs(const OpenView& v, const u64* index, size_t n, bool positions, size_t off, std::vector<msmerkle::OpenJob<F>>& jobs) const;
  int open_launch(const std::vector<msmerkle::OpenJob<F>>& jobs, size_t out_bytes, const Round* fin, u8* out);
  int msfi_plan(const u64* betas, int nq, u64 hd[6], size_t* body, std::vector<msmerkle::OpenJob<F>>* jobs);
  int tree_open(int tree, int round, const u64* index, size_t n, u8* out, size_t cap, size_t* len) override;
  int fri_query_index(const u64* betas, int nq, u8* out, size_t cap, size_t* len) override;
  int query_linked(const u64* betas, int nq, u8* out, size_t cap, size_t* len) override;
  // the FRI part of both folded query phases: the MSFF header into hd, the size of the blob behind it into *body (the final polynomial, then the rounds' paths), and
  // (jobs != nullptr) the openings, their offsets counted from the final polynomial's first byte
  int msff_plan(const u64* betas, int nq, u64 hd[7], size_t* body, std::vector<msmerkle::OpenJob<F>>* jobs);
  int query_linked_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) override;
  // ------------------------------------------------------------------ build-defined: the composition commitment and the DEEP stage (include/ministark.h; kernels:
  // mspoly::DeepCombineKernel, mspoly::DeepSumScaleKernel; host side: air_stages.cpp).  The validity polynomial's ve limb planes of VL coefficients are m = ve * VL / N
  // chunk columns of N coefficients, column k * ve + l = coefficients [kN, (k+1)N) of plane l: views of the polynomial where it lies, behind the constraint polynomials.
  // d_vlde holds their evaluations on the LDE coset (column j' at + j' * L), d_vlde_nodes the tree over its rows.  The tree lives while have_validity and have_lde
  // do and no mix stage has run since (vtree_live); the DEEP polynomial D' (d_deep: limb l at + l * N) lives at most as long.
  bool have_vtree = false, have_dpoly = false;
  DevBuf d_vlde, d_vlde_nodes, d_deep, d_deep_w, d_deep_tab;
  TreeShape vtree_ts; size_t vtree_m = 0;
  bool vtree_live() const { return have_vtree && have_validity && have_lde; }
  bool dpoly_live() const { return have_dpoly && vtree_live(); }
  void drop_vtree() { have_vtree = have_dpoly = false; }
  size_t chunk_off(size_t j) const { const size_t ve = (size_t)validity_ext; return (size_t)npolys * N + (j % ve) * validity_len + (j / ve) * N; }   // chunk column j in d_polys
  struct DeepPlan { std::vector<XE> z; std::vector<u32> pt_of; size_t entries = 0; };
  int deep_check(const char* who, const ms_deep* d, DeepPlan& pl);
  int validity_commit(size_t lpn, u8* root) override;
  int deep_evals(const ms_deep* deep, u64* evals) override;
  int deep_compose(const ms_deep* deep, const u64* gamma) override;
  int deep_len_() const override { return dpoly_live() ? (int)N : 0; }
  // ------------------------------------------------------------------ build-defined: proof-of-work grinding (include/ministark.h; kernel: grind.hpp, host side: merkle_tree.cpp)
  u64 grind_launch_max = (u64)1 << 30;   // MS_GRIND_LAUNCH_MAX: most nonces of one launch
  unsigned grind_grid = 0;               // MS_GRIND_GRID: workgroups of a launch (0: by the device's compute units at the kernel's occupancy)
  int grind(const u8* seed, u32 bits, u64 start, u64 limit, u64* nonce) override;
  int ntt(u64* data, size_t n, size_t batch, int inverse) override;
  int coset_lde(const u64* coeffs, size_t ncoef, size_t batch, u64 shift, u64* out, size_t L_) override;
};

inline CtxBase* B(ms_ctx* c) { return reinterpret_cast<CtxBase*>(c); }
inline const CtxBase* B(const ms_ctx* c) { return reinterpret_cast<const CtxBase*>(c); }

}  // namespace msctx
