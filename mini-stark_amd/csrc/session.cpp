// session.cpp — context life cycle, device pools, I/O staging, per-kernel profile, and the first stages of Stark::prove: trace commitment (starks.rs:68-73),
// interpolation (air.rs:147-160), constraint polynomials (air.rs:127-144).
#include "ctx.hpp"
#include "running.hpp"

#include <algorithm>

namespace msctx {

template <class F>
int Ctx<F>::profile_end(char* out, size_t cap) {
  static const char* names[K_COUNT] = {"ntt_pass", "scale_pow", "leaf_hash", "inner_hash", "transpose_in", "io_copy", "lincomb", "mix", "eval", "eval_reduce",
                                       "fold", "suffix_horner", "degree", "find_first", "merkle_path", "query_points", "fri_tail", "mix_terms", "mix_air", "air_inv", "aux_running", "grind", "mix_air_ext", "air_check", "deep_combine", "deep_scale"};
  msrt::sync(stream);
  double ms[K_COUNT] = {0}, by[K_COUNT] = {0}, ms_part = 0, ms_repl = 0, repl_by[K_COUNT] = {0}; unsigned long long cnt[K_COUNT] = {0};
  std::map<int, double> sub_ms, sub_by; std::map<int, unsigned long long> sub_cnt;
  for (auto& r : prof_recs) {
    float t = 0.f; msrt::event_elapsed_ms(&t, r.a.get(), r.b.get());
    ms[r.kid] += t; by[r.kid] += r.bytes; cnt[r.kid]++;
    if (r.part) ms_part += t; else { ms_repl += t; repl_by[r.kid] += t; }
    if (r.kid == K_NTT_PASS) { sub_ms[r.sub] += t; sub_by[r.sub] += r.bytes; sub_cnt[r.sub]++; }
  }
  prof_recs.clear(); prof_on = false;
  std::string j = "{";
  for (int k = 0; k < K_COUNT; k++) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s\"%s\": {\"launches\": %llu, \"ms\": %.6f, \"alg_bytes\": %.0f}", k ? ", " : "", names[k], cnt[k], ms[k], by[k]);
    j += buf;
  }
  // per template instance of the NTT pass kernel (matches the kernel names rocprofv3 reports)
  j += ", \"ntt_pass_variants\": {";
  bool first = true;
  for (auto& kv : sub_ms) {
    const int sub = kv.first; char buf[420];
    const char* name = ntt_names[(size_t)sub < ntt_names.size() ? sub : 0].c_str();
    snprintf(buf, sizeof buf, "%s\"%s\": {\"launches\": %llu, \"ms\": %.6f, \"alg_bytes\": %.0f}", first ? "" : ", ", name, sub_cnt[sub], kv.second, sub_by[sub]);
    j += buf; first = false;
  }
  j += "}";
  { char buf[200]; snprintf(buf, sizeof buf, ", \"shard\": {\"world\": %d, \"partitioned_ms\": %.6f, \"replicated_ms\": %.6f, \"replicated_by_kernel\": {", sh_world, ms_part, ms_repl); j += buf;
    bool first_k = true;
    for (int k = 0; k < K_COUNT; k++) if (repl_by[k] > 0) { snprintf(buf, sizeof buf, "%s\"%s\": %.4f", first_k ? "" : ", ", names[k], repl_by[k]); j += buf; first_k = false; }
    j += "}}}"; }
  if (out && cap) { size_t n = j.size() < cap - 1 ? j.size() : cap - 1; memcpy(out, j.data(), n); out[n] = 0; }
  return 0;
}

template <class F>
int Ctx<F>::tabs_host(size_t bytes, u8** out) {
  CK(msrt::sync(stream));                         // an upload out of the area may still be in flight if the stage that issued it left on an error path; free otherwise: the stream is idle here
  if (bytes > h_tabs.cap && h_tabs.alloc(bytes + bytes / 4 + 4096)) return fail(MS_ERR_NOMEM, "page-locked table staging");
  *out = h_tabs.as<u8>();
  return 0;
}

template <class F>
int Ctx<F>::zero_alloc(size_t bytes, void** out) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (!d_zero.p) { if (d_zero.ensure(256 << 10)) return fail(MS_ERR_NOMEM, "zero pool"); zero_cap = 256 << 10; zero_used = zero_cap; }
  if (bytes > zero_cap) return fail(MS_ERR_NOMEM, "zero pool request too large");
  if (zero_used + bytes > zero_cap) { CK(msrt::memset_dev(d_zero.p, 0, zero_cap, stream)); zero_used = 0; }
  *out = d_zero.as<u8>() + zero_used; zero_used += bytes;
  return 0;
}

template <class F>
int Ctx<F>::materialize(int i) {
  if (poly_mat[i]) return 0;
  const Lin& li = poly_lin[i];
  for (int ix : li.idx) RQ(materialize(ix));
  RQ(lincomb_into(d_polys.as<T>(), N, N, li.s.data(), li.idx.data(), (int)li.idx.size(), i, d_polys.as<T>() + (size_t)i * N));
  poly_mat[i] = 1;
  return 0;
}

template <class F>
int Ctx<F>::ensure_polys(size_t count) {
  if (count <= polys_cap) return 0;
  size_t ncap = polys_cap ? polys_cap * 2 : 8;
  while (ncap < count) ncap *= 2;
  DevBuf nb;
  if (nb.ensure(ncap * N * sizeof(T))) return fail(MS_ERR_NOMEM, "polys");
  // what is live moves along: the polynomials, or - between ms_trace_commit and ms_interpolate - the trace columns and the running columns behind them
  const size_t live = have_polys ? (size_t)npolys : (have_trace ? w + (size_t)naux : 0);
  if (d_polys.p && live > 0) { CK(msrt::d2d(nb.p, d_polys.p, live * N * sizeof(T), stream)); CK(msrt::sync(stream)); }
  d_polys = std::move(nb); polys_cap = ncap;
  return 0;
}

template <class F>
int Ctx<F>::init(int dev, u32 flags) {
  device = dev; zae = (flags & MS_FLAG_ZERO_DISPLAY_EMPTY) ? 1 : 0; trace_mont = (flags & MS_FLAG_TRACE_MONT64) ? 1 : 0; fri_overlap = (flags & MS_FLAG_LATENCY) ? 1 : 0; poll_sync = fri_overlap;
  if ((flags & MS_FLAG_DIGEST_BLAKE2S) && (flags & MS_FLAG_DIGEST_BLAKE3)) return fail(MS_ERR_ARG, "ms_create: MS_FLAG_DIGEST_BLAKE2S and MS_FLAG_DIGEST_BLAKE3 exclude each other");
  { const u32 d = flags & (MS_FLAG_DIGEST_BLAKE2S | MS_FLAG_DIGEST_BLAKE3 | MS_FLAG_DIGEST_KECCAK256 | MS_FLAG_DIGEST_SHA3_256); if (d & (d - 1)) return fail(MS_ERR_ARG, "ms_create: the MS_FLAG_DIGEST_* flags exclude each other"); }
  digest = (flags & MS_FLAG_DIGEST_KECCAK256) ? MS_DIGEST_KECCAK256 : (flags & MS_FLAG_DIGEST_SHA3_256) ? MS_DIGEST_SHA3_256
         : (flags & MS_FLAG_DIGEST_BLAKE3) ? MS_DIGEST_BLAKE3 : (flags & MS_FLAG_DIGEST_BLAKE2S) ? MS_DIGEST_BLAKE2S256 : MS_DIGEST_SHA256;
  if (const char* e = getenv("MS_NTT_KMAX")) { int v = atoi(e); if (v >= 5 && v <= msntt::MAX_LOG_R) ntt_kmax = v; }
  if (const char* e = getenv("MS_NTT_FAST")) ntt_fast = atoi(e);
  if (const char* e = getenv("MS_NTT_V2")) ntt_v2 = atoi(e);
  if (const char* e = getenv("MS_NTT_V2_REGPASS")) ntt_v2_regpass = atoi(e);
  if (const char* e = getenv("MS_NTT_SHARE")) ntt_share = atoi(e);
  if (const char* e = getenv("MS_NTT_COOP_WGS")) { int v = atoi(e); if (v >= 8 && v <= 65536) ntt_coop_wgs = v & ~7; }
  if (const char* e = getenv("MS_LDE_LINEAR")) lde_linear = atoi(e);
  if (const char* e = getenv("MS_LAZY_LINCOMB")) lazy_lin = atoi(e);
  if (const char* e = getenv("MS_LDE_MULTI")) lde_multi = atoi(e);
  if (const char* e = getenv("MS_LDE_VIRTUAL")) lde_virtual = atoi(e);
  if (const char* e = getenv("MS_FRI_POINTWISE")) fri_pointwise = atoi(e);
  if (const char* e = getenv("MS_FOLD_SMALL_MAX")) fold_small_max = (size_t)atol(e);
  if (const char* e = getenv("MS_FRI_TAIL_MAX")) fri_tail_max = (size_t)atol(e);
  if (const char* e = getenv("MS_FRI_OVERLAP")) fri_overlap = atoi(e);
  if (const char* e = getenv("MS_SYNC_POLL")) poll_sync = atoi(e);
  if (const char* e = getenv("MS_EVAL_SMALL_MAX")) eval_small_max = (size_t)atol(e);
  if (const char* e = getenv("MS_TREE_SUBTREE_PARENTS")) subtree_parents = (size_t)atol(e);
  if (const char* e = getenv("MS_GRIND_LAUNCH_MAX")) { const long long v = atoll(e); if (v >= 1 && v <= ((long long)1 << 40)) grind_launch_max = (u64)v; }
  if (const char* e = getenv("MS_GRIND_GRID")) { const long v = atol(e); if (v >= 1 && v <= 65536) grind_grid = (unsigned)v; }
  if (const char* e = getenv("MS_AUX_TILE")) { const int v = atoi(e); if (v >= msrun::THREADS && v <= AUX_TILE_DEFAULT && !(v & (v - 1))) aux_tile = v; }
  // the boundary's bulk copies (r04): page-locked trace in / FRI proof out on SDMA engines through the HSA runtime by default (measured with 8 provers in flight,
  // tools/io_probe3.py: resident 251 proofs/s; upload by hipMemcpyAsync 238, by SDMA 251; read-back by hipMemcpyAsync 217-223, by SDMA 242-248; both by SDMA 245.5 = 0.978)
  if (const char* e = getenv("MS_UPLOAD")) upload_sdma = !strcmp(e, "hip") ? 0 : 1;
  if (const char* e = getenv("MS_SDMA_TIMEOUT_S")) { const double v = atof(e); if (v > 0) sdma_timeout_s = v; }
  if (const char* e = getenv("MS_READBACK")) readback_sdma = !strcmp(e, "hip") ? 0 : (!strcmp(e, "sdma-async") ? 1 : 2);   // sdma-async: only ms_fri_proof_read_async on the engine
  if (const char* e = getenv("MS_LEAF_LAZY_MIN")) leaf_lazy_min = atoi(e);
  if (const char* e = getenv("MS_TREE_TOP")) { int v = atoi(e); if (v >= 1 && v <= 65536) tree_top_parents = v; }
  if (const char* e = getenv("MS_SHARD_MIN_LEAVES")) { long v = atol(e); if (v >= 1) shard_min_leaves = (size_t)v; }
  if (const char* e = getenv("MS_SHARD_DIST")) shard_dist = atoi(e);
  if (const char* e = getenv("MS_SHARD_WORLD1")) allow_w1 = atoi(e);
  if (const char* e = getenv("MS_SHARD_STUB")) shard_stub = atoi(e);
  if (const char* e = getenv("MS_SHARD_GATHER_CHUNK")) { long v = atol(e); if (v >= 64) shard_gather_chunk = (size_t)v & ~(size_t)63; }
  if (const char* e = getenv("MS_SHARD_SLICES")) { int v = atoi(e); if (v >= 1 && v <= 64) { shard_slices = v; shard_slices_set = true; } }
  if (const char* e = getenv("MS_SHARD_SLICE_MIN")) { long v = atol(e); if (v >= 1) shard_slice_min = (size_t)v; }
  if (const char* e = getenv("MS_RCCL_MAX_PIECE")) { long long v = atoll(e); if (v >= 64 && v <= ((long long)1 << 30)) rccl_max_piece = (size_t)v & ~(size_t)63; }
  CK(msrt::set_device(dev));
  CK(make(own_stream));
  stream = own_stream.get();
  pinned_cap = 1 << 16;
  CK(pinned.alloc(pinned_cap + Results::SLOT_BYTES, true));   // (+ the slots of the stage results: polled sequence number, word, root)
  *res.seq_slot() = 0;
  if (d_small.ensure(4096) || res.words.ensure(Results::WORD_BYTES)) return fail(MS_ERR_NOMEM, "small");
  CK(msrt::memset_dev(res.words.p, 0, Results::WORD_BYTES, stream));
  CK(msrt::sync(stream));   // (the caller may move the context to a stream of its own)
  return 0;
}

// staged copies between the u64 ABI and device storage
template <class F>
int Ctx<F>::upload_narrow(const u64* host, size_t n, T* dst) {
  if (d_io.ensure(n * 8)) return fail(MS_ERR_NOMEM, "io staging");
  CK(msrt::h2d(d_io.p, host, n * 8, stream));
  typename mspoly::NarrowKernel<F>::Params p{d_io.as<u64>(), dst, n};
  CK(run<mspoly::NarrowKernel<F>>(K_IO, grid1(n, mspoly::THREADS), 1, mspoly::THREADS, 0, p));
  return 0;
}

template <class F>
int Ctx<F>::download_widen(const T* src, size_t n, size_t limb_stride, u32 e, u64* host) {
  if (n == 0) return 0;
  if (d_io.ensure(n * e * 8)) return fail(MS_ERR_NOMEM, "io staging");
  typename mspoly::WidenKernel<F>::Params p{src, d_io.as<u64>(), n, limb_stride, e};
  CK(run<mspoly::WidenKernel<F>>(K_IO, grid1(n * e, mspoly::THREADS), 1, mspoly::THREADS, 0, p));
  CK(msrt::d2h(host, d_io.p, n * e * 8, stream));
  CK(msrt::sync(stream));
  return 0;
}

// ------------------------------------------------------------------ starks.rs:68-73
// row-major u64 matrix (rows x cols, device) -> column-major columns of T, `rows` apart: the range check (bad: a zeroed device word, or null) and the
// Montgomery conversion of MS_FLAG_TRACE_MONT64 ride along
template <class F>
int Ctx<F>::transpose_in(const u64* src, T* dst, size_t rows, size_t cols, T rinv, int mont, u32* bad) {
  typename mspoly::TransposeInKernel<F>::Params tp{src, dst, rows, cols, rows, rinv, mont, bad};
  if (cols >= 16 && rows >= 64) {   // wide traces: 64 x 64 tiles through LDS (coalesced both ways)
    typedef mspoly::TransposeInTiledKernel<F> TK;
    CK(run<TK>(K_TRANSPOSE, (unsigned)(rows / TK::TILE), (unsigned)((cols + TK::TILE - 1) / TK::TILE), TK::THREADS, TK::lds_bytes(), tp));
  } else
  CK(run<mspoly::TransposeInKernel<F>>(K_TRANSPOSE, grid1(rows * cols, mspoly::THREADS), 1, mspoly::THREADS, 0, tp));
  return 0;
}

template <class F>
int Ctx<F>::trace_commit(const u64* trace, bool on_device, size_t N_, size_t w_, size_t lpn, u8* root) {
  if (!trace || !root) return fail(MS_ERR_ARG, "null argument");
  if (!N_ || !w_ || !is_pow2(N_)) return fail(MS_ERR_SHAPE, "trace length must be a power of two (air.rs:23)");
  if (ctz64(N_) > F::TWO_ADICITY) return fail(MS_ERR_SHAPE, "trace domain larger than the field's two-adicity (air.rs:74)");
  TreeShape ts;
  RQ(tree_shape(N_ * w_, lpn, 2, &ts));
  // (the canonical range of the trace is checked by the transposing kernel for host and device input alike: a host-side scan of the N x w matrix
  //  cost ~3 ms of the proving thread per 2^20-row proof, with its stream idle - r04, I/O leg)
  have_trace = have_polys = have_lde = have_validity = have_stg = false; npolys = 0; naux = 0; stg_pending = stg_total = 0; nrounds_done = 0; have_deep = false; blob_size = 0;
  if (N_ != N) { polys_cap = 0; d_polys.release(); }
  N = N_; w = w_;
  const u64* dsrc;
  if (on_device) dsrc = trace;
  else {
    RQ(trace_to_device(trace, &dsrc));   // io.cpp: an SDMA engine for page-locked sources (a prefetched trace is already there), the HIP runtime's copy otherwise
  }
  RQ(ensure_polys(w + 1));
  // 2^-64 mod p: arkworks stores Montgomery representatives (R = 2^64 for the one-limb Fp of both fields)
  const T rinv = f_inv<F>(F::from_u64((u64)(((unsigned __int128)1 << 64) % F::P)));
  // device input cannot be range-checked on the host: the kernel flags elements >= p.  The flag word rides to the host on the tree's last launch, like a round's
  // length word (r05: the 4-byte copy behind the tree cost ~30 us of launch latency per proof); whoever takes it along leaves it zero for the next trace
  unsigned long long* badw = res.word(Results::TRACE_BAD), bad = 0;
  auto stage = res.expect(badw);
  RQ(transpose_in(dsrc, d_polys.as<T>(), N, w, rinv, trace_mont, reinterpret_cast<u32*>(badw)));
  // element f of trace.get_data() = column f % w, row f / w of the column-major copy
  // one proof over several ranks: every rank holds the whole trace, so rank k hashes the contiguous leaf groups [k*M/W, (k+1)*M/W) and only the W subtree roots travel (r04)
  if (sh_on && shard_dist && shardable(ts.leaf_num / ts.lpn)) RQ((tree_build_sharded_contiguous<1>(d_polys.as<T>(), N, 1, 0, (u32)w, ts, d_trace_nodes)));
  else
  RQ((tree_build<1>(d_polys.as<T>(), N, 1, 0, (u32)w, ts, d_trace_nodes)));
  trace_ts = ts;
  RQ(read_root(d_trace_nodes, ts, root, &bad));
  if (bad) return fail(MS_ERR_ARG, "trace element not canonical (>= p)");
  have_trace = true;
  return MS_OK;
}

// ------------------------------------------------------------------ build-defined: ms_aux_running, ms_aux_running_staged (include/ministark.h; kernels: running.hpp)
template <class F>
template <int EA, int SEG>
int Ctx<F>::aux_tile_launch(const T* cols, const void* prog, T* out, T* agg, size_t ntiles, u64* fin, u32* flag) {
  typedef msrun::AuxTileKernel<F, EA, SEG> TK;
  typename TK::Params tp{cols, N, N, reinterpret_cast<const typename TK::Program*>(prog), out, N, agg, ntiles, ntiles == 1 ? fin : nullptr, flag};
  CK(run_coop<TK>(K_AUX, (unsigned)ntiles, TK::THREADS, TK::lds_bytes(), tp));
  return 0;
}

template <class F>
template <int EA>
int Ctx<F>::aux_columns(const char* who, const ms_aux& a, const u32* term_col, const T* cols, size_t ncols, T* out, u64* fin_out) {
  typedef msrun::AuxProgram<F, EA> Program;
  const u32 nforms = 2 * a.nfrac, nterms = a.form_begin[nforms];
  const size_t tile = N < (size_t)aux_tile ? (N < (size_t)msrun::THREADS ? (size_t)msrun::THREADS : N) : (size_t)aux_tile;   // (a trace shorter than the tile: the smallest instance that holds it)
  const size_t ntiles = (N + tile - 1) / tile;
  // d_aux: [0, 8) the zero-denominator flag | [64, 64 + 8 EA) final as u64 limbs | [256, ..) the tile aggregates [EA][ntiles] | the carries [EA][ntiles]
  const size_t off_fin = 64, off_agg = 256, agg_bytes = ((size_t)EA * ntiles * sizeof(T) + 255) & ~(size_t)255;
  if (d_aux.ensure(off_agg + 2 * agg_bytes) || d_tabs.ensure(sizeof(Program) + 64)) return fail(MS_ERR_NOMEM, std::string(who) + " buffers");
  // the program, staged in page-locked memory (tabs_host synchronises the stream first: nothing of an earlier stage still reads the area)
  u8* ht;
  RQ(tabs_host(sizeof(Program) + 64, &ht));
  Program* pg = reinterpret_cast<Program*>(ht);
  memset(pg, 0, sizeof(Program));
  pg->op = a.op; pg->nfrac = a.nfrac;
  for (u32 f = 0; f <= nforms; f++) pg->form_begin[f] = a.form_begin[f];
  for (u32 m = 0; m < nterms; m++) { pg->term_col[m] = term_col[m]; for (int l = 0; l < EA; l++) pg->term_coef[m].c[l] = F::from_u64(a.term_coef[(size_t)m * EA + l]); }
  for (u32 f = 0; f < nforms; f++) for (int l = 0; l < EA; l++) pg->form_const[f].c[l] = F::from_u64(a.form_const[(size_t)f * EA + l]);
  CK(msrt::h2d(d_tabs.p, ht, sizeof(Program), stream));
  u32* flag = d_aux.as<u32>();
  u64* fin = reinterpret_cast<u64*>(d_aux.as<u8>() + off_fin);
  T* agg = reinterpret_cast<T*>(d_aux.as<u8>() + off_agg);
  T* carry = reinterpret_cast<T*>(d_aux.as<u8>() + off_agg + agg_bytes);
  CK(msrt::memset_dev(flag, 0, 8, stream));
  const double row_bytes = (double)N * sizeof(T);
  next_bytes = row_bytes * (double)(ncols + EA);      // (at most: the columns the forms name, and the column out)
  switch (tile / msrun::THREADS) {
    case 1: RQ((aux_tile_launch<EA, 1>(cols, d_tabs.p, out, agg, ntiles, fin, flag))); break;
    case 2: RQ((aux_tile_launch<EA, 2>(cols, d_tabs.p, out, agg, ntiles, fin, flag))); break;
    case 4: RQ((aux_tile_launch<EA, 4>(cols, d_tabs.p, out, agg, ntiles, fin, flag))); break;
    default: RQ((aux_tile_launch<EA, 8>(cols, d_tabs.p, out, agg, ntiles, fin, flag))); break;
  }
  if (ntiles > 1) {
    typedef msrun::AuxCarryKernel<F, EA> CKn;
    typename CKn::Params cp{agg, carry, ntiles, a.op, fin};
    CK(run_coop<CKn>(K_AUX, 1, CKn::THREADS, CKn::lds_bytes(), cp));
    typedef msrun::AuxApplyKernel<F, EA> AK;
    typename AK::Params ap{out, N, N, carry, ntiles, (u32)ctz64(tile), a.op};
    next_bytes = 2 * row_bytes * EA;
    CK(run<AK>(K_AUX, grid1(N, AK::THREADS), 1, AK::THREADS, 0, ap));
  }
  u64 res[8 + 4];   // [flag | 7 words of padding | final]
  CK(msrt::d2h(res, d_aux.p, off_fin + (size_t)EA * 8, stream));
  CK(msrt::sync(stream));
  if (res[0] & 0xFFFFFFFFu) return fail(MS_ERR_SHAPE, std::string(who) + ": a denominator is zero on some row (draw another challenge)");
  for (int l = 0; l < EA; l++) fin_out[l] = res[off_fin / 8 + l];
  return 0;
}

template <class F>
template <int EA>
int Ctx<F>::aux_running_t(const ms_aux& a, u64* final_out, u64* column_out) {
  RQ(ensure_polys(w + (size_t)naux + EA + 1));
  T* out = d_polys.as<T>() + (w + (size_t)naux) * N;
  u64 fin[4];
  RQ(aux_columns<EA>("aux_running", a, a.term_col, d_polys.as<T>(), w, out, fin));
  if (column_out) RQ(download_widen(out, N, N, (u32)EA, column_out));
  for (int l = 0; l < EA; l++) final_out[l] = fin[l];
  naux += EA;
  return MS_OK;
}

template <class F>
int Ctx<F>::aux_args_check(const char* who, const ms_aux& a, size_t used) {
  auto bad = [&](const char* what) { return fail(MS_ERR_ARG, std::string(who) + what); };
  if (a.op > 1) return bad(": op must be MS_AUX_SUM or MS_AUX_PRODUCT");
  if (a.ext != 1 && a.ext != (u32)E) return bad(": ext must be 1 or the extension degree");
  if (a.nfrac < 1 || a.nfrac > (u32)msrun::MAX_FRAC) return bad(": nfrac outside 1..4");
  if (!a.form_begin || !a.form_const) return bad(": null array");
  const u32 nforms = 2 * a.nfrac;
  if (a.form_begin[0] != 0) return bad(": form_begin[0] must be 0");
  for (u32 f = 0; f < nforms; f++) {
    if (a.form_begin[f + 1] < a.form_begin[f]) return bad(": form_begin decreases");
    if (a.form_begin[f + 1] - a.form_begin[f] > (u32)msrun::MAX_FORM_TERMS) return bad(": more than 16 terms in a form");
  }
  const u32 nterms = a.form_begin[nforms];
  if (nterms && (!a.term_col || !a.term_coef)) return bad(": null array");
  for (u32 m = 0; m < nterms; m++) if (a.term_col[m] >= w) return bad(": a term names a column >= w");
  if (!canonical(a.term_coef, (size_t)nterms * a.ext) || !canonical(a.form_const, (size_t)nforms * a.ext)) return bad(": limb not canonical");
  if (used + a.ext > (size_t)msrun::MAX_COLUMNS) return bad(": more than 16 limb columns in all");
  return 0;
}

template <class F>
int Ctx<F>::aux_running(const ms_aux* aux, u64* final_out, u64* column_out) {
  if (!aux || !final_out) return fail(MS_ERR_ARG, "aux_running: null argument");
  if (!have_trace) return fail(MS_ERR_STATE, "aux_running before trace_commit");
  if (have_polys) return fail(MS_ERR_STATE, "aux_running after interpolate: the trace columns have been transformed");
  if (sh_on) return fail(MS_ERR_STATE, "aux_running: not available on a context with sharding on");
  const ms_aux& a = *aux;
  RQ(aux_args_check("aux_running", a, (size_t)naux));
  return a.ext == 1 ? aux_running_t<1>(a, final_out, column_out) : aux_running_t<E>(a, final_out, column_out);
}

// ms_aux_running_staged: the same column, built while the LDE tree of the main columns is live.  The trace columns the forms name exist as polynomials only, so they
// are evaluated on the trace domain again - one forward size-N transform per maximal run of named columns, out of place into d_stg, term_col remapped to its
// slots - the launches of ms_aux_running run over that scratch, and one inverse transform puts the EA limb columns behind the polynomials.  Nothing the LDE tree
// covers is written; the polynomial store may move (ensure_polys), with everything live in it
template <class F>
template <int EA>
int Ctx<F>::aux_running_staged_t(const ms_aux& a, u64* final_out, u64* column_out) {
  const u32 nterms = a.form_begin[2 * a.nfrac];
  std::vector<u32> named(a.term_col, a.term_col + nterms), slot(nterms);
  std::sort(named.begin(), named.end());
  named.erase(std::unique(named.begin(), named.end()), named.end());
  for (u32 m = 0; m < nterms; m++) slot[m] = (u32)(std::lower_bound(named.begin(), named.end(), a.term_col[m]) - named.begin());
  const size_t ns = named.size();
  poly_lin.reserve((size_t)npolys + EA); poly_mat.reserve((size_t)npolys + EA);   // (what the end of the call appends cannot fail any more)
  if (d_stg.ensure((ns + EA) * N * sizeof(T))) return fail(MS_ERR_NOMEM, "aux_running_staged buffers");
  RQ(ensure_polys((size_t)npolys + EA));
  RQ(res.join_side());
  T* scr = d_stg.as<T>(); T* out = scr + ns * N;
  for (size_t i = 0; i < ns;) {   // maximal runs of named columns
    size_t j = i + 1;
    while (j < ns && named[j] == named[j - 1] + 1) j++;
    RQ(ntt_run(ctz64(N), false, d_polys.as<T>() + (size_t)named[i] * N, N, N, scr + i * N, N, j - i));
    i = j;
  }
  u64 fin[4];
  RQ(aux_columns<EA>("aux_running_staged", a, slot.data(), scr, ns, out, fin));
  if (column_out) RQ(download_widen(out, N, N, (u32)EA, column_out));
  RQ(ntt_run(ctz64(N), true, out, N, N, d_polys.as<T>() + (size_t)npolys * N, N, (size_t)EA));
  CK(msrt::sync(stream));   // (include/ministark.h, Streams: the stage returns with nothing in flight - the interpolation above is launched behind aux_columns' wait)
  for (int l = 0; l < EA; l++) { poly_lin.push_back(Lin()); poly_mat.push_back(1); final_out[l] = fin[l]; }
  npolys += EA; stg_pending += EA; stg_total += EA;
  return MS_OK;
}

template <class F>
int Ctx<F>::aux_running_staged(const ms_aux* aux, u64* final_out, u64* column_out) {
  if (!aux || !final_out) return fail(MS_ERR_ARG, "aux_running_staged: null argument");
  if (sh_on) return fail(MS_ERR_STATE, "aux_running_staged: not available on a context with sharding on");
  if (!have_polys || !have_lde || lde_ts.sharded) return fail(MS_ERR_STATE, "aux_running_staged: no committed LDE (ms_lde_commit, and no ms_polys_* since)");
  if (have_stg) return fail(MS_ERR_STATE, "aux_running_staged after lde_commit_stage: one stage per ms_lde_commit");
  if (have_validity) return fail(MS_ERR_STATE, "aux_running_staged after a mix stage: the validity polynomial lies behind the polynomials");
  RQ(aux_args_check("aux_running_staged", *aux, (size_t)naux + (size_t)stg_total));
  return aux->ext == 1 ? aux_running_staged_t<1>(*aux, final_out, column_out) : aux_running_staged_t<E>(*aux, final_out, column_out);
}

// ------------------------------------------------------------------ air.rs:147-160
template <class F>
int Ctx<F>::interpolate() {
  if (!have_trace) return fail(MS_ERR_STATE, "interpolate before trace_commit");
  const size_t cols = w + (size_t)naux;   // the trace columns and the running columns of ms_aux_running behind them
  RQ(ntt_run(ctz64(N), true, d_polys.as<T>(), N, N, d_polys.as<T>(), N, cols));
  poly_lin.assign(cols, Lin());   // (first: if this allocation fails the session keeps no half-set state)
  poly_mat.assign(cols, 1);
  npolys = (int)cols; have_polys = true; have_lde = have_validity = false;
  return MS_OK;
}

template <class F>
int Ctx<F>::polys_lincomb(const u64* s, const int* idx, int k) {
  if (!have_polys) return fail(MS_ERR_STATE, "lincomb before interpolate");
  if (!s || !idx || k < 1) return fail(MS_ERR_ARG, "bad lincomb arguments");
  for (int t = 0; t < k; t++) if (idx[t] < 0 || idx[t] >= npolys || s[t] >= F::P) return fail(MS_ERR_ARG, "lincomb index/scalar out of range");
  RQ(ensure_polys(npolys + 2));
  if (!lazy_lin) RQ(lincomb_into(d_polys.as<T>(), N, N, s, idx, k, npolys, d_polys.as<T>() + (size_t)npolys * N));
  poly_mat.push_back(lazy_lin ? 0 : 1);
  { Lin l; l.s.assign(s, s + k); l.idx.assign(idx, idx + k); poly_lin.push_back(l); }
  npolys++; have_lde = have_validity = false;
  return MS_OK;
}

template <class F>
int Ctx<F>::polys_append(const u64* coeffs, size_t n) {
  if (!have_polys) return fail(MS_ERR_STATE, "append before interpolate");
  if (!coeffs || n > N) return fail(MS_ERR_SHAPE, "constraint polynomial has more than N coefficients (starks.rs:118-119 asserts)");
  if (!canonical(coeffs, n)) return fail(MS_ERR_ARG, "coefficient not canonical");
  RQ(ensure_polys(npolys + 2));
  T* dst = d_polys.as<T>() + (size_t)npolys * N;
  CK(msrt::memset_dev(dst, 0, N * sizeof(T), stream));
  if (n) RQ(upload_narrow(coeffs, n, dst));
  CK(msrt::sync(stream));   // the caller's buffer is only read during the call, and the call returns with nothing in flight, n = 0 included (include/ministark.h)
  poly_mat.push_back(1);
  poly_lin.push_back(Lin());
  npolys++; have_lde = have_validity = false;
  return MS_OK;
}

template <class F>
int Ctx<F>::poly_read(int i, u64* out) {
  if (!have_polys || i < 0 || i >= npolys || !out) return fail(MS_ERR_ARG, "poly_read");
  RQ(materialize(i));
  return download_widen(d_polys.as<T>() + (size_t)i * N, N, 0, 1, out);
}

template <class F>
int Ctx<F>::arith_selftest(int op_word, const u64* a, const u64* b, u64* out, size_t n) {
  // op_word = operation | class << 8.  Which class holds which operation (include/ministark.h); cls becomes the instance that runs it: 1 GL, 2 GLT, 3 GLM, 0 BB
  const int op = op_word & 0xFF;
  int cls = op_word >> 8;
  bool ok = a && b && out && op_word >= 0;
  if (F::ID == 0) {
    const bool own = (op >= 8 && op <= 11) || op == 13 || op == 14 || (op >= 32 && op <= 36);   // GL's own code, whatever the class of the tiles: class 0 or 1
    if (op <= 7) ok = ok && cls <= 3 && !(cls == 1 && (op == 4 || op == 5 || op == 7));   // (compare + select has no mul_x32 / mul_x64 / fold_small; its shift, op 6, is GL::mul_pow2)
    else if (op == 12) ok = ok && (cls == 1 || cls == 2);
    else ok = ok && own && cls <= 1;
    if (cls == 0) cls = (own && op > 11) ? 1 : 3;    // (operations 8-11 of class 0 stay in the instance they have always run in)
  } else {
    ok = ok && cls == 0 && (op <= 3 || op == 14 || op == 15 || (op >= 32 && op <= 38));
  }
  if (!ok) return fail(MS_ERR_ARG, "arith_selftest: bad operation / class / null argument");
  if (op >= 32 && n % F::EXT) return fail(MS_ERR_ARG, "arith_selftest: an extension operation takes whole elements");
  if (!n) return MS_OK;
  if (op != 12 && (!canonical(a, n) || ((op < 6 || op == 15 || op >= 32) && !canonical(b, n)))) return fail(MS_ERR_ARG, "operand not canonical");
  DevBuf d;
  if (d.ensure(3 * n * 8)) return fail(MS_ERR_NOMEM, "arith_selftest");
  auto idle = scope_exit([&] { msrt::sync(stream); });   // (before d goes: a launch may still read it on an early exit)
  CK(msrt::h2d(d.p, a, n * 8, stream));
  CK(msrt::h2d(d.as<u64>() + n, b, n * 8, stream));
  CK(msrt::sync(stream));
  if constexpr (F::ID == 0) {
    if (cls == 1) CK(arith_launch<GL>(op, d.as<u64>(), n));
    else if (cls == 2) CK(arith_launch<GLT>(op, d.as<u64>(), n));
    else CK(arith_launch<GLM>(op, d.as<u64>(), n));
  } else CK(arith_launch<F>(op, d.as<u64>(), n));
  CK(msrt::d2h(out, d.as<u64>() + 2 * n, n * 8, stream));
  CK(msrt::sync(stream));
  return MS_OK;
}

template <class F> template <class A>
int Ctx<F>::arith_launch(int op, u64* buf, size_t n) {
  typedef mspoly::ArithKernel<F, A> AK;
  typename AK::Params ap{buf, buf + n, buf + 2 * n, n, op};
  return run<AK>(K_IO, grid1(n, AK::THREADS), 1, AK::THREADS, 0, ap);
}

// the members this unit defines, for both fields (the other units see declarations only)
#define MS_INSTANTIATE(FF) \
  template int Ctx<FF>::profile_end(char* out, size_t cap); \
  template int Ctx<FF>::tabs_host(size_t bytes, u8** out); \
  template int Ctx<FF>::zero_alloc(size_t bytes, void** out); \
  template int Ctx<FF>::materialize(int i); \
  template int Ctx<FF>::ensure_polys(size_t count); \
  template int Ctx<FF>::init(int dev, u32 flags); \
  template int Ctx<FF>::upload_narrow(const u64* host, size_t n, Ctx<FF>::T* dst); \
  template int Ctx<FF>::download_widen(const Ctx<FF>::T* src, size_t n, size_t limb_stride, u32 e, u64* host); \
  template int Ctx<FF>::transpose_in(const u64* src, Ctx<FF>::T* dst, size_t rows, size_t cols, Ctx<FF>::T rinv, int mont, u32* bad); \
  template int Ctx<FF>::trace_commit(const u64* trace, bool on_device, size_t N_, size_t w_, size_t lpn, u8* root); \
  template int Ctx<FF>::aux_running(const ms_aux* aux, u64* final_out, u64* column_out); \
  template int Ctx<FF>::aux_running_staged(const ms_aux* aux, u64* final_out, u64* column_out); \
  template int Ctx<FF>::interpolate(); \
  template int Ctx<FF>::polys_lincomb(const u64* s, const int* idx, int k); \
  template int Ctx<FF>::polys_append(const u64* coeffs, size_t n); \
  template int Ctx<FF>::poly_read(int i, u64* out); \
  template int Ctx<FF>::arith_selftest(int op, const u64* a, const u64* b, u64* out, size_t n);
MS_INSTANTIATE(GL)
MS_INSTANTIATE(BB)
#undef MS_INSTANTIATE

}  // namespace msctx
