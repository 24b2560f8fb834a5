// air_stages.cpp — constraint columns by linear provenance, coset LDE + commitment (starks.rs:80-95), constraint mixing (starks.rs:108-119; build-defined ms_mix_cubic,
// ms_mix_terms, ms_mix_air and ms_mix_air_ext: one host pipeline - gate, table, upload, compose launch, finish_mix - and a compose kernel each), DEEP-ALI evaluations (starks.rs:124-151).
#include "ctx.hpp"
#include "air_check.hpp"

#include <algorithm>

namespace msctx {

// ------------------------------------------------------------------ starks.rs:80-95
// one lincomb launch chain: dst = sum_t s[t] * base[idx[t]] over n elements (columns `stride` apart)
template <class F>
int Ctx<F>::lincomb_into(const T* base, size_t stride, size_t n, const u64* sc, const int* idx, int k, int self_index, T* dst) {
  for (int t = 0; t < k;) {  // MAX_TERMS terms per launch; launches after the first spend one slot on the partial result
    typename mspoly::LincombKernel<F>::Params p;
    p.polys = base; p.stride = stride; p.n = n; p.dst = dst;
    int kk = 0;
    if (t > 0) { p.s[kk] = F::from_u64(1); p.idx[kk] = self_index; kk++; }  // accumulate onto the partial result
    for (; t < k && kk < mspoly::MAX_TERMS; t++, kk++) { p.s[kk] = F::from_u64(sc[t]); p.idx[kk] = idx[t]; }
    p.k = kk;
    CK(run<mspoly::LincombKernel<F>>(K_LINCOMB, grid1(n, mspoly::THREADS), 1, mspoly::THREADS, 0, p));
  }
  return 0;
}

// The LDE columns of all polynomials with linear provenance (columns `stride` apart, n elements each).  Consecutive ones whose sources
// are all transformed columns (no linear column among them) and fit LincombMultiKernel (<= 4 outputs over <= 8 distinct sources) share
// one sweep; anything else goes through lincomb_into one by one.
template <class F>
int Ctx<F>::lincomb_linear_columns(T* base, size_t stride, size_t n) {
  const size_t c = (size_t)npolys;
  typedef mspoly::LincombMultiKernel<F> MK;
  typename MK::Params mp; int nout = 0, nsrc = 0;
  auto flush = [&]() -> int {
    if (!nout) return 0;
    mp.polys = base; mp.stride = stride; mp.n = n; mp.nout = nout; mp.nsrc = nsrc;
    next_bytes = (double)(nout + nsrc) * n * sizeof(T);
    int e = run<MK>(K_LINCOMB, grid1(n, mspoly::THREADS), 1, mspoly::THREADS, 0, mp);
    nout = nsrc = 0;
    return e;
  };
  for (size_t i = 0; i < c; i++) {
    const Lin& li = poly_lin[i];
    if (li.idx.empty()) continue;
    bool simple = (lde_multi < 0 ? c >= 16 : lde_multi != 0) && li.idx.size() <= (size_t)mspoly::LCM_SRC;
    for (int ix : li.idx) if (ix < 0 || (size_t)ix >= c || !poly_lin[ix].idx.empty()) simple = false;   // a source that is itself a linear column: keep the order
    if (simple) {
      for (int attempt = 0; attempt < 2; attempt++) {
        int map[mspoly::LCM_SRC], ns = nsrc; bool fits = nout < mspoly::LCM_OUT;
        int srcs[mspoly::LCM_SRC]; for (int u = 0; u < nsrc; u++) srcs[u] = mp.src[u];
        for (size_t t = 0; fits && t < li.idx.size(); t++) {
          int u = 0; while (u < ns && srcs[u] != li.idx[t]) u++;
          if (u == ns) { if (ns == mspoly::LCM_SRC) { fits = false; break; } srcs[ns++] = li.idx[t]; }
          map[t] = u;
        }
        if (!fits) { CK(flush()); continue; }   // second attempt on an empty group always fits (<= LCM_SRC terms)
        for (int u = nsrc; u < ns; u++) mp.src[u] = srcs[u];
        for (int u = 0; u < mspoly::LCM_SRC; u++) mp.m[nout][u] = 0;
        for (size_t t = 0; t < li.idx.size(); t++) mp.m[nout][map[t]] = F::add(mp.m[nout][map[t]], F::from_u64(li.s[t] % F::P));   // a column named twice: coefficients add up
        mp.dst[nout] = base + i * stride;
        nsrc = ns; nout++;
        break;
      }
    } else {
      CK(flush());
      RQ(lincomb_into(base, stride, n, li.s.data(), li.idx.data(), (int)li.idx.size(), (int)i, base + i * stride));
    }
  }
  CK(flush());
  return 0;
}

// starks.rs:80-91.  The coset evaluation is linear, so a polynomial that ms_polys_lincomb defined as
// sum_t s_t * P_idx[t] has LDE column sum_t s_t * LDE(P_idx[t]): only polynomials without such provenance
// (the trace columns, ms_polys_append uploads) go through the NTT.
template <class F>
int Ctx<F>::lde_compute(size_t blowup_, u64 shift) {
  const size_t c = (size_t)npolys;
  const size_t L_ = N * blowup_;
  if (d_coef.ensure(c * N * sizeof(T)) || d_lde.ensure(c * L_ * sizeof(T))) return fail(MS_ERR_NOMEM, "lde");
  if (!lde_linear) for (size_t i = 0; i < c; i++) RQ(materialize((int)i));
  const T sh = F::from_u64(shift);
  for (size_t i = 0; i < c;) {  // maximal runs of polynomials that need a transform
    if (lde_linear && !poly_lin[i].idx.empty()) { i++; continue; }
    size_t j = i;
    while (j < c && !(lde_linear && !poly_lin[j].idx.empty())) j++;
    RQ(scale_pow(d_polys.as<T>() + i * N, N, d_coef.as<T>() + i * N, N, N, sh, j - i));
    RQ(ntt_run(ctz64(L_), false, d_coef.as<T>() + i * N, N, N, d_lde.as<T>() + i * L_, L_, j - i));
    i = j;
  }
  if (lde_linear) RQ(finish_linear_columns(L_, L_));
  return 0;
}

template <class F>
int Ctx<F>::finish_linear_columns(size_t stride, size_t n) {
  const size_t c = (size_t)npolys;
  lde_cols_virtual = false; lde_col_stride = stride; lde_col_len = n;
  bool any = false, simple = lde_virtual < 0 ? c >= 16 : lde_virtual != 0;
  for (size_t i = 0; i < c; i++) {
    const Lin& li = poly_lin[i];
    if (li.idx.empty()) continue;
    any = true;
    if (li.idx.size() > (size_t)msmerkle::LIN_MAXT) simple = false;
    for (int ix : li.idx) if (ix < 0 || (size_t)ix >= c || !poly_lin[ix].idx.empty()) simple = false;
  }
  if (!any) return 0;
  if (!simple) return lincomb_linear_columns(d_lde.as<T>(), stride, n);
  std::vector<msmerkle::LinColSpec> spec(c);
  for (size_t i = 0; i < c; i++) {
    memset(&spec[i], 0, sizeof spec[i]);
    const Lin& li = poly_lin[i];
    spec[i].n = (u32)li.idx.size();
    for (size_t t = 0; t < li.idx.size(); t++) { spec[i].src[t] = (u32)li.idx[t]; spec[i].s[t] = li.s[t] % F::P; }
  }
  if (d_lin.ensure(c * sizeof(msmerkle::LinColSpec))) return fail(MS_ERR_NOMEM, "virtual column table");
  if (c * sizeof(msmerkle::LinColSpec) > pinned_cap - 8192) return lincomb_linear_columns(d_lde.as<T>(), stride, n);
  // staged through page-locked memory behind the small results: the previous proof's copy out of it completed before that proof's lde_commit returned
  memcpy(pinned.as<u8>() + 8192, spec.data(), c * sizeof(msmerkle::LinColSpec));
  CK(msrt::h2d(d_lin.p, pinned.as<u8>() + 8192, c * sizeof(msmerkle::LinColSpec), stream));
  lde_cols_virtual = true;
  return 0;
}

// lde_compute for a sharded proof: column i of the local LDE (rows rank + W*j) at d_lde + i*m, m = L/W
template <class F>
int Ctx<F>::lde_compute_sharded(size_t blowup_, u64 shift) {
  const size_t c = (size_t)npolys, L_ = N * blowup_, m = L_ / (size_t)sh_world;
  if (d_lde.ensure(c * m * sizeof(T))) return fail(MS_ERR_NOMEM, "lde");
  if (!lde_linear) for (size_t i = 0; i < c; i++) RQ(materialize((int)i));
  PartScope part(this);
  for (size_t i = 0; i < c;) {
    if (lde_linear && !poly_lin[i].idx.empty()) { i++; continue; }
    size_t j = i;
    while (j < c && !(lde_linear && !poly_lin[j].idx.empty())) j++;
    RQ(coset_eval(d_polys.as<T>() + i * N, N, N, ctz64(L_), F::from_u64(shift), 1, d_lde.as<T>() + i * m, m, j - i));
    i = j;
  }
  if (lde_linear) RQ(finish_linear_columns(m, m));
  return 0;
}

// what the three `_coset` commits ask of k and the domain, before anything else is decided
template <class F>
int Ctx<F>::coset_arity_check(const char* who, int k, size_t L_) {
  if (k < 1 || k > 3) return fail(MS_ERR_ARG, std::string(who) + ": log_arity outside 1..3");
  if (sh_on) return fail(MS_ERR_STATE, std::string(who) + ": not available on a context with sharding on");
  if (L_ < ((size_t)2 << k)) return fail(MS_ERR_SHAPE, std::string(who) + ": fewer than two leaf groups (L < 2 * arity)");
  return 0;
}

// leaf_hash's BLAKE3 rule for a leaf group of lpn one-limb elements, asked before a coset commit changes anything: the message may not exceed 16 KiB
template <class F>
int Ctx<F>::coset_leaf_check(const char* who, size_t lpn) {
  if (digest == MS_DIGEST_BLAKE3 && (lpn > 16384 || lpn * (size_t)F::MAX_DIGITS > 16384))
    return fail(MS_ERR_ARG, std::string(who) + ": BLAKE3: a leaf group's message may exceed 16384 bytes (arity x columns x longest decimal)");
  return 0;
}

// finish_linear_columns' decision for the polynomials as they stand: would ms_lde_commit leave the linear columns to the leaf kernel?
template <class F>
bool Ctx<F>::linear_columns_would_be_virtual() const {
  const size_t c = (size_t)npolys;
  if (!lde_linear) return false;
  bool any = false, simple = lde_virtual < 0 ? c >= 16 : lde_virtual != 0;
  for (size_t i = 0; i < c; i++) {
    const Lin& li = poly_lin[i];
    if (li.idx.empty()) continue;
    any = true;
    if (li.idx.size() > (size_t)msmerkle::LIN_MAXT) simple = false;
    for (int ix : li.idx) if (ix < 0 || (size_t)ix >= c || !poly_lin[ix].idx.empty()) simple = false;
  }
  return any && simple && c * sizeof(msmerkle::LinColSpec) <= pinned_cap - 8192;
}

template <class F>
int Ctx<F>::lde_commit(size_t blowup_, u64 shift, size_t lpn, u8* root) { return lde_commit_k(blowup_, shift, lpn, 0, root); }

// ms_lde_commit_coset: ms_lde_commit in every respect but the tree (ctx.hpp)
template <class F>
int Ctx<F>::lde_commit_coset(size_t blowup_, u64 shift, int log_arity, u8* root) {
  if (!have_polys) return fail(MS_ERR_STATE, "lde_commit_coset before interpolate");
  if (!root || !blowup_ || !is_pow2(blowup_) || shift == 0 || shift >= F::P) return fail(MS_ERR_ARG, "lde_commit_coset: bad blowup/shift");
  RQ(coset_arity_check("lde_commit_coset", log_arity, N * blowup_));
  RQ(coset_leaf_check("lde_commit_coset", (size_t)npolys << log_arity));
  if (linear_columns_would_be_virtual()) return fail(MS_ERR_STATE, "lde_commit_coset: the LDE would have virtual linear columns, which a coset leaf cannot name (MS_LDE_VIRTUAL=0, or ms_lde_commit)");
  return lde_commit_k(blowup_, shift, (size_t)npolys << log_arity, log_arity, root);
}

// k = 0: the plain tree, leaf groups of lpn consecutive elements of the row-major matrix.  k > 0 (lpn = c << k): the coset tree
template <class F>
int Ctx<F>::lde_commit_k(size_t blowup_, u64 shift, size_t lpn, int k, u8* root) {
  if (!have_polys) return fail(MS_ERR_STATE, "lde_commit before interpolate");
  if (!root || !blowup_ || !is_pow2(blowup_) || shift == 0 || shift >= F::P) return fail(MS_ERR_ARG, "bad blowup/shift");
  const size_t L_ = N * blowup_;
  if (ctz64(L_) > F::TWO_ADICITY) return fail(MS_ERR_SHAPE, "LDE domain larger than the field's two-adicity (starks.rs:82-83)");
  const size_t c = (size_t)npolys;
  TreeShape ts;
  RQ(tree_shape(L_ * c, lpn, 2, &ts));
  L = L_; blowup = blowup_; lde_c = lde_c0 = c; lde_shift = shift; drop_vtree();
  have_stg = false; stg_pending = 0;   // (staged columns not committed yet are ordinary polynomials of this tree)
  auto stage = res.expect();
  if (k) {   // group j = the rows j + t L / a: element col * a + t of the group is column col of row j + t L / a
    RQ(lde_compute(blowup_, shift));   // (no virtual column: ms_lde_commit_coset has refused an LDE that would have one)
    RQ((tree_build<1>(d_lde.as<T>(), L >> k, 1, 0, (u32)(c << k), ts, d_lde_nodes)));
  } else if (lpn == c && shardable(L_)) {  // one LDE row per leaf group: rank k evaluates and hashes the rows k (mod world)
    RQ(lde_compute_sharded(blowup_, shift));
    RQ((tree_build_sharded<1>(d_lde.as<T>(), L / (size_t)sh_world, 1, 0, (u32)c, ts, d_lde_nodes, lde_lin())));
  } else {
    RQ(lde_compute(blowup_, shift));
    RQ((tree_build<1>(d_lde.as<T>(), L, 1, 0, (u32)c, ts, d_lde_nodes, lde_lin())));
  }
  lde_ts = ts; lde_ck = k;   // (the tree's shape and its grouping change together: a launch refused above leaves the earlier tree's view)
  RQ(read_root(d_lde_nodes, ts, root));
  have_lde = true;
  return MS_OK;
}

// ms_lde_commit_stage (build-defined, include/ministark.h): the c1 polynomials ms_aux_running_staged appended, evaluated on the coset of the live LDE - lde_compute's
// own path, scale by shift^k and one size-L transform - into the columns c0 .. c0 + c1 - 1 of d_lde, and a second tree over that L x c1 row-major view.  Column j stays
// at d_lde + j * L: a buffer too small for c0 + c1 columns is replaced by a larger one with the c0 columns copied (DevBuf::ensure would free them).  Nothing the
// stage-0 tree covers is written; lde_c, the staged tree and the count change behind the root's arrival only
template <class F>
int Ctx<F>::lde_commit_stage(size_t lpn, u8* root) { return lde_commit_stage_k(lpn, 0, root); }

// ms_lde_commit_stage_coset: the staged columns under a coset tree of the live LDE tree's own k
template <class F>
int Ctx<F>::lde_commit_stage_coset(int log_arity, u8* root) {
  if (!root) return fail(MS_ERR_ARG, "lde_commit_stage_coset: null root");
  RQ(coset_arity_check("lde_commit_stage_coset", log_arity, have_lde ? L : ~(size_t)0));
  if (have_polys && have_lde && !lde_ts.sharded && lde_ck != log_arity) return fail(MS_ERR_STATE, "lde_commit_stage_coset: the live LDE tree is not a coset tree of this log_arity (ms_lde_commit_coset)");
  RQ(coset_leaf_check("lde_commit_stage_coset", (size_t)stg_pending << log_arity));
  return lde_commit_stage_k((size_t)stg_pending << log_arity, log_arity, root);
}

template <class F>
int Ctx<F>::lde_commit_stage_k(size_t lpn, int k, u8* root) {
  const char* const who = k ? "lde_commit_stage_coset" : "lde_commit_stage";   // (the entry point, for the messages)
  if (sh_on) return fail(MS_ERR_STATE, std::string(who) + ": not available on a context with sharding on");
  if (!root) return fail(MS_ERR_ARG, std::string(who) + ": null root");
  if (!have_polys || !have_lde || lde_ts.sharded) return fail(MS_ERR_STATE, std::string(who) + ": no committed LDE (ms_lde_commit, and no ms_polys_* since)");
  if (have_stg) return fail(MS_ERR_STATE, std::string(who) + ": the stage of this ms_lde_commit is committed already");
  if (stg_pending < 1) return fail(MS_ERR_STATE, std::string(who) + ": no staged columns (ms_aux_running_staged)");
  const size_t c0 = lde_c, c1 = (size_t)stg_pending;
  if (c0 + c1 != (size_t)npolys) return fail(MS_ERR_STATE, std::string(who) + ": the staged columns are not the last polynomials");
  TreeShape ts;
  RQ(tree_shape(L * c1, lpn, 2, &ts));
  RQ(res.join_side());
  if (d_coef.ensure(c1 * N * sizeof(T))) return fail(MS_ERR_NOMEM, std::string(who) + " buffers");
  const size_t need = (c0 + c1) * L * sizeof(T);
  if (need > d_lde.cap) {
    DevBuf nb;
    if (nb.ensure(need)) return fail(MS_ERR_NOMEM, std::string(who) + " buffers");
    CK(msrt::d2d(nb.p, d_lde.p, c0 * L * sizeof(T), stream)); CK(msrt::sync(stream));
    d_lde = std::move(nb);
  }
  auto stage = res.expect();
  T* dst = d_lde.as<T>() + c0 * L;
  RQ(scale_pow(d_polys.as<T>() + c0 * N, N, d_coef.as<T>(), N, N, F::from_u64(lde_shift), c1));
  RQ(ntt_run(ctz64(L), false, d_coef.as<T>(), N, N, dst, L, c1));
  RQ((tree_build<1>(dst, L >> k, 1, 0, (u32)(c1 << k), ts, d_stg_nodes)));   // (k = 0: the plain view, col_stride = L, width = c1)
  RQ(read_root(d_stg_nodes, ts, root));
  stg_ts = ts; stg_ck = k; lde_c = c0 + c1; stg_pending = 0; have_stg = true;
  return MS_OK;
}

template <class F>
int Ctx<F>::bench_lde(size_t blowup_, u64 shift) {
  if (!have_polys) return fail(MS_ERR_STATE, "bench_lde before interpolate");
  have_lde = false;                              // d_lde is overwritten: whatever ms_lde_commit left there is gone
  const int keep = lde_virtual; lde_virtual = 0; // time the columns as WRITTEN (a virtual column's work would move into a leaf kernel this entry does not run)
  auto restore = scope_exit([this, keep] { lde_virtual = keep; lde_cols_virtual = false; });   // (also when lde_compute throws: ADVICE r4)
  return lde_compute(blowup_, shift);
}

template <class F>
int Ctx<F>::lde_read(u64* out) {
  if (!have_lde || !out) return fail(MS_ERR_STATE, "lde_read");
  if (lde_ts.sharded) return fail(MS_ERR_STATE, "lde_read: the LDE of a sharded proof is distributed over the ranks");
  if (lde_cols_virtual) { RQ(lincomb_linear_columns(d_lde.as<T>(), lde_col_stride, lde_col_len)); lde_cols_virtual = false; }   // the virtual columns, written out on demand
  const size_t tot = L * lde_c;
  if (d_io.ensure(tot * 8)) return fail(MS_ERR_NOMEM, "io");
  typename mspoly::TransposeOutKernel<F>::Params p{d_lde.as<T>(), d_io.as<u64>(), L, lde_c, L};
  CK(run<mspoly::TransposeOutKernel<F>>(K_IO, grid1(tot, mspoly::THREADS), 1, mspoly::THREADS, 0, p));
  CK(msrt::d2h(out, d_io.p, tot * 8, stream));
  CK(msrt::sync(stream));
  return MS_OK;
}

// ------------------------------------------------------------------ starks.rs:108-119
template <class F>
int Ctx<F>::mix(u64 r) {
  if (!have_polys) return fail(MS_ERR_STATE, "mix before interpolate");
  if (stg_pending) return fail(MS_ERR_STATE, "mix: uncommitted staged columns (ms_lde_commit_stage, or ms_lde_commit)");
  if (r >= F::P) return fail(MS_ERR_ARG, "r not canonical");
  RQ(ensure_polys(npolys + 1));
  bool any_lazy = false;
  for (int i = 0; i < npolys; i++) any_lazy = any_lazy || !poly_mat[i];
  if (any_lazy) {   // sum_i r^i f_i as ONE combination of the polynomials without provenance (the lazily defined f_i are never formed)
    std::map<int, T> acc;
    T rp = F::from_u64(1);
    for (int i = 0; i < npolys; i++) { expand(i, rp, acc); rp = F::mul(rp, F::from_u64(r)); }
    std::vector<u64> sc; std::vector<int> ix;
    for (auto& kv : acc) if (kv.second != 0) { sc.push_back(F::to_u64(kv.second)); ix.push_back(kv.first); }
    T* dst = d_polys.as<T>() + (size_t)npolys * N;
    if (sc.empty()) CK(msrt::memset_dev(dst, 0, N * sizeof(T), stream));
    else RQ(lincomb_into(d_polys.as<T>(), N, N, sc.data(), ix.data(), (int)sc.size(), npolys, dst));
  } else {
  typename mspoly::MixKernel<F>::Params p{d_polys.as<T>(), N, N, npolys, F::from_u64(r), d_polys.as<T>() + (size_t)npolys * N};
  CK(run<mspoly::MixKernel<F>>(K_MIX, grid1(N, mspoly::THREADS), 1, mspoly::THREADS, 0, p));
  }
  // the trimmed length ms_fri_begin needs (fri.rs:74), found HERE: the word travels to the host on DEEP-ALI's last evaluation launch (ms_eval_ext), which the caller
  // waits for anyway - ms_fri_begin then starts its transform without a launch, a copy and a host round trip of its own (r05)
  validity_len_at = VLEN_RESCAN;
  if (!dist_eval()) {   // (a sharded proof's DEEP-ALI ends in a collective, not in an evaluation launch: ms_fri_begin keeps its own scan there)
    unsigned long long* vlen = res.word(Results::VALIDITY_LEN);   // (a word of its own, not the zero pool: the pool may be wiped before ms_eval_ext comes)
    CK(msrt::memset_dev(vlen, 0, 8, stream));
    typename mspoly::DegreeKernel<F, 1>::Params dp{d_polys.as<T>() + (size_t)npolys * N, 0, N, vlen, 0};
    CK(run<mspoly::DegreeKernel<F, 1>>(K_DEGREE, grid1(N, mspoly::THREADS), 1, mspoly::THREADS, 0, dp));
    validity_len_at = VLEN_DEVICE;
  }
  have_validity = true; validity_len = N; validity_ext = 1; nrounds_done = 0; drop_vtree();
  return MS_OK;
}

// ------------------------------------------------------------------ the build-defined mix stages: one pipeline
// ms_mix_cubic, ms_mix_terms and ms_mix_air (include/ministark.h) give the true quotient of a composition by x^N - 1.  Each stage is
//   mix_gate -> its own checks -> coset_vanishing_inv -> its host table -> upload_mix_table -> its ONE compose launch into d_cubic -> finish_mix
// and differs from the others in the checks, the table and the kernel only.  Everything that can be refused is refused before the first launch, except the
// exactness of the division, which only the interpolant shows; nothing of the session changes before that result (but see the store guard in finish_mix).
template <class F>
int Ctx<F>::mix_gate(const char* who, u64 r) {
  if (!have_lde) return fail(MS_ERR_STATE, std::string(who) + " before lde_commit");
  if (lde_ts.sharded) return fail(MS_ERR_STATE, std::string(who) + ": the LDE of a sharded proof is distributed over the ranks");
  if (stg_pending) return fail(MS_ERR_STATE, std::string(who) + ": uncommitted staged columns (ms_lde_commit_stage, or ms_lde_commit)");
  if (r >= F::P) return fail(MS_ERR_ARG, std::string(who) + " arguments");
  return 0;
}

template <class F>
int Ctx<F>::coset_vanishing_inv(const char* who, std::vector<T>& dinv) {
  const T one = F::from_u64(1), shN = f_pow<F>(F::from_u64(lde_shift), (u64)N), zeta = f_pow<F>(f_root_of_unity<F>(ctz64(L)), (u64)N);
  dinv.resize(blowup);
  T z = one;
  for (size_t k = 0; k < blowup; k++, z = F::mul(z, zeta)) {
    const T den = F::sub(F::mul(shN, z), one);
    if (den == 0) return fail(MS_ERR_SHAPE, std::string(who) + ": the LDE coset meets the trace domain (shift^N is a blowup-th root of unity)");
    dinv[k] = f_inv<F>(den);
  }
  return 0;
}

template <class F>
int Ctx<F>::check_term_program(const char* who, u32 ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, u32* deg_per_constraint, u32* d) {
  auto bad = [&](const char* what) { return fail(MS_ERR_ARG, std::string(who) + what); };
  if (term_begin[0] != 0) return bad(": term_begin[0] must be 0");
  for (u32 t = 0; t < ncons; t++) if (term_begin[t + 1] < term_begin[t] || term_begin[t + 1] > 65536) return bad(": term_begin not monotone, or more than 65536 terms");
  if (fac_begin[0] != 0) return bad(": fac_begin[0] must be 0");
  *d = 0;
  for (u32 t = 0; t < ncons; t++)
    for (u32 m = term_begin[t]; m < term_begin[t + 1]; m++) {
      if (fac_begin[m + 1] < fac_begin[m]) return bad(": fac_begin not monotone");
      const u32 nf = fac_begin[m + 1] - fac_begin[m];
      if (nf > (u32)mspoly::TERMS_MAX_FACTORS) return bad(": a term with more than 8 factors");
      if (coef[m] >= F::P) return bad(": coefficient not canonical");
      if (deg_per_constraint && nf > deg_per_constraint[t]) deg_per_constraint[t] = nf;
      if (nf > *d) *d = nf;
    }
  if (*d == 0) return bad(": no term has a factor (d = 0)");
  return 0;
}

template <class F>
int Ctx<F>::upload_mix_table(const char* who, const u8* tab, size_t bytes, size_t ne) {
  if (lde_cols_virtual) { RQ(lincomb_linear_columns(d_lde.as<T>(), lde_col_stride, lde_col_len)); lde_cols_virtual = false; }
  if (d_cubic.ensure(2 * L * ne * sizeof(T)) || d_tabs.ensure(bytes + 64)) return fail(MS_ERR_NOMEM, std::string(who) + " buffers");
  u8* ht;
  RQ(tabs_host(bytes + 64, &ht));     // (the previous user of the area, the last proof's query phase, ended with a stream synchronisation)
  memcpy(ht, tab, bytes);
  CK(msrt::h2d(d_tabs.p, ht, bytes, stream));
  return 0;
}

// evaluations on shift * <g_L> (d_cubic)  ->  coefficients of Q(shift y)  ->  q_k = coefficient_k * shift^-k.  The size-L interpolant I of the pointwise quotient satisfies
// I (x^N - 1) = numerator on L points: with both sides of degree < L (the stages' SHAPE conditions), "I has at most VL coefficients" is "the division is exact" - the
// reference's `assert_eq!(rest, zero)` of starks.rs:119, for the true quotient.  The stage's one stream synchronisation is here, for that answer.
// ne limb planes (ms_mix_air_ext: the interpolation is Fp-linear, so a K-valued quotient is ne base-field ones): planes of L evaluations at d_cubic, their
// coefficients behind them; exact means EVERY plane has at most VL coefficients (the scan takes the maximum over the limbs); limb l is stored at + l * VL.
template <class F>
int Ctx<F>::finish_mix(const char* refusal, size_t VL, int ne) {
  T* cf = d_cubic.as<T>() + (size_t)ne * L;
  RQ(ntt_run(ctz64(L), true, d_cubic.as<T>(), L, L, cf, L, (size_t)ne));
  const size_t slots = (size_t)ne * (VL / N);
  if ((size_t)npolys + slots > polys_cap) have_validity = false;   // (the polynomial store is about to move: an earlier validity polynomial behind the constraint polynomials does not move with it)
  RQ(ensure_polys(npolys + slots));
  unsigned long long* dres, ncoef = 0;
  if (ne == 1) RQ(degree_launch1(cf, L, &dres)); else RQ(degree_launch(cf, L, L, &dres));
  { auto scan = res.expect(dres, false, false); RQ(res.collect(nullptr, nullptr, &ncoef)); }
  if (ncoef > VL) return fail(MS_ERR_SHAPE, refusal);
  RQ(scale_pow(cf, L, d_polys.as<T>() + (size_t)npolys * N, VL, VL, f_inv<F>(F::from_u64(lde_shift)), (size_t)ne));
  CK(msrt::sync(stream));   // (include/ministark.h, Streams: these mix stages return with nothing in flight - the un-shift above is launched behind the exactness check's wait)
  validity_ncoef = (size_t)ncoef; validity_len_at = VLEN_HOST;   // (scaling by shift^-k keeps the trimmed length)
  have_validity = true; validity_len = VL; validity_ext = ne; nrounds_done = 0; drop_vtree();
  return MS_OK;
}

// Degree-3 composition, C_t = P_j(w x) - P_a P_b P_c - s P_d with the last row exempt: a quotient of 2N coefficients (the composition has 3N)
template <class F>
int Ctx<F>::mix_cubic(u64 r, const int* spec, const u64* sc, int ncons) {
  RQ(mix_gate("mix_cubic", r));
  if (!spec || !sc || ncons < 1 || ncons > 4096) return fail(MS_ERR_ARG, "mix_cubic arguments");
  if (blowup < 4) return fail(MS_ERR_SHAPE, "mix_cubic needs blowup >= 4 (the quotient has 2N coefficients, the composition 3N)");
  for (int t = 0; t < ncons; t++) { for (int u = 0; u < 5; u++) if (spec[5 * t + u] < 0 || (size_t)spec[5 * t + u] >= lde_c) return fail(MS_ERR_ARG, "mix_cubic: polynomial index out of range"); if (sc[t] >= F::P) return fail(MS_ERR_ARG, "mix_cubic: scalar not canonical"); }
  typedef mspoly::CubicSpec<F> CS; typedef mspoly::CubicComposeKernel<F> CK_;
  std::vector<T> dinv;
  RQ(coset_vanishing_inv("mix_cubic", dinv));
  // the device table: [constraints | den_inv], r^t beside constraint t
  const size_t off_d = (size_t)ncons * sizeof(CS), tab_bytes = off_d + dinv.size() * sizeof(T);
  std::vector<u8> tab(tab_bytes, 0);
  { CS* hs = reinterpret_cast<CS*>(tab.data());
    T rp = F::from_u64(1);
    for (int t = 0; t < ncons; t++) { hs[t].j = (u32)spec[5 * t]; hs[t].a = (u32)spec[5 * t + 1]; hs[t].b = (u32)spec[5 * t + 2]; hs[t].c = (u32)spec[5 * t + 3]; hs[t].d = (u32)spec[5 * t + 4]; hs[t].s = F::from_u64(sc[t]); hs[t].rpow = rp; rp = F::mul(rp, F::from_u64(r)); }
    memcpy(tab.data() + off_d, dinv.data(), dinv.size() * sizeof(T)); }
  RQ(upload_mix_table("mix_cubic", tab.data(), tab_bytes));
  const T gL = f_root_of_unity<F>(ctz64(L)), wN = f_root_of_unity<F>(ctz64(N));
  typename CK_::Params cp;
  cp.lde = d_lde.as<T>(); cp.L = L; cp.blowup = (u32)blowup; cp.ncons = (u32)ncons; cp.spec = d_tabs.as<CS>();
  cp.den_inv = reinterpret_cast<const T*>(d_tabs.as<u8>() + off_d);
  cp.shift = F::from_u64(lde_shift); cp.gL = gL; cp.gL_step = f_pow<F>(gL, (u64)CK_::THREADS); cp.w_last = f_pow<F>(wN, (u64)(N - 1)); cp.out = d_cubic.as<T>();
  CK(run<CK_>(K_MIX, grid1(L, CK_::THREADS * CK_::ITEMS), 1, CK_::THREADS, 0, cp));
  return finish_mix("mix_cubic: the constraints do not vanish on the trace domain (the quotient by x^N - 1 is not a polynomial of 2N coefficients)", 2 * N);
}

// Composition of any degree: the constraints as sums of monomials over the polynomials, factors at row offsets, the last nexempt rows exempt.
// VL = N * next_pow2(slots), slots = max(1, d - 1) (one more when nexempt > d - 1), d = the most factors of any term.
template <class F>
int Ctx<F>::mix_terms(u64 r, int ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, const u32* fac_poly, const u32* fac_row, int nexempt) {
  RQ(mix_gate("mix_terms", r));
  if (!term_begin || !coef || !fac_begin || !fac_poly || !fac_row) return fail(MS_ERR_ARG, "mix_terms: null array");
  if (ncons < 1 || ncons > 4096 || nexempt < 0 || nexempt > mspoly::TERMS_MAX_EXEMPT) return fail(MS_ERR_ARG, "mix_terms arguments");
  u32 d;
  RQ(check_term_program("mix_terms", (u32)ncons, term_begin, coef, fac_begin, nullptr, &d));
  const u32 nterms = term_begin[ncons], nfacs = fac_begin[nterms];
  for (u32 f = 0; f < nfacs; f++) if ((size_t)fac_poly[f] >= lde_c || (size_t)fac_row[f] >= N) return fail(MS_ERR_ARG, "mix_terms: polynomial index or row offset out of range");
  // the quotient has at most (d - 1) N - d + nexempt + 1 coefficients: d - 1 slots of N, one more when nexempt > d - 1
  const size_t need = (size_t)(d - 1) * N + (size_t)nexempt + 1 - d, need_slots = (need + N - 1) / N;
  size_t slots = d > 1 ? d - 1 : 1; if (need_slots > slots) slots = need_slots;
  size_t vmul = 1; while (vmul < slots) vmul <<= 1;
  const size_t VL = N * vmul;
  if (!((size_t)d * (N - 1) + (size_t)nexempt < L) || VL + N > L) return fail(MS_ERR_SHAPE, "mix_terms: the LDE domain is too small to decide exactness (need d (N - 1) + nexempt < L and VL + N <= L)");
  typedef mspoly::TermRec<F> TR; typedef mspoly::TermFac TF; typedef mspoly::ComposeTermsKernel<F> CK_;
  std::vector<T> dinv;
  RQ(coset_vanishing_inv("mix_terms", dinv));
  // the device table: [terms | factors | exemption roots | den_inv], r^t folded into the coefficients of constraint t's terms
  const size_t off_f = ((size_t)nterms * sizeof(TR) + 15) & ~(size_t)15, off_x = (off_f + (size_t)nfacs * sizeof(TF) + 15) & ~(size_t)15;
  const size_t off_d = off_x + mspoly::TERMS_MAX_EXEMPT * sizeof(T), tab_bytes = off_d + dinv.size() * sizeof(T);
  std::vector<u8> tab(tab_bytes, 0);
  { TR* ht = reinterpret_cast<TR*>(tab.data()); TF* hf = reinterpret_cast<TF*>(tab.data() + off_f); T* hx = reinterpret_cast<T*>(tab.data() + off_x);
    T rp = F::from_u64(1);
    for (int t = 0; t < ncons; t++) {
      for (u32 m = term_begin[t]; m < term_begin[t + 1]; m++) { ht[m].coef = F::mul(rp, F::from_u64(coef[m])); ht[m].nfac = fac_begin[m + 1] - fac_begin[m]; }
      rp = F::mul(rp, F::from_u64(r));
    }
    for (u32 f = 0; f < nfacs; f++) { hf[f].poly = fac_poly[f]; hf[f].rowoff = (u32)((size_t)fac_row[f] * blowup); }
    T wi = f_inv<F>(f_root_of_unity<F>(ctz64(N))), wk = wi;      // w^(N-k) = w^-k
    for (int k = 0; k < nexempt; k++) { hx[k] = wk; wk = F::mul(wk, wi); }
    memcpy(tab.data() + off_d, dinv.data(), dinv.size() * sizeof(T)); }
  RQ(upload_mix_table("mix_terms", tab.data(), tab_bytes));
  const T gL = f_root_of_unity<F>(ctz64(L));
  typename CK_::Params cp;
  cp.lde = d_lde.as<T>(); cp.L = L; cp.blowup = (u32)blowup; cp.nterms = nterms; cp.nexempt = (u32)nexempt;
  cp.terms = d_tabs.as<TR>(); cp.facs = reinterpret_cast<const TF*>(d_tabs.as<u8>() + off_f);
  cp.ex_roots = reinterpret_cast<const T*>(d_tabs.as<u8>() + off_x); cp.den_inv = reinterpret_cast<const T*>(d_tabs.as<u8>() + off_d);
  cp.shift = F::from_u64(lde_shift); cp.gL = gL; cp.gL_step = f_pow<F>(gL, (u64)CK_::THREADS); cp.out = d_cubic.as<T>();
  next_bytes = (double)(nfacs + 1) * L * sizeof(T);
  CK(run<CK_>(K_MIX_TERMS, grid1(L, CK_::THREADS * CK_::ITEMS), 1, CK_::THREADS, 0, cp));
  return finish_mix("mix_terms: the constraints do not vanish on the non-exempt rows (the quotient by x^N - 1 is not a polynomial of VL coefficients)", VL);
}

// ---- ms_mix_air: ms_mix_terms with an exemption set per constraint, periodic columns and boundary constraints, the program regrouped for mspoly::ComposeAirKernel -
// the constraints that share an exemption set form one group, the boundary constraints at one row another.
// Every MS_ERR_ARG refusal of the stage (and of ms_air_check, whose c is not the LDE's); fills pg
template <class F>
int Ctx<F>::air_validate(const ms_air& a, AirProgram& pg, size_t c) {
  if (!a.term_begin || !a.coef || !a.fac_begin || !a.fac_poly || !a.fac_row || !a.ex_begin) return fail(MS_ERR_ARG, "mix_air: null array");
  if (a.ncons < 1 || a.ncons > 4096 || a.nperiodic > (u32)mspoly::AIR_MAX_PERIODIC || a.nbound > 4096) return fail(MS_ERR_ARG, "mix_air arguments");
  if ((a.nperiodic && (!a.per_begin || !a.per_val)) || (a.nbound && (!a.bnd_poly || !a.bnd_row || !a.bnd_val))) return fail(MS_ERR_ARG, "mix_air: null array");
  const u32 ncons = a.ncons;
  u32 d;                                     // ---- the term program: the conditions of mix_terms, the degree per constraint
  pg.deg.assign(ncons, 0);
  RQ(check_term_program("mix_air", ncons, a.term_begin, a.coef, a.fac_begin, pg.deg.data(), &d));
  pg.nterms = a.term_begin[ncons]; pg.nfacs = a.fac_begin[pg.nterms];
  // ---- periodic columns
  pg.per_off.assign(a.nperiodic + 1, 0);
  if (a.nperiodic) {
    if (a.per_begin[0] != 0) return fail(MS_ERR_ARG, "mix_air: per_begin[0] must be 0");
    for (u32 k = 0; k < a.nperiodic; k++) {
      if (a.per_begin[k + 1] <= a.per_begin[k] || a.per_begin[k + 1] > (u32)mspoly::AIR_MAX_PERIOD_SUM) return fail(MS_ERR_ARG, "mix_air: per_begin not increasing, or the periods sum to more than 4096");
      const size_t q = a.per_begin[k + 1] - a.per_begin[k];
      if (!is_pow2(q) || q > N || q > (size_t)mspoly::AIR_MAX_PERIOD) return fail(MS_ERR_ARG, "mix_air: a period that is no power of two or exceeds min(N, 256)");
      pg.per_off[k + 1] = pg.per_off[k] + (u32)(q * blowup);
    }
    if (!canonical(a.per_val, a.per_begin[a.nperiodic])) return fail(MS_ERR_ARG, "mix_air: periodic value not canonical");
  }
  for (u32 f = 0; f < pg.nfacs; f++) {
    const u32 fp = a.fac_poly[f];
    if ((fp & MS_AIR_PERIODIC) ? (fp & ~MS_AIR_PERIODIC) >= a.nperiodic : (size_t)fp >= c) return fail(MS_ERR_ARG, "mix_air: polynomial or periodic column index out of range");
    if ((size_t)a.fac_row[f] >= N) return fail(MS_ERR_ARG, "mix_air: row offset out of range");
  }
  // ---- exemption sets: the constraints with the same set (as a set) share a group
  if (a.ex_begin[0] != 0) return fail(MS_ERR_ARG, "mix_air: ex_begin[0] must be 0");
  for (u32 t = 0; t < ncons; t++) if (a.ex_begin[t + 1] < a.ex_begin[t] || a.ex_begin[t + 1] - a.ex_begin[t] > (u32)mspoly::AIR_MAX_EXEMPT) return fail(MS_ERR_ARG, "mix_air: ex_begin not monotone, or more than 16 exempt rows for a constraint");
  if (a.ex_begin[ncons] && !a.ex_row) return fail(MS_ERR_ARG, "mix_air: null array");
  pg.set_of.assign(ncons, 0);
  std::map<std::vector<u32>, u32> seen;
  for (u32 t = 0; t < ncons; t++) {
    std::vector<u32> s(a.ex_row ? a.ex_row + a.ex_begin[t] : nullptr, a.ex_row ? a.ex_row + a.ex_begin[t + 1] : nullptr);
    std::sort(s.begin(), s.end());
    for (size_t k = 0; k < s.size(); k++) if ((size_t)s[k] >= N || (k && s[k] == s[k - 1])) return fail(MS_ERR_ARG, "mix_air: exempt row out of range, or named twice in one set");
    auto it = seen.find(s);
    if (it == seen.end()) {
      if (pg.sets.size() == (size_t)mspoly::AIR_MAX_SETS) return fail(MS_ERR_ARG, "mix_air: more than 32 distinct exemption sets");
      it = seen.emplace(s, (u32)pg.sets.size()).first; pg.sets.push_back(s);
    }
    pg.set_of[t] = it->second;
  }
  // ---- boundary constraints: one group per distinct row
  pg.brow_of.assign(a.nbound, 0);
  for (u32 b = 0; b < a.nbound; b++) {
    if ((size_t)a.bnd_poly[b] >= c || (size_t)a.bnd_row[b] >= N || a.bnd_val[b] >= F::P) return fail(MS_ERR_ARG, "mix_air: boundary polynomial or row out of range, or value not canonical");
    size_t k = 0; while (k < pg.brows.size() && pg.brows[k] != a.bnd_row[b]) k++;
    if (k == pg.brows.size()) { if (k == (size_t)mspoly::AIR_MAX_BOUNDARY_ROWS) return fail(MS_ERR_ARG, "mix_air: more than 16 distinct boundary rows"); pg.brows.push_back(a.bnd_row[b]); }
    pg.brow_of[b] = (u32)k;
  }
  return 0;
}

// Sizes, and the stage's MS_ERR_SHAPE refusal.  Constraint t's quotient has d_t (N - 1) + e_t - N + 1 coefficients, a boundary quotient N - 1
template <class F>
int Ctx<F>::air_layout(const ms_air& a, const AirProgram& pg, AirLayout& lay) {
  size_t top = 0;                                      // max_t (d_t (N - 1) + e_t): >= N - 1, some d_t is at least 1
  for (u32 t = 0; t < a.ncons; t++) { const size_t v = (size_t)pg.deg[t] * (N - 1) + (a.ex_begin[t + 1] - a.ex_begin[t]); if (v > top) top = v; }
  size_t nq = top + 1 - N;
  if (a.nbound && N - 1 > nq) nq = N - 1;
  if (nq < 1) nq = 1;
  size_t vmul = 1; while (vmul < (nq + N - 1) / N) vmul <<= 1;
  lay.VL = N * vmul;
  // multiplied by x^N - 1 the pointwise sum is a polynomial of degree < L under exactly these conditions: then "the size-L interpolant has at most VL coefficients"
  // is "every division is exact" (for the random combination)
  if (!(top < L) || (a.nbound && !(2 * N - 2 < L)) || lay.VL + N > L)
    return fail(MS_ERR_SHAPE, "mix_air: the LDE domain is too small to decide exactness (need max_t (d_t (N - 1) + e_t) < L, 2N - 2 < L with boundary constraints, VL + N <= L)");
  lay.ngroups = pg.sets.size() + pg.brows.size(); lay.tterms = (size_t)pg.nterms + a.nbound + pg.brows.size(); lay.tfacs = (size_t)pg.nfacs + a.nbound;
  size_t nroots = 0; for (auto& s : pg.sets) nroots += s.size();
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  lay.off_t = up16(lay.ngroups * sizeof(mspoly::AirGroup)); lay.off_f = up16(lay.off_t + lay.tterms * sizeof(mspoly::TermRec<F>)); lay.off_x = up16(lay.off_f + lay.tfacs * sizeof(mspoly::AirFac));
  lay.off_p = up16(lay.off_x + nroots * sizeof(T)); lay.off_d = up16(lay.off_p + (size_t)pg.per_off[a.nperiodic] * sizeof(T)); lay.bytes = lay.off_d + blowup * sizeof(T);
  return 0;
}

// The device table (lay.bytes zeroed bytes at tab), r^t folded into the coefficients of constraint t's terms, r^(ncons+b) into boundary constraint b's
template <class F>
void Ctx<F>::air_table(u64 r, const ms_air& a, const AirProgram& pg, const AirLayout& lay, const std::vector<T>& dinv, u8* tab) {
  typedef mspoly::AirFac AF; typedef mspoly::AirGroup AG;
  AG* hg = reinterpret_cast<AG*>(tab); mspoly::TermRec<F>* ht = reinterpret_cast<mspoly::TermRec<F>*>(tab + lay.off_t); AF* hf = reinterpret_cast<AF*>(tab + lay.off_f);
  T* hx = reinterpret_cast<T*>(tab + lay.off_x); T* hp = reinterpret_cast<T*>(tab + lay.off_p);
  const u32 ncons = a.ncons;
  const T wN = f_root_of_unity<F>(ctz64(N)), wi = f_inv<F>(wN), one = F::from_u64(1);
  std::vector<T> rpow((size_t)ncons + a.nbound);
  { T rp = one; for (auto& v : rpow) { v = rp; rp = F::mul(rp, F::from_u64(r)); } }
  size_t m_out = 0, f_out = 0, x_out = 0;
  for (size_t g = 0; g < pg.sets.size(); g++) {      // transition groups: the terms of the group's constraints in the caller's order
    const size_t m_first = m_out;
    for (u32 t = 0; t < ncons; t++) {
      if (pg.set_of[t] != g) continue;
      for (u32 m = a.term_begin[t]; m < a.term_begin[t + 1]; m++, m_out++) {
        ht[m_out].coef = F::mul(rpow[t], F::from_u64(a.coef[m])); ht[m_out].nfac = a.fac_begin[m + 1] - a.fac_begin[m];
        for (u32 f = a.fac_begin[m]; f < a.fac_begin[m + 1]; f++, f_out++) {
          const u32 fp = a.fac_poly[f];
          hf[f_out].rowoff = (u32)((size_t)a.fac_row[f] * blowup);
          if (fp & MS_AIR_PERIODIC) { const u32 k = fp & ~MS_AIR_PERIODIC; hf[f_out].src = pg.per_off[k]; hf[f_out].mask = pg.per_off[k + 1] - pg.per_off[k] - 1; hf[f_out].kind = 1; }
          else { hf[f_out].src = fp; hf[f_out].mask = (u32)(L - 1); hf[f_out].kind = 0; }
        }
      }
    }
    for (u32 rho : pg.sets[g]) hx[x_out++] = f_pow<F>(wN, (u64)rho);
    hg[g].nterms = (u32)(m_out - m_first); hg[g].nroots = (u32)pg.sets[g].size(); hg[g].kind = 0; hg[g].moff = 0;
  }
  for (size_t k = 0; k < pg.brows.size(); k++) {     // boundary groups: (sum_b r^(ncons+b) w^-rho (P_j - v_b)) * D[i - rho blowup]
    const size_t m_first = m_out;
    const T wr = f_pow<F>(wi, (u64)pg.brows[k]);
    T cst = 0;
    for (u32 b = 0; b < a.nbound; b++) {
      if (pg.brow_of[b] != k) continue;
      const T cf = F::mul(rpow[(size_t)ncons + b], wr);
      ht[m_out].coef = cf; ht[m_out].nfac = 1; m_out++;
      hf[f_out].src = a.bnd_poly[b]; hf[f_out].rowoff = 0; hf[f_out].mask = (u32)(L - 1); hf[f_out].kind = 0; f_out++;
      cst = F::add(cst, F::mul(cf, F::from_u64(a.bnd_val[b])));
    }
    ht[m_out].coef = F::neg(cst); ht[m_out].nfac = 0; m_out++;
    AG& gr = hg[pg.sets.size() + k];
    gr.nterms = (u32)(m_out - m_first); gr.nroots = 0; gr.kind = 1; gr.moff = (u32)(((N - pg.brows[k]) % N) * blowup);
  }
  air_periodic_tables(a, pg, hp);
  memcpy(tab + lay.off_d, dinv.data(), dinv.size() * sizeof(T));
}

// periodic column k on the domain: K_k(x_i) = Q_k(x_i^(N/q)) takes blowup * q values, tab[u] = Q_k(shift^(N/q) g_L^(u N/q))
template <class F>
void Ctx<F>::air_periodic_tables(const ms_air& a, const AirProgram& pg, T* hp) {
  const T gL = f_root_of_unity<F>(ctz64(L)), wi = f_inv<F>(f_root_of_unity<F>(ctz64(N))), sh = F::from_u64(lde_shift), one = F::from_u64(1);
  for (u32 k = 0; k < a.nperiodic; k++) {
    const size_t q = a.per_begin[k + 1] - a.per_begin[k], step = N / q;
    const u64* val = a.per_val + a.per_begin[k];
    const T eta_inv = f_pow<F>(wi, (u64)step), qinv = f_inv<F>(F::from_u64((u64)q));
    std::vector<T> Q(q);
    { T em = one;                                  // eta^-m
      for (size_t m = 0; m < q; m++) { T s = 0, e = one; for (size_t i = 0; i < q; i++) { s = F::add(s, F::mul(F::from_u64(val[i]), e)); e = F::mul(e, em); } Q[m] = F::mul(s, qinv); em = F::mul(em, eta_inv); } }
    const T zq = f_pow<F>(gL, (u64)step);
    T x = f_pow<F>(sh, (u64)step);
    for (size_t u = 0; u < q * blowup; u++) { T v = 0; for (size_t m = q; m-- > 0;) v = F::add(F::mul(v, x), Q[m]); hp[pg.per_off[k] + u] = v; x = F::mul(x, zq); }
  }
}

// ---- ms_mix_air_ext: the table of mspoly::ComposeAirExtKernel.  The groups are air_table's (one per exemption set, one per boundary row); inside a group every
// constraint is a segment of its own with the K weight r^t (r^(ncons+b)) beside it, its term coefficients as the caller gave them
template <class F>
typename Ctx<F>::AirLayoutExt Ctx<F>::air_layout_ext(const ms_air& a, const AirProgram& pg, const AirLayout& lay) const {
  AirLayoutExt lx;
  lx.nsegs = (size_t)a.ncons + a.nbound; lx.tterms = (size_t)pg.nterms + 2 * (size_t)a.nbound; lx.tfacs = (size_t)pg.nfacs + a.nbound;
  size_t nroots = 0; for (auto& s : pg.sets) nroots += s.size();
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  lx.off_s = up16(lay.ngroups * sizeof(mspoly::AirGroupExt)); lx.off_t = up16(lx.off_s + lx.nsegs * sizeof(mspoly::AirSeg<F, E>));
  lx.off_f = up16(lx.off_t + lx.tterms * sizeof(mspoly::TermRec<F>)); lx.off_x = up16(lx.off_f + lx.tfacs * sizeof(mspoly::AirFac));
  lx.off_p = up16(lx.off_x + nroots * sizeof(T)); lx.off_d = up16(lx.off_p + (size_t)pg.per_off[a.nperiodic] * sizeof(T)); lx.bytes = lx.off_d + blowup * sizeof(T);
  return lx;
}

template <class F>
void Ctx<F>::air_table_ext(const XE& r, const ms_air& a, const AirProgram& pg, const AirLayoutExt& lx, const std::vector<T>& dinv, u8* tab) {
  typedef mspoly::AirFac AF; typedef mspoly::AirGroupExt AG; typedef mspoly::AirSeg<F, E> AS;
  AG* hg = reinterpret_cast<AG*>(tab); AS* hs = reinterpret_cast<AS*>(tab + lx.off_s); mspoly::TermRec<F>* ht = reinterpret_cast<mspoly::TermRec<F>*>(tab + lx.off_t);
  AF* hf = reinterpret_cast<AF*>(tab + lx.off_f); T* hx = reinterpret_cast<T*>(tab + lx.off_x);
  const u32 ncons = a.ncons;
  const T wN = f_root_of_unity<F>(ctz64(N)), wi = f_inv<F>(wN);
  std::vector<XE> rpow((size_t)ncons + a.nbound);
  { XE rp = e_one<F, E>(); for (auto& v : rpow) { v = rp; rp = e_mul<F>(rp, r); } }
  size_t s_out = 0, m_out = 0, f_out = 0, x_out = 0;
  for (size_t g = 0; g < pg.sets.size(); g++) {      // transition groups: the group's constraints in the caller's order, a segment each
    const size_t s_first = s_out;
    for (u32 t = 0; t < ncons; t++) {
      if (pg.set_of[t] != g) continue;
      for (int l = 0; l < E; l++) hs[s_out].w[l] = rpow[t].c[l];
      hs[s_out].nterms = a.term_begin[t + 1] - a.term_begin[t]; s_out++;
      for (u32 m = a.term_begin[t]; m < a.term_begin[t + 1]; m++, m_out++) {
        ht[m_out].coef = F::from_u64(a.coef[m]); ht[m_out].nfac = a.fac_begin[m + 1] - a.fac_begin[m];
        for (u32 f = a.fac_begin[m]; f < a.fac_begin[m + 1]; f++, f_out++) {
          const u32 fp = a.fac_poly[f];
          hf[f_out].rowoff = (u32)((size_t)a.fac_row[f] * blowup);
          if (fp & MS_AIR_PERIODIC) { const u32 k = fp & ~MS_AIR_PERIODIC; hf[f_out].src = pg.per_off[k]; hf[f_out].mask = pg.per_off[k + 1] - pg.per_off[k] - 1; hf[f_out].kind = 1; }
          else { hf[f_out].src = fp; hf[f_out].mask = (u32)(L - 1); hf[f_out].kind = 0; }
        }
      }
    }
    for (u32 rho : pg.sets[g]) hx[x_out++] = f_pow<F>(wN, (u64)rho);
    hg[g].nsegs = (u32)(s_out - s_first); hg[g].nroots = (u32)pg.sets[g].size(); hg[g].kind = 0; hg[g].moff = 0;
  }
  for (size_t k = 0; k < pg.brows.size(); k++) {     // boundary groups: (sum_b r^(ncons+b) (w^-rho P_j - w^-rho v_b)) * D[i - rho blowup]
    const size_t s_first = s_out;
    const T wr = f_pow<F>(wi, (u64)pg.brows[k]);
    for (u32 b = 0; b < a.nbound; b++) {
      if (pg.brow_of[b] != k) continue;
      for (int l = 0; l < E; l++) hs[s_out].w[l] = rpow[(size_t)ncons + b].c[l];
      hs[s_out].nterms = 2; s_out++;
      ht[m_out].coef = wr; ht[m_out].nfac = 1; m_out++;
      hf[f_out].src = a.bnd_poly[b]; hf[f_out].rowoff = 0; hf[f_out].mask = (u32)(L - 1); hf[f_out].kind = 0; f_out++;
      ht[m_out].coef = F::neg(F::mul(wr, F::from_u64(a.bnd_val[b]))); ht[m_out].nfac = 0; m_out++;
    }
    AG& gr = hg[pg.sets.size() + k];
    gr.nsegs = (u32)(s_out - s_first); gr.nroots = 0; gr.kind = 1; gr.moff = (u32)(((N - pg.brows[k]) % N) * blowup);
  }
  air_periodic_tables(a, pg, reinterpret_cast<T*>(tab + lx.off_p));
  memcpy(tab + lx.off_d, dinv.data(), dinv.size() * sizeof(T));
}

// D[i] = 1 / (x_i - 1) over the LDE domain: one table for every boundary row, kept while (N, blowup, shift) stay what it was built for
template <class F>
int Ctx<F>::air_inv_table(T gL_step) {
  if (air_inv_valid && air_inv_N == N && air_inv_blowup == blowup && air_inv_shift == lde_shift) return 0;
  typedef mspoly::CosetInvKernel<F> IK;
  static_assert(IK::THREADS == mspoly::ComposeAirKernel<F>::THREADS, "gL_step is shared");
  air_inv_valid = false;
  if (d_air_inv.ensure(L * sizeof(T))) return fail(MS_ERR_NOMEM, "mix_air: boundary inverse table");
  typename IK::Params ip{L, F::from_u64(lde_shift), f_root_of_unity<F>(ctz64(L)), gL_step, d_air_inv.as<T>()};
  next_bytes = (double)L * sizeof(T);
  CK(run<IK>(K_AIR_INV, grid1(L, IK::THREADS * IK::ITEMS), 1, IK::THREADS, 0, ip));
  air_inv_valid = true; air_inv_N = N; air_inv_blowup = blowup; air_inv_shift = lde_shift;
  return 0;
}

template <class F>
int Ctx<F>::mix_air(u64 r, const ms_air* air) {
  RQ(mix_gate("mix_air", r));
  if (!air) return fail(MS_ERR_ARG, "mix_air: null program");
  const ms_air& a = *air;
  AirProgram pg; AirLayout lay; std::vector<T> dinv;
  RQ(air_validate(a, pg, lde_c));
  RQ(air_layout(a, pg, lay));
  RQ(coset_vanishing_inv("mix_air", dinv));
  std::vector<u8> tab(lay.bytes, 0);
  air_table(r, a, pg, lay, dinv, tab.data());
  typedef mspoly::ComposeAirKernel<F> CK_;
  const T gL = f_root_of_unity<F>(ctz64(L)), gstep = f_pow<F>(gL, (u64)CK_::THREADS);
  RQ(upload_mix_table("mix_air", tab.data(), lay.bytes));
  if (a.nbound) RQ(air_inv_table(gstep));   // (behind the buffers' sizing, as every refusal for want of memory but its own)
  typename CK_::Params cp;
  cp.lde = d_lde.as<T>(); cp.L = L; cp.blowup = (u32)blowup; cp.ngroups = (u32)lay.ngroups;
  cp.groups = d_tabs.as<mspoly::AirGroup>(); cp.terms = reinterpret_cast<const mspoly::TermRec<F>*>(d_tabs.as<u8>() + lay.off_t); cp.facs = reinterpret_cast<const mspoly::AirFac*>(d_tabs.as<u8>() + lay.off_f);
  cp.roots = reinterpret_cast<const T*>(d_tabs.as<u8>() + lay.off_x); cp.ptab = reinterpret_cast<const T*>(d_tabs.as<u8>() + lay.off_p);
  cp.den_inv = reinterpret_cast<const T*>(d_tabs.as<u8>() + lay.off_d); cp.inv = a.nbound ? d_air_inv.as<T>() : nullptr;
  cp.shift = F::from_u64(lde_shift); cp.gL = gL; cp.gL_step = gstep; cp.out = d_cubic.as<T>();
  next_bytes = (double)(lay.tfacs + lay.ngroups + 1) * L * sizeof(T);
  CK(run<CK_>(K_MIX_AIR, grid1(L, CK_::THREADS * CK_::ITEMS), 1, CK_::THREADS, 0, cp));
  return finish_mix("mix_air: a transition constraint fails on a non-exempt row or a boundary value is wrong (the pointwise quotients do not interpolate to a polynomial of VL coefficients)", lay.VL);
}

template <class F>
int Ctx<F>::mix_air_ext(const u64* r, const ms_air* air) {
  RQ(mix_gate("mix_air_ext", 0));
  if (sh_on) return fail(MS_ERR_STATE, "mix_air_ext: not available on a context with sharding on");
  XE rr;
  if (!r || !load_ext(r, &rr)) return fail(MS_ERR_ARG, "mix_air_ext: r null or a limb not canonical");
  if (!air) return fail(MS_ERR_ARG, "mix_air_ext: null program");
  const ms_air& a = *air;
  AirProgram pg; AirLayout lay; std::vector<T> dinv;
  RQ(air_validate(a, pg, lde_c));
  RQ(air_layout(a, pg, lay));
  RQ(coset_vanishing_inv("mix_air_ext", dinv));
  const AirLayoutExt lx = air_layout_ext(a, pg, lay);
  std::vector<u8> tab(lx.bytes, 0);
  air_table_ext(rr, a, pg, lx, dinv, tab.data());
  typedef mspoly::ComposeAirExtKernel<F, E> CK_;
  static_assert(CK_::THREADS == mspoly::CosetInvKernel<F>::THREADS, "gL_step is shared");
  const T gL = f_root_of_unity<F>(ctz64(L)), gstep = f_pow<F>(gL, (u64)CK_::THREADS);
  RQ(upload_mix_table("mix_air_ext", tab.data(), lx.bytes, (size_t)E));
  if (a.nbound) RQ(air_inv_table(gstep));
  const u8* dt = d_tabs.as<u8>();
  typename CK_::Params cp;
  cp.lde = d_lde.as<T>(); cp.L = L; cp.blowup = (u32)blowup; cp.ngroups = (u32)lay.ngroups;
  cp.groups = reinterpret_cast<const mspoly::AirGroupExt*>(dt); cp.segs = reinterpret_cast<const mspoly::AirSeg<F, E>*>(dt + lx.off_s);
  cp.terms = reinterpret_cast<const mspoly::TermRec<F>*>(dt + lx.off_t); cp.facs = reinterpret_cast<const mspoly::AirFac*>(dt + lx.off_f);
  cp.roots = reinterpret_cast<const T*>(dt + lx.off_x); cp.ptab = reinterpret_cast<const T*>(dt + lx.off_p);
  cp.den_inv = reinterpret_cast<const T*>(dt + lx.off_d); cp.inv = a.nbound ? d_air_inv.as<T>() : nullptr;
  cp.shift = F::from_u64(lde_shift); cp.gL = gL; cp.gL_step = gstep; cp.out = d_cubic.as<T>();
  next_bytes = (double)(lx.tfacs + lay.ngroups + E) * L * sizeof(T);
  CK(run<CK_>(K_MIX_AIR_EXT, grid1(L, CK_::THREADS * CK_::ITEMS), 1, CK_::THREADS, 0, cp));
  return finish_mix("mix_air_ext: a transition constraint fails on a non-exempt row or a boundary value is wrong (a limb of the pointwise quotients does not interpolate to a polynomial of VL coefficients)", lay.VL, E);
}

// ---- ms_air_check: the program of ms_mix_air on the rows of the trace domain (mspoly::AirCheckKernel).  Diagnostic: it writes buffers of its own only (d_chk_eval,
// d_chk_tab, the table staging area) and changes nothing a later stage reads - apart from writing out lazily defined polynomials, as ms_poly_read does.
// The device table: [constraints | terms | factors | exempt rows | periodic values | boundary (poly, row) | results: count[ncons], first row[ncons], value[nbound]],
// uploaded in one copy that also sets the results to (0, N, 0); the results come back with one copy behind the launch.
template <class F>
int Ctx<F>::air_check(const ms_air* air, u64* nfail, u64* cons_count, u64* cons_first_row, u64* bnd_got) {
  if (!have_trace) return fail(MS_ERR_STATE, "air_check before trace_commit");
  if (sh_on) return fail(MS_ERR_STATE, "air_check: not available on a context with sharding on");
  if (!air || !nfail) return fail(MS_ERR_ARG, "air_check: null program or null nfail");
  const ms_air& a = *air;
  const size_t c = have_polys ? (size_t)npolys : w + (size_t)naux;   // before ms_interpolate: the trace columns and the running columns behind them
  AirProgram pg;
  if (const int e = air_validate(a, pg, c)) { if (err.compare(0, 7, "mix_air") == 0) err.replace(0, 7, "air_check"); return e; }
  typedef mspoly::AirCheckKernel<F> CKn; typedef mspoly::AirCheckCons AC; typedef mspoly::TermRec<F> TR; typedef mspoly::AirFac AF;
  const u32 ncons = a.ncons, nex = a.ex_begin[ncons], nper = a.nperiodic ? a.per_begin[a.nperiodic] : 0;
  const size_t nres = 2 * (size_t)ncons + a.nbound;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t off_t = up16((size_t)ncons * sizeof(AC)), off_f = up16(off_t + (size_t)pg.nterms * sizeof(TR)), off_x = up16(off_f + (size_t)pg.nfacs * sizeof(AF));
  const size_t off_p = up16(off_x + (size_t)nex * sizeof(u32)), off_b = up16(off_p + (size_t)nper * sizeof(T)), off_r = up16(off_b + (size_t)a.nbound * 2 * sizeof(u32));
  const size_t bytes = off_r + nres * sizeof(u64);
  if (d_chk_tab.ensure(bytes) || (have_polys && d_chk_eval.ensure(c * N * sizeof(T)))) return fail(MS_ERR_NOMEM, "air_check buffers");
  std::vector<u64> out(nres);
  u8* tab;
  RQ(tabs_host(bytes, &tab));
  memset(tab, 0, bytes);
  { AC* hc = reinterpret_cast<AC*>(tab); TR* ht = reinterpret_cast<TR*>(tab + off_t); AF* hf = reinterpret_cast<AF*>(tab + off_f);
    u32* hx = reinterpret_cast<u32*>(tab + off_x); T* hp = reinterpret_cast<T*>(tab + off_p); u32* hb = reinterpret_cast<u32*>(tab + off_b); u64* hr = reinterpret_cast<u64*>(tab + off_r);
    for (u32 t = 0; t < ncons; t++) { hc[t].nterms = a.term_begin[t + 1] - a.term_begin[t]; hc[t].nex = a.ex_begin[t + 1] - a.ex_begin[t]; hr[ncons + t] = (u64)N; }
    for (u32 m = 0; m < pg.nterms; m++) { ht[m].coef = F::from_u64(a.coef[m]); ht[m].nfac = a.fac_begin[m + 1] - a.fac_begin[m]; }
    for (u32 f = 0; f < pg.nfacs; f++) {
      const u32 fp = a.fac_poly[f];
      hf[f].rowoff = a.fac_row[f];
      if (fp & MS_AIR_PERIODIC) { const u32 k = fp & ~MS_AIR_PERIODIC; hf[f].src = a.per_begin[k]; hf[f].mask = a.per_begin[k + 1] - a.per_begin[k] - 1; hf[f].kind = 1; }
      else { hf[f].src = fp; hf[f].mask = (u32)(N - 1); hf[f].kind = 0; }
    }
    for (u32 k = 0; k < nex; k++) hx[k] = a.ex_row[k];
    for (u32 k = 0; k < nper; k++) hp[k] = F::from_u64(a.per_val[k]);
    for (u32 b = 0; b < a.nbound; b++) { hb[2 * b] = a.bnd_poly[b]; hb[2 * b + 1] = a.bnd_row[b]; } }
  // everything is decided: from here on only the runtime can fail
  const T* cols = d_polys.as<T>();
  if (have_polys) {   // the polynomials' values on the trace domain: ONE forward transform of all of them, out of place
    for (size_t i = 0; i < c; i++) RQ(materialize((int)i));
    RQ(ntt_run(ctz64(N), false, d_polys.as<T>(), N, N, d_chk_eval.as<T>(), N, c));
    cols = d_chk_eval.as<T>();
  }
  CK(msrt::h2d(d_chk_tab.p, tab, bytes, stream));
  const u8* dt = d_chk_tab.as<u8>();
  typename CKn::Params cp;
  cp.cols = cols; cp.N = N; cp.ncons = ncons; cp.nbound = a.nbound;
  cp.cons = reinterpret_cast<const AC*>(dt); cp.terms = reinterpret_cast<const TR*>(dt + off_t); cp.facs = reinterpret_cast<const AF*>(dt + off_f);
  cp.ex_rows = reinterpret_cast<const u32*>(dt + off_x); cp.ptab = reinterpret_cast<const T*>(dt + off_p); cp.bnd = reinterpret_cast<const u32*>(dt + off_b);
  cp.count = reinterpret_cast<unsigned long long*>(d_chk_tab.as<u8>() + off_r); cp.first = cp.count + ncons; cp.bnd_got = cp.first + ncons;
  next_bytes = (double)pg.nfacs * N * sizeof(T);
  CK(run_coop<CKn>(K_AIR_CHECK, grid1(N, CKn::THREADS * CKn::ITEMS), CKn::THREADS, CKn::lds_bytes(), cp));
  CK(msrt::d2h(out.data(), cp.count, nres * sizeof(u64), stream));
  CK(msrt::sync(stream));
  u64 nf = 0;
  for (u32 t = 0; t < ncons; t++) if (out[t]) nf++;
  for (u32 b = 0; b < a.nbound; b++) if (out[2 * (size_t)ncons + b] != a.bnd_val[b]) nf++;
  if (cons_count) memcpy(cons_count, out.data(), (size_t)ncons * sizeof(u64));
  if (cons_first_row) memcpy(cons_first_row, out.data() + ncons, (size_t)ncons * sizeof(u64));
  if (bnd_got && a.nbound) memcpy(bnd_got, out.data() + 2 * (size_t)ncons, (size_t)a.nbound * sizeof(u64));
  *nfail = nf;
  return MS_OK;
}

// trimmed length of a base-field coefficient vector
template <class F>
int Ctx<F>::degree_launch1(const T* poly, size_t n, unsigned long long** dres_out) {
  void* zr;
  RQ(zero_alloc(8, &zr));
  typename mspoly::DegreeKernel<F, 1>::Params dp{poly, 0, n, reinterpret_cast<unsigned long long*>(zr), 0};
  CK(run<mspoly::DegreeKernel<F, 1>>(K_DEGREE, grid1(n, mspoly::THREADS), 1, mspoly::THREADS, 0, dp));
  *dres_out = reinterpret_cast<unsigned long long*>(zr);
  return 0;
}

template <class F>
int Ctx<F>::validity_read(u64* out) {
  if (!have_validity || !out) return fail(MS_ERR_STATE, "validity_read");
  return download_widen(d_polys.as<T>() + (size_t)npolys * N, validity_len, validity_len, (u32)validity_ext, out);   // (the limbs of a coefficient consecutive)
}

// evaluate `npoly` polynomials (views) at ext point z into dst as [npoly][E] T
template <class F> template <int EC>
int Ctx<F>::eval_views(const T* base, size_t poly_stride, size_t limb_stride, size_t kstride, const size_t* off, const size_t* count, int npoly, const XE& z, T* dst, bool stage_end) {
  size_t maxc = 0;
  for (int i = 0; i < npoly; i++) if (count[i] > maxc) maxc = count[i];
  return maxc <= eval_small_max ? eval_views_i<EC, 4>(base, poly_stride, limb_stride, kstride, off, count, npoly, z, dst, maxc, stage_end)
                                : eval_views_i<EC, 16>(base, poly_stride, limb_stride, kstride, off, count, npoly, z, dst, maxc, stage_end);
}

template <class F> template <int EC, int ITEMS>
int Ctx<F>::eval_views_i(const T* base, size_t poly_stride, size_t limb_stride, size_t kstride, const size_t* off, const size_t* count, int npoly, const XE& z, T* dst, size_t maxc, bool stage_end) {
  typedef mspoly::EvalKernel<F, EC, E, ITEMS> EK;
  const size_t chunk = (size_t)EK::THREADS * EK::ITEMS;
  const size_t nblocks = maxc ? (maxc + chunk - 1) / chunk : 1;
  if (nblocks > 1 && d_partials.ensure(nblocks * npoly * E * sizeof(T))) return fail(MS_ERR_NOMEM, "partials");
  typename EK::Params p;
  p.base = base; p.poly_stride = poly_stride; p.limb_stride = limb_stride; p.kstride = kstride; p.npoly = npoly;
  for (int i = 0; i < mspoly::MAX_POLYS; i++) { p.off[i] = i < npoly ? off[i] : 0; p.count[i] = i < npoly ? count[i] : 0; }
  XE sq = z;
  for (int i = 0; i < 9; i++) { p.zpow2[i] = sq; sq = e_mul<F>(sq, sq); }
  p.partials = nblocks > 1 ? d_partials.as<T>() : dst;  // single block: P_0 is the value
  p.flag = msrt::HostFlag{nullptr, 0}; p.aux_src = nullptr; p.aux_dst = nullptr; p.single = nblocks == 1;
  if (stage_end && nblocks == 1) RQ(res.attach(p));   // the caller's LAST evaluation: its results end the stage
  CK(run_coop<EK>(K_EVAL, (unsigned)nblocks, EK::THREADS, EK::lds_bytes(), p));
  if (nblocks > 1) {
    typedef mspoly::ReducePartialsKernel<F, E> RK;
    typename RK::Params rp;
    memset(&rp, 0, sizeof rp);
    rp.partials = d_partials.as<T>(); rp.nblocks = nblocks; rp.per_thread = (nblocks + RK::THREADS - 1) / RK::THREADS; rp.npoly = npoly; rp.out = dst;
    XE zc = p.zpow2[8];  // z^256
    for (int i = 256; i < (int)chunk; i *= 2) zc = e_mul<F>(zc, zc);  // z^CH
    XE zs = zc;
    for (int i = 0; i < 8; i++) { rp.zs2[i] = zs; zs = e_mul<F>(zs, zs); }   // zc^(2^i)
    rp.zc_step = zs;                                                          // zc^256 = zc^THREADS
    static_assert(RK::THREADS == 256, "zc_step = zc^THREADS");
    if (stage_end) RQ(res.attach(rp));
    CK(run_coop<RK>(K_EVAL_REDUCE, 1, RK::THREADS, RK::lds_bytes(), rp));
  }
  return 0;
}

// sharded proof: out[i] = sum_r part_r[i] * zstep^r for n extension elements of the all-gathered partials (rank r's payload rank_stride limbs apart, the elements from `off` on)
template <class F>
int Ctx<F>::shard_combine_launch(size_t off, size_t rank_stride, u32 n, const XE& zstep, T* out) {
  typedef mspoly::ShardCombineKernel<F, E> CKn;
  typename CKn::Params cp{reinterpret_cast<const T*>(xr) + off, rank_stride, n, (u32)sh_world, zstep, out};
  CK(run<CKn>(K_EVAL_REDUCE, grid1(n, CKn::THREADS), 1, CKn::THREADS, 0, cp));
  return 0;
}

// page-locked results [q][ev.size()][E] -> out [q][npolys + 1][E] (u64)
template <class F>
int Ctx<F>::eval_finish(int q, const std::vector<int>& ev, u64* out) {
  const size_t nev = ev.size(), np = (size_t)npolys + 1;
  const T* h = pinned.as<const T>();
  std::vector<int> slot(np, -1);
  for (size_t k = 0; k < nev; k++) slot[ev[k]] = (int)k;
  std::vector<std::map<int, T>> exp_(np);
  for (int i = 0; i < npolys; i++) if (slot[i] < 0) expand(i, F::from_u64(1), exp_[i]);
  for (int t = 0; t < q; t++) {
    const T* ht = h + (size_t)t * nev * E;
    for (size_t i = 0; i < np; i++) {
      u64* o = out + ((size_t)t * np + i) * E;
      if (slot[i] >= 0) { for (int l = 0; l < E; l++) o[l] = F::to_u64(ht[(size_t)slot[i] * E + l]); continue; }
      XE acc = e_zero<F, E>();
      for (auto& kv : exp_[i]) { XE v; for (int l = 0; l < E; l++) v.c[l] = ht[(size_t)slot[kv.first] * E + l]; acc = e_add<F, E>(acc, e_mul_base<F, E>(v, kv.second)); }
      for (int l = 0; l < E; l++) o[l] = F::to_u64(acc.c[l]);
    }
  }
  return MS_OK;
}

template <class F>
int Ctx<F>::eval_ext_sharded(const u64* z, int q, u64* out) {
  const std::vector<int> ev = eval_set();
  const int nev = (int)ev.size();
  const size_t tot = (size_t)q * nev * E, W = (size_t)sh_world;
  const size_t maxlen = validity_len > N ? validity_len : N, Sx = maxlen / W, lo = (size_t)sh_rank * Sx;
  if (tot * sizeof(T) > pinned_cap) return fail(MS_ERR_ARG, "too many evaluation points");
  if (tot * sizeof(T) * W > xcap) return fail(MS_ERR_NOMEM, "exchange buffers too small for the DEEP-ALI partial sums");
  std::vector<XE> zs((size_t)q);
  for (int t = 0; t < q; t++) {
    if (!load_ext(z + (size_t)t * E, &zs[t])) return fail(MS_ERR_ARG, "query point not canonical");
    for (int i0 = 0; i0 < nev; i0 += mspoly::MAX_POLYS) {
      const int nb = (nev - i0 < mspoly::MAX_POLYS) ? nev - i0 : mspoly::MAX_POLYS;
      size_t off[mspoly::MAX_POLYS], cnt[mspoly::MAX_POLYS];
      for (int i = 0; i < nb; i++) { const int pi = ev[i0 + i]; const size_t len = (pi == npolys) ? validity_len : N; off[i] = (size_t)pi * N + lo; cnt[i] = len <= lo ? 0 : (len - lo < Sx ? len - lo : Sx); }
      { PartScope part(this); RQ((eval_views<1>(d_polys.as<T>(), 0, 0, 1, off, cnt, nb, zs[t], reinterpret_cast<T*>(xs) + ((size_t)t * nev + i0) * E))); }
    }
  }
  if (tot) {
    RQ(exchange(MS_XCHG_ALL_GATHER, tot * sizeof(T)));
    for (int t = 0; t < q; t++) RQ(shard_combine_launch((size_t)t * nev * E, tot, (u32)nev, e_pow<F, E>(zs[t], (u64)Sx), pinned.as<T>() + (size_t)t * nev * E));
    CK(msrt::sync(stream));
    RQ(eval_finish(q, ev, out));
  }
  return MS_OK;
}

// ------------------------------------------------------------------ starks.rs:124-151
template <class F>
int Ctx<F>::eval_ext(const u64* z, int q, u64* out) {
  if (!have_validity) return fail(MS_ERR_STATE, "eval_ext before mix");
  if (!z || !out || q < 0) return fail(MS_ERR_ARG, "eval_ext");
  const bool vx = validity_ext > 1;   // K-valued validity polynomial (ms_mix_air_ext): out of the base-coefficient batches, one launch of its own per point
  if (vx && sh_on) return fail(MS_ERR_STATE, "eval_ext: a validity polynomial over the extension on a context with sharding on");   // (sharding switched on behind the stage)
  if (dist_eval()) return eval_ext_sharded(z, q, out);
  const std::vector<int> ev = eval_set();
  const int nev = (int)ev.size(), nb1 = vx ? nev - 1 : nev;   // (the validity polynomial is the set's last entry)
  const size_t tot = (size_t)q * nev * E;
  if (d_small.ensure(tot * sizeof(T) + 4096)) return fail(MS_ERR_NOMEM, "small");
  if (tot * sizeof(T) > pinned_cap) return fail(MS_ERR_ARG, "too many evaluation points");
  if (!tot) return MS_OK;
  // the validity polynomial's trimmed length (ms_mix's scan) comes along on the last evaluation launch; until it has arrived, ms_fri_begin would scan for itself
  const bool fwd = validity_len_at == VLEN_DEVICE;
  unsigned long long vlen = 0;
  auto stage = res.expect(fwd ? res.word(Results::VALIDITY_LEN) : nullptr);
  if (fwd) validity_len_at = VLEN_RESCAN;
  for (int t = 0; t < q; t++) {
    XE zz;
    if (!load_ext(z + (size_t)t * E, &zz)) return fail(MS_ERR_ARG, "query point not canonical");
    for (int i0 = 0; i0 < nb1; i0 += mspoly::MAX_POLYS) {
      const int nb = (nb1 - i0 < mspoly::MAX_POLYS) ? nb1 - i0 : mspoly::MAX_POLYS;
      size_t off[mspoly::MAX_POLYS], cnt[mspoly::MAX_POLYS];
      for (int i = 0; i < nb; i++) { const int pi = ev[i0 + i]; off[i] = (size_t)pi * N; cnt[i] = (pi == npolys) ? validity_len : N; }   // the validity polynomial has 2N coefficients after ms_mix_cubic
      RQ((eval_views<1>(d_polys.as<T>(), 0, 0, 1, off, cnt, nb, zz, pinned.as<T>() + ((size_t)t * nev + i0) * E, !vx && t == q - 1 && i0 + mspoly::MAX_POLYS >= nb1)));   // results land in page-locked host memory
    }
    if (vx) {
      const size_t off = 0, cnt = validity_len;
      RQ((eval_views<E>(d_polys.as<T>() + (size_t)npolys * N, 0, validity_len, 1, &off, &cnt, 1, zz, pinned.as<T>() + ((size_t)t * nev + nb1) * E, t == q - 1)));
    }
  }
  RQ(res.collect(nullptr, nullptr, &vlen));
  if (fwd) { validity_ncoef = (size_t)vlen; validity_len_at = VLEN_HOST; }
  return eval_finish(q, ev, out);
}

// ------------------------------------------------------------------ build-defined: the composition commitment and the DEEP stage (include/ministark.h)
// ms_validity_commit: the m chunk columns of the validity polynomial evaluated on the LDE's coset - the LDE commit's own path, scale by shift^k and one size-L
// transform, a limb plane's VL / N chunks per batch - and the tree over the L x m row-major matrix.  Reads the validity polynomial, writes d_coef (scratch), d_vlde
// and d_vlde_nodes only: the polynomial, its trimmed length and a following ms_fri_begin are what they were.
template <class F>
int Ctx<F>::validity_commit(size_t lpn, u8* root) { return validity_commit_k(lpn, 0, root); }

// ms_validity_commit_coset: the chunk columns under a coset tree
template <class F>
int Ctx<F>::validity_commit_coset(int log_arity, u8* root) {
  if (!root) return fail(MS_ERR_ARG, "validity_commit_coset: null root");
  RQ(coset_arity_check("validity_commit_coset", log_arity, have_lde ? L : ~(size_t)0));
  const size_t m = have_validity ? (size_t)validity_ext * (validity_len / N) : 0;
  RQ(coset_leaf_check("validity_commit_coset", m << log_arity));
  return validity_commit_k(m << log_arity, log_arity, root);
}

template <class F>
int Ctx<F>::validity_commit_k(size_t lpn, int k, u8* root) {
  const char* const who = k ? "validity_commit_coset" : "validity_commit";
  if (sh_on) return fail(MS_ERR_STATE, std::string(who) + ": not available on a context with sharding on");
  if (stg_pending) return fail(MS_ERR_STATE, std::string(who) + ": uncommitted staged columns (ms_lde_commit_stage, or ms_lde_commit)");
  if (!have_validity) return fail(MS_ERR_STATE, std::string(who) + " before a mix stage");
  if (!have_lde || lde_ts.sharded) return fail(MS_ERR_STATE, std::string(who) + ": no committed LDE (ms_lde_commit, and no ms_polys_* since)");
  const size_t ve = (size_t)validity_ext, nch = validity_len / N, m = ve * nch;
  if (!root || lpn != m << k) return fail(MS_ERR_ARG, std::string(who) + ": null root, or lpn is not the number of chunk columns (ms_validity_ext * ms_validity_len / N)");
  TreeShape ts;
  RQ(tree_shape(L * m, lpn, 2, &ts));
  drop_vtree();   // (the buffers are rewritten from here on)
  if (d_coef.ensure(nch * N * sizeof(T)) || d_vlde.ensure(m * L * sizeof(T))) return fail(MS_ERR_NOMEM, std::string(who) + " buffers");
  auto stage = res.expect();
  const T* v = d_polys.as<T>() + (size_t)npolys * N;
  for (size_t l = 0; l < ve; l++) {   // chunk column k * ve + l = coefficients [kN, (k+1)N) of plane l
    RQ(scale_pow(v + l * validity_len, N, d_coef.as<T>(), N, N, F::from_u64(lde_shift), nch));
    RQ(ntt_run(ctz64(L), false, d_coef.as<T>(), N, N, d_vlde.as<T>() + l * L, ve * L, nch));
  }
  RQ((tree_build<1>(d_vlde.as<T>(), L >> k, 1, 0, (u32)(m << k), ts, d_vlde_nodes)));   // (k = 0: the plain view)
  RQ(read_root(d_vlde_nodes, ts, root));
  vtree_ts = ts; vtree_m = m; val_ck = k; have_vtree = true;
  return MS_OK;
}

// what ms_deep_evals and ms_deep_compose ask of a ms_deep, all of it before anything is launched; the points come back in pl.z
template <class F>
int Ctx<F>::deep_check(const char* who, const ms_deep* d, DeepPlan& pl) {
  auto bad = [&](int code, const char* what) { return fail(code, std::string(who) + what); };
  if (sh_on) return bad(MS_ERR_STATE, ": not available on a context with sharding on");
  if (!vtree_live()) return bad(MS_ERR_STATE, ": no validity tree (ms_validity_commit, and no mix stage, ms_polys_*, ms_lde_commit or ms_trace_commit since)");
  if (!d || !d->z || !d->pt_begin || !d->pt_poly) return bad(MS_ERR_ARG, ": null argument");
  if (d->npts < 1 || d->npts > (u32)mspoly::DEEP_MAX_POINTS) return bad(MS_ERR_ARG, ": npts outside 1..8");
  if (d->pt_begin[0] != 0) return bad(MS_ERR_ARG, ": pt_begin[0] must be 0");
  for (u32 t = 0; t < d->npts; t++) {
    if (d->pt_begin[t + 1] < d->pt_begin[t]) return bad(MS_ERR_ARG, ": pt_begin decreases");
    if (d->pt_begin[t + 1] == d->pt_begin[t]) return bad(MS_ERR_ARG, ": a point without entries");
    if (d->pt_begin[t + 1] > (u32)mspoly::DEEP_MAX_ENTRIES) return bad(MS_ERR_ARG, ": more than 8192 entries");
  }
  pl.entries = d->pt_begin[d->npts];
  const size_t nf = lde_c + vtree_m;
  for (size_t n = 0; n < pl.entries; n++) if (d->pt_poly[n] >= nf) return bad(MS_ERR_ARG, ": an index at or above c + m");
  pl.z.resize(d->npts);
  for (u32 t = 0; t < d->npts; t++) if (!load_ext(d->z + (size_t)t * E, &pl.z[t])) return bad(MS_ERR_ARG, ": a point is not canonical");
  const T shL = f_pow<F>(F::from_u64(lde_shift), (u64)L);
  for (u32 t = 0; t < d->npts; t++) {   // z^L = shift^L: z lies in the LDE coset, where the verifier's (x - z) vanishes for some row x
    XE zL = e_pow<F, E>(pl.z[t], (u64)L);
    bool in_coset = zL.c[0] == shL;
    for (int l = 1; l < E; l++) in_coset = in_coset && zL.c[l] == 0;
    if (in_coset) return bad(MS_ERR_SHAPE, ": a point lies in the LDE coset (z^L = shift^L)");
  }
  pl.pt_of.resize(pl.entries);
  for (u32 t = 0; t < d->npts; t++) for (u32 n = d->pt_begin[t]; n < d->pt_begin[t + 1]; n++) pl.pt_of[n] = t;
  return 0;
}

// ms_deep_evals: F_{pt_poly[n]}(z_t) in entry order - the DEEP-ALI evaluation path over views of the coefficient storage, MAX_POLYS views per launch
template <class F>
int Ctx<F>::deep_evals(const ms_deep* deep, u64* evals) {
  DeepPlan pl;
  RQ(deep_check("deep_evals", deep, pl));
  if (!evals) return fail(MS_ERR_ARG, "deep_evals: null argument");
  if (d_small.ensure(pl.entries * E * sizeof(T) + 4096)) return fail(MS_ERR_NOMEM, "deep_evals results");
  for (size_t n = 0; n < pl.entries; n++) if (deep->pt_poly[n] < lde_c) RQ(materialize((int)deep->pt_poly[n]));   // (lazily defined polynomials are written out, as by ms_poly_read)
  for (u32 t = 0; t < deep->npts; t++)
    for (u32 n0 = deep->pt_begin[t]; n0 < deep->pt_begin[t + 1]; n0 += mspoly::MAX_POLYS) {
      const int nb = (int)(deep->pt_begin[t + 1] - n0 < (u32)mspoly::MAX_POLYS ? deep->pt_begin[t + 1] - n0 : (u32)mspoly::MAX_POLYS);
      size_t off[mspoly::MAX_POLYS], cnt[mspoly::MAX_POLYS];
      for (int i = 0; i < nb; i++) { const size_t j = deep->pt_poly[n0 + i]; off[i] = j < lde_c ? j * N : chunk_off(j - lde_c); cnt[i] = N; }
      RQ((eval_views<1>(d_polys.as<T>(), 0, 0, 1, off, cnt, nb, pl.z[t], d_small.as<T>() + (size_t)n0 * E)));
    }
  std::vector<T> h(pl.entries * E);
  CK(msrt::d2h(h.data(), d_small.p, h.size() * sizeof(T), stream));
  CK(msrt::sync(stream));
  for (size_t i = 0; i < h.size(); i++) evals[i] = F::to_u64(h[i]);
  return MS_OK;
}

// ms_deep_compose: A_t = sum_n gamma^n F_n over the entries of point t (DeepCombineKernel, one pass over the columns), Q_t = (A_t - A_t(z_t)) / (x - z_t) by synthetic
// division (the suffix-Horner scan, the npts jobs of a level in one launch), D'_k = shift^k sum_t Q_t[k] (DeepSumScaleKernel).  Launches: 1 + (2 levels - 1) + 1, with
// levels = 1 up to SH_BS = 2048 coefficients, 2 up to 2048^2, 3 beyond.  d_deep_w: [A_t | Q_t], npts * E planes of N each; d_deep_tab: [column records | weights | job tables].
template <class F>
int Ctx<F>::deep_compose(const ms_deep* deep, const u64* gamma) {
  DeepPlan pl;
  RQ(deep_check("deep_compose", deep, pl));
  XE g;
  if (!gamma || !load_ext(gamma, &g)) return fail(MS_ERR_ARG, "deep_compose: gamma null or not canonical");
  const u32 npts = deep->npts;
  const size_t nf = lde_c + vtree_m;
  // the weight table (host, as air_table_ext): per named column the points that name it and, for each, the sum of gamma^n over its entries there
  std::vector<u32> mask(nf, 0);
  std::vector<XE> wsum(nf * npts, e_zero<F, E>());
  { XE gp = e_one<F, E>();
    for (size_t n = 0; n < pl.entries; n++, gp = e_mul<F>(gp, g)) {
      const size_t j = deep->pt_poly[n]; const u32 t = pl.pt_of[n];
      mask[j] |= 1u << t; wsum[j * npts + t] = e_add<F, E>(wsum[j * npts + t], gp);
    } }
  std::vector<mspoly::DeepCol> cols; std::vector<T> wtab;
  for (size_t j = 0; j < nf; j++) {
    if (!mask[j]) continue;
    cols.push_back(mspoly::DeepCol{(unsigned long long)(j < lde_c ? j * N : chunk_off(j - lde_c)), mask[j], (u32)(wtab.size() / E)});
    for (u32 t = 0; t < npts; t++) if (mask[j] & (1u << t)) for (int l = 0; l < E; l++) wtab.push_back(wsum[j * npts + t].c[l]);
  }
  const size_t plane = (size_t)E * N, scr = sh_scratch_elems(N);
  if (d_deep.ensure(plane * sizeof(T)) || d_deep_w.ensure(2 * npts * plane * sizeof(T)) || d_sh.ensure(npts * scr * sizeof(T))) return fail(MS_ERR_NOMEM, "deep_compose buffers");
  T* A = d_deep_w.as<T>(); T* Q = A + npts * plane;
  std::vector<SHPlan> sp;
  for (u32 t = 0; t < npts; t++) sp.push_back(sh_plan(A + t * plane, N, 0, 1, N, pl.z[t], Q + t * plane, false, N, 0, 1, nullptr, d_sh.as<T>() + t * scr));
  const int nl = sp[0].nl;   // (every job has N elements: the same levels)
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t off_w = up16(cols.size() * sizeof(mspoly::DeepCol)), off_j = up16(off_w + wtab.size() * sizeof(T)), jtab = (size_t)npts * sizeof(SHJ);
  const size_t bytes = off_j + (size_t)(2 * nl - 1) * jtab;
  if (d_deep_tab.ensure(bytes)) return fail(MS_ERR_NOMEM, "deep_compose tables");
  u8* ht;
  RQ(tabs_host(bytes, &ht));
  memset(ht, 0, bytes);
  memcpy(ht, cols.data(), cols.size() * sizeof(mspoly::DeepCol));
  memcpy(ht + off_w, wtab.data(), wtab.size() * sizeof(T));
  // launch order of the scans: the aggregate launches bottom-up, then the final launches top-down
  for (int k = 0; k < 2 * nl - 1; k++) {
    SHJ* hj = reinterpret_cast<SHJ*>(ht + off_j + (size_t)k * jtab);
    for (u32 t = 0; t < npts; t++) hj[t] = k < nl - 1 ? sp[t].agg[k] : sp[t].fin[2 * nl - 2 - k];
  }
  // everything is decided: from here on only the runtime can fail
  have_dpoly = false;
  for (size_t n = 0; n < pl.entries; n++) if (deep->pt_poly[n] < lde_c) RQ(materialize((int)deep->pt_poly[n]));
  CK(msrt::h2d(d_deep_tab.p, ht, bytes, stream));
  const u8* dt = d_deep_tab.as<u8>();
  auto combine = [&](auto np) -> int {
    typedef mspoly::DeepCombineKernel<F, E, decltype(np)::value> DK;
    typename DK::Params cp{d_polys.as<T>(), reinterpret_cast<const mspoly::DeepCol*>(dt), reinterpret_cast<const T*>(dt + off_w), (u32)cols.size(), npts, N, A};
    next_bytes = (double)(cols.size() + (size_t)npts * E) * N * sizeof(T);
    CK(run<DK>(K_DEEP_COMBINE, grid1((N + DK::VEC - 1) / DK::VEC, DK::THREADS), 1, DK::THREADS, 0, cp));
    return 0;
  };
  if (npts == 1) RQ(combine(std::integral_constant<int, 1>()));
  else if (npts == 2) RQ(combine(std::integral_constant<int, 2>()));
  else if (npts <= 4) RQ(combine(std::integral_constant<int, 4>()));
  else RQ(combine(std::integral_constant<int, 8>()));
  const size_t maxnb = (N + mspoly::SH_BS - 1) / mspoly::SH_BS;
  for (int k = 0; k < 2 * nl - 1; k++) {
    size_t nb = maxnb;
    const int lvl = k < nl - 1 ? k : 2 * nl - 2 - k;
    for (int i = 0; i < lvl; i++) nb = (nb + mspoly::SH_BS - 1) / mspoly::SH_BS;
    RQ(sh_launch_table(reinterpret_cast<const SHJ*>(dt + off_j + (size_t)k * jtab), npts, nb ? nb : 1, k < nl - 1 ? 0 : 1));
  }
  typedef mspoly::DeepSumScaleKernel<F, E> SK;
  const T sh = F::from_u64(lde_shift);
  typename SK::Params kp{Q, npts, N, sh, f_pow<F>(sh, (u64)SK::THREADS), d_deep.as<T>()};
  next_bytes = (double)((size_t)npts + 1) * plane * sizeof(T);
  CK(run<SK>(K_DEEP_SCALE, grid1(N, SK::THREADS * SK::ITEMS), 1, SK::THREADS, 0, kp));
  CK(msrt::sync(stream));   // (the staged tables are free again; the caller's arrays are no longer read)
  have_dpoly = true;
  return MS_OK;
}

// the members this unit defines, for both fields (the other units see declarations only; the mix stages' shared steps are called from here alone and come with them)
#define MS_INSTANTIATE(FF) \
  template int Ctx<FF>::lincomb_into(const Ctx<FF>::T* base, size_t stride, size_t n, const u64* sc, const int* idx, int k, int self_index, Ctx<FF>::T* dst); \
  template int Ctx<FF>::lincomb_linear_columns(Ctx<FF>::T* base, size_t stride, size_t n); \
  template int Ctx<FF>::lde_compute(size_t blowup_, u64 shift); \
  template int Ctx<FF>::finish_linear_columns(size_t stride, size_t n); \
  template int Ctx<FF>::lde_compute_sharded(size_t blowup_, u64 shift); \
  template int Ctx<FF>::lde_commit(size_t blowup_, u64 shift, size_t lpn, u8* root); \
  template int Ctx<FF>::lde_commit_stage(size_t lpn, u8* root); \
  template int Ctx<FF>::coset_arity_check(const char* who, int k, size_t L_); \
  template int Ctx<FF>::coset_leaf_check(const char* who, size_t lpn); \
  template bool Ctx<FF>::linear_columns_would_be_virtual() const; \
  template int Ctx<FF>::lde_commit_k(size_t blowup_, u64 shift, size_t lpn, int k, u8* root); \
  template int Ctx<FF>::lde_commit_coset(size_t blowup_, u64 shift, int log_arity, u8* root); \
  template int Ctx<FF>::lde_commit_stage_k(size_t lpn, int k, u8* root); \
  template int Ctx<FF>::lde_commit_stage_coset(int log_arity, u8* root); \
  template int Ctx<FF>::validity_commit_k(size_t lpn, int k, u8* root); \
  template int Ctx<FF>::validity_commit_coset(int log_arity, u8* root); \
  template int Ctx<FF>::bench_lde(size_t blowup_, u64 shift); \
  template int Ctx<FF>::lde_read(u64* out); \
  template int Ctx<FF>::mix(u64 r); \
  template int Ctx<FF>::mix_cubic(u64 r, const int* spec, const u64* sc, int ncons); \
  template int Ctx<FF>::mix_terms(u64 r, int ncons, const u32* term_begin, const u64* coef, const u32* fac_begin, const u32* fac_poly, const u32* fac_row, int nexempt); \
  template int Ctx<FF>::mix_air(u64 r, const ms_air* air); \
  template int Ctx<FF>::mix_air_ext(const u64* r, const ms_air* air); \
  template int Ctx<FF>::air_check(const ms_air* air, u64* nfail, u64* cons_count, u64* cons_first_row, u64* bnd_got); \
  template int Ctx<FF>::degree_launch1(const Ctx<FF>::T* poly, size_t n, unsigned long long** dres_out); \
  template int Ctx<FF>::validity_read(u64* out); \
  template int Ctx<FF>::shard_combine_launch(size_t off, size_t rank_stride, u32 n, const Ctx<FF>::XE& zstep, Ctx<FF>::T* out); \
  template int Ctx<FF>::eval_finish(int q, const std::vector<int>& ev, u64* out); \
  template int Ctx<FF>::eval_ext_sharded(const u64* z, int q, u64* out); \
  template int Ctx<FF>::eval_ext(const u64* z, int q, u64* out); \
  template int Ctx<FF>::deep_check(const char* who, const ms_deep* d, Ctx<FF>::DeepPlan& pl); \
  template int Ctx<FF>::validity_commit(size_t lpn, u8* root); \
  template int Ctx<FF>::deep_evals(const ms_deep* deep, u64* evals); \
  template int Ctx<FF>::deep_compose(const ms_deep* deep, const u64* gamma);
MS_INSTANTIATE(GL)
MS_INSTANTIATE(BB)
#undef MS_INSTANTIATE

// eval_views<EC>: base-field coefficients (DEEP-ALI, EC = 1) here, extension coefficients (a FRI round's even(z) / odd(z)) from fri_commit.cpp
#define MS_INSTANTIATE_EC(FF, EC) \
  template int Ctx<FF>::eval_views<EC>(const Ctx<FF>::T*, size_t, size_t, size_t, const size_t*, const size_t*, int, const Ctx<FF>::XE&, Ctx<FF>::T*, bool);
MS_INSTANTIATE_EC(GL, 1)
MS_INSTANTIATE_EC(GL, 2)
MS_INSTANTIATE_EC(BB, 1)
MS_INSTANTIATE_EC(BB, 4)
#undef MS_INSTANTIATE_EC

}  // namespace msctx
