// fri_query.cpp — the FRI query phase (fri.rs:115-189, merkle.rs:216-288) as a handful of batched launches over device job tables, the standalone ms_merkle_prove,
// and the build-defined openings by index (ms_tree_open, ms_fri_query_index, ms_query_linked, ms_query_linked_folded).  (The proof's way to the host: io.cpp.)
#include "ctx.hpp"

namespace msctx {

// ---- The query phase in five steps over one QueryPlan (ctx.hpp): layout of the MSFP blob -> job tables (host) -> the quotient scans -> the ranks' slices into the
// blob (sharded proofs) -> opened points, leaf lookup by value, Merkle paths.  Whatever the number of rounds and queries it is a fixed handful of batched launches:
// every per-(window, query) step is a job in a device-side table.

// 1. layout of the MSFP blob (include/ministark.h): per window and query a record (points, quotient) and two Merkle paths
template <class F>
int Ctx<F>::query_layout(QueryPlan& q, int nq) {
  const size_t W = fri_rounds - 1;  // windows (previous, round); round W is only evaluated
  q.W = W; q.nq = nq;
  q.rec_off.assign(W * nq, 0); q.path_off.assign(W * nq * 2, 0); q.qlen.assign(W ? W : 1, 0);
  size_t pos = 0;
  for (size_t i = 0; i < W; i++) {
    Round* pr = rounds[i].get();
    if (pr->D / 2 != rounds[i + 1]->D) return fail(MS_ERR_SHAPE, "round domains do not halve (fri.rs:134-137)");
    q.qlen[i] = pr->ncoef >= 3 ? pr->ncoef - 2 : 0;
    const size_t nlev = pr->ts.levels - 1;
    const size_t path_bytes = 8 + 2 * E * 8 + 8 + nlev * 2 * 32;
    for (int j = 0; j < nq; j++) {
      q.rec_off[i * nq + j] = pos;
      pos += 6 * E * 8 + 8 + q.qlen[i] * E * 8;
      q.path_off[(i * nq + j) * 2] = pos; pos += path_bytes;
      q.path_off[(i * nq + j) * 2 + 1] = pos; pos += path_bytes;
    }
  }
  q.pos = pos;
  return 0;
}

// 2. the job tables, built on the host and uploaded in ONE copy: [scan tables][find jobs][path jobs][record offsets][quotient lengths][x1][carry jobs][slice copies]
template <class F>
int Ctx<F>::query_build(QueryPlan& q, const u64* betas) {
  const size_t W = q.W; const int nq = q.nq; u8* blob = q.blob;
  T* d_h0 = q.d_h0; T* d_tg = q.d_tg; unsigned long long* d_ix = q.d_ix;
  // ---- suffix Horner jobs: (f - g)/((x-x1)(x-x2)) = Qe(x^2) + x Qo(x^2), Qe = (even(y) - even(x3))/(y - x3) and the
  //      same for odd (fri.rs:159-167); the H_0 outputs are even(x3), odd(x3) (fri.rs:151-153)
  q.x1h.assign((W + 1) * nq, 0);
  // ---- sharded proof, distributed rounds (r04): the quotient jobs BY COEFFICIENT RANGE.  Rank k runs every job over its own half-range [k*S/2, (k+1)*S/2) of the even / odd
  // coefficients with the sum over the higher ranks as carry-in (ONE all-gather of the jobs' aggregates, ShardCarryKernel, which also gives every rank the H_0's),
  // and writes its slice of every quotient polynomial - a contiguous range [t0, t1) of the record's interleaved (even, odd) coefficients - into a packed buffer;
  // the slices are then all-gathered (or gathered to rank 0: ms_shard_proof_on_root) and copied into the blob.
  typedef typename QueryPlan::CJ CJ;
  const size_t Wr = (size_t)sh_world;
  std::vector<size_t> sl_t0(Wr * W * nq, 0), sl_len(Wr * W * nq, 0), sl_off(Wr * W * nq, 0), sl_tot(Wr, 0);   // per rank and (window, query): slice start / length (extension elements) / packed byte offset
  q.any_dist = false;
  for (size_t i = 0; i <= W; i++) q.any_dist = q.any_dist || rounds[i]->dist;
  for (size_t i = 0; i < W; i++) {
    Round* pr = rounds[i].get();
    if (!pr->dist) continue;
    const size_t Sh = pr->S / 2;
    for (size_t r = 0; r < Wr; r++) for (int j = 0; j < nq; j++) {
      const size_t lo_h = r * Sh, hi_h = lo_h + Sh, q_ = q.qlen[i];
      size_t t1 = 2 * (hi_h - 1); if (t1 > q_) t1 = q_;
      size_t t0 = 2 * ((lo_h > 1 ? lo_h : 1) - 1); if (t0 > t1) t0 = t1;
      const size_t k = (r * W + i) * nq + j;
      sl_t0[k] = t0; sl_len[k] = t1 - t0; sl_off[k] = sl_tot[r]; sl_tot[r] += (t1 - t0) * E * 8;
    }
  }
  size_t pack_max = 0;
  for (size_t r = 0; r < Wr; r++) if (sl_tot[r] > pack_max) pack_max = sl_tot[r];
  if (q.any_dist && (d_pack.ensure(pack_max + 64) || d_carry.ensure(((W + 1) * nq * 2 + 1) * E * sizeof(T)))) return fail(MS_ERR_NOMEM, "query slices");
  if (q.any_dist && ((W + 1) * nq * 2 * E * sizeof(T) * Wr > xcap || xcap / Wr < 4096)) return fail(MS_ERR_NOMEM, "exchange buffers too small for the query phase");
  {
    std::vector<SHPlan> shplans;
    T* scr = d_sh.as<T>();
    for (size_t i = 0; i <= W; i++) {
      Round* pr = rounds[i].get();
      const T gp = f_root_of_unity<F>(ctz64(pr->D));
      const size_t n = pr->ncoef, mm[2] = {(n + 1) / 2, n / 2};
      for (int j = 0; j < nq; j++) {
        u64 beta = betas[j];
        if (i < W) { if (beta > pr->D) beta %= pr->D; }  // fri.rs:144-146 (quirk Q6: `>`)
        else beta %= pr->D;                             // round.domain.element(beta) wraps (fri.rs:150)
        const T x1 = f_pow<F>(gp, beta);                // fri.rs:148
        q.x1h[i * nq + j] = x1;
        const XE X3 = e_from_base<F, E>(F::mul(x1, x1));
        for (int sgn = 0; sgn < 2; sgn++) {
          void* out = nullptr;
          T* h0 = d_h0 + ((i * nq + j) * 2 + sgn) * E;
          if (pr->dist) {
            const size_t Sh = pr->S / 2, lo_h = (size_t)sh_rank * Sh, cl = mm[sgn] <= lo_h ? 0 : (mm[sgn] - lo_h < Sh ? mm[sgn] - lo_h : Sh);
            const size_t qi = q.carry_jobs.size();
            T* slot_carry = d_carry.as<T>() + qi * E;
            size_t out_off = 0;
            if (i < W) {   // the record's coefficient t sits E u64 words after coefficient t - 1: `out` is where coefficient 0 WOULD be in the packed buffer
              const size_t k = ((size_t)sh_rank * W + i) * nq + j;
              out = reinterpret_cast<u64*>(d_pack.as<u8>() + sl_off[k]) - sl_t0[k] * E;
              out_off = (size_t)sgn * E + lo_h * 2 * E;
            }
            CJ cj; memset(&cj, 0, sizeof cj);
            cj.agg_off = (u32)(qi * E); cj.has_first = 0; cj.zA = e_one<F, E>(); cj.zB = e_pow<F, E>(X3, (u64)Sh);
            cj.carry_out = slot_carry; cj.tail_out = nullptr; cj.h0_out = h0; cj.scale = e_zero<F, E>();
            if (cl) {
              SHPlan pl = sh_plan(lpoly(pr), lstride(pr), sgn, 2, cl, X3, out, true, 1, out_off, 2 * E, nullptr, scr, slot_carry, reinterpret_cast<T*>(xs) + qi * E, sh_rank > 0);
              cj.scale = carry_scale(X3, cl, pl.P);
              pl.dist = true;
              shplans.push_back(pl);
              scr += sh_scratch_elems(cl);
            }
            q.carry_jobs.push_back(cj);
            continue;
          }
          if (i < W) out = blob + q.rec_off[i * nq + j] + (6 * E + 1) * 8;
          shplans.push_back(sh_plan(pr->poly.template as<T>(), pr->cap, sgn, 2, mm[sgn], X3, out, true, 1, (size_t)sgn * E, 2 * E, h0, scr));
          scr += sh_scratch_elems(mm[sgn]);
        }
      }
    }
    int max_nl = 1;
    for (auto& pl : shplans) if (pl.nl > max_nl) max_nl = pl.nl;
    // group by level count so that every launch is homogeneous: aggregates bottom-up (the ranks' top-level aggregates last), finals top-down
    auto add = [&](std::vector<SHJ>& t, int mode, bool part) { if (!t.empty()) { q.tables.push_back(t); q.table_mode.push_back(mode); q.table_part.push_back(part ? 1 : 0); } };
    for (int nl = 1; nl <= max_nl; nl++) {
      for (int l = 0; l + 1 < nl; l++) { std::vector<SHJ> t; bool ad = true; for (auto& pl : shplans) if (pl.nl == nl) { t.push_back(pl.agg[l]); ad = ad && pl.dist; } add(t, 0, ad); }
      { std::vector<SHJ> t; for (auto& pl : shplans) if (pl.nl == nl && pl.has_top_agg) t.push_back(pl.top_agg); add(t, 0, true); }
    }
    q.n_agg_tables = q.tables.size();
    for (int nl = 1; nl <= max_nl; nl++)
      for (int l = nl - 1; l >= 0; l--) { std::vector<SHJ> t; bool ad = true; for (auto& pl : shplans) if (pl.nl == nl) { t.push_back(pl.fin[l]); ad = ad && pl.dist; } add(t, 1, ad); }
  }
  // ---- the slices' way into the blob: chunks of at most xcap / world bytes per rank and exchange
  if (q.any_dist && pack_max) {
    size_t Cb = (pack_max < ((xcap / Wr) & ~(size_t)63)) ? pack_max : ((xcap / Wr) & ~(size_t)63);
    if (shard_gather_chunk && shard_gather_chunk < Cb) Cb = shard_gather_chunk;   // MS_SHARD_GATHER_CHUNK (tests): several exchanges at small sizes
    for (size_t c0 = 0; c0 < pack_max; c0 += Cb) {
      const size_t len = pack_max - c0 < Cb ? pack_max - c0 : Cb;
      q.chunk_c0.push_back(c0); q.chunk_len.push_back(len); q.unp_first.push_back(q.unp.size());
      for (size_t r = 0; r < Wr; r++) for (size_t i = 0; i < W; i++) for (int j = 0; j < nq; j++) {
        const size_t k = (r * W + i) * nq + j, b0 = sl_off[k], b1 = b0 + sl_len[k] * E * 8;
        const size_t p0 = b0 > c0 ? b0 : c0, p1 = b1 < c0 + len ? b1 : c0 + len;
        if (p0 >= p1) continue;
        q.unp.push_back(msmerkle::CopyJob{xr + r * len + (p0 - c0), blob + q.rec_off[i * nq + j] + (6 * E + 1) * 8 + sl_t0[k] * E * 8 + (p0 - b0), p1 - p0});
      }
      q.unp_cnt.push_back(q.unp.size() - q.unp_first.back());
    }
  }
  // ---- find-first and path jobs
  typedef typename QueryPlan::FJ FJ;
  typedef typename QueryPlan::PJ PJ;
  // Sharded proof (ms_set_shard): paths are staged in the exchange buffer — every byte written by exactly one rank
  // (replicated rounds: rank 0), summed over the ranks, then copied into the blob.
  typedef typename QueryPlan::SPJ SPJ;
  const bool shard = sh_on;
  q.fjobs.resize(W);
  q.stage_bytes = 0;
  for (size_t i = 0; i < W; i++) {
    Round* pr = rounds[i].get();
    const size_t nlev = pr->ts.levels - 1, path_bytes = 8 + 2 * E * 8 + 8 + nlev * 2 * 32;
    if (pr->ts.sharded) {
      q.fjobs[i] = FJ{pr->cw.template as<T>(), 2 * pr->m, 2 * pr->m, d_tg + i * 2 * nq * E, 2 * nq, d_ix + i * 2 * nq, 2, (u32)sh_world, (u32)sh_rank, pr->m};
    } else q.fjobs[i] = FJ{pr->cw.template as<T>(), pr->D, pr->D, d_tg + i * 2 * nq * E, 2 * nq, d_ix + i * 2 * nq, 0, 0, 0, 0};
    for (int t = 0; t < 2 * nq; t++) {
      u8* dst = blob + q.path_off[(i * nq + t / 2) * 2 + (t & 1)];
      u8* out = dst;
      if (shard) { out = xs + q.stage_bytes; q.cjobs.push_back(msmerkle::CopyJob{out, dst, path_bytes}); q.stage_bytes += path_bytes; }
      if (pr->ts.sharded)
        q.sjobs.push_back(SPJ{pr->cw.template as<T>(), 2 * pr->m, pr->m, pr->nodes.template as<u32>(), pr->nodes.template as<u32>() + (2 * pr->ts.Mloc - 1) * 8, pr->ts.Mloc,
                              2, (u32)sh_world, (u32)sh_rank, (u32)nlev, d_ix + i * 2 * nq + t, out});
      else if (!shard || sh_rank == 0)
        q.pjobs.push_back(PJ{pr->cw.template as<T>(), pr->D, pr->nodes.template as<u32>(), pr->D, 2, 2, (u32)nlev, d_ix + i * 2 * nq + t, out});
    }
  }
  if (shard && (q.stage_bytes > xcap || W * nq * 2 * 8 > xcap)) return fail(MS_ERR_NOMEM, "exchange buffers too small for the query phase");
  // ---- one upload
  size_t bytes = 0;
  q.toff.assign(q.tables.size(), 0);
  for (size_t k = 0; k < q.tables.size(); k++) { q.toff[k] = bytes; bytes += q.tables[k].size() * sizeof(SHJ); }
  q.off_f = bytes; bytes += q.fjobs.size() * sizeof(FJ);
  q.off_p = bytes; bytes += q.pjobs.size() * sizeof(PJ);
  q.off_sp = bytes; bytes += q.sjobs.size() * sizeof(SPJ);
  q.off_cj = bytes; bytes += q.cjobs.size() * sizeof(msmerkle::CopyJob);
  q.off_rec = bytes; bytes += q.rec_off.size() * sizeof(size_t);
  q.off_ql = bytes; bytes += q.qlen.size() * 8;
  q.off_x1 = bytes; bytes += q.x1h.size() * sizeof(T);
  bytes = (bytes + 15) & ~(size_t)15;
  q.off_cr = bytes; bytes += q.carry_jobs.size() * sizeof(CJ);
  q.off_un = bytes; bytes += q.unp.size() * sizeof(msmerkle::CopyJob);
  u8* tab;
  RQ(tabs_host(bytes + 8, &tab));
  for (size_t k = 0; k < q.tables.size(); k++) memcpy(tab + q.toff[k], q.tables[k].data(), q.tables[k].size() * sizeof(SHJ));
  if (!q.fjobs.empty()) memcpy(tab + q.off_f, q.fjobs.data(), q.fjobs.size() * sizeof(FJ));
  if (!q.pjobs.empty()) memcpy(tab + q.off_p, q.pjobs.data(), q.pjobs.size() * sizeof(PJ));
  if (!q.sjobs.empty()) memcpy(tab + q.off_sp, q.sjobs.data(), q.sjobs.size() * sizeof(SPJ));
  if (!q.cjobs.empty()) memcpy(tab + q.off_cj, q.cjobs.data(), q.cjobs.size() * sizeof(msmerkle::CopyJob));
  if (!q.rec_off.empty()) memcpy(tab + q.off_rec, q.rec_off.data(), q.rec_off.size() * sizeof(size_t));
  memcpy(tab + q.off_ql, q.qlen.data(), q.qlen.size() * 8);
  memcpy(tab + q.off_x1, q.x1h.data(), q.x1h.size() * sizeof(T));
  if (!q.carry_jobs.empty()) memcpy(tab + q.off_cr, q.carry_jobs.data(), q.carry_jobs.size() * sizeof(CJ));
  if (!q.unp.empty()) memcpy(tab + q.off_un, q.unp.data(), q.unp.size() * sizeof(msmerkle::CopyJob));
  if (d_tabs.ensure(bytes + 8)) return fail(MS_ERR_NOMEM, "query tables");
  CK(msrt::h2d(d_tabs.p, tab, bytes + 8, stream));   // page-locked source: no synchronisation here (this stage ends with one; the area is next written by the next proof)
  q.dt = d_tabs.as<u8>();
  return 0;
}

// 3. the quotient scans: every aggregate launch, (sharded proofs) the carry exchange, every final launch
template <class F>
int Ctx<F>::query_scans(QueryPlan& q) {
  typedef typename QueryPlan::CJ CJ;
  const size_t ncarry = q.carry_jobs.size();
  auto carries = [&]() -> int {   // every aggregate is in the send buffer: one all-gather, then the carry-ins of this rank's jobs and every job's H_0
    RQ(exchange(MS_XCHG_ALL_GATHER, ncarry * E * sizeof(T)));
    return shard_carry_table(reinterpret_cast<const CJ*>(q.dt + q.off_cr), ncarry);
  };
  if (ncarry) CK(msrt::memset_dev(xs, 0, ncarry * E * sizeof(T), stream));   // aggregates of the jobs this rank has no coefficients for
  for (size_t k = 0; k < q.tables.size(); k++) {
    if (k == q.n_agg_tables && ncarry) RQ(carries());
    size_t maxnb = 1;
    for (auto& j : q.tables[k]) { size_t nb = j.m ? (j.m + mspoly::SH_BS - 1) / mspoly::SH_BS : 1; if (nb > maxnb) maxnb = nb; }
    PartScopeIf part(this, q.table_part[k] != 0);
    RQ(sh_launch_table(reinterpret_cast<const SHJ*>(q.dt + q.toff[k]), q.tables[k].size(), maxnb, q.table_mode[k]));
  }
  if (q.n_agg_tables == q.tables.size() && ncarry) RQ(carries());   // (no job on this rank at all: the exchange still has to happen - the other ranks are in it)
  return 0;
}

// 4. sharded proofs: the ranks' slices of the quotient polynomials into the blob (all-gathered, or gathered to rank 0)
template <class F>
int Ctx<F>::query_shard_assembly(QueryPlan& q) {
  for (size_t c = 0; c < q.chunk_c0.size(); c++) {
    CK(msrt::d2d(xs, d_pack.as<u8>() + q.chunk_c0[c], q.chunk_len[c], stream));
    RQ(exchange(proof_root_only ? MS_XCHG_GATHER : MS_XCHG_ALL_GATHER, q.chunk_len[c]));
    if (q.unp_cnt[c] && (!proof_root_only || sh_rank == 0)) {
      size_t maxw = 1;
      for (size_t u = 0; u < q.unp_cnt[c]; u++) { const size_t wgs = (q.unp[q.unp_first[c] + u].bytes / 8 + msmerkle::CopyRangesKernel::WORDS - 1) / msmerkle::CopyRangesKernel::WORDS; if (wgs > maxw) maxw = wgs; }
      msmerkle::CopyRangesKernel::Params up{reinterpret_cast<const msmerkle::CopyJob*>(q.dt + q.off_un) + q.unp_first[c], (u32)q.unp_cnt[c]};
      CK(run<msmerkle::CopyRangesKernel>(K_IO, (unsigned)maxw, (unsigned)q.unp_cnt[c], msmerkle::CopyRangesKernel::THREADS, 0, up));
    }
  }
  return 0;
}

// 5. the opened points (fri.rs:148-154), the leaf lookup BY VALUE (merkle.rs:216-225, quirk Q7) and the Merkle paths (merkle.rs:230-288); ends with the stage's one
// stream synchronisation
template <class F>
int Ctx<F>::query_openings(QueryPlan& q) {
  typedef typename QueryPlan::FJ FJ;
  typedef typename QueryPlan::PJ PJ;
  typedef typename QueryPlan::SPJ SPJ;
  const size_t W = q.W; const int nq = q.nq; const u8* dt = q.dt;
  const bool shard = sh_on;
  if (!W) { CK(msrt::sync(stream)); return 0; }
  typename mspoly::QueryPointsKernel<F, E>::Params qp{q.d_h0, reinterpret_cast<const T*>(dt + q.off_x1), reinterpret_cast<const u64*>(dt + q.off_ql), (int)W, nq, q.blob,
                                                     reinterpret_cast<const size_t*>(dt + q.off_rec), q.d_tg};
  CK(run<mspoly::QueryPointsKernel<F, E>>(K_QUERY_POINTS, grid1(W * nq, 64), 1, 64, 0, qp));
  CK(msrt::memset_dev(q.d_ix, 0xFF, W * nq * 2 * 8, stream));
  // first match: big codewords one launch each, the rest batched
  size_t first_small = W;
  for (size_t i = 0; i < W; i++) if (rounds[i]->D <= ((size_t)1 << 16)) { first_small = i; break; }
  for (size_t i = 0; i < first_small; i++) {
    typename mspoly::FindFirstKernel<F, E>::Params fp; fp.jobs = nullptr; fp.inline_job = q.fjobs[i];
    PartScopeIf part(this, rounds[i]->ts.sharded);
    CK(run<mspoly::FindFirstKernel<F, E>>(K_FIND_FIRST, grid1(rounds[i]->ts.sharded ? 2 * rounds[i]->m : rounds[i]->D, mspoly::THREADS), 1, mspoly::THREADS, 0, fp));
  }
  if (first_small < W) {
    typename mspoly::FindFirstKernel<F, E>::Params fp; fp.jobs = reinterpret_cast<const FJ*>(dt + q.off_f) + first_small; fp.inline_job = q.fjobs[first_small];
    CK(run<mspoly::FindFirstKernel<F, E>>(K_FIND_FIRST, grid1(rounds[first_small]->D, mspoly::THREADS), (unsigned)(W - first_small), mspoly::THREADS, 0, fp));
  }
  if (shard) {  // first match over ALL ranks' parts: minimum global index (replicated rounds: every rank holds the same value)
    CK(msrt::d2d(xs, q.d_ix, W * nq * 2 * 8, stream));
    RQ(exchange(MS_XCHG_ALL_REDUCE_MIN_U64, W * nq * 2 * 8));
    CK(msrt::d2d(q.d_ix, xs, W * nq * 2 * 8, stream));
    CK(msrt::memset_dev(xs, 0, q.stage_bytes, stream));
  }
  if (!q.pjobs.empty()) {
    typename msmerkle::PathKernel<F, E>::Params pk{reinterpret_cast<const PJ*>(dt + q.off_p), (u32)q.pjobs.size()};
    CK(run<msmerkle::PathKernel<F, E>>(K_PATH, (unsigned)q.pjobs.size(), 1, 64, 0, pk));   // one wave per opening
  }
  if (!q.sjobs.empty()) {
    typename msmerkle::ShardPathKernel<F, E>::Params sk{reinterpret_cast<const SPJ*>(dt + q.off_sp), (u32)q.sjobs.size()};
    CK(run<msmerkle::ShardPathKernel<F, E>>(K_PATH, grid1(q.sjobs.size(), 64), 1, 64, 0, sk));
  }
  if (shard) {
    RQ(exchange(MS_XCHG_ALL_REDUCE_SUM_U8, q.stage_bytes));
    msmerkle::CopyJobsKernel::Params ck{reinterpret_cast<const msmerkle::CopyJob*>(dt + q.off_cj), (u32)q.cjobs.size()};
    CK(run<msmerkle::CopyJobsKernel>(K_PATH, (unsigned)q.cjobs.size(), 1, msmerkle::CopyJobsKernel::THREADS, 0, ck));
  }
  CK(msrt::d2h(pinned.p, q.d_ix, W * nq * 2 * 8, stream));
  CK(msrt::sync(stream));
  const unsigned long long* hidx = pinned.as<const unsigned long long>();
  for (size_t t = 0; t < W * nq * 2; t++) if (hidx[t] == ~0ULL) return fail(MS_ERR_LEAF_NOT_FOUND, "leaf is not included in the tree");
  return 0;
}

// ------------------------------------------------------------------ fri.rs:115-189
// ext_out != nullptr (ms_fri_query_into): the query-phase kernels write the MSFP blob straight into the caller's buffer - page-locked host
// memory (ms_pinned_alloc; hipHostMalloc memory is mapped into the device's address space) or device memory - instead of d_blob
template <class F>
int Ctx<F>::fri_query(const u64* betas, int nq, u8* ext_out, size_t ext_cap, size_t* ext_len) {
  RQ(fri_folded_refusal("fri_query"));
  if (nrounds_done != fri_rounds || fri_rounds == 0) return fail(MS_ERR_STATE, "fri_query before the commit phase finished");
  if (!betas || nq < 1) return fail(MS_ERR_ARG, "fri_query");
  QueryPlan q;
  RQ(query_layout(q, nq));
  const size_t W = q.W, pos = q.pos;
  if (ext_len) *ext_len = pos;
  if (ext_out && ext_cap == 0) return MS_OK;   // size query: nothing is computed and the previous proof stays readable
  if (ext_out && ext_cap < pos) return fail(MS_ERR_ARG, "ms_fri_query_into: buffer too small (the size needed is in *len)");
  if (W * nq * 2 * 8 > pinned_cap) return fail(MS_ERR_ARG, "too many queries");
  blob_size = 0;
  // ---- device buffers
  size_t sh_elems = 0;
  for (size_t i = 0; i <= W; i++) sh_elems += (size_t)nq * (sh_scratch_elems((rounds[i]->ncoef + 1) / 2) + sh_scratch_elems(rounds[i]->ncoef / 2));
  const size_t n_h0 = (W + 1) * nq * 2 * E, n_tg = (W ? W : 1) * 2 * nq * E;
  if (copy_pending && !ext_out) {   // an asynchronous read-back of the previous proof: finish it before the blob moves, order it before the blob is rewritten
    if (sdma_pending || pos + 8 > d_blob.cap) RQ(fri_proof_wait()); else CK(msrt::stream_wait_event(stream, ev_copy.get()));   // (an SDMA copy is waited for on the host: it ended a whole proof ago)
  }
  if ((!ext_out && d_blob.ensure(pos + 8)) || d_sh.ensure(sh_elems * sizeof(T)) || d_targets.ensure((n_h0 + n_tg) * sizeof(T)) || d_idx.ensure((W ? W : 1) * nq * 2 * 8))
    return fail(MS_ERR_NOMEM, "query buffers");
  q.blob = ext_out ? ext_out : d_blob.as<u8>();
  blob_external = ext_out != nullptr;
  q.d_h0 = d_targets.as<T>();
  q.d_tg = q.d_h0 + n_h0;
  q.d_ix = d_idx.as<unsigned long long>();
  RQ(query_build(q, betas));
  RQ(query_scans(q));
  RQ(query_shard_assembly(q));
  RQ(query_openings(q));
  blob_size = (proof_root_only && sh_world > 1 && sh_rank != 0) ? 0 : pos;   // ms_shard_proof_on_root: the blob is whole on rank 0 only
  return MS_OK;
}

// ------------------------------------------------------------------ build-defined: Merkle openings by index (include/ministark.h)
// The view LeafHashKernel hashed and the node array of one of the context's trees; MS_ERR_STATE with the reason when the tree is not there (any more)
template <class F>
int Ctx<F>::open_view(int tree, int round, OpenView* v) {
  OpenView o;
  const TreeShape* ts = nullptr;
  if (tree == MS_TREE_TRACE) {
    if (!have_trace) return fail(MS_ERR_STATE, "tree_open: no committed trace");
    if (have_polys) return fail(MS_ERR_STATE, "tree_open: ms_interpolate has transformed the trace rows in place");
    ts = &trace_ts;
    o.base = d_polys.template as<T>(); o.col_stride = N; o.row_stride = 1; o.limb_stride = 0; o.width = (u32)w; o.nodes = d_trace_nodes.template as<u32>();
  } else if (tree == MS_TREE_LDE) {
    if (!have_lde) return fail(MS_ERR_STATE, "tree_open: no committed LDE (ms_lde_commit, and no ms_polys_* since)");
    ts = &lde_ts;
    o.base = d_lde.template as<T>(); o.col_stride = L; o.row_stride = 1; o.limb_stride = 0; o.width = (u32)lde_c0; o.lin = lde_lin(); o.nodes = d_lde_nodes.template as<u32>();   // (lde_c0: the columns ms_lde_commit hashed; a staged tree covers the ones behind them)
    if (lde_ck) { o.col_stride = L >> lde_ck; o.width = (u32)(lde_c0 << lde_ck); o.lin = nullptr; }   // coset tree: leaf group j = the rows j + t L / a, element col * a + t
  } else if (tree == MS_TREE_LDE_STAGED) {
    if (!stg_live()) return fail(MS_ERR_STATE, "tree_open: no staged LDE tree (ms_lde_commit_stage, and nothing that kills the LDE tree since)");
    ts = &stg_ts;
    o.base = d_lde.template as<T>() + lde_c0 * L; o.col_stride = L; o.row_stride = 1; o.limb_stride = 0; o.width = (u32)(lde_c - lde_c0); o.nodes = d_stg_nodes.template as<u32>();
    if (stg_ck) { o.col_stride = L >> stg_ck; o.width = (u32)((lde_c - lde_c0) << stg_ck); }
  } else if (tree == MS_TREE_VALIDITY) {
    if (!vtree_live()) return fail(MS_ERR_STATE, "tree_open: no validity tree (ms_validity_commit, and no mix stage, ms_polys_*, ms_lde_commit or ms_trace_commit since)");
    ts = &vtree_ts;
    o.base = d_vlde.template as<T>(); o.col_stride = L; o.row_stride = 1; o.limb_stride = 0; o.width = (u32)vtree_m; o.nodes = d_vlde_nodes.template as<u32>();
    if (val_ck) { o.col_stride = L >> val_ck; o.width = (u32)(vtree_m << val_ck); }
  } else if (tree == MS_TREE_FRI) {
    if (nrounds_done == 0) return fail(MS_ERR_STATE, "tree_open: no FRI round committed (ms_fri_begin)");
    if (round < 0 || (size_t)round >= nrounds_done) return fail(MS_ERR_ARG, "tree_open: round index");
    const Round* r = rounds[round].get();
    ts = &r->ts;
    o.base = r->cw.template as<T>(); o.col_stride = 0; o.row_stride = 1; o.limb_stride = r->D; o.width = 1; o.nodes = r->nodes.template as<u32>(); o.el = E;
    if (folded()) { o.col_stride = r->D >> fri_k; o.width = 1u << fri_k; }   // folded FRI: leaf group j = the coset {j + t D / a}
  } else return fail(MS_ERR_ARG, "tree_open: unknown tree id");
  if (ts->sharded || ts->ic != 2) return fail(MS_ERR_STATE, "tree_open: the tree is distributed over the ranks");
  o.lpn = (u32)ts->lpn; o.ngroups = ts->leaf_num / ts->lpn; o.nlevels = (u32)(ts->levels - 1);
  *v = o;
  return 0;
}

// The one launch of the three entry points.  jobs[k].out holds the OFFSET of the path in the output; `fin` (ms_fri_query_index, ms_query_linked): the round whose
// polynomial goes to offset 0 of the output in the same launch.  Ends with the copy to the caller and the stream synchronisation.
template <class F>
int Ctx<F>::open_launch(const std::vector<msmerkle::OpenJob<F>>& jobs, size_t out_bytes, const Round* fin, u8* out) {
  typedef msmerkle::OpenJob<F> OJ;
  typedef msmerkle::OpenKernel<F, E> OKn;
  const size_t tab_bytes = (jobs.size() * sizeof(OJ) + 255) & ~(size_t)255;
  if (d_open.ensure(tab_bytes + out_bytes + 8)) return fail(MS_ERR_NOMEM, "opening buffers");
  RQ(res.join_side());   // (MS_FLAG_LATENCY: nothing of a round's side stream is still writing what is read here)
  u8* tab;
  RQ(tabs_host(tab_bytes + 8, &tab));
  u8* dout = d_open.template as<u8>() + tab_bytes;
  if (!jobs.empty()) {
    memcpy(tab, jobs.data(), jobs.size() * sizeof(OJ));
    OJ* hj = reinterpret_cast<OJ*>(tab);
    for (size_t k = 0; k < jobs.size(); k++) hj[k].out = dout + reinterpret_cast<size_t>(jobs[k].out);
    CK(msrt::h2d(d_open.p, tab, jobs.size() * sizeof(OJ), stream));   // page-locked source; the stage ends with a synchronisation
  }
  typename OKn::Params pk{d_open.template as<const OJ>(), (u32)jobs.size(), nullptr, 0, 0, nullptr};
  size_t fin_wgs = 0;
  if (fin && fin->ncoef) {
    pk.fin = fin->poly.template as<T>(); pk.fin_stride = fin->cap; pk.fin_n = fin->ncoef; pk.fin_out = reinterpret_cast<u64*>(dout);
    fin_wgs = (fin->ncoef * (size_t)E + OKn::FIN_WORDS - 1) / OKn::FIN_WORDS;
  }
  CK(run<OKn>(K_PATH, (unsigned)(jobs.size() + fin_wgs), 1, OKn::THREADS, 0, pk));   // one wave per opening
  if (out_bytes) CK(msrt::d2h(out, dout, out_bytes, stream));
  CK(msrt::sync(stream));
  return MS_OK;
}

// n openings of one view, path k at offset off + k * path_bytes of the output: group index[k], or (`positions`: a FRI window) group index[k] / 2 with the position
// index[k] as the word the path carries
template <class F>
void Ctx<F>::open_jobs(const OpenView& v, const u64* index, size_t n, bool positions, size_t off, std::vector<msmerkle::OpenJob<F>>& jobs) const {
  const size_t pb = v.path_bytes();
  for (size_t k = 0; k < n; k++)
    jobs.push_back(msmerkle::OpenJob<F>{v.base, v.col_stride, v.row_stride, v.limb_stride, v.lin, v.nodes, v.ngroups, (size_t)(positions ? index[k] / 2 : index[k]),
                                        positions ? index[k] : index[k] * v.lpn, v.width, v.lpn, v.nlevels, (u32)v.el, reinterpret_cast<unsigned char*>(off + k * pb)});
}

template <class F>
int Ctx<F>::tree_open(int tree, int round, const u64* index, size_t n, u8* out, size_t cap, size_t* len) {
  if (!index || !len || (!out && cap)) return fail(MS_ERR_ARG, "tree_open: null argument");
  if (n < 1 || n > 65536) return fail(MS_ERR_ARG, "tree_open: n outside 1..65536");
  if (tree != MS_TREE_TRACE && tree != MS_TREE_LDE && tree != MS_TREE_FRI && tree != MS_TREE_VALIDITY && tree != MS_TREE_LDE_STAGED) return fail(MS_ERR_ARG, "tree_open: unknown tree id");
  if (sh_on) return fail(MS_ERR_STATE, "tree_open: not available on a context with sharding on");
  OpenView v;
  RQ(open_view(tree, round, &v));
  const size_t total = n * v.path_bytes();
  *len = total;
  if (!out) return MS_OK;   // size query
  if (cap < total) return fail(MS_ERR_ARG, "tree_open: buffer too small (the size needed is in *len)");
  for (size_t k = 0; k < n; k++) if (index[k] >= v.ngroups) return fail(MS_ERR_OUT_OF_RANGE, "tree_open: leaf-group index out of range");
  std::vector<msmerkle::OpenJob<F>> jobs;
  jobs.reserve(n);
  open_jobs(v, index, n, false, 0, jobs);
  return open_launch(jobs, total, nullptr, out);
}

// The FRI part of both query phases by index: the MSFI header into hd, the size of the blob behind it into *body (the final polynomial, then the windows' paths), and
// (jobs != nullptr) the openings, their offsets counted from the final polynomial's first byte.  MSFI: b_(0,j) = beta mod D_0, b_(i+1,j) = b_(i,j) mod D_(i+1), a plain modulus
template <class F>
int Ctx<F>::msfi_plan(const u64* betas, int nq, u64 hd[6], size_t* body, std::vector<msmerkle::OpenJob<F>>* jobs) {
  const size_t R = fri_rounds, W = R - 1;
  std::vector<OpenView> views(W);
  const Round* last = rounds[W].get();
  size_t pos = last->ncoef * (size_t)E * 8;
  for (size_t i = 0; i < W; i++) {
    if (rounds[i]->D / 2 != rounds[i + 1]->D) return fail(MS_ERR_SHAPE, "round domains do not halve (fri.rs:134-137)");
    RQ(open_view(MS_TREE_FRI, (int)i, &views[i]));
  }
  std::vector<u64> b(betas, betas + nq), position(2 * (size_t)nq);
  for (size_t i = 0; i < W; i++) {
    const u64 D = rounds[i]->D;
    for (int j = 0; j < nq; j++) { b[j] %= D; position[2 * j] = b[j]; position[2 * j + 1] = (b[j] + D / 2) % D; }
    if (jobs) open_jobs(views[i], position.data(), position.size(), true, pos, *jobs);
    pos += views[i].path_bytes() * position.size();
  }
  const u64 h[6] = {0x4946534DULL /* 'MSFI' */, (u64)E, (u64)R, (u64)nq, (u64)rounds[0]->D, (u64)last->ncoef};
  memcpy(hd, h, sizeof h);
  *body = pos;
  return 0;
}

// The compact query phase (MSFI, include/ministark.h): the positions ms_fri_query opens by value, opened by index, and the last round's polynomial
template <class F>
int Ctx<F>::fri_query_index(const u64* betas, int nq, u8* out, size_t cap, size_t* len) {
  RQ(fri_folded_refusal("fri_query_index"));
  if (nrounds_done != fri_rounds || fri_rounds == 0) return fail(MS_ERR_STATE, "fri_query_index before the commit phase finished");
  if (sh_on) return fail(MS_ERR_STATE, "fri_query_index: not available on a context with sharding on");
  if (!betas || !len || (!out && cap)) return fail(MS_ERR_ARG, "fri_query_index: null argument");
  if (nq < 1 || nq > 4096) return fail(MS_ERR_ARG, "fri_query_index: nq outside 1..4096");
  u64 hd[6]; size_t body;
  RQ(msfi_plan(betas, nq, hd, &body, nullptr));
  *len = sizeof hd + body;
  if (!out) return MS_OK;   // size query
  if (cap < *len) return fail(MS_ERR_ARG, "fri_query_index: buffer too small (the size needed is in *len)");
  std::vector<msmerkle::OpenJob<F>> jobs;
  jobs.reserve((fri_rounds - 1) * (size_t)nq * 2);
  RQ(msfi_plan(betas, nq, hd, &body, &jobs));
  memcpy(out, hd, sizeof hd);
  return open_launch(jobs, body, rounds[fri_rounds - 1].get(), out + sizeof hd);
}

// The whole query phase of a linked proof (MSLQ, include/ministark.h): MSFI, then the rows of the LDE tree and of the validity tree that lie under round 0's positions,
// every opening and the last round's polynomial in ONE launch.  The device image is the blob behind both headers: final polynomial | FRI paths | LDE paths | validity paths
template <class F>
int Ctx<F>::query_linked(const u64* betas, int nq, u8* out, size_t cap, size_t* len) {
  RQ(fri_folded_refusal("query_linked"));
  if (sh_on) return fail(MS_ERR_STATE, "query_linked: not available on a context with sharding on");
  if (nrounds_done != fri_rounds || fri_rounds == 0) return fail(MS_ERR_STATE, "query_linked before the commit phase finished");
  if (!dpoly_live()) return fail(MS_ERR_STATE, "query_linked: no DEEP polynomial installed (ms_validity_commit, ms_deep_compose, and nothing that kills the validity tree since)");
  const u64 D0 = rounds[0]->D;
  if (D0 > L || L % D0) return fail(MS_ERR_STATE, "query_linked: round 0's domain does not divide the LDE domain (ms_fri_begin with the LDE's blowup)");
  if (!betas || !len || (!out && cap)) return fail(MS_ERR_ARG, "query_linked: null argument");
  if (nq < 1 || nq > 4096) return fail(MS_ERR_ARG, "query_linked: nq outside 1..4096");
  const bool staged = stg_live();   // the staged layout (MSLS): a section of staged openings between the LDE and the validity openings, its length in the header
  OpenView lde, stg, val;
  RQ(open_view(MS_TREE_LDE, 0, &lde));
  if (staged) RQ(open_view(MS_TREE_LDE_STAGED, 0, &stg));
  RQ(open_view(MS_TREE_VALIDITY, 0, &val));
  if (lde.ngroups != L || val.ngroups != L) return fail(MS_ERR_STATE, "query_linked: the LDE tree does not hold one row per leaf group (ms_lde_commit with lpn = the number of polynomials)");
  if (staged && stg.ngroups != L) return fail(MS_ERR_STATE, "query_linked: the staged LDE tree does not hold one row per leaf group (ms_lde_commit_stage with lpn = the number of staged columns)");
  const size_t nh = staged ? 5 : 4;
  u64 hd[5 + 6]; size_t body;
  RQ(msfi_plan(betas, nq, hd + nh, &body, nullptr));
  const size_t nrows = 2 * (size_t)nq, len_lde = nrows * lde.path_bytes(), len_stg = staged ? nrows * stg.path_bytes() : 0, len_val = nrows * val.path_bytes();
  hd[0] = staged ? 0x534C534DULL /* 'MSLS' */ : 0x514C534DULL /* 'MSLQ' */; hd[1] = 6 * 8 + body; hd[2] = len_lde; hd[nh - 2] = staged ? len_stg : len_lde; hd[nh - 1] = len_val;
  const size_t hbytes = (nh + 6) * 8;
  *len = hbytes + body + len_lde + len_stg + len_val;
  if (!out) return MS_OK;   // size query
  if (cap < *len) return fail(MS_ERR_ARG, "query_linked: buffer too small (the size needed is in *len)");
  std::vector<msmerkle::OpenJob<F>> jobs;
  jobs.reserve(((fri_rounds - 1) + 3) * nrows);
  RQ(msfi_plan(betas, nq, hd + nh, &body, &jobs));
  std::vector<u64> rows(nrows);   // round-0 position b is LDE row b * (L / D_0); its partner b + D_0 / 2 is row + L / 2
  for (int j = 0; j < nq; j++) { rows[2 * j] = betas[j] % D0 * (L / D0); rows[2 * j + 1] = (rows[2 * j] + L / 2) % L; }
  open_jobs(lde, rows.data(), nrows, false, body, jobs);
  if (staged) open_jobs(stg, rows.data(), nrows, false, body + len_lde, jobs);
  open_jobs(val, rows.data(), nrows, false, body + len_lde + len_stg, jobs);
  memcpy(out, hd, hbytes);
  return open_launch(jobs, body + len_lde + len_stg + len_val, rounds[fri_rounds - 1].get(), out + hbytes);
}

// The query phase of a folded FRI (MSFF, include/ministark.h): per round and query ONE opening, the leaf group b_(i+1,j) = the coset holding position b_(i,j), and the
// final polynomial, in one launch.  Each path is what ms_tree_open(MS_TREE_FRI, i, [b_(i+1,j)]) returns
template <class F>
int Ctx<F>::fri_query_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) {
  if (!folded()) return fail(MS_ERR_STATE, "fri_query_folded outside folded mode (ms_fri_begin_folded)");
  if (!fold_final_done) return fail(MS_ERR_STATE, "fri_query_folded before fri_fold_final");
  if (sh_on) return fail(MS_ERR_STATE, "fri_query_folded: not available on a context with sharding on");
  if (!betas || !len || (!out && cap)) return fail(MS_ERR_ARG, "fri_query_folded: null argument");
  if (nq < 1 || nq > 4096) return fail(MS_ERR_ARG, "fri_query_folded: nq outside 1..4096");
  u64 hd[7]; size_t body;
  RQ(msff_plan(betas, nq, hd, &body, nullptr));
  *len = sizeof hd + body;
  if (!out) return MS_OK;   // size query
  if (cap < *len) return fail(MS_ERR_ARG, "fri_query_folded: buffer too small (the size needed is in *len)");
  std::vector<msmerkle::OpenJob<F>> jobs;
  jobs.reserve(nrounds_done * (size_t)nq);
  RQ(msff_plan(betas, nq, hd, &body, &jobs));
  memcpy(out, hd, sizeof hd);
  return open_launch(jobs, body, &fold_fin, out + sizeof hd);
}

template <class F>
int Ctx<F>::msff_plan(const u64* betas, int nq, u64 hd[7], size_t* body, std::vector<msmerkle::OpenJob<F>>* jobs) {
  const size_t R = nrounds_done, nfinal = fold_fin.ncoef;
  std::vector<OpenView> views(R);
  for (size_t i = 0; i < R; i++) RQ(open_view(MS_TREE_FRI, (int)i, &views[i]));
  std::vector<u64> b(betas, betas + nq);
  size_t pos = nfinal * (size_t)E * 8;
  for (int j = 0; j < nq; j++) b[j] %= rounds[0]->D;                       // b_(0,j)
  for (size_t i = 0; i < R; i++) {
    for (int j = 0; j < nq; j++) b[j] %= rounds[i]->D >> fri_k;            // b_(i+1,j): the leaf group of round i
    if (jobs) open_jobs(views[i], b.data(), (size_t)nq, false, pos, *jobs);
    pos += views[i].path_bytes() * (size_t)nq;
  }
  const u64 h[7] = {0x4646534DULL /* 'MSFF' */, (u64)E, (u64)fri_k, (u64)R, (u64)nq, (u64)rounds[0]->D, (u64)nfinal};
  memcpy(hd, h, sizeof h);
  *body = pos;
  return 0;
}

// The whole query phase of a linked proof over a folded FRI (MSLF, include/ministark.h): MSFF, then ONE leaf group per query of every coset row tree - the group that holds the LDE rows
// under round 0's coset - every opening and the final polynomial in ONE launch.  The device image is the blob behind both headers: final polynomial | FRI paths | LDE
// paths | staged paths | validity paths
template <class F>
int Ctx<F>::query_linked_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len) {
  if (!folded()) return fail(MS_ERR_STATE, "query_linked_folded outside folded mode (ms_fri_begin_folded)");
  if (!fold_final_done) return fail(MS_ERR_STATE, "query_linked_folded before fri_fold_final");
  if (sh_on) return fail(MS_ERR_STATE, "query_linked_folded: not available on a context with sharding on");
  if (!dpoly_live()) return fail(MS_ERR_STATE, "query_linked_folded: no DEEP polynomial installed (ms_validity_commit_coset, ms_deep_compose, and nothing that kills the validity tree since)");
  const u64 D0 = rounds[0]->D;
  if (D0 > L || L % D0) return fail(MS_ERR_STATE, "query_linked_folded: round 0's domain does not divide the LDE domain (ms_fri_begin_folded with the LDE's blowup)");
  const bool staged = stg_live();
  if (lde_ck != fri_k || val_ck != fri_k || (staged && stg_ck != fri_k))
    return fail(MS_ERR_STATE, "query_linked_folded: a row tree is not a coset tree of the FRI's log_arity (ms_lde_commit_coset, ms_lde_commit_stage_coset, ms_validity_commit_coset)");
  if (!betas || !len || (!out && cap)) return fail(MS_ERR_ARG, "query_linked_folded: null argument");
  if (nq < 1 || nq > 4096) return fail(MS_ERR_ARG, "query_linked_folded: nq outside 1..4096");
  OpenView lde, stg, val;
  RQ(open_view(MS_TREE_LDE, 0, &lde));
  if (staged) RQ(open_view(MS_TREE_LDE_STAGED, 0, &stg));
  RQ(open_view(MS_TREE_VALIDITY, 0, &val));
  u64 hd[5 + 7]; size_t body;
  RQ(msff_plan(betas, nq, hd + 5, &body, nullptr));
  const size_t n = (size_t)nq, len_lde = n * lde.path_bytes(), len_stg = staged ? n * stg.path_bytes() : 0, len_val = n * val.path_bytes();
  hd[0] = 0x464C534DULL /* 'MSLF' */; hd[1] = 7 * 8 + body; hd[2] = len_lde; hd[3] = len_stg; hd[4] = len_val;
  *len = sizeof hd + body + len_lde + len_stg + len_val;
  if (!out) return MS_OK;   // size query
  if (cap < *len) return fail(MS_ERR_ARG, "query_linked_folded: buffer too small (the size needed is in *len)");
  std::vector<msmerkle::OpenJob<F>> jobs;
  jobs.reserve((nrounds_done + 3) * n);
  RQ(msff_plan(betas, nq, hd + 5, &body, &jobs));
  std::vector<u64> groups(n);   // round 0's coset {q + t D_1} lies over the LDE rows q s + t L / a, s = L / D_0: leaf group q s
  for (int j = 0; j < nq; j++) groups[j] = betas[j] % D0 % (D0 >> fri_k) * (L / D0);
  open_jobs(lde, groups.data(), n, false, body, jobs);
  if (staged) open_jobs(stg, groups.data(), n, false, body + len_lde, jobs);
  open_jobs(val, groups.data(), n, false, body + len_lde + len_stg, jobs);
  memcpy(out, hd, sizeof hd);
  return open_launch(jobs, body + len_lde + len_stg + len_val, &fold_fin, out + sizeof hd);
}

// src/merkle.rs:272-288 on a standalone binary tree: leaves de-interleaved to SoA limbs, then the same
// LeafHash / InnerHash / FindFirst / MerklePath kernels the FRI query phase uses
template <class F> template <int EL>
int Ctx<F>::merkle_prove_t(const u64* leafs, size_t leaf_num, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len) {
  TreeShape ts;
  RQ(tree_shape(leaf_num, lpn, 2, &ts));
  if (!canonical(leafs, leaf_num * EL) || !canonical(leaf, EL)) return fail(MS_ERR_ARG, "leaf not canonical");
  const size_t plen = 8 + lpn * EL * 8 + 8 + (ts.levels - 1) * 2 * 32;
  if (len) *len = plen;
  if (!out || cap < plen) return fail(MS_ERR_ARG, "path buffer too small");
  DevBuf ds, dn, dw;  // SoA leaves | nodes | {target | idx | job tables | path}
  typedef mspoly::FindJob<F, EL> FJ;
  typedef msmerkle::PathJob<F, EL> PJ;
  const size_t off_ix = 256, off_pj = 512, off_path = 1024;
  auto idle = scope_exit([&] { msrt::sync(stream); });   // (before ds, dn and dw go: a launch may still read them on an early exit; the stack sources below likewise)
  if (ds.ensure(leaf_num * EL * sizeof(T)) || dw.ensure(off_path + plen) || d_io.ensure(leaf_num * EL * 8)) return fail(MS_ERR_NOMEM, "merkle_prove");
  CK(msrt::h2d(d_io.p, leafs, leaf_num * EL * 8, stream));
  RQ(transpose_in(d_io.as<u64>(), ds.as<T>(), leaf_num, (size_t)EL, F::from_u64(1), 0, nullptr));
  RQ(tree_build<EL>(ds.as<T>(), 0, 1, leaf_num, 1, ts, dn));
  T tgt[EL]; for (int l = 0; l < EL; l++) tgt[l] = F::from_u64(leaf[l]);
  unsigned long long none = ~0ULL;
  u8* base = dw.as<u8>();
  PJ pj{ds.as<T>(), leaf_num, dn.as<u32>(), leaf_num, (u32)lpn, 2, (u32)(ts.levels - 1), reinterpret_cast<unsigned long long*>(base + off_ix), base + off_path};
  CK(msrt::h2d(base, tgt, sizeof tgt, stream));
  CK(msrt::h2d(base + off_ix, &none, 8, stream));
  CK(msrt::h2d(base + off_pj, &pj, sizeof pj, stream));
  CK(msrt::sync(stream));  // stack sources
  typename mspoly::FindFirstKernel<F, EL>::Params fp; fp.jobs = nullptr;
  fp.inline_job = FJ{ds.as<T>(), leaf_num, leaf_num, reinterpret_cast<const T*>(base), 1, reinterpret_cast<unsigned long long*>(base + off_ix)};
  CK(run<mspoly::FindFirstKernel<F, EL>>(K_FIND_FIRST, grid1(leaf_num, mspoly::THREADS), 1, mspoly::THREADS, 0, fp));   // merkle.rs:216-225
  typename msmerkle::PathKernel<F, EL>::Params pk{reinterpret_cast<const PJ*>(base + off_pj), 1};
  CK(run<msmerkle::PathKernel<F, EL>>(K_PATH, 1, 1, 64, 0, pk));                                                          // merkle.rs:230-288
  CK(msrt::d2h(pinned.p, base + off_ix, 8, stream));
  CK(msrt::d2h(out, base + off_path, plen, stream));
  CK(msrt::sync(stream));
  if (*pinned.as<unsigned long long>() == ~0ULL) return fail(MS_ERR_LEAF_NOT_FOUND, "leaf is not included in the tree");
  return MS_OK;
}

template <class F>
int Ctx<F>::merkle_prove(const u64* leafs, size_t leaf_num, int ext, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len) {
  if (!leafs || !leaf) return fail(MS_ERR_ARG, "null argument");
  if (ext == 1) return merkle_prove_t<1>(leafs, leaf_num, lpn, leaf, out, cap, len);
  if (ext == E) return merkle_prove_t<E>(leafs, leaf_num, lpn, leaf, out, cap, len);
  return fail(MS_ERR_ARG, "ext must be 1 or the field's extension degree");
}

// the members this unit defines, for both fields (the other units see declarations only)
#define MS_INSTANTIATE(FF) \
  template int Ctx<FF>::query_layout(Ctx<FF>::QueryPlan& q, int nq); \
  template int Ctx<FF>::query_build(Ctx<FF>::QueryPlan& q, const u64* betas); \
  template int Ctx<FF>::query_scans(Ctx<FF>::QueryPlan& q); \
  template int Ctx<FF>::query_shard_assembly(Ctx<FF>::QueryPlan& q); \
  template int Ctx<FF>::query_openings(Ctx<FF>::QueryPlan& q); \
  template int Ctx<FF>::fri_query(const u64* betas, int nq, u8* ext_out, size_t ext_cap, size_t* ext_len); \
  template int Ctx<FF>::merkle_prove(const u64* leafs, size_t leaf_num, int ext, size_t lpn, const u64* leaf, u8* out, size_t cap, size_t* len); \
  template int Ctx<FF>::open_view(int tree, int round, Ctx<FF>::OpenView* v); \
  template int Ctx<FF>::tree_open(int tree, int round, const u64* index, size_t n, u8* out, size_t cap, size_t* len); \
  template int Ctx<FF>::fri_query_index(const u64* betas, int nq, u8* out, size_t cap, size_t* len); \
  template int Ctx<FF>::query_linked(const u64* betas, int nq, u8* out, size_t cap, size_t* len); \
  template int Ctx<FF>::fri_query_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len); \
  template int Ctx<FF>::msff_plan(const u64* betas, int nq, u64 hd[7], size_t* body, std::vector<msmerkle::OpenJob<FF>>* jobs); \
  template int Ctx<FF>::query_linked_folded(const u64* betas, int nq, u8* out, size_t cap, size_t* len);
MS_INSTANTIATE(GL)
MS_INSTANTIATE(BB)
#undef MS_INSTANTIATE

}  // namespace msctx
