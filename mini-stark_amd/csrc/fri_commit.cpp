// fri_commit.cpp — the FRI commit phase (fri.rs:64-113, 301-377): round commitments, even(z) / odd(z), fold + DEEP quotient (replicated and by coefficient range),
// and the suffix-Horner job planning the query phase shares.
#include "ctx.hpp"
#include "digest.hpp"
#include "fri_tail.hpp"

namespace msctx {

// codeword + tree of rounds[i] from its coefficient limbs (ncoef_in valid coefficients)
// `nonzero_limbs`: limbs >= this are identically zero (round 0: extend_poly embeds base coefficients), so their
// transform is all zeros and is not computed
// `prev` != nullptr: the codeword is folded out of prev's codeword in the evaluation domain (FriFoldEvalKernel / FriFoldWgKernel) instead of
// transforming the round polynomial — same values, a quarter of the arithmetic
template <class F>
int Ctx<F>::round_commit(Round* r, size_t ncoef_in, int nonzero_limbs, const Round* prev, const XE* alpha) {
  if (ctz64(r->D) > F::TWO_ADICITY) return fail(MS_ERR_SHAPE, "FRI domain larger than the field's two-adicity");
  RQ(tree_shape(r->D, 2, 2, &r->ts));  // starks.rs:290-295: leafs_per_node 2, inner_children 2
  r->m = 0;
  r->base_cw = false;
  {
    const bool shard_next = shardable(r->D / 2);
    bool z_outside_base = false;   // then y - z != 0 on the whole (base-field) domain
    for (int l = 1; l < E; l++) z_outside_base = z_outside_base || cur_z.c[l] != 0;
    if (prev && fri_pointwise && z_outside_base && prev->D == 2 * r->D && prev->ts.sharded == shard_next) {
      Plan* pl;
      RQ(get_plan(ctz64(prev->D), 0, false, &pl));   // w_D^e tables of the previous domain
      // one output per thread in the late rounds (at most MS_FOLD_SMALL_MAX outputs: their launches are latency, not throughput), eight otherwise (FriFoldWgKernel)
      const size_t W = (size_t)sh_world;
      const size_t m_out = shard_next ? r->D / (2 * W) : r->D;
      const size_t local = shard_next ? 2 * m_out : r->D;       // elements per limb held here
      if (shard_next) r->m = m_out;
      if (r->cw.ensure(local * E * sizeof(T))) return fail(MS_ERR_NOMEM, "codeword");
      const size_t total = m_out * (shard_next ? 2 : 1);
      const XE c = e_add<F, E>(cur_B[0], e_mul<F>(cur_B[1], *alpha));   // B(alpha), fri.rs:99
      auto fold_params = [&](auto& fp) {
        fp.src = prev->cw.template as<T>(); fp.src_limb_stride = shard_next ? 2 * prev->m : prev->D;
        fp.dst = r->cw.template as<T>(); fp.dst_limb_stride = local;
        fp.m_out = m_out; fp.log_m = (u32)ctz64(m_out); fp.groups = shard_next ? 2 : 1; fp.shard_W = shard_next ? (u32)W : 0; fp.shard_k = (u32)sh_rank;
        fp.tw_lo = pl->tw_lo.template as<T>(); fp.tw_hi = pl->tw_hi.template as<T>(); fp.lo_bits = (u32)pl->lo_bits; fp.log_D = (u32)ctz64(prev->D);
        fp.alpha = *alpha;
        fp.c2 = e_add<F, E>(c, c);
        fp.z = cur_z;
        fp.inv2 = f_inv<F>(F::from_u64(2));
      };
      auto fold_launch = [&](auto* kernel) {   // the latency form: one output per thread
        typedef typename std::remove_pointer<decltype(kernel)>::type FK;
        typename FK::Params fp;
        fold_params(fp);
        return run<FK>(K_FOLD, grid1(total, FK::THREADS * FK::ITEMS), 1, FK::THREADS, 0, fp);
      };
      // Octet layout of the throughput form (Goldilocks): the plan's w_D^(D/16) is a primitive 16th root of unity, so it is (2^12)^mm for ONE odd mm (2 has order 192);
      // item k of a thread then wants the position e = k / mm (mod 16) of its sixteen points x0 w_16^e, i.e. output e mod 8 with f(x) and f(-x) swapped if e >= 8
      // (w_16^8 = -1), and 2^(-12 k) = -2^(96 - 12 k) for k > 0 flips the sign once more.  No mm found (another field, a root that is no power of 2): item layout.
      u32 oct_q[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oct_neg = 0;
      bool oct = false;
      if constexpr (F::ID == 0) {
        if (!shard_next && m_out >= 8 && (m_out & (m_out - 1)) == 0) {
          const T w16 = f_pow<F>(pl->root, (u64)(prev->D / 16));
          for (u32 mm = 1; mm < 16 && !oct; mm += 2) {
            if (f_pow<F>(F::from_u64((u64)1 << 12), mm) != w16) continue;
            u32 minv = 1; while ((mm * minv) % 16 != 1) minv += 2;
            for (u32 k = 0; k < 8; k++) { const u32 e = (k * minv) % 16; oct_q[k] = e % 8; if ((e >= 8) != (k > 0)) oct_neg |= 1u << k; }
            oct = true;
          }
        }
      }
      auto wg_launch = [&](auto* kernel) {     // the throughput form: eight outputs per thread, one inversion per workgroup
        typedef typename std::remove_pointer<decltype(kernel)>::type FK;
        typename FK::Params wp;
        fold_params(wp.f);
        for (int k = 0; k < 8; k++) wp.oct_q[k] = oct_q[k];
        wp.oct_neg = oct_neg;
        return run_coop<FK>(K_FOLD, grid1(FK::grid_items(wp), FK::THREADS), FK::THREADS, FK::lds_bytes(), wp);
      };
      const bool src1 = prev->base_cw;          // round 0 -> 1: f(x) +- f(-x) are base elements
      next_bytes = (double)total * (E + 2 * (src1 ? 1 : E)) * sizeof(T);   // two inputs read, one output written per element
      { PartScopeIf part(this, shard_next);
        if (total <= fold_small_max) CK(fold_launch((mspoly::FriFoldEvalKernel<F, E, 1>*)nullptr));
        else if constexpr (F::ID == 0) {
          if (oct) CK(src1 ? wg_launch((mspoly::FriFoldWgKernel<F, E, 1, true>*)nullptr) : wg_launch((mspoly::FriFoldWgKernel<F, E, E, true>*)nullptr));
          else CK(src1 ? wg_launch((mspoly::FriFoldWgKernel<F, E, 1, false>*)nullptr) : wg_launch((mspoly::FriFoldWgKernel<F, E, E, false>*)nullptr));
        } else CK(src1 ? wg_launch((mspoly::FriFoldWgKernel<F, E, 1, false>*)nullptr) : wg_launch((mspoly::FriFoldWgKernel<F, E, E, false>*)nullptr)); }
      if (shard_next) RQ((tree_build_sharded<E>(r->cw.template as<T>(), m_out, 1, 2 * m_out, 2, r->ts, r->nodes)));
      else RQ((tree_build<E>(r->cw.template as<T>(), 0, 1, r->D, 1, r->ts, r->nodes)));
      return 0;
    }
  }
  RQ(res.join_side());   // from here on the round polynomial itself is transformed: the side stream's quotient must be complete
  if (shardable(r->D / 2)) {  // leaf group j = codeword elements 2j, 2j+1: rank k owns the groups k (mod world) = two cosets of size m
    const size_t m = r->D / (2 * (size_t)sh_world);
    r->m = m;
    if (r->cw.ensure(2 * m * E * sizeof(T))) return fail(MS_ERR_NOMEM, "codeword");
    const T* coef = r->poly.template as<T>(); size_t coef_stride = r->cap;
    if (r->local_store) {   // the transform needs every coefficient (a DEEP point in the base field / MS_FRI_POINTWISE=0): gather the parts of the distributed polynomial
      const size_t full = r->S * (size_t)sh_world;
      if (d_fullpoly.ensure(full * E * sizeof(T))) return fail(MS_ERR_NOMEM, "gathered polynomial");
      if (ncoef_in) RQ(gather_poly(lpoly(r), r->S, ncoef_in, d_fullpoly.as<T>(), full));
      coef = d_fullpoly.as<T>(); coef_stride = full;
    }
    { PartScope part(this); RQ(coset_eval(coef, coef_stride, ncoef_in, ctz64(r->D), F::from_u64(1), 2, r->cw.template as<T>(), 2 * m, (size_t)nonzero_limbs)); }
    if (nonzero_limbs < E) CK(msrt::memset_dev(r->cw.template as<T>() + (size_t)nonzero_limbs * 2 * m, 0, (size_t)(E - nonzero_limbs) * 2 * m * sizeof(T), stream));
    r->base_cw = nonzero_limbs == 1;
    RQ((tree_build_sharded<E>(r->cw.template as<T>(), m, 1, 2 * m, 2, r->ts, r->nodes)));
    return 0;
  }
  if (r->cw.ensure(r->D * E * sizeof(T))) return fail(MS_ERR_NOMEM, "codeword");
  RQ(ntt_run(ctz64(r->D), false, r->poly.template as<T>(), r->cap, ncoef_in, r->cw.template as<T>(), r->D, (size_t)nonzero_limbs));  // fri.rs:350
  if (nonzero_limbs < E) CK(msrt::memset_dev(r->cw.template as<T>() + (size_t)nonzero_limbs * r->D, 0, (size_t)(E - nonzero_limbs) * r->D * sizeof(T), stream));
  r->base_cw = nonzero_limbs == 1;
  RQ((tree_build<E>(r->cw.template as<T>(), 0, 1, r->D, 1, r->ts, r->nodes)));                                       // fri.rs:351
  return 0;
}

// trimmed length of a round polynomial (DegreeKernel) into a zeroed device word
template <class F>
int Ctx<F>::degree_launch(const T* poly, size_t limb_stride, size_t n, unsigned long long** dres_out) {
  void* zr;
  RQ(zero_alloc(8, &zr));
  unsigned long long* dres = reinterpret_cast<unsigned long long*>(zr);
  if (n) {
    typename mspoly::DegreeKernel<F, E>::Params dp{poly, limb_stride, n, dres, 0};
    CK(run<mspoly::DegreeKernel<F, E>>(K_DEGREE, grid1(n, mspoly::THREADS), 1, mspoly::THREADS, 0, dp));
  }
  *dres_out = dres;
  return 0;
}

// fri.rs:73-82
template <class F>
int Ctx<F>::fri_begin(size_t blowup_, size_t nrounds, u8* root0) {
  if (!have_validity) return fail(MS_ERR_STATE, "fri_begin before mix");
  if (!root0 || nrounds < 1 || !blowup_) return fail(MS_ERR_ARG, "fri_begin");
  nrounds_done = 0; have_deep = false; blob_size = 0;
  fri_rounds = nrounds; fri_blowup = blowup_; fri_k = 0; fold_final_done = false;   // (either ms_fri_begin* starts afresh)
  // the self-clearing length word (and completion counter) of ms_fri_fold_commit: zeroed HERE, behind this stage's stream synchronisation - zeroing it
  // lazily in the first ms_fri_fold_commit raced with the side stream's length scan (r05: first proof of a context, eight lanes in flight) - and zero again even if
  // an earlier proof was abandoned mid-round
  static_assert(Results::TAIL_DONE == Results::FRI_LEN + 128, "one fill clears both lines");
  CK(msrt::memset_dev(res.word(Results::FRI_LEN), 0, 256, stream));
  Round* r = round_slot(0);
  const bool dp = dpoly_live();       // ms_deep_compose: round 0 starts from the DEEP polynomial D' (N coefficients, E limbs N apart) in place of the validity polynomial
  const size_t VL = dp ? N : validity_len;   // N (ms_mix) or 2N (ms_mix_cubic)
  r->cap = VL;
  if (r->poly.ensure(VL * E * sizeof(T))) return fail(MS_ERR_NOMEM, "round poly");
  const bool vx = dp || validity_ext > 1;   // ms_mix_air_ext: the validity polynomial has its E limbs already, VL apart as the round's are
  if (vx && sh_on) return fail(MS_ERR_STATE, "fri_begin: a validity polynomial over the extension on a context with sharding on");
  if (dp) CK(msrt::d2d(r->poly.p, d_deep.p, VL * E * sizeof(T), stream));
  else if (vx) CK(msrt::d2d(r->poly.p, d_polys.as<T>() + (size_t)npolys * N, VL * E * sizeof(T), stream));
  else {
  // field.rs:23-32 extend_poly: limb 0 = validity, higher limbs zero
  CK(msrt::memset_dev(r->poly.p, 0, VL * E * sizeof(T), stream));
  CK(msrt::d2d(r->poly.p, d_polys.as<T>() + (size_t)npolys * N, VL * sizeof(T), stream));
  }
  unsigned long long nc = validity_ncoef;   // (came to the host with DEEP-ALI's values: ms_mix scans, ms_eval_ext forwards)
  if (dp || validity_len_at != VLEN_HOST) {   // a scan of its own and a copy behind it (the validity polynomial's length, where known, is not D''s)
    unsigned long long* dres;
    RQ(degree_launch(r->poly.template as<T>(), r->cap, VL, &dres));
    auto scan = res.expect(dres, false, false);
    RQ(res.collect(nullptr, nullptr, &nc));
  }
  r->ncoef = (size_t)nc;
  const size_t deg = nc ? nc - 1 : 0;
  size_t dsize = (deg + 1) * blowup_;  // fri.rs:74 (quirk Q11)
  size_t D = 1; while (D < dsize) D <<= 1;
  r->D = D;
  r->S = dist_chunk(D); r->dist = r->S != 0; r->local_store = false;   // the validity polynomial is replicated: a distributed round 0 means every rank WORKS on its range of it
  auto stage = res.expect();
  RQ(round_commit(r, (size_t)nc, vx ? E : 1));
  RQ(read_root(r->nodes, r->ts, root0));
  nrounds_done = 1;
  return MS_OK;
}

// fri.rs:89-94
template <class F>
int Ctx<F>::fri_deep(const u64* z, u64* B) {
  RQ(fri_folded_refusal("fri_deep"));
  if (nrounds_done == 0 || nrounds_done >= fri_rounds) return fail(MS_ERR_STATE, "fri_deep out of order");
  if (!z || !B) return fail(MS_ERR_ARG, "fri_deep");
  if (!load_ext(z, &cur_z)) return fail(MS_ERR_ARG, "z not canonical");
  Round* r = rounds[nrounds_done - 1].get();
  auto stage = res.expect();
  size_t off[2] = {0, 1}, cnt[2] = {(r->ncoef + 1) / 2, r->ncoef / 2};
  T* dst = pinned.as<T>();   // the last kernel of the evaluation stores its 2 E words straight into page-locked host memory
  if (r->dist) {   // even(z), odd(z) by coefficient range: partial sums over this rank's coefficients, one all-gather, combination with z^(S/2)
    const size_t lc = lcount(r, r->ncoef);
    cnt[0] = (lc + 1) / 2; cnt[1] = lc / 2;   // (the rank's first coefficient has an even index: S is even)
    { PartScope part(this); RQ((eval_views<E>(lpoly(r), 0, lstride(r), 2, off, cnt, 2, cur_z, reinterpret_cast<T*>(xs)))); }
    RQ(exchange(MS_XCHG_ALL_GATHER, 2 * E * sizeof(T)));
    RQ(shard_combine_launch(0, 2 * E, 2, e_pow<F, E>(cur_z, (u64)(r->S / 2)), dst));
  } else
  RQ((eval_views<E>(r->poly.template as<T>(), 0, r->cap, 2, off, cnt, 2, cur_z, dst, true)));  // fri.rs:354-359
  RQ(res.collect());
  const T* h = pinned.as<const T>();
  for (int s = 0; s < 2; s++) for (int l = 0; l < E; l++) { cur_B[s].c[l] = h[s * E + l]; B[s * E + l] = F::to_u64(h[s * E + l]); }
  have_deep = true;
  return MS_OK;
}

// `scratch` must hold sh_scratch_elems(m) elements of T
// ext_carry (E limbs, device): carry-in of the top level (a rank of a sharded proof: the suffix sum over the higher ranks, scaled - ShardCarryKernel);
// top_agg (E limbs, device): the job's aggregate over all its elements, stored by one extra AGG launch of the top level; out_h0: see SHJob
template <class F>
typename Ctx<F>::SHPlan Ctx<F>::sh_plan(const T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const XE& z,
               void* out, bool out_u64, size_t out_limb_stride, size_t out_off, size_t out_stride, T* h0, T* scratch,
               const T* ext_carry, T* top_agg, bool out_h0) {
  const size_t BS = mspoly::SH_BS;
  std::vector<size_t> ms; ms.push_back(m);
  while ((ms.back() ? (ms.back() + BS - 1) / BS : 1) > 1) ms.push_back((ms.back() + BS - 1) / BS);
  const int nl = (int)ms.size();
  std::vector<size_t> aoff(nl), coff(nl), nbs(nl);
  size_t tot = 0;
  for (int l = 0; l < nl; l++) { nbs[l] = ms[l] ? (ms[l] + BS - 1) / BS : 1; aoff[l] = tot; tot += nbs[l] * E; coff[l] = tot; tot += nbs[l] * E; }
  SHPlan pl; pl.nl = nl; pl.agg.resize(nl > 1 ? nl - 1 : 0); pl.fin.resize(nl);
  XE zl = z;
  for (int l = 0; l < nl; l++) {
    SHJ j;
    memset(&j, 0, sizeof j);
    j.z = zl;
    XE sq = e_pow<F, E>(zl, mspoly::SH_SEG);
    for (int i = 0; i < 9; i++) { j.zpow[i] = sq; sq = e_mul<F>(sq, sq); }
    zl = j.zpow[8];  // z^(SEG*256) = z^BS: multiplier of the level above
    j.m = ms[l];
    if (l == 0) { j.in = in; j.in_limb_stride = in_limb_stride; j.in_off = in_off; j.in_stride = in_stride; }
    else { j.in = scratch + aoff[l - 1]; j.in_limb_stride = nbs[l - 1]; j.in_off = 0; j.in_stride = 1; }
    if (l + 1 < nl) {  // aggregate job feeding level l+1
      SHJ a = j; a.agg = scratch + aoff[l]; a.agg_limb_stride = nbs[l];
      pl.agg[l] = a;
      j.carry = scratch + coff[l]; j.carry_limb_stride = nbs[l];
    } else {
      if (top_agg) { SHJ a = j; a.agg = top_agg; a.agg_limb_stride = 1; pl.top_agg = a; pl.has_top_agg = true; }
      if (ext_carry) { j.carry = ext_carry; j.carry_limb_stride = 1; }
    }
    if (l == 0) { j.out = out; j.out_u64 = out_u64 ? 1 : 0; j.out_limb_stride = out_limb_stride; j.out_off = out_off; j.out_stride = out_stride; j.h0 = h0; j.out_h0 = out_h0 ? 1 : 0; }
    else { j.out = scratch + coff[l - 1]; j.out_u64 = 0; j.out_limb_stride = nbs[l - 1]; j.out_off = 0; j.out_stride = 1; j.tail_zero = ext_carry ? 2 : 1; }
    pl.fin[l] = j;
  }
  pl.P = 1; for (int l = 0; l < nl; l++) pl.P *= BS;
  return pl;
}

template <class F>
int Ctx<F>::sh_launch_inline(const SHJ& j, int final_mode) {
  typename SHK::Params p; p.jobs = nullptr; p.inline_job = j; p.final_mode = final_mode;
  const size_t nb = j.m ? (j.m + mspoly::SH_BS - 1) / mspoly::SH_BS : 1;
  CK(run_coop<SHK>(K_SUFFIX_HORNER, (unsigned)nb, SHK::THREADS, SHK::lds_bytes(), p));
  return 0;
}

// a device table of `njobs` homogeneous jobs (the query phase's batched scans): blockIdx.y = job, `maxnb` = blocks of the longest one
template <class F>
int Ctx<F>::sh_launch_table(const SHJ* d_jobs, size_t njobs, size_t maxnb, int final_mode) {
  typename SHK::Params p; p.jobs = d_jobs; p.final_mode = final_mode;
  memset(&p.inline_job, 0, sizeof p.inline_job);
  CK(run_coop<SHK>(K_SUFFIX_HORNER, (unsigned)maxnb, SHK::THREADS, SHK::lds_bytes(), p, (unsigned)njobs));
  return 0;
}
// the carry-ins (and H_0's) of a device table of jobs from the all-gathered aggregates in the receive buffer (rank r's payload: njobs * E limbs)
template <class F>
int Ctx<F>::shard_carry_table(const mspoly::CarryJob<F, E>* d_jobs, size_t njobs) {
  typedef mspoly::ShardCarryKernel<F, E> CKn;
  typename CKn::Params cp; memset(&cp, 0, sizeof cp);
  cp.jobs = d_jobs; cp.njobs = (u32)njobs; cp.W = (u32)sh_world; cp.rank = (u32)sh_rank;
  cp.gathered = reinterpret_cast<const T*>(xr); cp.rank_stride = njobs * E;
  CK(run<CKn>(K_SUFFIX_HORNER, grid1(njobs, CKn::THREADS), 1, CKn::THREADS, 0, cp));
  return 0;
}
// one logical job, launched level by level with the job inline in the kernel arguments
template <class F>
int Ctx<F>::suffix_horner(const T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const XE& z,
                  T* out, size_t out_limb_stride, size_t out_off, size_t out_stride, T* h0) {
  if (d_sh.ensure(sh_scratch_elems(m) * sizeof(T))) return fail(MS_ERR_NOMEM, "scan levels");
  SHPlan pl = sh_plan(in, in_limb_stride, in_off, in_stride, m, z, out, false, out_limb_stride, out_off, out_stride, h0, d_sh.as<T>());
  for (int l = 0; l + 1 < pl.nl; l++) RQ(sh_launch_inline(pl.agg[l], 0));
  for (int l = pl.nl - 1; l >= 0; l--) RQ(sh_launch_inline(pl.fin[l], 1));
  return 0;
}

// all-gather of a distributed round polynomial's parts into one replicated vector (dst: E limbs, dst_stride apart, `count` coefficients)
template <class F>
int Ctx<F>::gather_poly(const T* local, size_t S, size_t count, T* dst, size_t dst_stride) {
  const size_t bytes = S * E * sizeof(T);
  if (bytes * (size_t)sh_world > xcap) return fail(MS_ERR_NOMEM, "exchange buffers too small to gather a round polynomial");
  CK(msrt::d2d(xs, local, bytes, stream));
  RQ(exchange(MS_XCHG_ALL_GATHER, bytes));
  typedef mspoly::GatherPolyKernel<F, E> GK;
  typename GK::Params gp{reinterpret_cast<const T*>(xr), S * E, S, count, dst, dst_stride};
  CK(run<GK>(K_IO, grid1(count * E, GK::THREADS), 1, GK::THREADS, 0, gp));
  return 0;
}

// fri.rs:96-101 on a DISTRIBUTED round polynomial (r04): rank k folds its own coefficient pairs, runs the suffix Horner of (folded - B(alpha)) / (x - z) over its
// own range with the sum over the higher ranks as carry-in (one all-gather of [first folded element | aggregate] per rank, ShardCarryKernel), and ends up with
// its range [k*S', (k+1)*S') of the quotient = the next round polynomial, S' = S/2.  If the next round is too small to stay distributed the parts are
// all-gathered into a replicated polynomial.  H_j for j in (lo, hi) comes from the rank's own job over f[lo+1 .. hi); H_hi = q_(hi-1) IS the carry-in.
template <class F>
int Ctx<F>::fold_dist(Round* pr, Round* nr, const XE& a, size_t* nq_coef_out) {
  const size_t n = pr->ncoef, m = (n + 1) / 2, Sn = pr->S / 2;
  const bool next_dist = dist_chunk(nr->D) == Sn;
  const size_t cntp = lcount(pr, n), cnt = (cntp + 1) / 2;   // this rank's coefficients of the round polynomial / of the folded polynomial
  T* lq;
  if (next_dist) { if (nr->poly.ensure(Sn * E * sizeof(T))) return fail(MS_ERR_NOMEM, "fold"); lq = nr->poly.template as<T>(); }
  else { if (d_lq.ensure(Sn * E * sizeof(T))) return fail(MS_ERR_NOMEM, "fold"); lq = d_lq.as<T>(); }
  if (d_folded.ensure((Sn + 1) * E * sizeof(T)) || d_carry.ensure(4096)) return fail(MS_ERR_NOMEM, "fold");
  if (4 * E * sizeof(T) * (size_t)sh_world > xcap) return fail(MS_ERR_NOMEM, "exchange buffers");
  size_t nq_coef = 0;
  PartScope part(this);
  if (m >= 2) {
    T* pay = reinterpret_cast<T*>(xs);        // [first folded element (E limbs) | aggregate of the job (E limbs)]: the fold's first thread writes [f_0 | 0], the aggregate launch the rest
    typename mspoly::FoldKernel<F, E>::Params fp{lpoly(pr), lstride(pr), cntp, d_folded.as<T>(), Sn, a, pay};  // fri.rs:361-372
    if (cnt) CK(run<mspoly::FoldKernel<F, E>>(K_FOLD, grid1(cnt, mspoly::THREADS), 1, mspoly::THREADS, 0, fp));
    else CK(msrt::memset_dev(xs, 0, 2 * E * sizeof(T), stream));   // (a rank with no coefficient of this round: an all-zero payload)
    const size_t mj = cnt ? cnt - 1 : 0;
    SHPlan pl; pl.nl = 0;
    if (mj) {
      if (d_sh.ensure(sh_scratch_elems(mj) * sizeof(T))) return fail(MS_ERR_NOMEM, "scan levels");
      pl = sh_plan(d_folded.as<T>(), Sn, 1, 1, mj, cur_z, lq, false, Sn, 1, 1, nullptr, d_sh.as<T>(), d_carry.as<T>(), pay + E, true);
      for (int l = 0; l + 1 < pl.nl; l++) RQ(sh_launch_inline(pl.agg[l], 0));
      RQ(sh_launch_inline(pl.top_agg, 0));
    }
    RQ(exchange(MS_XCHG_ALL_GATHER, 2 * E * sizeof(T)));
    typedef mspoly::ShardCarryKernel<F, E> CKn;
    typename CKn::Params cp;
    memset(&cp, 0, sizeof cp);
    cp.jobs = nullptr; cp.njobs = 1; cp.W = (u32)sh_world; cp.rank = (u32)sh_rank; cp.gathered = reinterpret_cast<const T*>(xr); cp.rank_stride = 2 * E;
    cp.inline_job.first_off = 0; cp.inline_job.agg_off = E; cp.inline_job.has_first = 1;
    cp.inline_job.zA = cur_z; cp.inline_job.zB = e_pow<F, E>(cur_z, (u64)(Sn - 1));
    cp.inline_job.scale = mj ? carry_scale(cur_z, mj, pl.P) : e_one<F, E>();
    cp.inline_job.carry_out = d_carry.as<T>();
    cp.inline_job.tail_out = cnt ? lq + (cnt - 1) : nullptr; cp.inline_job.tail_stride = Sn;   // q_(hi-1) = H_hi (zero, and beyond the polynomial, on the rank that holds its top)
    cp.inline_job.h0_out = nullptr;
    CK(run<CKn>(K_SUFFIX_HORNER, 1, 1, CKn::THREADS, 0, cp));
    if (mj) for (int l = pl.nl - 1; l >= 0; l--) RQ(sh_launch_inline(pl.fin[l], 1));
    nq_coef = m - 1;
  }
  nr->S = Sn;
  if (next_dist) { nr->dist = true; nr->local_store = true; }
  else {   // the round after this one is small: replicate the quotient (one all-gather of S' coefficients per rank) and go on as an unsharded prover would
    if (nr->poly.ensure(nr->cap * E * sizeof(T))) return fail(MS_ERR_NOMEM, "fold");
    if (nq_coef) RQ(gather_poly(lq, Sn, nq_coef, nr->poly.template as<T>(), nr->cap));
    nr->S = 0;
  }
  *nq_coef_out = nq_coef;
  return 0;
}

// fri.rs:96-109 for a round of the latency-bound tail, as ONE launch (fri_tail.hpp): fold, DEEP quotient, trimmed length, pointwise codeword, leaf digests, every tree
// level, root and length word into page-locked memory.  *done = false: the round does not qualify (the caller takes the launch-per-step path).
template <class F>
int Ctx<F>::fri_tail_round(Round* pr, Round* nr, const XE& a, bool* done) {
  // (BLAKE3: a round's leaf group is 2 extension elements, far below one chunk)
  return msmerkle::with_digest(digest, [&](auto family) { return fri_tail_round_t<decltype(family)>(pr, nr, a, done); });
}
template <class F> template <class DG>
int Ctx<F>::fri_tail_round_t(Round* pr, Round* nr, const XE& a, bool* done) {
  *done = false;
  const size_t n = pr->ncoef, m = (n + 1) / 2, Dn = nr->D, M = Dn / 2;
  bool z_outside_base = false;
  for (int l = 1; l < E; l++) z_outside_base = z_outside_base || cur_z.c[l] != 0;
  // replicated rounds only (a sharded proof's tail is replicated on every rank); the pointwise codeword needs y - z != 0 on the base-field domain; one scan block
  if (!fri_tail_max || pr->D > fri_tail_max || pr->dist || pr->ts.sharded || shardable(M) || !fri_pointwise || !z_outside_base || m > (size_t)mspoly::SH_BS || M < 1) return 0;
  typedef msfri::FriTailKernel<F, E, DG> TK;
  if (M > (size_t)TK::WG_GROUPS << TK::TreeK::MAX_LEVELS) return 0;
  if (ctz64(Dn) > F::TWO_ADICITY) return fail(MS_ERR_SHAPE, "FRI domain larger than the field's two-adicity");
  RQ(tree_shape(Dn, 2, 2, &nr->ts));
  nr->m = 0; nr->base_cw = false;
  if (nr->poly.ensure(nr->cap * E * sizeof(T)) || d_folded.ensure((m + 1) * E * sizeof(T)) || nr->cw.ensure(Dn * E * sizeof(T)) || nr->nodes.ensure(nr->ts.nodes * 32) ||
      d_sh.ensure(sh_scratch_elems(m) * sizeof(T)))
    return fail(MS_ERR_NOMEM, "fused FRI round");
  Plan* pl;
  RQ(get_plan(ctz64(pr->D), 0, false, &pl));   // w_D^e tables of the previous domain
  typename TK::Params tp;
  memset(&tp, 0, sizeof tp);
  // ---- coefficient side
  tp.do_coef = m >= 2 ? 1 : 0;
  tp.fold = typename TK::FoldK::Params{pr->poly.template as<T>(), pr->cap, n, d_folded.as<T>(), m, a, nullptr};
  if (tp.do_coef) {
    SHPlan sp = sh_plan(d_folded.as<T>(), m, 0, 1, m, cur_z, nr->poly.template as<T>(), false, nr->cap, 0, 1, nullptr, d_sh.as<T>());
    if (sp.nl != 1) return fail(MS_ERR_STATE, "fused FRI round: scan of more than one block");
    tp.scan.jobs = nullptr; tp.scan.inline_job = sp.fin[0]; tp.scan.final_mode = 1;
  }
  tp.deg = typename TK::DegK::Params{nr->poly.template as<T>(), nr->cap, m >= 2 ? m - 1 : 0, res.word(Results::FRI_LEN), 0};   // the length word: zero between rounds (the forwarding thread clears it)
  // ---- evaluation side
  const size_t per = M < (size_t)TK::WG_GROUPS ? M : (size_t)TK::WG_GROUPS, G = M / per;
  tp.G = (u32)G;
  const XE c = e_add<F, E>(cur_B[0], e_mul<F>(cur_B[1], a));         // B(alpha), fri.rs:99
  tp.eval.src = pr->cw.template as<T>(); tp.eval.src_limb_stride = pr->D; tp.eval.dst = nr->cw.template as<T>(); tp.eval.dst_limb_stride = Dn;
  tp.eval.m_out = Dn; tp.eval.log_m = (u32)ctz64(Dn); tp.eval.groups = 1; tp.eval.shard_W = 0; tp.eval.shard_k = 0;
  tp.eval.tw_lo = pl->tw_lo.template as<T>(); tp.eval.tw_hi = pl->tw_hi.template as<T>(); tp.eval.lo_bits = (u32)pl->lo_bits; tp.eval.log_D = (u32)ctz64(pr->D);
  tp.eval.alpha = a; tp.eval.c2 = e_add<F, E>(c, c); tp.eval.z = cur_z; tp.eval.inv2 = f_inv<F>(F::from_u64(2));
  tp.leaf.base = nr->cw.template as<T>(); tp.leaf.col_stride = 0; tp.leaf.row_stride = 1; tp.leaf.limb_stride = Dn; tp.leaf.width = 1; tp.leaf.lpn = 2;
  tp.leaf.zero_as_empty = zae; tp.leaf.ngroups = M; tp.leaf.nodes = nr->nodes.template as<u32>();   // (ovf* = null: pad-only blocks in place; no runs, no virtual columns)
  u32 nl = 0; while (((size_t)1 << nl) < per) nl++;
  tp.sub.nodes = nr->nodes.template as<u32>(); tp.sub.child_off = 0; tp.sub.nchildren = M; tp.sub.ic = 2; tp.sub.nlevels = nl;
  u32 tl = 0; while (((size_t)1 << tl) < G) tl++;
  tp.top.nodes = nr->nodes.template as<u32>(); tp.top.child_off = 2 * M - 2 * G; tp.top.nchildren = G; tp.top.ic = 2; tp.top.nlevels = tl;
  RQ(res.attach(tp.top));
  tp.root_index = nr->ts.nodes - 1;
  tp.done = reinterpret_cast<u32*>(res.word(Results::TAIL_DONE));    // (zeroed with the length word; the last workgroup leaves it zero)
  next_bytes = (double)Dn * E * sizeof(T) * 3 + (double)M * 96;
  CK(run_coop<TK>(K_FRI_TAIL, (unsigned)(G + 1), TK::THREADS, TK::lds_bytes(), tp));
  *done = true;
  return 0;
}

// fri.rs:96-109
template <class F>
int Ctx<F>::fri_fold_commit(const u64* alpha, u8* root) {
  RQ(fri_folded_refusal("fri_fold_commit"));
  if (!have_deep) return fail(MS_ERR_STATE, "fri_fold_commit before fri_deep");
  XE a;
  if (!alpha || !root || !load_ext(alpha, &a)) return fail(MS_ERR_ARG, "alpha");
  Round* pr = rounds[nrounds_done - 1].get();
  if (pr->D < 4) return fail(MS_ERR_SHAPE, "FRI round domain too small to fold (merkle.rs:93-104 panics)");
  const size_t n = pr->ncoef, m = (n + 1) / 2;
  Round* nr = round_slot(nrounds_done);
  nr->cap = m ? m : 1;
  nr->D = pr->D / 2;  // fri.rs:104, 374-376
  nr->dist = false; nr->local_store = false; nr->S = 0;
  size_t nq_coef = 0;
  bool fused = false, side = false;
  // the round brings home its root and the next round polynomial's trimmed length; that word is scanned BEFORE the commitment, whose last launch forwards it with the
  // root: no copy launch in front of the round's one host round trip (r03; the trace showed a 4 us copyBuffer kernel + its launch gap per round).  A distributed
  // next round: this rank's part reports the GLOBAL length and the maximum over the ranks comes back with the subtree roots (finish_sharded_tree)
  unsigned long long* dres = res.word(Results::FRI_LEN), ncoef = 0;   // (zeroed by ms_fri_begin, left zero by whoever forwards it)
  auto stage = res.expect(dres, pr->dist && dist_chunk(nr->D) == pr->S / 2);
  RQ(fri_tail_round(pr, nr, a, &fused));   // one launch does the whole round, if it qualifies
  if (!fused) {
  if (pr->dist) RQ(fold_dist(pr, nr, a, &nq_coef));
  else {
  if (nr->poly.ensure(nr->cap * E * sizeof(T)) || d_folded.ensure((m + 1) * E * sizeof(T))) return fail(MS_ERR_NOMEM, "fold");
  if (m >= 2) {
    // the coefficient side on the side stream (every stage ends with a synchronisation of the context's stream behind a join: the side stream starts on finished data)
    side = fri_overlap && !prof_on;   // (the per-kernel profile times launches one behind the other on ONE stream)
    if (side) RQ(res.fork_side());
    StreamScope on_side(this, side ? side_stream.get() : stream);
    typename mspoly::FoldKernel<F, E>::Params fp{pr->poly.template as<T>(), pr->cap, n, d_folded.as<T>(), m, a, nullptr};  // fri.rs:361-372
    CK(run<mspoly::FoldKernel<F, E>>(K_FOLD, grid1(m, mspoly::THREADS), 1, mspoly::THREADS, 0, fp));
    // (folded - B(alpha)) / (x - z): quotient coefficients are H_1.. of the suffix Horner in z (fri.rs:99-101)
    RQ(suffix_horner(d_folded.as<T>(), m, 0, 1, m, cur_z, nr->poly.template as<T>(), nr->cap, 0, 1, nullptr));
    nq_coef = m - 1;
  }
  }
  if (nr->dist) {
    const size_t lc = lcount(nr, nq_coef);
    if (lc) {
      typename mspoly::DegreeKernel<F, E>::Params dp{lpoly(nr), lstride(nr), lc, dres, (size_t)sh_rank * nr->S};
      PartScope part(this);
      CK(run<mspoly::DegreeKernel<F, E>>(K_DEGREE, grid1(lc, mspoly::THREADS), 1, mspoly::THREADS, 0, dp));
    }
  } else if (nq_coef) {
    StreamScope on_side(this, side ? side_stream.get() : stream);
    typename mspoly::DegreeKernel<F, E>::Params dp{nr->poly.template as<T>(), nr->cap, nq_coef, dres, 0};
    CK(run<mspoly::DegreeKernel<F, E>>(K_DEGREE, grid1(nq_coef, mspoly::THREADS), 1, mspoly::THREADS, 0, dp));
  }
  RQ(res.side_done());
  RQ(round_commit(nr, nq_coef, E, pr, &a));
  }
  RQ(read_root(nr->nodes, nr->ts, root, &ncoef));   // (whatever path the commitment took, the context's stream ends behind the side stream; the flag of the last launch is polled if nothing was enqueued behind it)
  nr->ncoef = (size_t)ncoef;
  nrounds_done++; have_deep = false;
  return MS_OK;
}

template <class F>
int Ctx<F>::fri_round_info(int r, u64* ncoef, u64* D) {
  if (r < 0 || (size_t)r >= nrounds_done) return fail(MS_ERR_ARG, "round index");
  if (ncoef) *ncoef = rounds[r]->ncoef;
  if (D) *D = rounds[r]->D;
  return MS_OK;
}

template <class F>
int Ctx<F>::fri_round_poly_read(int r, u64* out) {
  RQ(fri_folded_refusal("fri_round_poly_read"));
  if (r < 0 || (size_t)r >= nrounds_done || !out) return fail(MS_ERR_ARG, "round index");
  if (rounds[r]->local_store) return fail(MS_ERR_STATE, "round_poly_read: the polynomial of a sharded round is distributed over the ranks");
  return download_widen(rounds[r]->poly.template as<T>(), rounds[r]->ncoef, rounds[r]->cap, E, out);
}

template <class F>
int Ctx<F>::fri_round_codeword_read(int r, u64* out) {
  if (r < 0 || (size_t)r >= nrounds_done || !out) return fail(MS_ERR_ARG, "round index");
  if (rounds[r]->ts.sharded) return fail(MS_ERR_STATE, "codeword_read: the codeword of a sharded round is distributed over the ranks");
  return download_widen(rounds[r]->cw.template as<T>(), rounds[r]->D, rounds[r]->D, E, out);
}

// ------------------------------------------------------------------ build-defined: folded FRI (include/ministark.h)
// Round i's codeword c_i on <g_i> in natural order; a fold takes the a = 2^fri_k values of a coset {x w^t} to P(alpha), P their interpolant (FriFoldArityKernel).
// No round polynomial, no DEEP quotient, no scan, no side stream: a round is one fold launch and the tree over the coset view.
template <class F>
int Ctx<F>::fold_arity_launch(const Round* pr, const XE& a, T* dst) {
  const size_t A = (size_t)1 << fri_k, m_out = pr->D / A;
  Plan* pl;
  RQ(get_plan(ctz64(pr->D), 0, false, &pl));   // w_D^e tables of the domain being folded
  const T w_inv = f_pow<F>(pl->root, (u64)(pr->D - m_out));   // (w_D^(D/a))^-1
  auto launch = [&](auto* kernel) {
    typedef typename std::remove_pointer<decltype(kernel)>::type FK;
    typename FK::Params fp;
    fp.src = pr->cw.template as<T>(); fp.src_limb_stride = pr->D; fp.dst = dst; fp.dst_limb_stride = m_out; fp.m_out = m_out;
    fp.tw_lo = pl->tw_lo.template as<T>(); fp.tw_hi = pl->tw_hi.template as<T>(); fp.lo_bits = (u32)pl->lo_bits; fp.log_D = (u32)ctz64(pr->D);
    fp.alpha = a;
    T wj = F::from_u64(1);
    for (int j = 0; j < 4; j++) { fp.wt[j] = F::to_tw(wj); wj = F::mul(wj, w_inv); }
    fp.inv_a = F::to_tw(f_inv<F>(F::from_u64((u64)A)));
    next_bytes = (double)m_out * (A + 1) * E * sizeof(T);   // a E words read, E written per output
    return run<FK>(K_FOLD, grid1(m_out, FK::THREADS), 1, FK::THREADS, 0, fp);
  };
  if (fri_k == 1) CK(launch((mspoly::FriFoldArityKernel<F, E, 1>*)nullptr));
  else if (fri_k == 2) CK(launch((mspoly::FriFoldArityKernel<F, E, 2>*)nullptr));
  else CK(launch((mspoly::FriFoldArityKernel<F, E, 3>*)nullptr));
  return 0;
}

// leaf group j = the a elements c[j + t D / a], t < a: the view width = lpn = a, col_stride = D / a (r->ts: tree_shape(D, a, 2))
template <class F>
int Ctx<F>::coset_tree(Round* r) {
  const size_t A = (size_t)1 << fri_k;
  return tree_build<E>(r->cw.template as<T>(), r->D / A, 1, r->D, (u32)A, r->ts, r->nodes);
}

template <class F>
int Ctx<F>::fri_begin_folded(size_t blowup_, int log_arity, u8* root0) {
  if (!have_validity) return fail(MS_ERR_STATE, "fri_begin_folded before mix");
  if (!root0 || !blowup_ || (blowup_ & (blowup_ - 1)) || log_arity < 1 || log_arity > 3) return fail(MS_ERR_ARG, "fri_begin_folded: null root, log_arity outside 1..3, or a blowup that is zero or no power of two");
  if (sh_on) return fail(MS_ERR_STATE, "fri_begin_folded: not available on a context with sharding on");
  const size_t A = (size_t)1 << log_arity;
  if (blowup_ > ((size_t)1 << F::TWO_ADICITY) / A) return fail(MS_ERR_SHAPE, "fri_begin_folded: arity * blowup is above the field's two-adicity, no domain can hold a fold");   // (D_0 >= blowup whatever the degree: refused without the scan)
  // round 0's polynomial where it lies (ms_fri_begin's rule): D' while a DEEP polynomial is installed (N coefficients, E limbs N apart), otherwise the validity polynomial
  const bool dp = dpoly_live();
  const size_t VL = dp ? N : validity_len;
  const bool vx = dp || validity_ext > 1;
  const T* src = dp ? d_deep.template as<T>() : d_polys.template as<T>() + (size_t)npolys * N;
  unsigned long long nc = validity_ncoef;
  if (dp || validity_len_at != VLEN_HOST) {   // the trimmed length, scanned in place (a base-field polynomial: every limb of the scan reads the one plane)
    unsigned long long* dres;
    RQ(degree_launch(src, vx ? VL : 0, VL, &dres));
    auto scan = res.expect(dres, false, false);
    RQ(res.collect(nullptr, nullptr, &nc));
  }
  size_t D = 1; while (D < (nc ? nc : 1) * blowup_) D <<= 1;   // next_pow2(ncoef * blowup), as ms_fri_begin
  if (ctz64(D) > F::TWO_ADICITY) return fail(MS_ERR_SHAPE, "FRI domain larger than the field's two-adicity");
  if (D / A < blowup_) return fail(MS_ERR_SHAPE, "fri_begin_folded: D_0 < arity * blowup, no fold is possible");
  TreeShape ts;
  RQ(tree_shape(D, A, 2, &ts));
  if (copy_pending) RQ(fri_proof_wait());   // (a read-back of an earlier MSFP blob in flight: ms_fri_proof_wait is refused from here on)
  // ---- decided: from here on the FRI state is this call's
  nrounds_done = 0; have_deep = false; blob_size = 0;
  fri_rounds = 0; fri_blowup = blowup_; fri_k = log_arity; fold_final_done = false;
  Round* r = round_slot(0);
  r->D = D; r->cap = 0; r->ncoef = D / blowup_; r->ts = ts; r->m = 0; r->dist = false; r->local_store = false; r->S = 0;
  const int live = vx ? E : 1;
  r->base_cw = live == 1;
  auto stage = res.expect();
  RQ(res.join_side());
  if (r->cw.ensure(D * E * sizeof(T))) return fail(MS_ERR_NOMEM, "codeword");
  RQ(ntt_run(ctz64(D), false, src, VL, (size_t)nc, r->cw.template as<T>(), D, (size_t)live));
  if (live < E) CK(msrt::memset_dev(r->cw.template as<T>() + (size_t)live * D, 0, (size_t)(E - live) * D * sizeof(T), stream));
  RQ(coset_tree(r));
  RQ(read_root(r->nodes, r->ts, root0));
  nrounds_done = 1;
  return MS_OK;
}

template <class F>
int Ctx<F>::fri_fold_folded(const u64* alpha, u8* root) {
  if (!folded()) return fail(MS_ERR_STATE, "fri_fold_folded outside folded mode (ms_fri_begin_folded)");
  if (fold_final_done) return fail(MS_ERR_STATE, "fri_fold_folded after fri_fold_final");
  XE a;
  if (!alpha || !root || !load_ext(alpha, &a)) return fail(MS_ERR_ARG, "alpha");
  const size_t A = (size_t)1 << fri_k;
  const Round* pr = rounds[nrounds_done - 1].get();
  const size_t Dn = pr->D / A;
  if (Dn / A < fri_blowup) return fail(MS_ERR_SHAPE, "fri_fold_folded: D_(i+1) < arity * blowup, only the final fold is left");
  TreeShape ts;
  RQ(tree_shape(Dn, A, 2, &ts));
  Round* nr = round_slot(nrounds_done);
  pr = rounds[nrounds_done - 1].get();
  if (nr->cw.ensure(Dn * E * sizeof(T))) return fail(MS_ERR_NOMEM, "codeword");
  nr->D = Dn; nr->cap = 0; nr->ncoef = Dn / fri_blowup; nr->ts = ts; nr->m = 0; nr->dist = false; nr->local_store = false; nr->S = 0; nr->base_cw = false;
  auto stage = res.expect();
  RQ(fold_arity_launch(pr, a, nr->cw.template as<T>()));
  RQ(coset_tree(nr));
  RQ(read_root(nr->nodes, nr->ts, root));
  nrounds_done++;
  return MS_OK;
}

template <class F>
int Ctx<F>::fri_fold_final(const u64* alpha, u64* coeffs, size_t cap, size_t* n) {
  if (!folded()) return fail(MS_ERR_STATE, "fri_fold_final outside folded mode (ms_fri_begin_folded)");
  if (fold_final_done) return fail(MS_ERR_STATE, "fri_fold_final: the final fold has been made");
  XE a;
  if (!alpha || !n || (!coeffs && cap) || !load_ext(alpha, &a)) return fail(MS_ERR_ARG, "fri_fold_final: null argument, or alpha not canonical");
  const Round* pr = rounds[nrounds_done - 1].get();
  const size_t DR = pr->D >> fri_k, nfinal = DR / fri_blowup;   // (D_(R-1) >= arity * blowup: nfinal >= 1)
  *n = nfinal;
  if (!coeffs) return MS_OK;   // size query
  if (cap < nfinal * E) return fail(MS_ERR_ARG, "fri_fold_final: buffer too small (the coefficients needed are in *n)");
  if (d_fold_cw.ensure(DR * E * sizeof(T)) || fold_fin.poly.ensure(DR * E * sizeof(T))) return fail(MS_ERR_NOMEM, "final polynomial");
  RQ(fold_arity_launch(pr, a, d_fold_cw.template as<T>()));
  RQ(ntt_run(ctz64(DR), true, d_fold_cw.template as<T>(), DR, DR, fold_fin.poly.template as<T>(), DR, (size_t)E));
  if (DR > nfinal) {   // nothing at or above nfinal: the codeword was of the degree the domain rule assumes
    unsigned long long* dres; unsigned long long top = 0;
    RQ(degree_launch(fold_fin.poly.template as<T>() + nfinal, DR, DR - nfinal, &dres));
    auto scan = res.expect(dres, false, false);
    RQ(res.collect(nullptr, nullptr, &top));
    if (top) return fail(MS_ERR_SHAPE, "fri_fold_final: the folded codeword is of higher degree than D_R / blowup (round 0 was not of the degree its domain assumes)");
  }
  RQ(download_widen(fold_fin.poly.template as<T>(), nfinal, DR, E, coeffs));
  fold_fin.cap = DR; fold_fin.ncoef = nfinal; fold_fin.D = DR;
  fold_final_done = true;
  return MS_OK;
}

// the members this unit defines, for both fields (the other units see declarations only)
#define MS_INSTANTIATE(FF) \
  template int Ctx<FF>::round_commit(Ctx<FF>::Round* r, size_t ncoef_in, int nonzero_limbs, const Ctx<FF>::Round* prev, const Ctx<FF>::XE* alpha); \
  template int Ctx<FF>::degree_launch(const Ctx<FF>::T* poly, size_t limb_stride, size_t n, unsigned long long** dres_out); \
  template int Ctx<FF>::fri_begin(size_t blowup_, size_t nrounds, u8* root0); \
  template int Ctx<FF>::fri_deep(const u64* z, u64* B); \
  template Ctx<FF>::SHPlan Ctx<FF>::sh_plan(const Ctx<FF>::T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const Ctx<FF>::XE& z, void* out, bool out_u64, size_t out_limb_stride, size_t out_off, size_t out_stride, Ctx<FF>::T* h0, Ctx<FF>::T* scratch, const Ctx<FF>::T* ext_carry, Ctx<FF>::T* top_agg, bool out_h0); \
  template int Ctx<FF>::sh_launch_inline(const Ctx<FF>::SHJ& j, int final_mode); \
  template int Ctx<FF>::sh_launch_table(const Ctx<FF>::SHJ* d_jobs, size_t njobs, size_t maxnb, int final_mode); \
  template int Ctx<FF>::shard_carry_table(const mspoly::CarryJob<FF, Ctx<FF>::E>* d_jobs, size_t njobs); \
  template int Ctx<FF>::suffix_horner(const Ctx<FF>::T* in, size_t in_limb_stride, size_t in_off, size_t in_stride, size_t m, const Ctx<FF>::XE& z, Ctx<FF>::T* out, size_t out_limb_stride, size_t out_off, size_t out_stride, Ctx<FF>::T* h0); \
  template int Ctx<FF>::gather_poly(const Ctx<FF>::T* local, size_t S, size_t count, Ctx<FF>::T* dst, size_t dst_stride); \
  template int Ctx<FF>::fold_dist(Ctx<FF>::Round* pr, Ctx<FF>::Round* nr, const Ctx<FF>::XE& a, size_t* nq_coef_out); \
  template int Ctx<FF>::fri_tail_round(Ctx<FF>::Round* pr, Ctx<FF>::Round* nr, const Ctx<FF>::XE& a, bool* done); \
  template int Ctx<FF>::fri_fold_commit(const u64* alpha, u8* root); \
  template int Ctx<FF>::fri_round_info(int r, u64* ncoef, u64* D); \
  template int Ctx<FF>::fri_round_poly_read(int r, u64* out); \
  template int Ctx<FF>::fri_round_codeword_read(int r, u64* out); \
  template int Ctx<FF>::fold_arity_launch(const Ctx<FF>::Round* pr, const Ctx<FF>::XE& a, Ctx<FF>::T* dst); \
  template int Ctx<FF>::coset_tree(Ctx<FF>::Round* r); \
  template int Ctx<FF>::fri_begin_folded(size_t blowup_, int log_arity, u8* root0); \
  template int Ctx<FF>::fri_fold_folded(const u64* alpha, u8* root); \
  template int Ctx<FF>::fri_fold_final(const u64* alpha, u64* coeffs, size_t cap, size_t* n);
MS_INSTANTIATE(GL)
MS_INSTANTIATE(BB)
#undef MS_INSTANTIATE

}  // namespace msctx
