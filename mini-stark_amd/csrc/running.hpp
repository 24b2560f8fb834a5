// running.hpp — the running column of a permutation or lookup argument (ms_aux_running, include/ministark.h; build-defined, no reference counterpart).
//
//   s_i = sum_k a_{2k}(i) / a_{2k+1}(i)   (MS_AUX_SUM)   or   prod_k a_{2k}(i) / a_{2k+1}(i)   (MS_AUX_PRODUCT),   a_f(i) = const_f + sum_m coef_m T_{col_m}[i]
//   z_0 = identity,  z_{i+1} = z_i o s_i,  final = z_{N-1} o s_{N-1}
//
// over K = Fp (EA = 1) or the field's extension (EA = E).  An EXCLUSIVE prefix scan over the field, in three launches, none of which waits for another workgroup:
//   AuxTile    one workgroup per tile of 256 * SEG rows: fractions folded into one A_i / B_i per row, the B_i inverted through their base-field norms with
//              Montgomery's trick (one field inversion per thread), s_i scanned in LDS; writes the tile-local exclusive prefix and the tile's aggregate
//   AuxCarry   ONE workgroup: aggregates -> exclusive carries, 256 at a time with a running carry; writes `final`
//   AuxApply   z_i = carry[tile] o local_i, elementwise
// o is commutative and associative and the arithmetic exact, so the grouping changes no bit of the result.
// HBM-bound: per row the tile launch reads the columns its forms name and writes EA limbs; the apply launch reads and writes EA limbs.
#pragma once
#include <type_traits>

#include "field.hpp"
#include "poly.hpp"

namespace msrun {

constexpr int THREADS = 256;
constexpr int MAX_FRAC = 4, MAX_FORMS = 2 * MAX_FRAC, MAX_FORM_TERMS = 16, MAX_TERMS = MAX_FORMS * MAX_FORM_TERMS, MAX_SEG = 8, MAX_COLUMNS = 16;

// the program of one call, in device memory: every access is uniform over the launch
template <class F, int EA> struct AuxProgram {
  u32 op, nfrac;
  u32 form_begin[MAX_FORMS + 1];
  u32 term_col[MAX_TERMS];
  Ext<F, EA> form_const[MAX_FORMS];
  Ext<F, EA> term_coef[MAX_TERMS];
};

template <class F, int EA> MS_HD Ext<F, EA> aux_identity(u32 op) { return op ? e_one<F, EA>() : e_zero<F, EA>(); }
template <class F, int EA> MS_HD Ext<F, EA> aux_comb(u32 op, const Ext<F, EA>& a, const Ext<F, EA>& b) { return op ? e_mul<F>(a, b) : e_add<F, EA>(a, b); }

// b * C = n with n in the base field (C: the product of b's conjugates, n: its norm); n = 0 exactly when b = 0.  The formulas of e_inv (field.hpp), without the inversion
template <class F> MS_HD void aux_conj_norm(const Ext<F, 1>& b, Ext<F, 1>* C, typename F::T* n) { C->c[0] = F::from_u64(1); *n = b.c[0]; }
template <class F> MS_HD void aux_conj_norm(const Ext<F, 2>& b, Ext<F, 2>* C, typename F::T* n) {
  const typename F::T nr = F::to_tw(F::from_u64(F::NR2));
  C->c[0] = b.c[0]; C->c[1] = F::neg(b.c[1]);
  *n = F::sub(F::mul(b.c[0], b.c[0]), F::mul_tw(F::mul(b.c[1], b.c[1]), nr));
}
template <class F> MS_HD void aux_conj_norm(const Ext<F, 4>& b, Ext<F, 4>* C, typename F::T* n) {   // b = a0 + a1 v, v^2 = u - 11: b (a0 - a1 v) = M in Fp2, M conj(M) = n
  const typename F::T nr = F::to_tw(F::from_u64(F::NR2));
  const Ext<F, 2> a0{{b.c[0], b.c[1]}}, a1{{b.c[2], b.c[3]}};
  const Ext<F, 2> M = e_sub<F, 2>(e_mul<F>(a0, a0), e_mul_nr4<F>(e_mul<F>(a1, a1)));
  const Ext<F, 2> Mc{{M.c[0], F::neg(M.c[1])}};
  *n = F::sub(F::mul(M.c[0], M.c[0]), F::mul_tw(F::mul(M.c[1], M.c[1]), nr));
  const Ext<F, 2> c0 = e_mul<F>(a0, Mc), c1 = e_mul<F>(a1, Mc);
  C->c[0] = c0.c[0]; C->c[1] = c0.c[1]; C->c[2] = F::neg(c1.c[0]); C->c[3] = F::neg(c1.c[1]);
}

// f(integral_constant<int, I>) for I = FROM .. TO-1, and for I = FROM-1 .. 0: a loop whose index is a compile-time constant in every iteration
#define MS_LAMBDA_INLINE __attribute__((always_inline))
template <int FROM, int TO, class Fn> MS_DEV void aux_static_for(Fn& f) { if constexpr (FROM < TO) { f(std::integral_constant<int, FROM>()); aux_static_for<FROM + 1, TO>(f); } }
template <int FROM, class Fn> MS_DEV void aux_static_rfor(Fn& f) { if constexpr (FROM > 0) { f(std::integral_constant<int, FROM - 1>()); aux_static_rfor<FROM - 1>(f); } }

// inclusive scan of one value per thread over the workgroup (Hillis-Steele, 8 steps, ping-pong between sa and sb, both [EA][THREADS]); the result is in sa.
// Every thread of the workgroup calls it; the caller puts a barrier behind its last read of sa before the next call.
template <class F, int EA> MS_DEV void aux_wg_scan(u32 op, const Ext<F, EA>& mine, int tid, typename F::T* sa, typename F::T* sb) {
  typedef Ext<F, EA> X;
  for (int l = 0; l < EA; l++) sa[l * THREADS + tid] = mine.c[l];
  msrt::wg_barrier();
#pragma unroll
  for (int step = 0; step < 8; step++) {
    const int d = 1 << step;
    const typename F::T* src = (step & 1) ? sb : sa;
    typename F::T* dst = (step & 1) ? sa : sb;
    X v; for (int l = 0; l < EA; l++) v.c[l] = src[l * THREADS + tid];
    if (tid >= d) {
      X u; for (int l = 0; l < EA; l++) u.c[l] = src[l * THREADS + tid - d];
      v = aux_comb<F, EA>(op, u, v);
    }
    for (int l = 0; l < EA; l++) dst[l * THREADS + tid] = v.c[l];
    msrt::wg_barrier();
  }
}

// ---------------------------------------------------------------- tile launch
// Grid: ceil(N / TILE) workgroups.  Rows are taken STRIPED for the global accesses and the fractions (row j0 + it * THREADS + tid: coalesced; which rows share a
// field inversion does not matter) and BLOCKED for the scan (thread t owns the rows j0 + t * SEG .. + SEG - 1 of the tile), with the tile's s_i in LDS between the two.
// Rows >= N (a trace shorter than the tile) count as the identity.  A zero denominator raises *zero_flag and is replaced by 1: the other rows of the thread still
// get defined values; the host discards the whole result then.
template <class F, int EA, int SEG_> struct AuxTileKernel {
  typedef typename F::T T;
  typedef Ext<F, EA> X;
  typedef AuxProgram<F, EA> Program;
  static_assert(SEG_ >= 1 && SEG_ <= MAX_SEG && (SEG_ & (SEG_ - 1)) == 0, "rows per thread: a power of two up to MAX_SEG");
  static constexpr int THREADS = msrun::THREADS, SEG = SEG_, TILE = THREADS * SEG;
  struct Params {
    const T* cols; size_t col_stride, N;        // trace column c, row i at cols[c * col_stride + i]
    const Program* prog;
    T* out; size_t out_stride;                   // limb l of the column at out[l * out_stride + i]: the tile-local exclusive prefix
    T* agg; size_t ntiles;                       // [EA][ntiles] tile aggregates
    u64* final_out;                              // EA limbs, non-null for a trace of ONE tile: the aggregate is `final`
    u32* zero_flag;                              // a device word the host cleared: 1 when some denominator vanished
  };
  static MS_HD size_t lds_bytes() { return ((size_t)EA * TILE + 2 * (size_t)EA * THREADS) * sizeof(T); }
  static MS_DEV X form(const Params& p, const Program& g, u32 f, size_t row) {
    X a = g.form_const[f];
    for (u32 m = g.form_begin[f]; m < g.form_begin[f + 1]; m++) a = e_add<F, EA>(a, e_mul_base<F, EA>(g.term_coef[m], p.cols[(size_t)g.term_col[m] * p.col_stride + row]));
    return a;
  }
  static MS_DEV void run(const Params& p, int bx, int, int, int tid, unsigned char* lds) {
    const Program& g = *p.prog;
    const u32 op = g.op, nfrac = g.nfrac;
    T* sbuf = reinterpret_cast<T*>(lds);               // [EA][TILE]
    T* sa = sbuf + (size_t)EA * TILE;                  // [EA][THREADS] ping
    T* sb = sa + (size_t)EA * THREADS;                 // pong
    const size_t j0 = (size_t)bx * TILE;
    const T one = F::from_u64(1);
    {
      // The rows of a thread are walked by compile-time index (aux_static_for), not by an unrolled loop: a body of this size is past the optimiser's threshold for
      // `#pragma unroll`, and norm / prefix arrays indexed by a loop variable would then live in scratch memory.  The numerators wait in the row's own LDS slot.
      T nrm[SEG], pre[SEG];
      T prod = one; bool zero = false;
      auto fwd = [&](auto I) MS_LAMBDA_INLINE {
        constexpr int it = decltype(I)::value;
        const size_t j = j0 + (size_t)it * THREADS + tid;
        X t = aux_identity<F, EA>(op); T n = one;
        if (j < p.N) {
          X A = form(p, g, 0, j), B = form(p, g, 1, j);
          for (u32 k = 1; k < nfrac; k++) {          // A / B o num / den
            const X num = form(p, g, 2 * k, j), den = form(p, g, 2 * k + 1, j);
            A = op ? e_mul<F>(A, num) : e_add<F, EA>(e_mul<F>(A, den), e_mul<F>(num, B));
            B = e_mul<F>(B, den);
          }
          X C;
          aux_conj_norm<F>(B, &C, &n);
          if (n == 0) { zero = true; n = one; }
          if constexpr (EA == 1) t = A; else t = e_mul<F>(A, C);
        }
        for (int l = 0; l < EA; l++) sbuf[(size_t)l * TILE + it * THREADS + tid] = t.c[l];
        nrm[it] = n;
        pre[it] = prod;                               // product of the norms before this one
        prod = F::mul(prod, n);
      };
      aux_static_for<0, SEG>(fwd);
      if (zero) *p.zero_flag = 1;                      // (racing writers all store the same value)
      T inv = mspoly::fold_base_inv<F>(prod);
      auto bwd = [&](auto I) MS_LAMBDA_INLINE {
        constexpr int it = decltype(I)::value;
        const T ni = F::mul(inv, pre[it]);            // 1 / norm_it
        inv = F::mul(inv, nrm[it]);
        for (int l = 0; l < EA; l++) { T* q = sbuf + (size_t)l * TILE + it * THREADS + tid; *q = F::mul(*q, ni); }
      };
      aux_static_rfor<SEG>(bwd);
    }
    msrt::wg_barrier();
    X a;
    for (int l = 0; l < EA; l++) a.c[l] = sbuf[(size_t)l * TILE + tid * SEG];
#pragma unroll
    for (int i = 1; i < SEG; i++) {
      X c; for (int l = 0; l < EA; l++) c.c[l] = sbuf[(size_t)l * TILE + tid * SEG + i];
      a = aux_comb<F, EA>(op, a, c);
    }
    aux_wg_scan<F, EA>(op, a, tid, sa, sb);
    if (tid == THREADS - 1) {
      for (int l = 0; l < EA; l++) {
        const T v = sa[l * THREADS + tid];
        p.agg[(size_t)l * p.ntiles + bx] = v;
        if (p.final_out) p.final_out[l] = F::to_u64(v);
      }
    }
    X h = aux_identity<F, EA>(op);
    if (tid) for (int l = 0; l < EA; l++) h.c[l] = sa[l * THREADS + tid - 1];
#pragma unroll
    for (int i = 0; i < SEG; i++) {                    // s_i -> the exclusive prefix, in place (a thread touches its own SEG entries only)
      X c; for (int l = 0; l < EA; l++) c.c[l] = sbuf[(size_t)l * TILE + tid * SEG + i];
      for (int l = 0; l < EA; l++) sbuf[(size_t)l * TILE + tid * SEG + i] = h.c[l];
      h = aux_comb<F, EA>(op, h, c);
    }
    msrt::wg_barrier();
#pragma unroll
    for (int it = 0; it < SEG; it++) {
      const size_t j = j0 + (size_t)it * THREADS + tid;
      if (j < p.N) for (int l = 0; l < EA; l++) p.out[(size_t)l * p.out_stride + j] = sbuf[(size_t)l * TILE + it * THREADS + tid];
    }
  }
};

// ---------------------------------------------------------------- carry launch
// ONE workgroup: carry[t] = agg[0] o .. o agg[t-1], final = agg[0] o .. o agg[ntiles-1].  THREADS aggregates at a time; every thread keeps the running carry.
// The loop is bounded by ntiles (2^24 rows in tiles of 256: 256 chunks).
template <class F, int EA> struct AuxCarryKernel {
  typedef typename F::T T;
  typedef Ext<F, EA> X;
  static constexpr int THREADS = msrun::THREADS;
  struct Params { const T* agg; T* carry; size_t ntiles; u32 op; u64* final_out; };
  static MS_HD size_t lds_bytes() { return 2 * (size_t)EA * THREADS * sizeof(T); }
  static MS_DEV void run(const Params& p, int, int, int, int tid, unsigned char* lds) {
    T* sa = reinterpret_cast<T*>(lds);
    T* sb = sa + (size_t)EA * THREADS;
    X carry = aux_identity<F, EA>(p.op);
    for (size_t c0 = 0; c0 < p.ntiles; c0 += THREADS) {
      const size_t t = c0 + tid;
      X v = aux_identity<F, EA>(p.op);
      if (t < p.ntiles) for (int l = 0; l < EA; l++) v.c[l] = p.agg[(size_t)l * p.ntiles + t];
      aux_wg_scan<F, EA>(p.op, v, tid, sa, sb);
      X ex = aux_identity<F, EA>(p.op), tot;
      if (tid) for (int l = 0; l < EA; l++) ex.c[l] = sa[l * THREADS + tid - 1];
      for (int l = 0; l < EA; l++) tot.c[l] = sa[l * THREADS + THREADS - 1];
      if (t < p.ntiles) {
        const X c = aux_comb<F, EA>(p.op, carry, ex);
        for (int l = 0; l < EA; l++) p.carry[(size_t)l * p.ntiles + t] = c.c[l];
      }
      carry = aux_comb<F, EA>(p.op, carry, tot);
      msrt::wg_barrier();                              // the next chunk overwrites sa
    }
    if (tid == 0) for (int l = 0; l < EA; l++) p.final_out[l] = F::to_u64(carry.c[l]);
  }
};

// ---------------------------------------------------------------- apply launch
// z_i = carry[i >> log_tile] o local_i, in place; one row per thread
template <class F, int EA> struct AuxApplyKernel {
  typedef typename F::T T;
  typedef Ext<F, EA> X;
  static constexpr int THREADS = msrun::THREADS;
  struct Params { T* out; size_t out_stride, N; const T* carry; size_t ntiles; u32 log_tile, op; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = (size_t)bx * nthreads + tid;
    if (j >= p.N) return;
    const size_t t = j >> p.log_tile;
    X c, v;
    for (int l = 0; l < EA; l++) { c.c[l] = p.carry[(size_t)l * p.ntiles + t]; v.c[l] = p.out[(size_t)l * p.out_stride + j]; }
    v = aux_comb<F, EA>(p.op, c, v);
    for (int l = 0; l < EA; l++) p.out[(size_t)l * p.out_stride + j] = v.c[l];
  }
};

}  // namespace msrun
