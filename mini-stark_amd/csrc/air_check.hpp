// air_check.hpp — ms_air_check (include/ministark.h; build-defined, diagnostic): the ms_air program of ms_mix_air evaluated on the ROWS of the trace domain, so that a
// refused trace can be told which constraints it violates, and where.  One streaming kernel over column values T_j[i] = P_j(w^i), column-major, N apart:
//   C_t(i) = sum_m coef_m prod_f factor_f(i),   factor (j, row) = T_j[(i + row) mod N],   factor (periodic k, row) = per_val_k[(i + row) mod q_k]
// and row i violates constraint t when C_t(i) != 0 and i is not in X_t.  Per constraint the launch leaves the number of violating rows and the smallest one.
// Shape of mspoly::ComposeAirKernel: a thread owns ITEMS strided rows and walks the program once for all of them; constraint, term, factor and exemption records are the
// same for every lane and the loop counters uniform; the ITEMS loads of a factor are issued first and multiplied behind; every index is masked by a power of two
// minus one (N - 1, q_k - 1), so it is in bounds for every lane.  What differs:
// * nothing is merged: the answer is per constraint, and no combiner r appears;
// * rows past N are MASKED, not computed and dropped - a masked index aliases a real row, which would be counted twice - so `i < N` enters the violation test.  No lane
//   of a live wave leaves early (the cross-lane reduction below needs every lane); a wave whose first row is past N has nothing to do and skips the walk as a whole;
// * the reduction uses no LDS: a wave votes whether any lane saw a violation of constraint t (on a trace that satisfies the AIR: never, and the launch issues no
//   atomic at all); only then it reduces count and smallest row over its lanes by xor-shuffles and ONE lane issues one 64-bit add and one 64-bit minimum on the result
//   words of t - integer atomics, at most one pair per wave and constraint, behind a per-wave partial reduction.  Sums and minima commute: the result does not depend
//   on grid, wave order or launch split.  The result words start at (0, N), written by the host's table upload in front of the launch;
// * the exemption test (a scan of at most 16 rows) runs only for items whose value is not zero;
// * the boundary values T_poly[row] are plain gathers, stored behind the walk by the first workgroup.
// ITEMS = 4: the walk is a chain of dependent steps (record, loads, multiply) as long as the program, so a launch over N rows lasts about one chain whatever ITEMS is
// while the grid fits the chip; fewer rows per thread keep more waves on it for the short domains this runs on (N rows, not blowup N), more would only amortise
// the scalar record reads, which the multiplications outweigh.
// The atomics sit INSIDE the walk, so the records are read with msrt::load_uniform (rt.hpp): behind an atomic the compiler would otherwise read them lane by lane
// (seen in the listing: global_load_dwordx4 per factor record until then, s_load_dwordx4 since).  56 VGPRs (Goldilocks) / 34 (BabyBear), no scratch, no LDS.
#pragma once
#include "poly.hpp"

namespace mspoly {

struct AirCheckCons { u32 nterms, nex; };
template <class F> struct AirCheckKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 4;
  struct Params { const T* cols; size_t N; u32 ncons, nbound; const AirCheckCons* cons; const TermRec<F>* terms; const AirFac* facs /* rowoff = the row offset itself */;
                  const u32* ex_rows /* constraint by constraint */; const T* ptab /* the periodic values */; const u32* bnd /* (poly, row) pairs */;
                  unsigned long long* count; unsigned long long* first; unsigned long long* bnd_got; };
  static MS_HD size_t lds_bytes() { return 0; }
  static MS_DEV void run(const Params& p, int bx, int, int, int tid, unsigned char*) {
    const size_t i0 = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i0 - (size_t)(tid & 63) < p.N) {                // (the wave's first row: the same for its 64 lanes)
      u32 m = 0, f = 0, x = 0;
      for (u32 t = 0; t < p.ncons; t++) {
        const AirCheckCons cr = msrt::load_uniform(p.cons + t);
        T acc[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; it++) acc[it] = 0;
        for (u32 mg = 0; mg < cr.nterms; mg++, m++) {
          const TermRec<F> tr = msrt::load_uniform(p.terms + m);
          T v[ITEMS];
#pragma unroll
          for (int it = 0; it < ITEMS; it++) v[it] = tr.coef;
          for (u32 k = 0; k < tr.nfac; k++, f++) {
            const AirFac fc = msrt::load_uniform(p.facs + f);
            const T* col = fc.kind ? p.ptab + fc.src : p.cols + (size_t)fc.src * p.N;
            T c[ITEMS];                                 // (loaded first, multiplied behind, as in ComposeAirKernel)
#pragma unroll
            for (int it = 0; it < ITEMS; it++) c[it] = col[(i0 + (size_t)it * THREADS + fc.rowoff) & (size_t)fc.mask];
#pragma unroll
            for (int it = 0; it < ITEMS; it++) v[it] = F::mul(v[it], c[it]);
          }
#pragma unroll
          for (int it = 0; it < ITEMS; it++) acc[it] = F::add(acc[it], v[it]);
        }
        unsigned long long cnt = 0, mn = p.N;
#pragma unroll
        for (int it = ITEMS - 1; it >= 0; it--) {       // (descending: the last hit recorded is the smallest row)
          const size_t i = i0 + (size_t)it * THREADS;
          bool bad = i < p.N && acc[it] != 0;
          if (bad) for (u32 k = 0; k < cr.nex; k++) if ((size_t)msrt::load_uniform(p.ex_rows + x + k) == i) bad = false;
          if (bad) { cnt++; mn = i; }
        }
        x += cr.nex;
        if (msrt::wave_vote_any(cnt != 0)) {
          for (int s = 1; s < 64; s <<= 1) {
            cnt += msrt::wave_shfl_xor(cnt, s);
            const unsigned long long o = msrt::wave_shfl_xor(mn, s);
            if (o < mn) mn = o;
          }
          if ((tid & 63) == 0) { msrt::atomic_add_u64(p.count + t, cnt); msrt::atomic_min_u64(p.first + t, mn); }
        }
      }
    }
    if (bx == 0)
      for (u32 b = (u32)tid; b < p.nbound; b += (u32)THREADS) p.bnd_got[b] = F::to_u64(p.cols[(size_t)p.bnd[2 * b] * p.N + p.bnd[2 * b + 1]]);
  }
};

}  // namespace mspoly
