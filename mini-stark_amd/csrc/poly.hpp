// poly.hpp — coefficient-domain kernels of the prover path.
//
//   TransposeIn   row-major trace -> column-major columns   (src/air.rs:151-153 gather)
//   Lincomb       constraint poly = sum_t s_t * P_idx[t]     (tests/e2e_goldilocks.rs:48-59 closures)
//   Mix           validity = sum_i r^i f_i                   (src/starks.rs:108-119, quirk Q1)
//   Eval          sum_k c_k z^k at an extension point        (src/starks.rs:142-149, src/fri.rs:354-359,151-153)
//   Fold          even + alpha * odd                         (src/fri.rs:361-372)
//   SuffixHorner  H_j = sum_{k>=j} f_k z^(k-j): quotient by (x - z) is q_j = H_{j+1},
//                 remainder/evaluation is H_0                (src/fri.rs:91-101 and 159-167)
//   Degree        trimmed length of a coefficient vector     ([ark-mem] DensePolynomial trims)
//   FindFirst     first index whose leaf equals a value      (src/merkle.rs:216-225, quirk Q7)
//
// All are streaming kernels over SoA limb arrays: HBM-bound, algorithmic bytes
// = elements read + written once.
#pragma once
#include <type_traits>
#include "field.hpp"
#include "ntt.hpp"

namespace mspoly {

constexpr int THREADS = 256;

// ---------------------------------------------------------------- TransposeIn
template <class F> struct TransposeInKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  // bad: optional device word (zeroed by the caller) set to 1 when an input element is not canonical (>= p)
  struct Params { const u64* src; T* dst; size_t N, w, dst_stride; T rinv; int mont; /* mont: src holds x*2^64 mod p; rinv = 2^-64 mod p */ u32* bad; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t f = (size_t)bx * nthreads + tid;
    if (f >= p.N * p.w) return;
    const size_t row = f / p.w, col = f - row * p.w;
    const u64 raw = p.src[f];
    const bool oob = raw >= F::P;
    if (oob && p.bad) *p.bad = 1;            // racing writers all store the same value; the call then fails with MS_ERR_ARG
    T v = F::from_u64(oob ? 0 : raw);
    if (p.mont) v = F::mul(v, p.rinv);
    p.dst[col * p.dst_stride + row] = v;
  }
};
// The same for WIDE traces (r04: the 64-column AIR of BASELINE configs[4]): with one thread per element the writes of a wave scatter over 64 columns, 8 bytes each
// (3.8 ms for 2^22 rows x 64 columns = 4.4 x what the bytes cost); here a workgroup moves a 64 x 64 tile through LDS - rows in as 512-byte runs, columns out as
// 512-byte runs.  Grid: (rows / 64, ceil(w / 64)).
template <class F> struct TransposeInTiledKernel {
  typedef typename F::T T;
  static constexpr int THREADS = 256, TILE = 64;
  typedef typename TransposeInKernel<F>::Params Params;
  static MS_HD int nphases(const Params&) { return 2; }
  static MS_HD size_t lds_bytes() { return (size_t)TILE * (TILE + 1) * sizeof(T); }
  static MS_DEV void phase(int ph, const Params& p, int bx, int by, int tid, int nthreads, unsigned char* lds) {
    T* tile = reinterpret_cast<T*>(lds);   // [col][row], pitch TILE + 1
    const size_t row0 = (size_t)bx * TILE, col0 = (size_t)by * TILE;
    if (ph == 0) {
      for (int idx = tid; idx < TILE * TILE; idx += nthreads) {
        const int r = idx / TILE, c = idx % TILE;
        const size_t row = row0 + r, col = col0 + c;
        if (row >= p.N || col >= p.w) continue;
        const u64 raw = p.src[row * p.w + col];
        const bool oob = raw >= F::P;
        if (oob && p.bad) *p.bad = 1;
        T v = F::from_u64(oob ? 0 : raw);
        if (p.mont) v = F::mul(v, p.rinv);
        tile[c * (TILE + 1) + r] = v;
      }
      return;
    }
    for (int idx = tid; idx < TILE * TILE; idx += nthreads) {
      const int c = idx / TILE, r = idx % TILE;
      const size_t row = row0 + r, col = col0 + c;
      if (row >= p.N || col >= p.w) continue;
      p.dst[col * p.dst_stride + row] = tile[c * (TILE + 1) + r];
    }
  }
};
// plain widening / narrowing copies between the u64 ABI and device storage
template <class F> struct NarrowKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const u64* src; T* dst; size_t n; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t f = (size_t)bx * nthreads + tid;
    if (f < p.n) p.dst[f] = F::from_u64(p.src[f]);
  }
};
// dst[j*out_stride + l] (u64) = src[l*limb_stride + j]   (SoA device limbs -> AoS u64 ABI order)
template <class F> struct WidenKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* src; u64* dst; size_t n, limb_stride; u32 E; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t f = (size_t)bx * nthreads + tid;
    if (f >= p.n * p.E) return;
    const size_t j = f / p.E; const u32 l = (u32)(f - j * p.E);
    p.dst[f] = F::to_u64(p.src[(size_t)l * p.limb_stride + j]);
  }
};
// row-major u64 matrix out of column-major device columns (LDE read-back: src/air.rs:52-58 layout)
template <class F> struct TransposeOutKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* src; u64* dst; size_t rows, cols, src_stride; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t f = (size_t)bx * nthreads + tid;
    if (f >= p.rows * p.cols) return;
    const size_t row = f / p.cols, col = f - row * p.cols;
    p.dst[f] = F::to_u64(p.src[col * p.src_stride + row]);
  }
};

// ---------------------------------------------------------------- Lincomb / Mix
constexpr int MAX_TERMS = 8;
template <class F> struct LincombKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* polys; size_t stride, n; T* dst; T s[MAX_TERMS]; int idx[MAX_TERMS]; int k; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = (size_t)bx * nthreads + tid;
    if (j >= p.n) return;
    T acc = 0;
    const T one = F::from_u64(1), minus_one = F::neg(one);
    for (int t = 0; t < p.k; t++) {   // the scalars are uniform over the launch: +1 / -1 (most of an AIR's transition constraints) are scalar branches, not multiplications - same canonical values
      const T v = p.polys[(size_t)p.idx[t] * p.stride + j];
      if (p.s[t] == one) acc = F::add(acc, v);
      else if (p.s[t] == minus_one) acc = F::sub(acc, v);
      else acc = F::add(acc, F::mul(p.s[t], v));
    }
    p.dst[j] = acc;
  }
};
// Several linear combinations of the SAME few columns in one sweep: out[o][j] = sum_u m[o][u] * col[src[u]][j].  Every source element is
// loaded once for all outputs (the three constraint columns of the Fibonacci LDE: 6 column transfers instead of 10).  m is uniform over the
// launch, so the zero tests are scalar branches; field addition is exact, so the order of the terms does not matter.
constexpr int LCM_SRC = 8, LCM_OUT = 4;
template <class F> struct LincombMultiKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* polys; size_t stride, n; T* dst[LCM_OUT]; int src[LCM_SRC]; T m[LCM_OUT][LCM_SRC]; int nsrc, nout; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = (size_t)bx * nthreads + tid;
    if (j >= p.n) return;
    T v[LCM_SRC];
#pragma unroll
    for (int u = 0; u < LCM_SRC; u++) v[u] = (u < p.nsrc) ? p.polys[(size_t)p.src[u] * p.stride + j] : (T)0;
#pragma unroll
    for (int o = 0; o < LCM_OUT; o++) {
      if (o < p.nout) {
        T acc = 0;
#pragma unroll
        for (int u = 0; u < LCM_SRC; u++)
          if (u < p.nsrc && p.m[o][u] != 0) {
            if (p.m[o][u] == F::from_u64(1)) acc = F::add(acc, v[u]);
            else if (p.m[o][u] == F::neg(F::from_u64(1))) acc = F::sub(acc, v[u]);
            else acc = F::add(acc, F::mul(p.m[o][u], v[u]));
          }
        p.dst[o][j] = acc;
      }
    }
  }
};
template <class F> struct MixKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* polys; size_t stride, n; int c; T r; T* dst; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = (size_t)bx * nthreads + tid;
    if (j >= p.n) return;
    T acc = p.polys[(size_t)(p.c - 1) * p.stride + j];
    for (int i = p.c - 2; i >= 0; i--) acc = F::add(F::mul(acc, p.r), p.polys[(size_t)i * p.stride + j]);
    p.dst[j] = acc;
  }
};

// ---------------------------------------------------------------- Eval
// Up to MAX_POLYS polynomials with EC-limb coefficients evaluated at one E-limb
// point.  Coefficient k of poly i, limb l: base[i*poly_stride + l*limb_stride + off[i] + k*kstride].
// Workgroup b owns coefficients [b*CH, (b+1)*CH), CH = THREADS*ITEMS: thread t accumulates
// sum_j c[b*CH + t + j*THREADS] * z^(t + j*THREADS) (its z^t is a product of the host-supplied
// z^(2^i), no per-thread exponentiation), the block sums the threads and writes the partial
// P_b (WITHOUT the factor z^(b*CH)).  ReducePartials then forms sum_b P_b (z^CH)^b.
// With a single block the result goes straight to `dst`.
constexpr int MAX_POLYS = 8;
// ITEMS_ = coefficients per thread: 16 for long polynomials, 4 up to 2^19 coefficients (MS_EVAL_SMALL_MAX), whose launches are latency - 16 dependent
// load + multiply-add iterations per thread made a 2^15-coefficient evaluation as slow as a 2^19-coefficient one, 28-34 us; with 4: 12-18 us, the Eval launches of
// one proof 400 -> 260 us, ReducePartials 62 -> 77 us; eight proofs in flight: neutral (profiles/r04_small_round_kernels_ab.log).
template <class F, int EC, int E, int ITEMS_ = 16> struct EvalKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = ITEMS_;
  struct Params {
    const T* base; size_t poly_stride, limb_stride, kstride;
    size_t off[MAX_POLYS], count[MAX_POLYS]; int npoly;
    Ext<F, E> zpow2[9];   // z^(2^i), i <= 8  (zpow2[8] = z^THREADS)
    T* partials;          // [nblocks][npoly][E]
    // a SINGLE workgroup whose partial sums are the values, stored to page-locked host memory: flag and aux word as ReducePartialsKernel's.  (More than one workgroup:
    // ReducePartialsKernel follows as a launch of its own - letting the last workgroup to finish sum the partials, as the fused FRI round does, was tried in r05 and
    // cost 8-9 us MORE per evaluation than the second launch: 512 workgroups each paying a device-scope release in front of the counter.)
    msrt::HostFlag flag;
    const unsigned long long* aux_src; unsigned long long* aux_dst;
    unsigned single;      // 1: this launch is that single workgroup
  };
  static MS_HD size_t lds_bytes() { return ((size_t)MAX_POLYS * E * (THREADS / 64) + 32 * (size_t)E) * sizeof(T); }
  // coefficient * power, the power in table form (e_to_tw)
  static MS_DEV Ext<F, E> mul_coef(const Ext<F, E>& pwt, const T* c) {
    if (EC == 1) { Ext<F, E> r; for (int l = 0; l < E; l++) r.c[l] = F::mul_tw(c[0], pwt.c[l]); return r; }
    Ext<F, E> cc; for (int l = 0; l < E; l++) cc.c[l] = c[l < EC ? l : 0];
    return e_mul_tw<F>(cc, pwt);
  }
  // Cooperative kernel (barrier inside): the block sum runs as a butterfly of wave shuffles (6 steps) plus one LDS hop between the
  // four waves, instead of `width` threads each adding 256 LDS values one after the other (a ~3 us dependent chain per launch, and
  // these launches sit on the proof's latency path: 2 per FRI round).
  static MS_DEV void run(const Params& p, int bx, int, int, int tid, unsigned char* lds) {
    T* red = reinterpret_cast<T*>(lds);  // [npoly*E][waves]
    constexpr int WAVES = THREADS / 64;
    // z^tid = z^(tid & 15) * z^(16 (tid >> 4)): 32 lanes build the two 16-entry tables (4 multiplications each), every thread then needs ONE multiplication
    // instead of the eight of a per-thread bit product (which were a third of a thread's multiplications with two polynomials and 16 coefficients each)
    T* tab = red + (size_t)MAX_POLYS * E * WAVES;  // [32][E]
    if (tid < 32) {
      Ext<F, E> tw = e_one<F, E>();
      const int j = tid & 15, b0 = tid & 16 ? 4 : 0;
#pragma unroll
      for (int i = 0; i < 4; i++) if ((j >> i) & 1) tw = e_mul<F>(tw, p.zpow2[b0 + i]);
      for (int l = 0; l < E; l++) tab[(size_t)tid * E + l] = tw.c[l];
    }
    msrt::wg_barrier();
    Ext<F, E> acc[MAX_POLYS];
    for (int i = 0; i < MAX_POLYS; i++) acc[i] = e_zero<F, E>();
    size_t k = (size_t)bx * (THREADS * ITEMS) + tid;
    size_t kmax = 0;
    for (int i = 0; i < MAX_POLYS; i++) if (i < p.npoly && p.count[i] > kmax) kmax = p.count[i];
    if (k < kmax) {
      Ext<F, E> plo, phi;
      for (int l = 0; l < E; l++) { plo.c[l] = tab[(size_t)(tid & 15) * E + l]; phi.c[l] = tab[(size_t)(16 + (tid >> 4)) * E + l]; }
      const Ext<F, E> zstep = e_to_tw<F, E>(p.zpow2[8]);
      Ext<F, E> pw = e_to_tw<F, E>(e_mul<F>(plo, phi));   // z^k in table form from here on: every product below is one multiplication + one reduction per limb pair
      for (int it = 0; it < ITEMS && k < kmax; it++, k += THREADS) {
#pragma unroll
        for (int i = 0; i < MAX_POLYS; i++) {
          if (i < p.npoly && k < p.count[i]) {
            T c[EC];
            const T* ptr = p.base + (size_t)i * p.poly_stride + p.off[i] + k * p.kstride;
            for (int l = 0; l < EC; l++) c[l] = ptr[(size_t)l * p.limb_stride];
            acc[i] = e_add<F, E>(acc[i], mul_coef(pw, c));
          }
        }
        pw = e_mul_tw<F>(pw, zstep);
      }
    }
    const int width = p.npoly * E;
#pragma unroll
    for (int i = 0; i < MAX_POLYS; i++) {
      if (i < p.npoly) {
#pragma unroll
        for (int l = 0; l < E; l++) {
          T v = acc[i].c[l];
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) v = F::add(v, (T)msrt::wave_shfl_xor((unsigned long long)v, m));
          if ((tid & 63) == 0) red[(size_t)(i * E + l) * WAVES + (tid >> 6)] = v;
        }
      }
    }
    msrt::wg_barrier();
    if (tid < width) {
      T s = 0;
      for (int t = 0; t < WAVES; t++) s = F::add(s, red[(size_t)tid * WAVES + t]);
      p.partials[(size_t)bx * width + tid] = s;
    }
    if (p.single) {
      if (tid == 0 && p.aux_src) *p.aux_dst = *p.aux_src;
      msrt::raise_host_flag_wg(p.flag, tid);
    }
  }
};
// out[i] = sum_b partials[b][i] * zc^b,  i < npoly (E limbs each), zc = z^CH.
// One workgroup: thread t runs Horner over its contiguous range of blocks, scales by
// (zc^S)^t (bit product of zs2[i] = (zc^S)^(2^i)) and the block adds the threads.
template <class F, int E> struct ReducePartialsKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  // sum_b P_b zc^b with thread t taking the blocks b = t, t + THREADS, t + 2 THREADS, ...: neighbouring lanes read neighbouring partials and the loads of a
  // thread do not depend on each other (r03: with a contiguous run of blocks per thread every iteration waited for its own uncoalesced load - 6.4 ms of the
  // 66 ms of a 2^24-row proof sat in this one-workgroup kernel).  zc = z^CH; zs2[i] = zc^(2^i), i < 8; zc_step = zc^THREADS.
  struct Params { const T* partials; size_t nblocks, per_thread /* ceil(nblocks / THREADS) */; int npoly; Ext<F, E> zc_step; Ext<F, E> zs2[8]; T* out; msrt::HostFlag flag; /* raised behind `out` (page-locked host memory then) */
                  const unsigned long long* aux_src; unsigned long long* aux_dst; /* optional: a device word that travels to page-locked host memory with the values (the validity polynomial's trimmed length, found by ms_mix, on DEEP-ALI's last evaluation) */ };
  static MS_HD size_t lds_bytes() { return (size_t)MAX_POLYS * E * (THREADS / 64) * sizeof(T); }
  static MS_DEV void run(const Params& p, int, int, int, int tid, unsigned char* lds) {   // cooperative: wave-shuffle block sum, as EvalKernel
    T* red = reinterpret_cast<T*>(lds);
    constexpr int WAVES = THREADS / 64;
    const int width = p.npoly * E;
    Ext<F, E> acc[MAX_POLYS];
    for (int i = 0; i < MAX_POLYS; i++) acc[i] = e_zero<F, E>();
    if ((size_t)tid < p.nblocks) {
      for (size_t j = p.per_thread; j-- > 0;) {   // Horner in zc^THREADS over this thread's blocks, last one first
        const size_t b = (size_t)tid + j * THREADS;
        const bool have = b < p.nblocks;
#pragma unroll
        for (int i = 0; i < MAX_POLYS; i++) {
          if (i < p.npoly) {
            Ext<F, E> v; for (int l = 0; l < E; l++) v.c[l] = have ? p.partials[b * width + i * E + l] : (T)0;
            acc[i] = e_add<F, E>(e_mul<F>(acc[i], p.zc_step), v);
          }
        }
      }
      Ext<F, E> sc = e_one<F, E>();   // zc^tid
#pragma unroll
      for (int i = 0; i < 8; i++) if ((tid >> i) & 1) sc = e_mul<F>(sc, p.zs2[i]);
#pragma unroll
      for (int i = 0; i < MAX_POLYS; i++) if (i < p.npoly) acc[i] = e_mul<F>(acc[i], sc);
    }
#pragma unroll
    for (int i = 0; i < MAX_POLYS; i++) {
      if (i < p.npoly) {
#pragma unroll
        for (int l = 0; l < E; l++) {
          T v = acc[i].c[l];
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) v = F::add(v, (T)msrt::wave_shfl_xor((unsigned long long)v, m));
          if ((tid & 63) == 0) red[(size_t)(i * E + l) * WAVES + (tid >> 6)] = v;
        }
      }
    }
    msrt::wg_barrier();
    if (tid < width) {
      T s = 0;
      for (int t = 0; t < WAVES; t++) s = F::add(s, red[(size_t)tid * WAVES + t]);
      p.out[tid] = s;
    }
    if (tid == 0 && p.aux_src) *p.aux_dst = *p.aux_src;
    msrt::raise_host_flag_wg(p.flag, tid);
  }
};

// ---------------------------------------------------------------- Fold
// dst_j = src[2j] + alpha * src[2j+1],  j < m = ceil(n/2)   (fri.rs:329-343 split + 361-372 fold)
template <class F, int E> struct FoldKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  // first_out (optional; a rank of a sharded proof): the first folded element also goes to first_out[0 .. E) and E zero limbs behind it - the payload of the scan's carry
  // exchange ([first element | aggregate]; the aggregate launch overwrites the zeros), which took a fill and a copy launch of its own until r05
  struct Params { const T* src; size_t src_limb_stride, n; T* dst; size_t dst_limb_stride; Ext<F, E> alpha; T* first_out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = (size_t)bx * nthreads + tid;
    const size_t m = (p.n + 1) / 2;
    if (j >= m) return;
    Ext<F, E> ev, od = e_zero<F, E>();
    for (int l = 0; l < E; l++) ev.c[l] = p.src[(size_t)l * p.src_limb_stride + 2 * j];
    if (2 * j + 1 < p.n) for (int l = 0; l < E; l++) od.c[l] = p.src[(size_t)l * p.src_limb_stride + 2 * j + 1];
    Ext<F, E> r = e_add<F, E>(ev, e_mul<F>(p.alpha, od));
    for (int l = 0; l < E; l++) p.dst[(size_t)l * p.dst_limb_stride + j] = r.c[l];
    if (j == 0 && p.first_out) for (int l = 0; l < E; l++) { p.first_out[l] = r.c[l]; p.first_out[E + l] = 0; }
  }
};

// ---------------------------------------------------------------- SuffixHorner
// A job describes one vector f_j (j < m): limb l at in[l*in_limb_stride + in_off + j*in_stride].
// Block b of a job owns [b*BS, (b+1)*BS), BS = THREADS*SEG.  Jobs are batched over blockIdx.y
// (a device table, or one job inline in the kernel arguments).
//   mode AGG  : agg[l*agg_limb_stride + b] = sum_{k in block} f_k z^(k - b*BS)
//   mode FINAL: with carry-in Hin_b = carry[l*carry_limb_stride + b] (carry == null: 0),
//               writes H_j for j >= 1 to out[l*out_limb_stride + out_off + (j-1)*out_stride]
//               (u64 or T elements, out == null: discarded) and H_0 to h0[l];
//               tail_zero: also stores 0 at out index m-1 (the output is the carry array of
//               the level below, whose last block has no carry-in); tail_zero == 2: stores the
//               carry-in propagated to position m instead (jobs with a carry-in at the top level).
// zpow[i] = z^(SEG * 2^i), i < 9.
constexpr int SH_SEG = 8;
constexpr int SH_BS = THREADS * SH_SEG;
template <class F, int E> struct SHJob {
  typedef typename F::T T;
  const T* in; size_t in_limb_stride, in_off, in_stride, m;
  void* out; size_t out_limb_stride, out_off, out_stride;
  T* h0;
  T* agg; size_t agg_limb_stride;
  const T* carry; size_t carry_limb_stride;
  u32 out_u64, tail_zero;
  u32 out_h0;   // H_0 also goes to `out`, one out_stride below out_off (a rank of a sharded proof whose range does not start at coefficient 0: its H_0 is a quotient coefficient)
  Ext<F, E> z; Ext<F, E> zpow[9];
};
template <class F, int E> struct SuffixHornerKernel {
  typedef typename F::T T;
  typedef SHJob<F, E> Job;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const Job* jobs; Job inline_job; int final_mode; };
  static MS_HD size_t lds_bytes() { return ((size_t)E * SH_BS + 2 * (size_t)E * (THREADS + 1)) * sizeof(T); }
  // Cooperative kernel (r04; thirteen barrier-separated phases of the generic phase harness until then): the job is read ONCE - as phases, every step fetched its
  // fields from the job table again behind a barrier that also drains vector memory, and a launch cost 17-19 us whatever its size; these launches sit on the proof's
  // latency path (one to three per FRI round).
  static MS_DEV void run(const Params& p, int bx, int by, int, int tid, unsigned char* lds) {
    const Job jb = p.jobs ? p.jobs[by] : p.inline_job;
    const size_t nb = jb.m ? (jb.m + SH_BS - 1) / SH_BS : 1;
    if ((size_t)bx >= nb) return;   // (the whole workgroup)
    T* fbuf = reinterpret_cast<T*>(lds);                 // [E][BS]
    T* sa = fbuf + (size_t)E * SH_BS;                    // [E][THREADS+1]  ping
    T* sb = sa + (size_t)E * (THREADS + 1);              // pong
    const size_t j0 = (size_t)bx * SH_BS;
    // coalesced load
    for (int i = tid; i < SH_BS; i += THREADS) {
      const size_t j = j0 + i;
      for (int l = 0; l < E; l++)
        fbuf[(size_t)l * SH_BS + i] = (j < jb.m) ? jb.in[(size_t)l * jb.in_limb_stride + jb.in_off + j * jb.in_stride] : (T)0;
    }
    msrt::wg_barrier();
    const Ext<F, E> z = e_to_tw<F, E>(jb.z);   // table form: the multiplicand of every Horner step (e_mul_tw)
    {  // per-thread segment aggregate a_t
      Ext<F, E> a = e_zero<F, E>();
#pragma unroll
      for (int i = SH_SEG - 1; i >= 0; i--) {
        Ext<F, E> c; for (int l = 0; l < E; l++) c.c[l] = fbuf[(size_t)l * SH_BS + tid * SH_SEG + i];
        a = e_add<F, E>(e_mul_tw<F>(a, z), c);
      }
      for (int l = 0; l < E; l++) sa[(size_t)l * (THREADS + 1) + tid] = a.c[l];
      if (tid == 0) {  // virtual element THREADS = carry-in
        for (int l = 0; l < E; l++) {
          T cv = 0;
          if (p.final_mode && jb.carry) cv = jb.carry[(size_t)l * jb.carry_limb_stride + bx];
          sa[(size_t)l * (THREADS + 1) + THREADS] = cv;
        }
      }
    }
    msrt::wg_barrier();
#pragma unroll
    for (int step = 0; step < 9; step++) {  // suffix scan over THREADS+1 entries, distance d = 2^step
      const int d = 1 << step;
      T* src = (step & 1) ? sb : sa;
      T* dst = (step & 1) ? sa : sb;
      const Ext<F, E> zp = e_to_tw<F, E>(jb.zpow[step]);
      for (int t = tid; t <= THREADS; t += THREADS) {
        Ext<F, E> v; for (int l = 0; l < E; l++) v.c[l] = src[(size_t)l * (THREADS + 1) + t];
        if (t + d <= THREADS) {
          Ext<F, E> u; for (int l = 0; l < E; l++) u.c[l] = src[(size_t)l * (THREADS + 1) + t + d];
          v = e_add<F, E>(v, e_mul_tw<F>(u, zp));
        }
        for (int l = 0; l < E; l++) dst[(size_t)l * (THREADS + 1) + t] = v.c[l];
      }
      msrt::wg_barrier();
    }
    T* sc = sb;  // 9 steps: the last one (step 8, even) wrote sb
    if (!p.final_mode) {
      if (tid == 0) for (int l = 0; l < E; l++) jb.agg[(size_t)l * jb.agg_limb_stride + bx] = sc[(size_t)l * (THREADS + 1)];
      return;
    }
    {
      Ext<F, E> h; for (int l = 0; l < E; l++) h.c[l] = sc[(size_t)l * (THREADS + 1) + tid + 1];
#pragma unroll
      for (int i = SH_SEG - 1; i >= 0; i--) {
        Ext<F, E> c; for (int l = 0; l < E; l++) c.c[l] = fbuf[(size_t)l * SH_BS + tid * SH_SEG + i];
        h = e_add<F, E>(e_mul_tw<F>(h, z), c);
        for (int l = 0; l < E; l++) fbuf[(size_t)l * SH_BS + tid * SH_SEG + i] = h.c[l];
      }
    }
    msrt::wg_barrier();
    for (int i = tid; i < SH_BS; i += THREADS) {
      const size_t j = j0 + i;
      if (j >= jb.m && !(j == 0)) continue;
      for (int l = 0; l < E; l++) {
        const T v = fbuf[(size_t)l * SH_BS + i];
        if (j == 0) {
          if (jb.h0) jb.h0[l] = v;
          if (jb.out_h0 && jb.out) {
            const size_t o = (size_t)l * jb.out_limb_stride + jb.out_off - jb.out_stride;
            if (jb.out_u64) reinterpret_cast<u64*>(jb.out)[o] = F::to_u64(v); else reinterpret_cast<T*>(jb.out)[o] = v;
          }
        } else if (jb.out) {
          const size_t o = (size_t)l * jb.out_limb_stride + jb.out_off + (j - 1) * jb.out_stride;
          if (jb.out_u64) reinterpret_cast<u64*>(jb.out)[o] = F::to_u64(v); else reinterpret_cast<T*>(jb.out)[o] = v;
        }
      }
      if (jb.tail_zero && jb.out && j + 1 == jb.m) {
        for (int l = 0; l < E; l++) {
          // tail_zero == 2 (a job with an external carry-in at its top level): the last block of the level below is not the end of the vector - its carry-in is the
          // suffix sum at position m of THIS level = the block's carry-in propagated through the zero padding behind element m - 1 (fbuf holds H at every position)
          T tv = 0;
          if (jb.tail_zero == 2) tv = (i + 1 < SH_BS) ? fbuf[(size_t)l * SH_BS + i + 1] : sc[(size_t)l * (THREADS + 1) + THREADS];
          const size_t o = (size_t)l * jb.out_limb_stride + jb.out_off + j * jb.out_stride;
          if (jb.out_u64) reinterpret_cast<u64*>(jb.out)[o] = F::to_u64(tv); else reinterpret_cast<T*>(jb.out)[o] = tv;
        }
      }
    }
  }
};

// ---------------------------------------------------------------- FRI fold in the evaluation domain
// The codeword of FRI round i+1 straight from the codeword of round i, without a transform:
// with f = even(x^2) + x odd(x^2) the round polynomial is g(y) = (even(y) + alpha odd(y) - c) / (y - z)
// (fri.rs:96-101: fold, subtract B(alpha), exact division by (x - z)), and on the next domain y = x^2
//   even(y) = (f(x) + f(-x)) / 2,   odd(y) = (f(x) - f(-x)) / (2x),   1/(y - z) = C(y) / n(y)
// with C the product of the conjugates of (y - z) and n its norm down to the base field:
//   Fp2 (Goldilocks):  C = (y - z0) + z1 u,                    n = (y - z0)^2 - 7 z1^2
//   Fp4 (BabyBear):    A = (y - z0) - z1 u, M = A^2 - (z2 + z3 u)^2 (u - 11), C = (A conj(M), (z2 + z3 u) conj(M)), n = M0^2 - 11 M1^2.
// Field arithmetic is exact, so these are the values the size-D/2 NTT of g's coefficients (fri.rs:350) would give.
// z outside the base field keeps the norm non-zero; the host falls back to the NTT otherwise.
// One thread owns ITEMS outputs and inverts their norms together (Montgomery's trick + one field inversion).
// Index maps: output j = t*m_out + i (t < groups), inputs f(x) at t*2*m_out + i and f(-x) m_out further, domain index
// r = i (replicated round) or 2*(rank + W*i) + t (sharded round: this rank's two cosets).
template <class F> MS_HD typename F::T fold_base_inv(typename F::T x) { return f_inv<F>(x); }
template <> MS_HD u64 fold_base_inv<GL>(u64 x) { return gl_inv_chain(x); }
// ITEMS_: outputs per thread, one field inversion per thread (Montgomery's trick over its norms).  1 is the LATENCY form for the small late rounds, where a launch is
// one wave deep anyway and eight serial outputs per thread only stretch it (with 8 a launch took 22 us whatever its size; one proof alone on the GPU: 118.6 -> 120.4
// proofs/s, eight in flight: neutral - profiles/r04_small_round_kernels_ab.log); 2 is the evaluation side of the fused tail rounds (fri_tail.hpp).  The large rounds
// run the THROUGHPUT form, FriFoldWgKernel below (until then: this kernel with 8).
template <class F, int E, int ITEMS_ = 8> struct FriFoldEvalKernel {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  static_assert(E == 2 || E == 4, "quadratic or quartic tower");
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = ITEMS_;
  struct Params {
    const T* src; size_t src_limb_stride; T* dst; size_t dst_limb_stride;
    size_t m_out; u32 log_m /* log2 m_out */, groups, shard_W, shard_k;
    const T* tw_lo; const T* tw_hi; u32 lo_bits, log_D;   // F::to_tw(w_D^e) = tw_lo[e & mask] * tw_hi[e >> lo_bits] (the size-D forward plan)
    X alpha, c2 /* 2 (B0 + B1 alpha) */, z;
    T inv2;
  };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV T w_tab(const Params& p, size_t e) {
    T tw = p.tw_lo[e & (((size_t)1 << p.lo_bits) - 1)];
    const size_t eh = e >> p.lo_bits;
    if (eh) tw = F::mul_tw(tw, p.tw_hi[eh]);
    return tw;
  }
  // conjugate product C and base-field norm n of (y - z), yd = y - z0
  static MS_DEV void inv_parts(const Params& p, T yd, X* C, T* n) {
    const T nr = F::from_u64(F::NR2);
    if constexpr (E == 2) {
      C->c[0] = yd; C->c[1] = p.z.c[1];
      *n = F::sub(F::mul(yd, yd), F::mul(nr, F::mul(p.z.c[1], p.z.c[1])));
    } else {
      Ext<F, 2> A, zb, K;
      A.c[0] = yd; A.c[1] = F::neg(p.z.c[1]);
      zb.c[0] = p.z.c[2]; zb.c[1] = p.z.c[3];
      K = e_mul_nr4<F>(e_mul<F>(zb, zb));
      const Ext<F, 2> M = e_sub<F, 2>(e_mul<F>(A, A), K);
      Ext<F, 2> Mc; Mc.c[0] = M.c[0]; Mc.c[1] = F::neg(M.c[1]);
      *n = F::sub(F::mul(M.c[0], M.c[0]), F::mul(nr, F::mul(M.c[1], M.c[1])));
      const Ext<F, 2> c0 = e_mul<F>(A, Mc), c1 = e_mul<F>(zb, Mc);
      C->c[0] = c0.c[0]; C->c[1] = c0.c[1]; C->c[2] = c1.c[0]; C->c[3] = c1.c[1];
    }
  }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t total = p.m_out * p.groups, Dm = ((size_t)1 << p.log_D) - 1;
    const size_t j0 = (size_t)bx * ((size_t)nthreads * ITEMS) + tid;
    X tt[ITEMS]; T nrm[ITEMS], pre[ITEMS];
    T run = F::from_u64(1);
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      const size_t j = j0 + (size_t)it * nthreads;
      tt[it] = e_zero<F, E>(); nrm[it] = F::from_u64(1);
      if (j < total) {
        const size_t t = j >> p.log_m, i = j & (p.m_out - 1);
        const size_t ia = t * 2 * p.m_out + i, ib = ia + p.m_out;
        const size_t r = p.shard_W ? 2 * ((size_t)p.shard_k + (size_t)p.shard_W * i) + t : i;
        X a, b;
#pragma unroll
        for (int l = 0; l < E; l++) { a.c[l] = p.src[(size_t)l * p.src_limb_stride + ia]; b.c[l] = p.src[(size_t)l * p.src_limb_stride + ib]; }
        const X s = e_add<F, E>(a, b), d = e_sub<F, E>(a, b);
        const T xinv = w_tab(p, (Dm + 1 - r) & Dm);                       // table form of x^-1 = w_D^(D - r)
        X u;                                                               // alpha / x
#pragma unroll
        for (int l = 0; l < E; l++) u.c[l] = F::mul_tw(p.alpha.c[l], xinv);
        const X num = e_sub<F, E>(e_add<F, E>(s, e_mul<F>(u, d)), p.c2);   // 2 (folded - c)
        const T y = F::from_tw(w_tab(p, (2 * r) & Dm));                   // y = x^2
        X C;
        inv_parts(p, F::sub(y, p.z.c[0]), &C, &nrm[it]);
        tt[it] = e_mul<F>(num, C);
      }
      pre[it] = run;                 // product of the norms before this one
      run = F::mul(run, nrm[it]);
    }
    T inv = F::mul(fold_base_inv<F>(run), p.inv2);   // 1 / (2 * product of all norms)
#pragma unroll
    for (int it = ITEMS - 1; it >= 0; it--) {
      const size_t j = j0 + (size_t)it * nthreads;
      const T ni = F::mul(inv, pre[it]);             // 1 / (2 norm_it)
      inv = F::mul(inv, nrm[it]);
      if (j < total) {
#pragma unroll
        for (int l = 0; l < E; l++) p.dst[(size_t)l * p.dst_limb_stride + j] = F::mul(tt[it].c[l], ni);
      }
    }
  }
};

// ---------------------------------------------------------------- folded FRI (build-defined; include/ministark.h): the fold by a = 2^K_ in the evaluation domain
// Output b < m_out = D / a of the next codeword from the a values of the coset {x w^t}, x = w_D^b, w = w_D^(D/a), which lie m_out apart in the source:
// with P the interpolant of degree < a of those values, P(X) = sum_s p_s X^s, the unnormalised inverse DFT gives u_s = sum_t v_t w^(-ts) = a p_s x^s, and
//   P(alpha) = (1/a) sum_s u_s (alpha / x)^s
// is a Horner scan in alpha x^-1 over the DFT outputs.  x^-1 = w_D^(D - b) comes from the plan's tables (as FriFoldEvalKernel::w_tab), the powers of w^-1 and 1/a
// from the host in table form: no inversion here.  The DFT is decimation in frequency, its outputs left in bit-reversed order and read in that order by the scan;
// every array index is a compile-time constant (a * E limbs in registers: 32 u32 for BabyBear at a = 8, 16 u64 for Goldilocks).
// One thread owns one output; lanes hold consecutive b, so each of the a * E loads of a wave is one contiguous run.  a E words read, E written per output.
template <class F, int E, int K_> struct FriFoldArityKernel {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  static_assert(K_ >= 1 && K_ <= 3, "arity 2, 4 or 8");
  static constexpr int THREADS = mspoly::THREADS, A = 1 << K_;
  struct Params {
    const T* src; size_t src_limb_stride; T* dst; size_t dst_limb_stride;
    size_t m_out;                                          // D / a outputs
    const T* tw_lo; const T* tw_hi; u32 lo_bits, log_D;   // F::to_tw(w_D^e) = tw_lo[e & mask] * tw_hi[e >> lo_bits] (the size-D forward plan)
    X alpha;
    T wt[4];                                               // table form of w^-j, j < a / 2 (wt[0] is not read)
    T inv_a;                                               // table form of 1 / a
  };
  static MS_HD int nphases(const Params&) { return 1; }
  static constexpr int bitrev(int s) { int r = 0; for (int k = 0; k < K_; k++) r |= ((s >> k) & 1) << (K_ - 1 - k); return r; }
  // one decimation-in-frequency stage over blocks of 2 LEN: (x, y) -> (x + y, (x - y) w^(-j a / (2 LEN)))
  template <int LEN> static MS_DEV void stage(X (&v)[A], const Params& p) {
#pragma unroll
    for (int i = 0; i < A; i += 2 * LEN) {
#pragma unroll
      for (int j = 0; j < LEN; j++) {
        const X x = v[i + j], y = v[i + j + LEN];
        v[i + j] = e_add<F, E>(x, y);
        X d = e_sub<F, E>(x, y);
        constexpr int STEP = A / (2 * LEN);
        if (j * STEP != 0) {
#pragma unroll
          for (int l = 0; l < E; l++) d.c[l] = F::mul_tw(d.c[l], p.wt[(j * STEP) & 3]);
        }
        v[i + j + LEN] = d;
      }
    }
  }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t b = (size_t)bx * nthreads + tid;
    if (b >= p.m_out) return;
    X v[A];
#pragma unroll
    for (int t = 0; t < A; t++) {
#pragma unroll
      for (int l = 0; l < E; l++) v[t].c[l] = p.src[(size_t)l * p.src_limb_stride + (size_t)t * p.m_out + b];
    }
    if constexpr (K_ >= 3) stage<4>(v, p);
    if constexpr (K_ >= 2) stage<2>(v, p);
    stage<1>(v, p);
    const size_t Dm = ((size_t)1 << p.log_D) - 1;
    const T xinv = w_tab(p, (Dm + 1 - b) & Dm);                        // table form of x^-1 = w_D^(D - b)
    X y;                                                                // alpha / x
#pragma unroll
    for (int l = 0; l < E; l++) y.c[l] = F::mul_tw(p.alpha.c[l], xinv);
    X r = v[bitrev(A - 1)];
#pragma unroll
    for (int s = A - 2; s >= 0; s--) r = e_add<F, E>(e_mul<F>(r, y), v[bitrev(s)]);
#pragma unroll
    for (int l = 0; l < E; l++) p.dst[(size_t)l * p.dst_limb_stride + b] = F::mul_tw(r.c[l], p.inv_a);
  }
  static MS_DEV T w_tab(const Params& p, size_t e) {
    T tw = p.tw_lo[e & (((size_t)1 << p.lo_bits) - 1)];
    const size_t eh = e >> p.lo_bits;
    if (eh) tw = F::mul_tw(tw, p.tw_hi[eh]);
    return tw;
  }
};

// The THROUGHPUT form of the fold (launches above MS_FOLD_SMALL_MAX outputs): eight outputs per thread like FriFoldEvalKernel<F, E, 8> before it, same values, fewer
// multiplications per output (Goldilocks: ~28 -> ~19 general-product equivalents, ~16 in the first fold):
//  * ONE field inversion per workgroup instead of one per thread (a wave executes the 73-product chain whether one lane needs it or all): every thread leaves the
//    product of its norms in LDS, the lanes of wave 0 combine the NW products of their column with Montgomery's trick, run one chain and unwind it, and every thread
//    reads 1 / (2 x its product) back behind a barrier.  A thread with no output in range contributes 1; every thread reaches both barriers (cooperative style,
//    like SuffixHornerKernel: per-thread state lives across the barriers, the emulation build runs it on fibers).
//  * SRC_LIMBS = 1: the source codeword is a base-field one (round 0: the transform of the validity polynomial, limbs >= 1 are zero and not even loaded), so
//    f(x) +- f(-x) are base elements and (alpha / x) d is E products instead of a tower product.
//  * what depends on z alone (nr z1^2; BabyBear: zb, K = (u - 11) zb^2) is computed once per thread, not per output.
//  * OCT (Goldilocks, replicated rounds with m_out >= 8): a thread's eight outputs lie m_out / 8 = D / 16 apart, so their points differ by powers of w_16, and in
//    Goldilocks every 16th root of unity is +-2^(12 k) (2 has order 192).  x0^-1, y0 = x0^2 and u0 = alpha / x0 come from the tables once per thread; output k takes
//    the point x = s_k x0 2^(12 k): (alpha / x) d = u0 (+-d 2^(96 - 12 k)) with the sign as a swap of f(x) and f(-x), y = y0 2^(24 k) (2^96 = -1) - shifts with the
//    special-form reduction (GL::mul_pow2) instead of four general products.  WHICH of the eight positions i0 + q m_out / 8 has the point x0 2^(12 k), and with which
//    sign, depends on the root of the plan: w_D^(D / 16) = 2^(12 m) for some odd m, found by the host at launch (oct_q[k], oct_neg; nothing assumes the generator).
// Layouts: OCT as above (lanes still read and write consecutive elements); otherwise FriFoldEvalKernel's (output j0 + it x THREADS; sharded rounds, BabyBear, m_out < 8).
template <class F, int E, int SRC_LIMBS_ = E, bool OCT_ = false> struct FriFoldWgKernel {
  typedef typename F::T T;
  typedef Ext<F, E> X;
  typedef FriFoldEvalKernel<F, E, 1> Lat;
  static_assert(E == 2 || E == 4, "quadratic or quartic tower");
  static_assert(SRC_LIMBS_ == 1 || SRC_LIMBS_ == E, "base-field or full source");
  static_assert(!OCT_ || F::ID == 0, "the octet layout needs Goldilocks' roots of unity");
  static constexpr int THREADS = mspoly::THREADS, ITEMS = 8, NW = THREADS / 64, SRC_LIMBS = SRC_LIMBS_;
  static constexpr bool OCT = OCT_;
  struct Params {
    typename Lat::Params f;
    u32 oct_q[8];    // OCT: item k works on output i0 + oct_q[k] * m_out / 8 ...
    u32 oct_neg;     // ... and bit k says that its d = f(x) - f(-x) enters negated
  };
  static MS_HD size_t lds_bytes() { return (size_t)THREADS * sizeof(T); }
  static MS_HD size_t grid_items(const Params& p) { return OCT ? p.f.m_out / 8 : (p.f.m_out * p.f.groups + ITEMS - 1) / ITEMS; }   // threads the launch needs
  struct ZPre { T nz; Ext<F, 2> zb, K; };   // functions of z alone
  static MS_DEV ZPre z_pre(const X& z) {
    ZPre zp;
    const T nr = F::from_u64(F::NR2);
    zp.nz = 0; zp.zb = e_zero<F, 2>(); zp.K = e_zero<F, 2>();
    if constexpr (E == 2) zp.nz = F::mul(nr, F::mul(z.c[1], z.c[1]));
    else { zp.zb.c[0] = z.c[2]; zp.zb.c[1] = z.c[3]; zp.K = e_mul_nr4<F>(e_mul<F>(zp.zb, zp.zb)); }
    return zp;
  }
  // conjugate product C and base-field norm n of (y - z), yd = y - z0 (FriFoldEvalKernel::inv_parts with the z-only parts taken out)
  static MS_DEV void inv_parts(const X& z, const ZPre& zp, T yd, X* C, T* n) {
    if constexpr (E == 2) {
      C->c[0] = yd; C->c[1] = z.c[1];
      *n = F::sub(F::mul(yd, yd), zp.nz);
    } else {
      const T nr = F::from_u64(F::NR2);
      Ext<F, 2> A;
      A.c[0] = yd; A.c[1] = F::neg(z.c[1]);
      const Ext<F, 2> M = e_sub<F, 2>(e_mul<F>(A, A), zp.K);
      Ext<F, 2> Mc; Mc.c[0] = M.c[0]; Mc.c[1] = F::neg(M.c[1]);
      *n = F::sub(F::mul(M.c[0], M.c[0]), F::mul(nr, F::mul(M.c[1], M.c[1])));
      const Ext<F, 2> c0 = e_mul<F>(A, Mc), c1 = e_mul<F>(zp.zb, Mc);
      C->c[0] = c0.c[0]; C->c[1] = c0.c[1]; C->c[2] = c1.c[0]; C->c[3] = c1.c[1];
    }
  }
  // one output: a = f(x) at ia, b = f(-x) at ib, u = alpha / x up to the factor 2^S that d takes instead, y = x^2.  *tt = 2 (folded - c) C, *nrm = the norm
  template <int S> static MS_DEV void item(const typename Lat::Params& p, const ZPre& zp, size_t ia, size_t ib, const X& u, T y, X* tt, T* nrm) {
    T a[SRC_LIMBS], b[SRC_LIMBS];
#pragma unroll
    for (int l = 0; l < SRC_LIMBS; l++) { a[l] = p.src[(size_t)l * p.src_limb_stride + ia]; b[l] = p.src[(size_t)l * p.src_limb_stride + ib]; }
    X num;
    if constexpr (SRC_LIMBS == E) {
      X s, d;
#pragma unroll
      for (int l = 0; l < E; l++) {
        s.c[l] = F::add(a[l], b[l]); d.c[l] = F::sub(a[l], b[l]);
        if constexpr (S != 0) d.c[l] = F::template mul_pow2<S>(d.c[l]);
      }
      num = e_sub<F, E>(e_add<F, E>(s, e_mul<F>(u, d)), p.c2);
    } else {
      const T s0 = F::add(a[0], b[0]);
      T d0 = F::sub(a[0], b[0]);
      if constexpr (S != 0) d0 = F::template mul_pow2<S>(d0);
      num.c[0] = F::sub(F::add(s0, F::mul(u.c[0], d0)), p.c2.c[0]);
#pragma unroll
      for (int l = 1; l < E; l++) num.c[l] = F::sub(F::mul(u.c[l], d0), p.c2.c[l]);
    }
    X C;
    inv_parts(p.z, zp, F::sub(y, p.z.c[0]), &C, nrm);
    *tt = e_mul<F>(num, C);
  }
  // OCT: items K .. 7 of the thread whose first position is i0 (Q = m_out / 8); compile-time K for the shifts
  template <int K> static MS_DEV void oct_items(const Params& pp, const ZPre& zp, bool act, size_t i0, size_t Q, const X& u0, T y0, X* tt, T* nrm, T* pre, T* prod) {
    if constexpr (K < ITEMS) {
      tt[K] = e_zero<F, E>(); nrm[K] = F::from_u64(1);
      if (act) {
        const size_t i = i0 + (size_t)pp.oct_q[K] * Q;
        const bool ng = (pp.oct_neg >> K) & 1u;
        T y = F::template mul_pow2<24 * (K & 3)>(y0);
        if constexpr (K >= 4) y = F::neg(y);
        item<(K ? 96 - 12 * K : 0)>(pp.f, zp, ng ? i + pp.f.m_out : i, ng ? i : i + pp.f.m_out, u0, y, &tt[K], &nrm[K]);
      }
      pre[K] = *prod;
      *prod = F::mul(*prod, nrm[K]);
      oct_items<K + 1>(pp, zp, act, i0, Q, u0, y0, tt, nrm, pre, prod);
    }
  }
  static MS_DEV void run(const Params& pp, int bx, int, int, int tid, unsigned char* lds) {
    const typename Lat::Params& p = pp.f;
    const size_t total = p.m_out * p.groups, Dm = ((size_t)1 << p.log_D) - 1;
    const ZPre zp = z_pre(p.z);
    X tt[ITEMS]; T nrm[ITEMS], pre[ITEMS];
    T prod = F::from_u64(1);
    const size_t Q = p.m_out / 8;
    size_t j0;
    if constexpr (OCT) {
      j0 = (size_t)bx * THREADS + tid;
      const bool act = j0 < Q;
      X u0 = e_zero<F, E>(); T y0 = 0;
      if (act) {
        const T xinv = Lat::w_tab(p, (Dm + 1 - j0) & Dm);                // table form of x0^-1 = w_D^(D - i0)
#pragma unroll
        for (int l = 0; l < E; l++) u0.c[l] = F::mul_tw(p.alpha.c[l], xinv);
        y0 = F::from_tw(Lat::w_tab(p, (2 * j0) & Dm));
      }
      oct_items<0>(pp, zp, act, j0, Q, u0, y0, tt, nrm, pre, &prod);
    } else {
      j0 = (size_t)bx * ((size_t)THREADS * ITEMS) + tid;
#pragma unroll
      for (int it = 0; it < ITEMS; it++) {
        const size_t j = j0 + (size_t)it * THREADS;
        tt[it] = e_zero<F, E>(); nrm[it] = F::from_u64(1);
        if (j < total) {
          const size_t t = j >> p.log_m, i = j & (p.m_out - 1);
          const size_t ia = t * 2 * p.m_out + i;
          const size_t r = p.shard_W ? 2 * ((size_t)p.shard_k + (size_t)p.shard_W * i) + t : i;
          const T xinv = Lat::w_tab(p, (Dm + 1 - r) & Dm);               // table form of x^-1 = w_D^(D - r)
          X u;                                                            // alpha / x
#pragma unroll
          for (int l = 0; l < E; l++) u.c[l] = F::mul_tw(p.alpha.c[l], xinv);
          item<0>(p, zp, ia, ia + p.m_out, u, F::from_tw(Lat::w_tab(p, (2 * r) & Dm)), &tt[it], &nrm[it]);
        }
        pre[it] = prod;                // product of the norms before this one
        prod = F::mul(prod, nrm[it]);
      }
    }
    // ---- 1 / (2 x product of this thread's norms) for every thread of the workgroup from ONE inversion per lane of wave 0
    T* sp = reinterpret_cast<T*>(lds);
    sp[tid] = prod;
    msrt::wg_barrier();
    // Wave 0 inverts for the workgroup (lane l: the products of threads l, l + 64, ...); the other waves wait at the barrier and other workgroups of the CU issue meanwhile.
    if (tid < 64) {
      const int ln = tid;
      T a[NW], ap[NW];
      T acc = F::from_u64(1);
#pragma unroll
      for (int w = 0; w < NW; w++) { a[w] = sp[ln + 64 * w]; ap[w] = acc; acc = w ? F::mul(acc, a[w]) : a[w]; }
      T iv = F::mul(fold_base_inv<F>(acc), p.inv2);
#pragma unroll
      for (int w = NW - 1; w >= 0; w--) { sp[ln + 64 * w] = w ? F::mul(iv, ap[w]) : iv; if (w) iv = F::mul(iv, a[w]); }
    }
    msrt::wg_barrier();
    T inv = sp[tid];
#pragma unroll
    for (int it = ITEMS - 1; it >= 0; it--) {
      size_t j; bool in;
      if constexpr (OCT) { in = j0 < Q; j = j0 + (size_t)pp.oct_q[it] * Q; }
      else { j = j0 + (size_t)it * THREADS; in = j < total; }
      const T ni = F::mul(inv, pre[it]);             // 1 / (2 norm_it)
      inv = F::mul(inv, nrm[it]);
      if (in) {
#pragma unroll
        for (int l = 0; l < E; l++) p.dst[(size_t)l * p.dst_limb_stride + j] = F::mul(tt[it].c[l], ni);
      }
    }
  }
};

// ---------------------------------------------------------------- Degree / FindFirst
// result = max(j+1) over nonzero elements (0 for the zero polynomial); caller zeroes result.
// Elements are visited from the top: the first workgroups to run see the leading coefficient, publish the
// answer, and every later workgroup leaves after one read of `result` (no loads, no atomics).
template <class F, int E> struct DegreeKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  // idx0: index of src[0] in the whole vector (a rank's part of a distributed polynomial reports GLOBAL lengths, which the ranks then max-reduce)
  struct Params { const T* src; size_t limb_stride, n; unsigned long long* result; size_t idx0; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t r = (size_t)bx * nthreads + tid;
    if (r >= p.n) return;
    const size_t j = p.n - 1 - r;
    if ((unsigned long long)(p.idx0 + j + 1) <= *reinterpret_cast<volatile unsigned long long*>(p.result)) return;
    bool nz = false, nz_next = false;
    for (int l = 0; l < E; l++) nz = nz || (p.src[(size_t)l * p.limb_stride + j] != 0);
    // only the top of a run of non-zero elements can be the answer: one atomic for a dense polynomial, not one per element
    if (nz && j + 1 < p.n) for (int l = 0; l < E; l++) nz_next = nz_next || (p.src[(size_t)l * p.limb_stride + j + 1] != 0);
    if (nz && !nz_next) msrt::atomic_max_u64(p.result, (unsigned long long)(p.idx0 + j + 1));
  }
};
// per window: result[t] = min index j with leaf_j == target_t (caller fills result with ~0).
// Jobs batched over blockIdx.y (device table) or one inline job.
// Sharded codewords (ms_set_shard): the local element j = t*map_m + i is global element map_g*(map_k + map_W*i) + t and the
// result is the minimum GLOBAL index (map_g = 0: identity).
template <class F, int E> struct FindJob {
  const typename F::T* src; size_t limb_stride, n;
  const typename F::T* targets /* [nt][E] */; int nt; unsigned long long* result;
  u32 map_g, map_W, map_k; size_t map_m;
};
template <class F, int E> struct FindFirstKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const FindJob<F, E>* jobs; FindJob<F, E> inline_job; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& pp, int bx, int by, int tid, int nthreads, unsigned char*) {
    const FindJob<F, E>& p = pp.jobs ? pp.jobs[by] : pp.inline_job;
    const size_t j = (size_t)bx * nthreads + tid;
    if (j >= p.n) return;
    T v[E];
    for (int l = 0; l < E; l++) v[l] = p.src[(size_t)l * p.limb_stride + j];
    for (int t = 0; t < p.nt; t++) {
      bool eq = true;
      for (int l = 0; l < E; l++) eq = eq && (v[l] == p.targets[(size_t)t * E + l]);
      if (eq) {
        unsigned long long gj = (unsigned long long)j;
        if (p.map_g) { const size_t tt = j / p.map_m, ii = j - tt * p.map_m; gj = (unsigned long long)p.map_g * (p.map_k + (unsigned long long)p.map_W * ii) + tt; }
        msrt::atomic_min_u64(p.result + t, gj);
      }
    }
  }
};

// ---------------------------------------------------------------- query points
// One thread per (window i, query j) (fri.rs:148-154).  h0[(i*nq + j)*2 + s] holds even(x3) (s=0) /
// odd(x3) (s=1) of round i's polynomial at x3 = x1^2 — the H_0 outputs of the suffix Horner runs;
// window W (the last round) is only evaluated.  y1 = Ee + x1*Eo, y2 = Ee - x1*Eo and
// y3 = p_{i+1}(x3) = Ee' + x1'*Eo' with x1' = x3 (the next window's y1).
// Writes x1 y1 x2 y2 x3 y3 | qlen into the proof blob and (y1, y2) to the find-first targets.
template <class F, int E> struct QueryPointsKernel {
  typedef typename F::T T;
  static constexpr int THREADS = 64;
  struct Params {
    const T* h0;            // [(W+1)*nq*2][E]
    const T* x1;            // [(W+1)*nq] base elements
    const u64* qlen;        // [W]
    int W, nq;
    unsigned char* blob; const size_t* rec_off;  // [W*nq] byte offset of the record
    T* targets;             // [W][2*nq][E]
  };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const int t = bx * nthreads + tid;
    if (t >= p.W * p.nq) return;
    const int i = t / p.nq, j = t - i * p.nq;
    Ext<F, E> ee, eo, ne, no;
    for (int l = 0; l < E; l++) {
      ee.c[l] = p.h0[((size_t)t * 2) * E + l]; eo.c[l] = p.h0[((size_t)t * 2 + 1) * E + l];
      ne.c[l] = p.h0[((size_t)(t + p.nq) * 2) * E + l]; no.c[l] = p.h0[((size_t)(t + p.nq) * 2 + 1) * E + l];
    }
    const T x1 = p.x1[t], x3 = p.x1[t + p.nq];
    Ext<F, E> d = e_mul_base<F, E>(eo, x1);
    Ext<F, E> y1 = e_add<F, E>(ee, d), y2 = e_sub<F, E>(ee, d);
    Ext<F, E> y3 = e_add<F, E>(ne, e_mul_base<F, E>(no, x3));
    u64* o = reinterpret_cast<u64*>(p.blob + p.rec_off[t]);
    Ext<F, E> X1 = e_from_base<F, E>(x1), X2 = e_from_base<F, E>(F::neg(x1)), X3 = e_from_base<F, E>(x3);
    for (int l = 0; l < E; l++) o[l] = F::to_u64(X1.c[l]);
    for (int l = 0; l < E; l++) o[E + l] = F::to_u64(y1.c[l]);
    for (int l = 0; l < E; l++) o[2 * E + l] = F::to_u64(X2.c[l]);
    for (int l = 0; l < E; l++) o[3 * E + l] = F::to_u64(y2.c[l]);
    for (int l = 0; l < E; l++) o[4 * E + l] = F::to_u64(X3.c[l]);
    for (int l = 0; l < E; l++) o[5 * E + l] = F::to_u64(y3.c[l]);
    o[6 * E] = p.qlen[i];
    T* tg = p.targets + ((size_t)i * 2 * p.nq + 2 * j) * E;
    for (int l = 0; l < E; l++) { tg[l] = y1.c[l]; tg[E + l] = y2.c[l]; }
  }
};


// ---------------------------------------------------------------- one proof over several ranks: coefficient-domain work by coefficient range
// ("fold/split/lincomb shard by coefficient index; the scan needs a carry all-gather; the evaluations an e-limb sum of partial dot products").
// Rank r of W holds the coefficients [r*S, (r+1)*S) of a polynomial.  A sum over all coefficients is the Horner combination of the ranks' partial sums in z^S;
// a suffix sum (SuffixHorner) takes the sum over the higher ranks as carry-in.  All ranks see the same all-gathered partials and compute the same field
// elements: the results are bit-identical to the unsharded kernels' (exact arithmetic), which the gloo tests check against the oracle at world 2 / 4 / 8.
//
// ShardCombine: out[i] = sum_r gathered[r][i] * zstep^r for n extension elements (a rank's payload = n*E limbs, rank_stride limbs apart)
template <class F, int E> struct ShardCombineKernel {
  typedef typename F::T T;
  static constexpr int THREADS = 64;
  struct Params { const T* gathered; size_t rank_stride; u32 n, W; Ext<F, E> zstep; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const u32 i = (u32)bx * (u32)nthreads + (u32)tid;
    if (i >= p.n) return;
    Ext<F, E> acc = e_zero<F, E>();
    for (int r = (int)p.W - 1; r >= 0; r--) {
      Ext<F, E> v; for (int l = 0; l < E; l++) v.c[l] = p.gathered[(size_t)r * p.rank_stride + (size_t)i * E + l];
      acc = e_add<F, E>(e_mul<F>(acc, p.zstep), v);
    }
    for (int l = 0; l < E; l++) p.out[(size_t)i * E + l] = acc.c[l];
  }
};
// ShardCarry: the suffix sums at the rank boundaries from the all-gathered per-rank aggregates.  With T_W = 0,
//     T_r = F_r + zA * (A_r + zB * T_(r+1))          A_r: rank r's aggregate (E limbs at agg_off of its payload), F_r: an optional leading element (first_off)
// For this rank k the job stores  carry_out = T_(k+1) * scale  (the top-level carry-in of its SuffixHorner job: that kernel places a top-level carry at the padded
// position BS^levels, so scale = z^(m - BS^levels) moves it to the job's true end m),  tail_out = T_(k+1) itself, and h0_out = T_0 (the sum over everything).
//   DEEP quotient of a FRI round (fold_commit): the job runs over the rank's folded elements f[1..cnt), F_r = f[0], zA = z, zB = z^(S-1);
//   query quotients: the job runs over the rank's whole half-range, no F, zA = 1, zB = x3^(S/2).
template <class F, int E> struct CarryJob {
  typedef typename F::T T;
  u32 first_off, agg_off, has_first, pad_;
  Ext<F, E> zA, zB, scale;
  T* carry_out; T* tail_out; size_t tail_stride; T* h0_out;
};
template <class F, int E> struct ShardCarryKernel {
  typedef typename F::T T;
  typedef CarryJob<F, E> Job;
  static constexpr int THREADS = 64;
  struct Params { const Job* jobs; Job inline_job; u32 njobs, W, rank; const T* gathered; size_t rank_stride; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const u32 q = (u32)bx * (u32)nthreads + (u32)tid;
    if (q >= p.njobs) return;
    const Job& jb = p.jobs ? p.jobs[q] : p.inline_job;
    Ext<F, E> t = e_zero<F, E>();
    for (int r = (int)p.W - 1; r >= 0; r--) {
      if ((u32)r == p.rank) {   // t = T_(rank+1)
        if (jb.carry_out) { const Ext<F, E> c = e_mul<F>(t, jb.scale); for (int l = 0; l < E; l++) jb.carry_out[l] = c.c[l]; }
        if (jb.tail_out) for (int l = 0; l < E; l++) jb.tail_out[(size_t)l * jb.tail_stride] = t.c[l];
        if (!jb.h0_out) return;
      }
      const T* pay = p.gathered + (size_t)r * p.rank_stride;
      Ext<F, E> a; for (int l = 0; l < E; l++) a.c[l] = pay[jb.agg_off + l];
      Ext<F, E> x = e_add<F, E>(a, e_mul<F>(jb.zB, t));
      if (jb.has_first) {
        Ext<F, E> f; for (int l = 0; l < E; l++) f.c[l] = pay[jb.first_off + l];
        t = e_add<F, E>(f, e_mul<F>(jb.zA, x));
      } else t = x;
    }
    if (jb.h0_out) for (int l = 0; l < E; l++) jb.h0_out[l] = t.c[l];
  }
};
// the all-gathered parts of a distributed polynomial (rank r: E limbs of S coefficients, rank_stride limbs apart) -> one replicated vector of `count` coefficients
template <class F, int E> struct GatherPolyKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  struct Params { const T* gathered; size_t rank_stride, S, count; T* dst; size_t dst_limb_stride; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t f = (size_t)bx * nthreads + tid;
    if (f >= p.count * E) return;
    const size_t l = f / p.count, g = f - l * p.count, r = g / p.S, i = g - r * p.S;
    p.dst[l * p.dst_limb_stride + g] = p.gathered[r * p.rank_stride + l * p.S + i];
  }
};

// ---------------------------------------------------------------- DEEP composition (ms_deep_compose)
// The gamma-weighted combinations of the committed columns, one per opened point, in ONE streaming pass:
//   A_t[k] = sum_{columns j that point t names} w_(j,t) * col_j[k]        w_(j,t) = the sum of gamma^n over the entries n of point t that name column j (host table)
// A thread owns 16 bytes of consecutive coefficients (VEC = 2 Goldilocks / 4 BabyBear elements).  It walks the column records - wave-uniform table reads: the record,
// then one weight of E limbs for every point in the record's mask - loads the column's coefficients ONCE, however many points name the column, and spends one
// base-by-extension multiply-add (e_mul_base) per coefficient and naming point.  The NP x VEC accumulators (NP = the number of points rounded up to a power of two)
// stay in registers; no LDS, no scratch, no atomics.  Four columns' loads are issued before the first of them is used.  Limb l of A_t goes to out[(t * E + l) * n ..).
// A vector access needs n to be a multiple of VEC (columns lie n apart): a shorter vector (n < VEC) takes the element-wise path.
struct DeepCol { unsigned long long off; u32 mask, wbase; };   // the column's coefficients at base + off | the points that name it | its first weight in the weight table (in elements of E limbs)
constexpr int DEEP_MAX_POINTS = 8, DEEP_MAX_ENTRIES = 8192;
template <class F, int E, int NP> struct DeepCombineKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int VEC = 16 / (int)sizeof(T), AHEAD = 4;
  typedef T V16 __attribute__((vector_size(16)));
  struct Params { const T* base; const DeepCol* cols; const T* w; u32 ncols, npts; size_t n; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int nthreads, unsigned char*) {
    const size_t j = ((size_t)bx * nthreads + tid) * VEC;
    if (j >= p.n) return;
    const bool whole = j + VEC <= p.n && (p.n % VEC) == 0;
    Ext<F, E> acc[NP][VEC];
#pragma unroll
    for (int t = 0; t < NP; t++)
#pragma unroll
      for (int i = 0; i < VEC; i++) acc[t][i] = e_zero<F, E>();
    for (u32 c0 = 0; c0 < p.ncols; c0 += AHEAD) {
      V16 v[AHEAD];
#pragma unroll
      for (int u = 0; u < AHEAD; u++) {
        if (c0 + u < p.ncols) {
          const T* src = p.base + p.cols[c0 + u].off + j;
          if (whole) v[u] = *reinterpret_cast<const V16*>(src);
          else
#pragma unroll
            for (int i = 0; i < VEC; i++) v[u][i] = (j + i < p.n) ? src[i] : (T)0;
        }
      }
#pragma unroll
      for (int u = 0; u < AHEAD; u++) {
        if (c0 + u < p.ncols) {
          const u32 mask = p.cols[c0 + u].mask;
          const T* w = p.w + (size_t)p.cols[c0 + u].wbase * E;
#pragma unroll
          for (int t = 0; t < NP; t++) {
            if (mask & (1u << t)) {
              Ext<F, E> wt;
#pragma unroll
              for (int l = 0; l < E; l++) wt.c[l] = w[l];
              w += E;
#pragma unroll
              for (int i = 0; i < VEC; i++) acc[t][i] = e_add<F, E>(acc[t][i], e_mul_base<F, E>(wt, v[u][i]));
            }
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NP; t++) {
      if ((u32)t < p.npts) {
#pragma unroll
        for (int l = 0; l < E; l++) {
          T* dst = p.out + ((size_t)t * E + l) * p.n + j;
          if (whole) {
            V16 o;
#pragma unroll
            for (int i = 0; i < VEC; i++) o[i] = acc[t][i].c[l];
            *reinterpret_cast<V16*>(dst) = o;
          } else
#pragma unroll
            for (int i = 0; i < VEC; i++) if (j + i < p.n) dst[i] = acc[t][i].c[l];
        }
      }
    }
  }
};
// D'_k = shift^k * sum_t Q_t[k] for k < n - 1, 0 at k = n - 1: the sum of the npts synthetic-division quotients (limb l of Q_t at q[(t * E + l) * n ..), written by the
// scans for k < n - 1 only) moved to the coset's own variable, D'(y) = D(shift y).  dst: limb l at dst[l * n ..).
template <class F, int E> struct DeepSumScaleKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 4;
  struct Params { const T* q; u32 npts; size_t n; T s, s_step /* s^THREADS */; T* dst; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    size_t k = (size_t)bx * (THREADS * ITEMS) + tid;
    if (k >= p.n) return;
    T pw = f_pow<F>(p.s, k);
    for (int it = 0; it < ITEMS && k < p.n; it++, k += THREADS) {
      for (int l = 0; l < E; l++) {
        T sum = 0;
        if (k + 1 < p.n) for (u32 t = 0; t < p.npts; t++) sum = F::add(sum, p.q[((size_t)t * E + l) * p.n + k]);
        p.dst[(size_t)l * p.n + k] = F::mul(sum, pw);
      }
      pw = F::mul(pw, p.s_step);
    }
  }
};

// ---------------------------------------------------------------- build-defined degree-3 composition (ms_mix_cubic)
// BASELINE configs[4] names "degree-3 constraints", which the reference cannot express (quirk Q1: its `validity` polynomial is the REMAINDER of the division by
// the vanishing polynomial, so any constraint polynomial with >= N coefficients panics).  The build-defined variant, with the TRUE quotient:
//   C_t(x)      = P_j(w x) - P_a(x) P_b(x) P_c(x) - s P_d(x)            transition constraint t = (j, a, b, c, d, s); w = the trace domain's generator
//   validity(x) = (sum_t r^t C_t(x)) (x - w^(N-1)) / (x^N - 1)           exact when every C_t vanishes on rows 0 .. N-2; 2N coefficients
// evaluated pointwise on the committed LDE domain x_i = shift g_L^i (column-major LDE, P(w x_i) = the value `blowup` rows further on); x^N - 1 takes only
// `blowup` distinct values there, whose inverses come in a table.  The caller interpolates (size-L INTT) and un-shifts.
template <class F> struct CubicSpec { u32 j, a, b, c, d; typename F::T s, rpow; };
template <class F> struct CubicComposeKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 8;
  struct Params { const T* lde; size_t L; u32 blowup, ncons; const CubicSpec<F>* spec; const T* den_inv; T shift, gL, gL_step /* gL^THREADS */, w_last /* w^(N-1) */; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    size_t i = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i >= p.L) return;
    T x = F::mul(p.shift, f_pow<F>(p.gL, i));
    for (int it = 0; it < ITEMS && i < p.L; it++, i += THREADS) {
      const size_t in = i + p.blowup < p.L ? i + p.blowup : i + p.blowup - p.L;   // w x_i = x_(i + blowup)
      T acc = 0;
      for (u32 t = 0; t < p.ncons; t++) {
        const CubicSpec<F> c = p.spec[t];
        T v = F::mul(F::mul(p.lde[(size_t)c.a * p.L + i], p.lde[(size_t)c.b * p.L + i]), p.lde[(size_t)c.c * p.L + i]);
        v = F::add(v, F::mul(c.s, p.lde[(size_t)c.d * p.L + i]));
        acc = F::add(acc, F::mul(c.rpow, F::sub(p.lde[(size_t)c.j * p.L + in], v)));
      }
      p.out[i] = F::mul(F::mul(acc, F::sub(x, p.w_last)), p.den_inv[i % p.blowup]);
      x = F::mul(x, p.gL_step);
    }
  }
};

// ---------------------------------------------------------------- build-defined composition of ANY degree (ms_mix_terms)
// The constraint system as a sum of monomials over the context's polynomials, factors at row offsets (include/ministark.h):
//   validity(x) = (sum_m c'_m prod_f P_poly_f(w^row_f x)) prod_{k=1..nexempt} (x - w^(N-k)) / (x^N - 1),   c'_m = r^t coef_m for a term of constraint t
// on the committed LDE domain, like CubicComposeKernel: P(w^row x_i) is the value row * blowup rows further on (mod L), x^N - 1 comes from the table of `blowup` inverses.
// The program is ONE device table, the same for every lane: terms (c', number of factors) in order, their factors (poly, row * blowup) in the same order.  A thread
// owns ITEMS strided points and walks the program ONCE for all of them - a term's coefficient and factor records are read once per ITEMS points, the ITEMS
// column loads of a factor are independent and in flight together - and stores only behind the walk: no store can precede a program read, the loop counters
// are uniform, so the program reads are scalar loads.  Column loads are coalesced along i; the index is masked by L - 1 (a power of two), so it is in
// bounds even for the points past L of a domain shorter than a workgroup's share, which are computed and dropped.  No LDS, no atomics, no cross-workgroup traffic.
template <class F> struct TermRec { typename F::T coef; u32 nfac; };
struct TermFac { u32 poly, rowoff; };
constexpr int TERMS_MAX_EXEMPT = 16, TERMS_MAX_FACTORS = 8;
template <class F> struct ComposeTermsKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 8;
  struct Params { const T* lde; size_t L; u32 blowup, nterms, nexempt; const TermRec<F>* terms; const TermFac* facs; const T* ex_roots /* w^(N-k), k = 1 .. nexempt */;
                  const T* den_inv; T shift, gL, gL_step /* gL^THREADS */; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    const size_t i0 = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i0 >= p.L) return;
    const size_t mask = p.L - 1;
    T acc[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; it++) acc[it] = 0;
    u32 f = 0;
    for (u32 m = 0; m < p.nterms; m++) {
      const TermRec<F> tr = p.terms[m];
      T v[ITEMS];
#pragma unroll
      for (int it = 0; it < ITEMS; it++) v[it] = tr.coef;
      for (u32 k = 0; k < tr.nfac; k++, f++) {
        const TermFac fc = p.facs[f];
        const T* col = p.lde + (size_t)fc.poly * p.L;
#pragma unroll
        for (int it = 0; it < ITEMS; it++) v[it] = F::mul(v[it], col[(i0 + (size_t)it * THREADS + fc.rowoff) & mask]);
      }
#pragma unroll
      for (int it = 0; it < ITEMS; it++) acc[it] = F::add(acc[it], v[it]);
    }
    T x[ITEMS];
    x[0] = F::mul(p.shift, f_pow<F>(p.gL, i0));
#pragma unroll
    for (int it = 1; it < ITEMS; it++) x[it] = F::mul(x[it - 1], p.gL_step);
    for (u32 k = 0; k < p.nexempt; k++) {
      const T root = p.ex_roots[k];
#pragma unroll
      for (int it = 0; it < ITEMS; it++) acc[it] = F::mul(acc[it], F::sub(x[it], root));
    }
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      const size_t i = i0 + (size_t)it * THREADS;
      if (i < p.L) p.out[i] = F::mul(acc[it], p.den_inv[i & (size_t)(p.blowup - 1)]);   // (blowup is a power of two: ms_lde_commit)
    }
  }
};

// ---------------------------------------------------------------- build-defined AIR composition (ms_mix_air)
// ms_mix_terms plus what makes the system an AIR (include/ministark.h): an exemption set per constraint, periodic columns, boundary constraints,
//   validity(x) = sum_t r^t C_t(x) Z_t(x) / (x^N - 1)  +  sum_b r^(ncons+b) (P_j(x) - v_b) / (x - w^rho_b),   Z_t(x) = prod_{rho in X_t} (x - w^rho)
// on the committed LDE domain.  The program is a sequence of GROUPS, each a ComposeTerms program of its own with a multiplier per point:
//   total_i += (sum_m c'_m prod_f factor_f(x_i)) * M_g(x_i)
// * transition group (kind 0): the constraints that share one exemption set (r^t folded into the coefficients by the host; field addition is exact, so the
//   grouping changes no bit).  M_g(x_i) = prod_k (x_i - root_k) * den_inv[i mod blowup], the `blowup` inverses of x^N - 1 as in ComposeTerms.
// * boundary group (kind 1): the boundary constraints at one row rho, as the terms r^(ncons+b) w^-rho P_j and one constant term - sum r^(ncons+b) w^-rho v_b.
//   1 / (x_i - w^rho) = w^-rho / (x_(i - rho blowup) - 1), so M_g(x_i) = D[(i + moff) mod L] with ONE table D[i] = 1 / (x_i - 1) over the domain (CosetInvKernel),
//   read like a column at the row offset moff = ((N - rho) mod N) blowup: no inversion per point, whatever the number of boundary rows.
// * a factor is a column of the LDE (kind 0: column src, index masked by L - 1) or a periodic column (kind 1): K_k(w^row x_i) takes only blowup q_k values
//   over the domain, tab_k[(i + row blowup) mod (blowup q_k)], in a table the host built (src = its offset in ptab, mask = blowup q_k - 1).
// Shape of ComposeTermsKernel: a thread owns ITEMS strided points and walks the program once for all of them; group, term and factor records are the same for every
// lane and the loop counters uniform, so program reads are scalar loads and the branches on the kind bits uniform; stores only behind the walk.  Every index is masked
// by a power of two minus one, so the points past L of a domain shorter than a workgroup's share stay in bounds; they are computed and dropped.  No LDS, no atomics.
struct AirGroup { u32 nterms, nroots, kind, moff; };
struct AirFac { u32 src, rowoff, mask, kind; };
constexpr int AIR_MAX_EXEMPT = 16, AIR_MAX_SETS = 32, AIR_MAX_BOUNDARY_ROWS = 16, AIR_MAX_PERIODIC = 64, AIR_MAX_PERIOD = 256, AIR_MAX_PERIOD_SUM = 4096;
template <class F> struct ComposeAirKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 8;
  struct Params { const T* lde; size_t L; u32 blowup, ngroups; const AirGroup* groups; const TermRec<F>* terms; const AirFac* facs; const T* roots /* w^rho, group by group */;
                  const T* ptab; const T* den_inv; const T* inv /* D, L entries; unused without boundary groups */; T shift, gL, gL_step /* gL^THREADS */; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    const size_t i0 = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i0 >= p.L) return;
    const size_t mask = p.L - 1;
    const T x0 = F::mul(p.shift, f_pow<F>(p.gL, i0));
    T total[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; it++) total[it] = 0;
    u32 m = 0, f = 0, rk = 0;
    for (u32 g = 0; g < p.ngroups; g++) {
      const AirGroup gr = p.groups[g];
      T acc[ITEMS];
#pragma unroll
      for (int it = 0; it < ITEMS; it++) acc[it] = 0;
      for (u32 mg = 0; mg < gr.nterms; mg++, m++) {
        const TermRec<F> tr = p.terms[m];
        T v[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; it++) v[it] = tr.coef;
        for (u32 k = 0; k < tr.nfac; k++, f++) {
          const AirFac fc = p.facs[f];
          const T* col = fc.kind ? p.ptab + fc.src : p.lde + (size_t)fc.src * p.L;
          T c[ITEMS];                                   // (loaded first, multiplied behind: written as one expression the 8 loads were issued one by one, each waited for)
#pragma unroll
          for (int it = 0; it < ITEMS; it++) c[it] = col[(i0 + (size_t)it * THREADS + fc.rowoff) & (size_t)fc.mask];
#pragma unroll
          for (int it = 0; it < ITEMS; it++) v[it] = F::mul(v[it], c[it]);
        }
#pragma unroll
        for (int it = 0; it < ITEMS; it++) acc[it] = F::add(acc[it], v[it]);
      }
      if (gr.nroots) {
        T x[ITEMS];
        x[0] = x0;
#pragma unroll
        for (int it = 1; it < ITEMS; it++) x[it] = F::mul(x[it - 1], p.gL_step);
        for (u32 k = 0; k < gr.nroots; k++, rk++) {
          const T root = p.roots[rk];
#pragma unroll
          for (int it = 0; it < ITEMS; it++) acc[it] = F::mul(acc[it], F::sub(x[it], root));
        }
      }
      const T* mt = gr.kind ? p.inv : p.den_inv;
      const size_t mm = gr.kind ? mask : (size_t)(p.blowup - 1);   // (blowup is a power of two: ms_lde_commit)
      T mv[ITEMS];
#pragma unroll
      for (int it = 0; it < ITEMS; it++) mv[it] = mt[(i0 + (size_t)it * THREADS + gr.moff) & mm];
#pragma unroll
      for (int it = 0; it < ITEMS; it++) total[it] = F::add(total[it], F::mul(acc[it], mv[it]));
    }
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      const size_t i = i0 + (size_t)it * THREADS;
      if (i < p.L) p.out[i] = total[it];
    }
  }
};

// ---------------------------------------------------------------- ms_mix_air with the combiner r in the extension K (ms_mix_air_ext)
// The same formula with the powers of r taken in K: the validity polynomial has coefficients in K, limb l of it is sum_t (r^t)_l * (quotient of constraint t).
// The constraint values stay in Fp - the column loads and factor products are those of ComposeAirKernel - so r^t is NOT folded into the term coefficients (E
// multiplications per term); the program gets one more level instead, group -> SEGMENT -> term -> factor:
// * a segment is one transition constraint, or one boundary constraint as the two terms w^-rho P_j and - w^-rho v_b; its value is accumulated in Fp and enters
//   the group's K accumulator as weight * value (E multiplications per segment and point), weight = r^t or r^(ncons+b);
// * the group multiplier M_g(x_i) of ComposeAirKernel is formed in Fp (den_inv or D, times the exemption roots) and applied once per group: E multiplications.
// Field arithmetic is exact: limb 0 for r = (r0, 0, ..) is ComposeAirKernel's output, element for element.  Output: E planes of L points, limb l at out + l L.
// Thread shape, masking and the store-behind-the-walk rule are ComposeAirKernel's; the accumulators are 2 ITEMS E words.
template <class F, int E> struct AirSeg { typename F::T w[E]; u32 nterms; };
struct AirGroupExt { u32 nsegs, nroots, kind, moff; };
template <class F, int E> struct ComposeAirExtKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 8;
  struct Params { const T* lde; size_t L; u32 blowup, ngroups; const AirGroupExt* groups; const AirSeg<F, E>* segs; const TermRec<F>* terms; const AirFac* facs;
                  const T* roots /* w^rho, group by group */; const T* ptab; const T* den_inv; const T* inv /* D, L entries; unused without boundary groups */;
                  T shift, gL, gL_step /* gL^THREADS */; T* out /* E planes of L */; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    const size_t i0 = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i0 >= p.L) return;
    const size_t mask = p.L - 1;
    const T x0 = F::mul(p.shift, f_pow<F>(p.gL, i0));
    T total[E][ITEMS];
#pragma unroll
    for (int l = 0; l < E; l++)
#pragma unroll
      for (int it = 0; it < ITEMS; it++) total[l][it] = 0;
    u32 s = 0, m = 0, f = 0, rk = 0;
    for (u32 g = 0; g < p.ngroups; g++) {
      const AirGroupExt gr = p.groups[g];
      T gacc[E][ITEMS];
#pragma unroll
      for (int l = 0; l < E; l++)
#pragma unroll
        for (int it = 0; it < ITEMS; it++) gacc[l][it] = 0;
      for (u32 sg = 0; sg < gr.nsegs; sg++, s++) {
        const AirSeg<F, E> seg = p.segs[s];
        T sv[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; it++) sv[it] = 0;
        for (u32 ms = 0; ms < seg.nterms; ms++, m++) {
          const TermRec<F> tr = p.terms[m];
          T v[ITEMS];
#pragma unroll
          for (int it = 0; it < ITEMS; it++) v[it] = tr.coef;
          for (u32 k = 0; k < tr.nfac; k++, f++) {
            const AirFac fc = p.facs[f];
            const T* col = fc.kind ? p.ptab + fc.src : p.lde + (size_t)fc.src * p.L;
            T c[ITEMS];                                 // (loaded first, multiplied behind, as in ComposeAirKernel)
#pragma unroll
            for (int it = 0; it < ITEMS; it++) c[it] = col[(i0 + (size_t)it * THREADS + fc.rowoff) & (size_t)fc.mask];
#pragma unroll
            for (int it = 0; it < ITEMS; it++) v[it] = F::mul(v[it], c[it]);
          }
#pragma unroll
          for (int it = 0; it < ITEMS; it++) sv[it] = F::add(sv[it], v[it]);
        }
#pragma unroll
        for (int l = 0; l < E; l++)
#pragma unroll
          for (int it = 0; it < ITEMS; it++) gacc[l][it] = F::add(gacc[l][it], F::mul(seg.w[l], sv[it]));
      }
      const T* mt = gr.kind ? p.inv : p.den_inv;
      const size_t mm = gr.kind ? mask : (size_t)(p.blowup - 1);   // (blowup is a power of two: ms_lde_commit)
      T mv[ITEMS];                                      // the group multiplier, in Fp
#pragma unroll
      for (int it = 0; it < ITEMS; it++) mv[it] = mt[(i0 + (size_t)it * THREADS + gr.moff) & mm];
      if (gr.nroots) {
        T x[ITEMS];
        x[0] = x0;
#pragma unroll
        for (int it = 1; it < ITEMS; it++) x[it] = F::mul(x[it - 1], p.gL_step);
        for (u32 k = 0; k < gr.nroots; k++, rk++) {
          const T root = p.roots[rk];
#pragma unroll
          for (int it = 0; it < ITEMS; it++) mv[it] = F::mul(mv[it], F::sub(x[it], root));
        }
      }
#pragma unroll
      for (int l = 0; l < E; l++)
#pragma unroll
        for (int it = 0; it < ITEMS; it++) total[l][it] = F::add(total[l][it], F::mul(gacc[l][it], mv[it]));
    }
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      const size_t i = i0 + (size_t)it * THREADS;
      if (i < p.L) {
#pragma unroll
        for (int l = 0; l < E; l++) p.out[(size_t)l * p.L + i] = total[l][it];
      }
    }
  }
};

// D[i] = 1 / (x_i - 1) over the LDE domain x_i = shift gL^i, for the boundary groups of ComposeAirKernel: a thread owns ITEMS strided points and inverts their
// product once (Montgomery's trick).  No x_i is 1: the stage has refused a coset that meets the trace domain, and the points past L of a short domain are
// points of the same coset again (computed, not stored).
template <class F> struct CosetInvKernel {
  typedef typename F::T T;
  static constexpr int THREADS = mspoly::THREADS;
  static constexpr int ITEMS = 8;
  struct Params { size_t L; T shift, gL, gL_step /* gL^THREADS */; T* out; };
  static MS_HD int nphases(const Params&) { return 1; }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    const size_t i0 = (size_t)bx * (THREADS * ITEMS) + tid;
    if (i0 >= p.L) return;
    T d[ITEMS], pre[ITEMS];
    T x = F::mul(p.shift, f_pow<F>(p.gL, i0)), run = F::from_u64(1);
#pragma unroll
    for (int it = 0; it < ITEMS; it++) { d[it] = F::sub(x, F::from_u64(1)); pre[it] = run; run = F::mul(run, d[it]); x = F::mul(x, p.gL_step); }
    T inv = fold_base_inv<F>(run);
#pragma unroll
    for (int it = ITEMS - 1; it >= 0; it--) {
      const size_t i = i0 + (size_t)it * THREADS;
      if (i < p.L) p.out[i] = F::mul(inv, pre[it]);
      inv = F::mul(inv, d[it]);
    }
  }
};

// a * 2^s for a run-time s < 96 through one of the compile-time shift forms: FORM 0 the chain of class A's fold_small / mul_x32 / mul_x64 (msntt::gl_mul_pow2<S, A>,
// the butterflies of the round-2 tiles), FORM 1 the round-1 form (msntt::gl_mul_pow2_v1), FORM 2 GL::mul_pow2 (one reduction whatever S: the FRI fold's octets)
template <int S, int FORM, class A> struct ArithShift {
  static MS_DEV u64 one(u64 x) {
    if constexpr (FORM == 0) return msntt::gl_mul_pow2<S, A>(x);
    else if constexpr (FORM == 1) return msntt::gl_mul_pow2_v1<S>(x);
    else return GL::mul_pow2<S>(x);
  }
  static MS_DEV u64 run(u64 x, int s) { return s == S ? one(x) : ArithShift<S - 1, FORM, A>::run(x, s); }
};
template <int FORM, class A> struct ArithShift<0, FORM, A> { static MS_DEV u64 run(u64 x, int) { return x; } };
// ms_arith_selftest: one operation of one arithmetic class per element.  A is the class of operations 0-7 and 12: GL (compare + select), GLT (sign bits through
// v_bitop3_b32) or GLM (inline asm with hand-managed gfx950 wait states, which only a run on the device can check) for Goldilocks, BB for BabyBear.  The operations
// that belong to no class (the round-1 shift form, the inversion chain, the table form of a run-time value, the extension arithmetic - all of it F's own) are
// compiled into the instance A = F only.  `op` is the operation without the class bits; the host (session.cpp) has refused what an instance does not hold.
// Ops: include/ministark.h.
template <class F, class A> struct ArithKernel {
  typedef typename F::T T;
  static constexpr int THREADS = 256;
  static constexpr int OP_EXT = 32;   // first extension operation: operands are elements of several consecutive limbs
  struct Params { const u64* a; const u64* b; u64* out; size_t n; int op; };
  static MS_HD int nphases(const Params&) { return 1; }
  template <int E> static MS_DEV Ext<F, E> load(const u64* v) { Ext<F, E> r; for (int k = 0; k < E; k++) r.c[k] = F::from_u64(v[k]); return r; }
  template <int E> static MS_DEV void store(u64* v, const Ext<F, E>& x) { for (int k = 0; k < E; k++) v[k] = F::to_u64(x.c[k]); }
  // operations 32-36 on elements of E limbs at limb offset o (o + E <= n: the host has refused an n that is no multiple of E)
  template <int E> static MS_DEV void ext_op(const Params& p, size_t o) {
    const Ext<F, E> a = load<E>(p.a + o), b = load<E>(p.b + o);
    Ext<F, E> r = a;
    if (p.op == 32) r = e_mul<F>(a, b);
    else if (p.op == 33) r = e_mul_tw<F>(a, e_to_tw<F, E>(b));
    else if (p.op == 34) r = e_add<F, E>(a, b);
    else if (p.op == 35) r = e_sub<F, E>(a, b);
    else if (p.op == 36) r = e_mul_base<F, E>(a, b.c[0]);
    store<E>(p.out + o, r);
  }
  static MS_DEV void phase(int, const Params& p, int bx, int, int tid, int, unsigned char*) {
    const size_t i = (size_t)bx * THREADS + tid;
    if constexpr (std::is_same<A, F>::value) {
      if (p.op >= OP_EXT) {
        if constexpr (F::ID == 1) {
          if (p.op >= 37) {   // an Fp4 operand read as two Fp2 values: thread i owns limbs 2 i, 2 i + 1
            if (2 * i + 2 > p.n) return;
            const Ext<F, 2> a = load<2>(p.a + 2 * i), b = load<2>(p.b + 2 * i);
            store<2>(p.out + 2 * i, p.op == 37 ? e_mul<F>(a, b) : e_mul_nr4<F>(a));
            return;
          }
        }
        if ((i + 1) * F::EXT > p.n) return;
        ext_op<F::EXT>(p, i * F::EXT);
        return;
      }
    }
    if (i >= p.n) return;
    if constexpr (F::ID == 0 && !std::is_same<A, GLM>::value) {
      if (p.op == 12) { p.out[i] = A::reduce128(p.a[i], p.b[i]); return; }   // raw words: lo = a, hi = b
    }
    const T a = F::from_u64(p.a[i]), b = F::from_u64(p.b[i]);
    T r = 0;
    if constexpr (std::is_same<A, F>::value) {
      if constexpr (F::ID == 0) {
        if (p.op == 13) r = ArithShift<95, 1, GL>::run(a, (int)(p.b[i] % 96));
        else if (p.op == 14) r = gl_inv_chain(a);
      } else {
        if (p.op == 14) r = f_inv<F>(a);
        else if (p.op == 15) { p.out[i] = (u64)F::mul_tw(a, F::tw_of(b)) | ((u64)F::from_tw(F::tw_of(a)) << 32); return; }
      }
    }
    if (p.op == 0) r = A::add(a, b);
    else if (p.op == 1) r = A::sub(a, b);
    else if (p.op == 2) r = A::mul(a, b);
    else if (p.op == 3) r = A::mul_tw(a, F::to_tw(b));
    if constexpr (F::ID == 0) {
      if constexpr (std::is_same<A, GL>::value) {   // compare + select has no fold_small / mul_x32 / mul_x64: its shift is GL::mul_pow2
        if (p.op == 6) r = ArithShift<95, 2, GL>::run(a, (int)(p.b[i] % 96));
      } else {
        if (p.op == 4) r = A::mul_x32(a);
        else if (p.op == 5) r = A::mul_x64(a);
        else if (p.op == 6) r = ArithShift<95, 0, A>::run(a, (int)(p.b[i] % 96));
        else if (p.op == 7) r = A::fold_small(a, (u32)p.b[i] & 0x7FFFFFFFu);
      }
      if (p.op == 8) r = GL::mul_2p24(a);
      else if (p.op == 9) r = GL::mul_2p48(a);
      else if (p.op == 10) r = GL::mul_2p72(a);
      else if (p.op == 11) {   // every shift of the fold's octets: a * 2^(12 (b mod 8))
        switch ((int)(p.b[i] & 7)) {
          case 0: r = a; break;
          case 1: r = GL::mul_pow2<12>(a); break;
          case 2: r = GL::mul_pow2<24>(a); break;
          case 3: r = GL::mul_pow2<36>(a); break;
          case 4: r = GL::mul_pow2<48>(a); break;
          case 5: r = GL::mul_pow2<60>(a); break;
          case 6: r = GL::mul_pow2<72>(a); break;
          default: r = GL::mul_pow2<84>(a); break;
        }
      }
    }
    p.out[i] = F::to_u64(r);
  }
};
}  // namespace mspoly
