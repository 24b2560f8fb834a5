//! Safe wrapper over `ffi`: one method per transcript-delimited stage of `Stark::prove` (src/starks.rs:59-169) and
//! `Fri::prove` (src/fri.rs:53-189).  `prove_gpu` in INTEGRATION.md §4 is written against this type; the Fiat–Shamir
//! transcript (nimue) stays on the Rust side of the boundary.
pub mod convert;
pub mod ffi;
// tree.rs, fri_proof.rs and prove.rs are CHILD modules of the reference's merkle.rs / fri.rs / starks.rs (they build types whose
// fields are private there); their headers say where each one goes.  This file and ffi.rs / convert.rs form `crate::gpu`.
use ffi::*;
use std::ffi::CStr;

#[derive(Debug)]
pub enum GpuError {
    Shape(String),        // -1: the conditions the reference assert!s / panics on (merkle.rs:93-104, air.rs:23, starks.rs:317-320)
    LeafNotFound,         // -2: MerkleProofError::LeafNotFound   (src/error.rs:13-21)
    OutOfRange,           // -3: MerkleProofError::OutOfRangeError
    Backend(i32, String), // state / argument / HIP / memory
}
pub type Digest = [u8; 32];

pub struct Gpu {
    ctx: *mut ms_ctx,
    pub ext: usize, // limbs per extension element: 2 (Goldilocks) / 4 (BabyBear)
}
unsafe impl Send for Gpu {} // one context per host thread (blocking calls, not thread-safe: SURVEY.md 8(b))

impl Gpu {
    pub fn new(device: i32, field: ms_field, flags: u32) -> Result<Self, GpuError> {
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe { ms_create(&mut ctx, device, field, flags) };
        if rc != 0 { return Err(GpuError::Backend(rc, "ms_create failed (no usable GPU / HIP runtime)".into())); }
        let ext = unsafe { ms_ext_degree(ctx) } as usize;
        Ok(Gpu { ctx, ext })
    }
    fn check(&self, rc: i32) -> Result<(), GpuError> {
        if rc == 0 { return Ok(()); }
        let msg = unsafe { CStr::from_ptr(ms_last_error(self.ctx)) }.to_string_lossy().into_owned();
        Err(match rc { -1 => GpuError::Shape(msg), -2 => GpuError::LeafNotFound, -3 => GpuError::OutOfRange, _ => GpuError::Backend(rc, msg) })
    }
    /// starks.rs:68-73: MerkleTree::new(trace.get_data(), lpn).root(); uploads the N x w row-major trace (canonical limbs)
    pub fn trace_commit(&mut self, trace: &[u64], n: usize, w: usize, lpn: usize) -> Result<Digest, GpuError> {
        assert_eq!(trace.len(), n * w);
        let mut root = [0u8; 32];
        self.check(unsafe { ms_trace_commit(self.ctx, trace.as_ptr(), n, w, lpn, root.as_mut_ptr()) })?;
        Ok(root)
    }
    /// Optional, for a pipelined prover: queues the upload of the NEXT proof's trace (page-locked memory from `ms_pinned_alloc`) on a copy engine while the
    /// current proof computes; the `trace_commit` that later passes the same slice finds it on the device.  A hint: `Ok(())` also when nothing was queued.
    /// SAFETY of the contract: `trace` must stay alive and unchanged until that `trace_commit` has returned.
    pub fn trace_upload_async(&mut self, trace: &[u64], n: usize, w: usize) -> Result<(), GpuError> {
        assert_eq!(trace.len(), n * w);
        self.check(unsafe { ms_trace_upload_async(self.ctx, trace.as_ptr(), n, w) })
    }
    /// air.rs:147-160: TraceTable::get_trace_polys (per-column INTT)
    /// build-defined (no reference counterpart): the running product / running sum column of a permutation or lookup argument, from the committed trace and
    /// challenges drawn after its root; between trace_commit and interpolate.  Returns `final` (ext limbs); Err(Shape) when a denominator vanished on some row.
    /// form 2k / 2k+1 = numerator / denominator of fraction k: form_begin has 2 * nfrac + 1 entries, term_coef and form_const hold ext limbs per element.
    pub fn aux_running(&mut self, op: u32, ext: u32, form_begin: &[u32], term_col: &[u32], term_coef: &[u64], form_const: &[u64]) -> Result<Vec<u64>, GpuError> {
        assert!(form_begin.len() >= 3 && form_begin.len() % 2 == 1);
        let nforms = form_begin.len() - 1;
        assert_eq!(term_col.len(), form_begin[nforms] as usize);
        assert_eq!(term_coef.len(), term_col.len() * ext as usize);
        assert_eq!(form_const.len(), nforms * ext as usize);
        let aux = MsAux { op, ext, nfrac: (nforms / 2) as u32, form_begin: form_begin.as_ptr(), term_col: term_col.as_ptr(), term_coef: term_coef.as_ptr(), form_const: form_const.as_ptr() };
        let mut fin = vec![0u64; ext as usize];
        self.check(unsafe { ms_aux_running(self.ctx, &aux, fin.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok(fin)
    }
    /// limb columns ms_aux_running has appended since the last trace_commit
    pub fn aux_count(&self) -> i32 { unsafe { ms_aux_count(self.ctx) } }
    pub fn interpolate(&mut self) -> Result<(), GpuError> { self.check(unsafe { ms_interpolate(self.ctx) }) }
    /// air.rs:127-144: a transition closure that is a linear combination of earlier polynomials (tests/e2e_goldilocks.rs:48-59)
    pub fn polys_lincomb(&mut self, scalars: &[u64], idx: &[i32]) -> Result<(), GpuError> {
        assert_eq!(scalars.len(), idx.len());
        self.check(unsafe { ms_polys_lincomb(self.ctx, scalars.as_ptr(), idx.as_ptr(), idx.len() as i32) })
    }
    /// ... or any closure's output, uploaded as coefficients (at most N of them: starks.rs:118-119 asserts)
    pub fn polys_append(&mut self, coeffs: &[u64]) -> Result<(), GpuError> { self.check(unsafe { ms_polys_append(self.ctx, coeffs.as_ptr(), coeffs.len()) }) }
    pub fn poly_read(&mut self, i: i32, n: usize) -> Result<Vec<u64>, GpuError> {
        let mut out = vec![0u64; n];
        self.check(unsafe { ms_poly_read(self.ctx, i, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// starks.rs:80-95: coset LDE of every constraint polynomial + MerkleTree::new over the L x c matrix
    pub fn lde_commit(&mut self, blowup: usize, shift: u64, lpn: usize) -> Result<Digest, GpuError> {
        let mut root = [0u8; 32];
        self.check(unsafe { ms_lde_commit(self.ctx, blowup, shift, lpn, root.as_mut_ptr()) })?;
        Ok(root)
    }
    /// starks.rs:108-119: validity = sum_i r^i f_i
    pub fn mix(&mut self, r: u64) -> Result<(), GpuError> { self.check(unsafe { ms_mix(self.ctx, r) }) }
    /// BUILD-DEFINED (no reference counterpart): polynomial constraints of any degree in place of `mix`, with the true quotient by x^N - 1.
    /// `constraints[t]` = the terms of constraint t, each `(coef, [(poly, row), ..])`: coef * prod P_poly(w^row x); the last `nexempt` rows are exempt.
    /// Returns the length of the validity polynomial (ms_validity_len: N * next_pow2(max(1, d - 1)) for nexempt <= d - 1).
    pub fn mix_terms(&mut self, r: u64, constraints: &[Vec<(u64, Vec<(u32, u32)>)>], nexempt: usize) -> Result<usize, GpuError> {
        let (mut term_begin, mut coef, mut fac_begin, mut fac_poly, mut fac_row) = (vec![0u32], Vec::new(), vec![0u32], Vec::new(), Vec::new());
        for terms in constraints {
            for (c, factors) in terms {
                coef.push(*c);
                for (poly, row) in factors {
                    fac_poly.push(*poly);
                    fac_row.push(*row);
                }
                fac_begin.push(fac_poly.len() as u32);
            }
            term_begin.push(coef.len() as u32);
        }
        // (an empty Vec's pointer is dangling but non-null, which is all the library asks of an array it reads nothing from)
        self.check(unsafe {
            ms_mix_terms(self.ctx, r, constraints.len() as i32, term_begin.as_ptr(), coef.as_ptr(), fac_begin.as_ptr(), fac_poly.as_ptr(), fac_row.as_ptr(), nexempt as i32)
        })?;
        Ok(unsafe { ms_validity_len(self.ctx) })
    }
    /// BUILD-DEFINED (no reference counterpart): the AIR composition of `ms_mix_air` with the combiner `r` drawn from the extension field (`self.ext` canonical
    /// limbs), so that the combination of the constraint quotients is |K|-sound, not |Fp|-sound.  `air` borrows its arrays for the call.  Returns the length of the
    /// validity polynomial in coefficients; each has `self.ext` limbs afterwards (`validity_ext`), and `eval_ext` / `fri_begin` work on that polynomial.
    pub fn mix_air_ext(&mut self, r: &[u64], air: &MsAir) -> Result<usize, GpuError> {
        assert_eq!(r.len(), self.ext);
        self.check(unsafe { ms_mix_air_ext(self.ctx, r.as_ptr(), air) })?;
        Ok(unsafe { ms_validity_len(self.ctx) })
    }
    /// limbs per coefficient of the validity polynomial: 0 none, 1 after `mix` / `mix_terms`, `self.ext` after `mix_air_ext`
    pub fn validity_ext(&self) -> i32 { unsafe { ms_validity_ext(self.ctx) } }
    /// starks.rs:124-151: out[t] = (f_0(z_t), .., f_{c-1}(z_t), validity(z_t)), E limbs each
    pub fn eval_ext(&mut self, z_limbs: &[u64], c: usize) -> Result<Vec<u64>, GpuError> {
        let q = z_limbs.len() / self.ext;
        let mut out = vec![0u64; q * (c + 1) * self.ext];
        self.check(unsafe { ms_eval_ext(self.ctx, z_limbs.as_ptr(), q as i32, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// BUILD-DEFINED: commits to the validity polynomial before z is drawn - the tree over its m = validity_ext * validity_len / N chunk columns on the LDE coset
    pub fn validity_commit(&mut self, lpn: usize) -> Result<Digest, GpuError> {
        let mut root = [0u8; 32];
        self.check(unsafe { ms_validity_commit(self.ctx, lpn, root.as_mut_ptr()) })?;
        Ok(root)
    }
    /// BUILD-DEFINED: the claimed evaluations F_{pt_poly[n]}(z_t) of the openings `deep`, `entries` of them, E limbs each, in entry order
    pub fn deep_evals(&mut self, deep: &MsDeep, entries: usize) -> Result<Vec<u64>, GpuError> {
        let mut out = vec![0u64; entries * self.ext];
        self.check(unsafe { ms_deep_evals(self.ctx, deep, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// BUILD-DEFINED: installs the DEEP polynomial of the openings `deep` under the challenge `gamma` (E limbs); `fri_begin` then starts round 0 from it.
    /// Returns its length in coefficients (N).
    pub fn deep_compose(&mut self, deep: &MsDeep, gamma: &[u64]) -> Result<usize, GpuError> {
        assert_eq!(gamma.len(), self.ext);
        self.check(unsafe { ms_deep_compose(self.ctx, deep, gamma.as_ptr()) })?;
        Ok(unsafe { ms_deep_len(self.ctx) } as usize)
    }
    /// fri.rs:73-82
    pub fn fri_begin(&mut self, blowup: usize, rounds: usize) -> Result<Digest, GpuError> {
        let mut root = [0u8; 32];
        self.check(unsafe { ms_fri_begin(self.ctx, blowup, rounds, root.as_mut_ptr()) })?;
        Ok(root)
    }
    /// fri.rs:89-94: z -> B = [even(z), odd(z)]
    pub fn fri_deep(&mut self, z_limbs: &[u64]) -> Result<Vec<u64>, GpuError> {
        let mut b = vec![0u64; 2 * self.ext];
        self.check(unsafe { ms_fri_deep(self.ctx, z_limbs.as_ptr(), b.as_mut_ptr()) })?;
        Ok(b)
    }
    /// fri.rs:96-109: alpha -> fold, DEEP quotient, next FriRound, its root
    pub fn fri_fold_commit(&mut self, alpha_limbs: &[u64]) -> Result<Digest, GpuError> {
        let mut root = [0u8; 32];
        self.check(unsafe { ms_fri_fold_commit(self.ctx, alpha_limbs.as_ptr(), root.as_mut_ptr()) })?;
        Ok(root)
    }
    /// fri.rs:115-189: the serialised FriProof (MSFP layout: include/ministark.h)
    pub fn fri_query(&mut self, betas: &[u64]) -> Result<Vec<u8>, GpuError> {
        self.check(unsafe { ms_fri_query(self.ctx, betas.as_ptr(), betas.len() as i32) })?;
        let mut blob = vec![0u8; unsafe { ms_fri_proof_size(self.ctx) }];
        self.check(unsafe { ms_fri_proof_read(self.ctx, blob.as_mut_ptr()) })?;
        Ok(blob)
    }
    /// Build-defined proof of work between `Fri::commit_phase` and `Fri::query_phase`: the smallest nonce in `[start, start + limit)` whose digest
    /// `D(seed || nonce.to_le_bytes())` starts with `bits` zero bits (`pow_ok` of include/ministark.h; D = the context's digest).  `Err(OutOfRange)` when the
    /// range holds none.  The caller draws `seed` from its transcript and absorbs the nonce's 8 bytes before it draws the query positions.
    pub fn grind(&mut self, seed: &[u8; 32], bits: u32, start: u64, limit: u64) -> Result<u64, GpuError> {
        let mut nonce = 0u64;
        self.check(unsafe { ms_grind(self.ctx, seed.as_ptr(), bits, start, limit, &mut nonce) })?;
        Ok(nonce)
    }
    /// `StarkConfig::num_queries` (starks.rs:312-332) with `grinding_bits` of the security taken by the proof of work: (constrain_queries, fri_queries)
    pub fn num_queries_grind(&self, field: ms_field, security_bits: u64, grinding_bits: u64, blowup: u64, steps: u64) -> Result<(u64, u64), GpuError> {
        let (mut cq, mut fq) = (0u64, 0u64);
        self.check(unsafe { ms_num_queries_grind(field, security_bits, grinding_bits, blowup, steps, &mut cq, &mut fq) })?;
        Ok((cq, fq))
    }
    /// merkle.rs:81-148 on its own (the `impl Tree` of INTEGRATION.md §5 calls this): all nodes, level-major, root last
    pub fn merkle_commit(&mut self, leaf_limbs: &[u64], leaf_num: usize, ext: i32, lpn: usize, ic: usize) -> Result<(Vec<u8>, Digest), GpuError> {
        let mut nn = 0usize;
        let mut root = [0u8; 32];
        let cap = 2 * (leaf_num / lpn) * 32;
        let mut nodes = vec![0u8; cap];
        self.check(unsafe { ms_merkle_commit(self.ctx, leaf_limbs.as_ptr(), leaf_num, ext, lpn, ic, nodes.as_mut_ptr(), cap, &mut nn, root.as_mut_ptr()) })?;
        nodes.truncate(nn * 32);
        Ok((nodes, root))
    }
}
impl Drop for Gpu {
    fn drop(&mut self) { unsafe { ms_destroy(self.ctx) } }
}
