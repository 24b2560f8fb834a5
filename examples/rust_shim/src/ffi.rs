//! `extern "C"` mirror of include/ministark.h, one declaration per exported symbol, in the header's order.
//! Status codes: 0 OK, -1 SHAPE (the reference's assert!/panic! sites), -2 LEAF_NOT_FOUND, -3 OUT_OF_RANGE (src/error.rs:13-21),
//! -4 STATE, -5 ARG, -6 HIP, -7 NOMEM.  Nothing unwinds across this boundary.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_long, c_void};

#[repr(C)]
pub struct ms_ctx {
    _private: [u8; 0],
}
pub type ms_field = c_int;
pub const MS_FIELD_GOLDILOCKS: ms_field = 0; // field.rs:36-56
pub const MS_FIELD_BABYBEAR: ms_field = 1; // field.rs:66-109
pub const MS_FLAG_ZERO_DISPLAY_EMPTY: u32 = 1; // ark-ff 0.5 prints Fp::ZERO as ""
pub const MS_FLAG_TRACE_MONT64: u32 = 2; // ms_trace_commit* reads arkworks memory (Montgomery form, R = 2^64)
pub const MS_FLAG_LATENCY: u32 = 4; // one proof alone on the GPU: independent chains of a stage on two streams, the calling thread spins for a stage's results
pub const MS_FLAG_DIGEST_BLAKE2S: u32 = 8; // D = Blake2s256: every commitment of the context hashes with BLAKE2s-256 instead of SHA-256
pub const MS_FLAG_DIGEST_BLAKE3: u32 = 0x10; // D = blake3::Hasher (the crate's `traits-preview` feature); excludes MS_FLAG_DIGEST_BLAKE2S (MS_ERR_ARG from ms_create)
pub const MS_FLAG_DIGEST_KECCAK256: u32 = 0x20; // D = sha3::Keccak256 (the original Keccak padding: Ethereum's hash); a context takes at most one MS_FLAG_DIGEST_* flag
pub const MS_FLAG_DIGEST_SHA3_256: u32 = 0x40; // D = sha3::Sha3_256 (FIPS 202)
pub const MS_FLAGS_DEFAULT: u32 = MS_FLAG_ZERO_DISPLAY_EMPTY;
pub const MS_DIGEST_SHA256: c_int = 0; // ms_digest_id
pub const MS_DIGEST_BLAKE2S256: c_int = 1;
pub const MS_DIGEST_BLAKE3: c_int = 2;
pub const MS_DIGEST_KECCAK256: c_int = 4; // (3 is unassigned)
pub const MS_DIGEST_SHA3_256: c_int = 5;
pub const MS_AIR_PERIODIC: u32 = 0x8000_0000; // fac_poly = MS_AIR_PERIODIC | k names periodic column k (ms_mix_air)
/// `ms_air` of include/ministark.h: the program of ms_mix_air.  Every pointer borrows from the caller for the duration of the call.
#[repr(C)]
pub struct MsAir {
    pub ncons: u32,
    pub term_begin: *const u32, // ncons + 1
    pub coef: *const u64,       // nterms
    pub fac_begin: *const u32,  // nterms + 1
    pub fac_poly: *const u32,   // nfacs: polynomial index, or MS_AIR_PERIODIC | k
    pub fac_row: *const u32,    // nfacs
    pub ex_begin: *const u32,   // ncons + 1
    pub ex_row: *const u32,     // may be null when ex_begin[ncons] == 0
    pub nperiodic: u32,
    pub per_begin: *const u32,  // nperiodic + 1
    pub per_val: *const u64,
    pub nbound: u32,
    pub bnd_poly: *const u32,
    pub bnd_row: *const u32,
    pub bnd_val: *const u64,
}
pub const MS_TREE_VALIDITY: c_int = 4; // ms_tree_open: the tree of ms_validity_commit (0 trace, 1 LDE, 2 FRI round; 3 is unassigned)
/// `ms_deep` of include/ministark.h: the openings of the DEEP stage.  Every pointer borrows from the caller for the duration of the call.
#[repr(C)]
pub struct MsDeep {
    pub npts: u32,              // 1..8 points
    pub z: *const u64,          // npts * E limbs: the verifier's z and its shifts z * w^row
    pub pt_begin: *const u32,   // npts + 1
    pub pt_poly: *const u32,    // entry n: j < c polynomial j of the LDE tree, c + j' chunk column j' of the validity tree
}
pub const MS_AUX_SUM: u32 = 0; // z_{i+1} = z_i + s_i, z_0 = 0 (LogUp)
pub const MS_AUX_PRODUCT: u32 = 1; // z_{i+1} = z_i * s_i, z_0 = 1 (grand product)
/// `ms_aux` of include/ministark.h: the program of ms_aux_running.  Every pointer borrows from the caller for the duration of the call.
#[repr(C)]
pub struct MsAux {
    pub op: u32,
    pub ext: u32,                // 1, or ms_ext_degree
    pub nfrac: u32,              // 1..4
    pub form_begin: *const u32,  // 2 * nfrac + 1
    pub term_col: *const u32,    // nterms: a trace column
    pub term_coef: *const u64,   // nterms * ext limbs
    pub form_const: *const u64,  // 2 * nfrac * ext limbs
}
pub type ms_exchange_fn = Option<unsafe extern "C" fn(user: *mut c_void, op: c_int, bytes: usize) -> c_int>;

extern "C" {
    // ---- context
    pub fn ms_create(out: *mut *mut ms_ctx, device: c_int, field: ms_field, flags: u32) -> c_int;
    pub fn ms_destroy(ctx: *mut ms_ctx);
    pub fn ms_last_error(ctx: *const ms_ctx) -> *const c_char;
    pub fn ms_ext_degree(ctx: *const ms_ctx) -> c_int;
    pub fn ms_digest(ctx: *const ms_ctx) -> c_int;
    pub fn ms_set_stream(ctx: *mut ms_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn ms_synchronize(ctx: *mut ms_ctx) -> c_int;
    pub fn ms_stream(ctx: *const ms_ctx) -> *mut c_void;
    pub fn ms_pinned_alloc(bytes: usize) -> *mut c_void;
    pub fn ms_pinned_free(p: *mut c_void);
    // ---- one proof over the GPUs of a node
    pub fn ms_set_shard(ctx: *mut ms_ctx, rank: c_int, world: c_int, d_send: *mut c_void, d_recv: *mut c_void, cap_bytes: usize,
                        f: ms_exchange_fn, user: *mut c_void) -> c_int;
    pub fn ms_shard_slice_layout(ctx: *mut ms_ctx, offset: *mut usize, stride: *mut usize) -> c_int;
    pub fn ms_rccl_unique_id(out: *mut u8 /* [128] */) -> c_int;
    pub fn ms_set_shard_rccl(ctx: *mut ms_ctx, rank: c_int, world: c_int, unique_id: *const u8 /* [128] */, cap_bytes: usize) -> c_int;
    pub fn ms_rccl_selftest(ctx: *mut ms_ctx) -> c_int;
    pub fn ms_shard_stats(ctx: *mut ms_ctx, out: *mut u64 /* [8] */) -> c_int;
    pub fn ms_shard_proof_on_root(ctx: *mut ms_ctx, on: c_int) -> c_int;
    pub fn ms_shard_proof_is_elsewhere(ctx: *const ms_ctx) -> c_int;
    pub fn ms_shard_round_is_distributed(ctx: *mut ms_ctx, round: c_int) -> c_int;
    // ---- src/util.rs:4-44, src/starks.rs:268-332
    pub fn ms_is_power_of_two(n: u64) -> c_int;
    pub fn ms_logarithm_of_two_k(n: u64, base: u64) -> c_long;
    pub fn ms_ceil_log2_k(n: u64, base: u64) -> u64;
    pub fn ms_num_queries(f: ms_field, security_bits: u64, blowup: u64, steps: u64, linking_queries: *mut u64, fri_queries_per_round: *mut u64) -> c_int;
    pub fn ms_num_queries_grind(f: ms_field, security_bits: u64, grinding_bits: u64, blowup: u64, steps: u64, constrain_queries: *mut u64, fri_queries: *mut u64) -> c_int;
    pub fn ms_root_of_unity(f: ms_field, n: u64) -> u64;
    // ---- Stark::prove stages (src/starks.rs:59-169)
    pub fn ms_trace_commit(ctx: *mut ms_ctx, trace_rowmajor: *const u64, n: usize, w: usize, lpn: usize, root: *mut u8 /* [32] */) -> c_int;
    pub fn ms_trace_commit_device(ctx: *mut ms_ctx, d_trace_rowmajor: *const c_void, n: usize, w: usize, lpn: usize, root: *mut u8) -> c_int;
    pub fn ms_trace_upload_async(ctx: *mut ms_ctx, trace_rowmajor: *const u64, n: usize, w: usize) -> c_int;
    pub fn ms_aux_running(ctx: *mut ms_ctx, aux: *const MsAux, final_out: *mut u64, column_out: *mut u64) -> c_int;
    pub fn ms_aux_count(ctx: *const ms_ctx) -> c_int;
    pub fn ms_aux_running_staged(ctx: *mut ms_ctx, aux: *const MsAux, final_out: *mut u64, column_out: *mut u64) -> c_int;
    pub fn ms_aux_staged_count(ctx: *const ms_ctx) -> c_int;
    pub fn ms_interpolate(ctx: *mut ms_ctx) -> c_int;
    pub fn ms_polys_lincomb(ctx: *mut ms_ctx, scalars: *const u64, idx: *const c_int, k: c_int) -> c_int;
    pub fn ms_polys_append(ctx: *mut ms_ctx, coeffs: *const u64, n: usize) -> c_int;
    pub fn ms_polys_count(ctx: *const ms_ctx) -> c_int;
    pub fn ms_poly_read(ctx: *mut ms_ctx, i: c_int, out: *mut u64) -> c_int;
    pub fn ms_lde_commit(ctx: *mut ms_ctx, blowup: usize, shift: u64, lpn: usize, root: *mut u8) -> c_int;
    pub fn ms_lde_commit_stage(ctx: *mut ms_ctx, lpn: usize, root: *mut u8) -> c_int;
    // coset-grouped row trees (build-defined): one leaf group per coset of the folded FRI's round 0
    pub fn ms_lde_commit_coset(ctx: *mut ms_ctx, blowup: usize, shift: u64, log_arity: c_int, root: *mut u8) -> c_int;
    pub fn ms_lde_commit_stage_coset(ctx: *mut ms_ctx, log_arity: c_int, root: *mut u8) -> c_int;
    pub fn ms_lde_read(ctx: *mut ms_ctx, out_rowmajor: *mut u64) -> c_int;
    pub fn ms_mix(ctx: *mut ms_ctx, r: u64) -> c_int;
    pub fn ms_validity_read(ctx: *mut ms_ctx, out: *mut u64) -> c_int;
    pub fn ms_mix_cubic(ctx: *mut ms_ctx, r: u64, spec: *const c_int, s: *const u64, ncons: c_int) -> c_int;
    pub fn ms_mix_terms(ctx: *mut ms_ctx, r: u64, ncons: c_int, term_begin: *const u32, coef: *const u64, fac_begin: *const u32, fac_poly: *const u32,
                        fac_row: *const u32, nexempt: c_int) -> c_int;
    pub fn ms_mix_air(ctx: *mut ms_ctx, r: u64, air: *const MsAir) -> c_int;
    pub fn ms_mix_air_ext(ctx: *mut ms_ctx, r: *const u64, air: *const MsAir) -> c_int;
    /// diagnostic: which constraints of `air` the trace violates and on which rows (every out-pointer but `nfail` may be null)
    pub fn ms_air_check(ctx: *mut ms_ctx, air: *const MsAir, nfail: *mut u64, cons_count: *mut u64, cons_first_row: *mut u64, bnd_got: *mut u64) -> c_int;
    pub fn ms_validity_ext(ctx: *const ms_ctx) -> c_int;
    pub fn ms_validity_len(ctx: *const ms_ctx) -> usize;
    pub fn ms_eval_ext(ctx: *mut ms_ctx, z: *const u64, q: c_int, out: *mut u64) -> c_int;
    // ---- Fri::prove stages (src/fri.rs:53-189)
    pub fn ms_fri_begin(ctx: *mut ms_ctx, blowup: usize, rounds: usize, root0: *mut u8) -> c_int;
    pub fn ms_fri_deep(ctx: *mut ms_ctx, z: *const u64, b: *mut u64) -> c_int;
    pub fn ms_fri_fold_commit(ctx: *mut ms_ctx, alpha: *const u64, root: *mut u8) -> c_int;
    pub fn ms_fri_round_info(ctx: *mut ms_ctx, round: c_int, ncoef: *mut u64, domain_size: *mut u64) -> c_int;
    pub fn ms_fri_round_poly_read(ctx: *mut ms_ctx, round: c_int, out: *mut u64) -> c_int;
    pub fn ms_fri_round_codeword_read(ctx: *mut ms_ctx, round: c_int, out: *mut u64) -> c_int;
    pub fn ms_fri_query(ctx: *mut ms_ctx, betas: *const u64, nq: c_int) -> c_int;
    pub fn ms_fri_query_into(ctx: *mut ms_ctx, betas: *const u64, nq: c_int, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn ms_fri_proof_size(ctx: *const ms_ctx) -> usize;
    pub fn ms_fri_proof_read(ctx: *mut ms_ctx, out: *mut u8) -> c_int;
    pub fn ms_fri_proof_read_async(ctx: *mut ms_ctx, out: *mut u8) -> c_int;
    pub fn ms_fri_proof_wait(ctx: *mut ms_ctx) -> c_int;
    pub fn ms_io_engine(ctx: *const ms_ctx) -> c_int;
    pub fn ms_io_runtime_path() -> *const c_char;
    // ---- Merkle openings by index (build-defined): tree 0 trace / 1 LDE / 2 FRI round `round`; MerklePaths of the leaf groups `index`, concatenated.  out = null, cap = 0: size query
    pub fn ms_tree_open(ctx: *mut ms_ctx, tree: c_int, round: c_int, index: *const u64, n: usize, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    // ---- the compact query phase (build-defined): the MSFI blob - openings by position, the last round's polynomial in the clear
    pub fn ms_fri_query_index(ctx: *mut ms_ctx, betas: *const u64, nq: c_int, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn ms_query_linked(ctx: *mut ms_ctx, betas: *const u64, nq: c_int, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    // ---- folded FRI (build-defined): arity 2^log_arity, one coset per leaf group; R committed rounds, the final fold's polynomial in the clear, the MSFF blob
    pub fn ms_fri_begin_folded(ctx: *mut ms_ctx, blowup: usize, log_arity: c_int, root0: *mut u8) -> c_int;
    pub fn ms_fri_fold_folded(ctx: *mut ms_ctx, alpha: *const u64, root: *mut u8) -> c_int;
    pub fn ms_fri_fold_final(ctx: *mut ms_ctx, alpha: *const u64, coeffs: *mut u64, cap: usize, n: *mut usize) -> c_int;
    pub fn ms_fri_query_folded(ctx: *mut ms_ctx, betas: *const u64, nq: c_int, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn ms_query_linked_folded(ctx: *mut ms_ctx, betas: *const u64, nq: c_int, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    // ---- the composition commitment and the DEEP stage (build-defined): the tree over the validity polynomial's chunk columns on the LDE coset; the claimed evaluations;
    // D' = sum_t (A_t - A_t(z_t)) / (x - z_t) on the coset's own variable, which ms_fri_begin then starts from
    pub fn ms_validity_commit(ctx: *mut ms_ctx, lpn: usize, root: *mut u8) -> c_int;
    pub fn ms_validity_commit_coset(ctx: *mut ms_ctx, log_arity: c_int, root: *mut u8) -> c_int;
    pub fn ms_deep_evals(ctx: *mut ms_ctx, deep: *const MsDeep, evals: *mut u64) -> c_int;
    pub fn ms_deep_compose(ctx: *mut ms_ctx, deep: *const MsDeep, gamma: *const u64) -> c_int;
    pub fn ms_deep_len(ctx: *const ms_ctx) -> c_int;
    // ---- proof-of-work grinding (build-defined): the smallest nonce of [start, start + limit) whose digest D(seed || nonce LE) starts with `bits` zero bits
    pub fn ms_grind(ctx: *mut ms_ctx, seed: *const u8 /* [32] */, bits: u32, start: u64, limit: u64, nonce: *mut u64) -> c_int;
    // ---- Tree trait (src/merkle.rs:8-30) on its own
    pub fn ms_merkle_commit(ctx: *mut ms_ctx, leafs: *const u64, leaf_num: usize, ext: c_int, lpn: usize, ic: usize,
                            nodes_out: *mut u8, nodes_cap: usize, nnodes: *mut usize, root: *mut u8) -> c_int;
    pub fn ms_merkle_prove(ctx: *mut ms_ctx, leafs: *const u64, leaf_num: usize, ext: c_int, lpn: usize, leaf: *const u64,
                           path_out: *mut u8, cap: usize, path_len: *mut usize) -> c_int;
    // ---- standalone transforms and measurement aids
    pub fn ms_ntt(ctx: *mut ms_ctx, data: *mut u64, n: usize, batch: usize, inverse: c_int) -> c_int;
    pub fn ms_coset_lde(ctx: *mut ms_ctx, coeffs: *const u64, ncoef: usize, batch: usize, shift: u64, out: *mut u64, l: usize) -> c_int;
    pub fn ms_bench_lde(ctx: *mut ms_ctx, blowup: usize, shift: u64) -> c_int;
    pub fn ms_arith_selftest(ctx: *mut ms_ctx, op: c_int, a: *const u64, b: *const u64, out: *mut u64, n: usize) -> c_int;
    pub fn ms_profile_begin(ctx: *mut ms_ctx) -> c_int;
    pub fn ms_profile_end(ctx: *mut ms_ctx, json_out: *mut c_char, cap: usize) -> c_int;
}
