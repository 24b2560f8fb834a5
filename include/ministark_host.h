/* ministark_host.h — C entry points of libministark_host.so: the host-side mirror of the reference's prover API ABOVE
 * the C ABI of ministark.h (mini-stark_amd/host/stark_host.cpp: StarkConfig::new src/starks.rs:268-310, Stark::prove
 * src/starks.rs:59-169, Stark::verify src/starks.rs:171-235 with Fri::verify src/fri.rs:191-290 and MerkleRoot::check_proof
 * src/merkle.rs:312-338) and the whole-proof wire format.  The reference is Rust and derives no serialisation for StarkProof
 * (src/starks.rs:21-28), FriProof (src/fri.rs:17-22) or MerklePath (src/merkle.rs:293-298): both layouts below are build-defined.
 *
 * MSSP v1 (little-endian):
 *   u32 magic 'MSSP' | u32 version 1 | u32 E | u32 c | u32 q | u32 rounds | u64 len(arthur) | u64 len(fri blob)
 *   trace_commit[32] | constrain_trace_commit[32]
 *   constrain_queries q*c*E u64 | validity_queries q*E u64                     (StarkProof.constrain_queries / validity_query)
 *   fri_roots rounds*32   (round 0 first; not in the reference's StarkProof: round 0's root never reaches its transcript)
 *   arthur bytes          (the prover's transcript, StarkProof.arthur; build-defined hash chain over the context's digest, NOT nimue's bytes.  With grinding
 *                          bits configured - msh_stark_set_grinding - arthur also carries the proof of work's nonce, 8 little-endian bytes behind the last
 *                          round's root: the layout and the version stay what they are, arthur is 8 bytes longer)
 *   FriProof in the MSFP layout of ministark.h
 * The Python mirror writes the same bytes (mini_stark_amd.stark.StarkProof.to_bytes). */
#ifndef MINISTARK_HOST_H
#define MINISTARK_HOST_H
#include <stddef.h>
#include <stdint.h>
#include "ministark.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct msh_stark msh_stark;
typedef struct {
  uint32_t e, c, q, rounds;
  uint64_t arthur_len, fri_blob_len;
  const uint8_t *trace_commit, *constrain_trace_commit, *fri_roots, *arthur, *fri_blob;
  const uint64_t *constrain_queries, *validity_queries;
} msh_proof_view;
/* one MerklePath / one (window, query) record of the MSFP blob (ministark.h): views INTO the parsed buffer */
typedef struct { uint64_t leaf_index, nlevels; const uint64_t* leaf_neighbours; /* 2*E */ const uint8_t* levels; /* nlevels * 2 * 32 */ } msh_merkle_path_view;
typedef struct { const uint64_t* points; /* 6*E: x1 y1 x2 y2 x3 y3 */ uint64_t qlen; const uint64_t* quotient; /* qlen*E */ msh_merkle_path_view path[2]; } msh_fri_query_view;

/* StarkConfig::new + Stark::new (starks.rs:268-310, 40-57); NULL and *err = MS_ERR_SHAPE for < 20 security bits (starks.rs:317-320) */
msh_stark* msh_stark_new(ms_ctx* ctx, int field, uint64_t security_bits, uint64_t blowup, uint64_t steps, uint64_t trace_columns, int* err);
void msh_stark_free(msh_stark* h);
int msh_stark_config(const msh_stark* h, uint64_t* rounds, uint64_t* constrain_queries, uint64_t* fri_queries);
/* Build-defined proof of work (ministark.h: pow_ok, ms_grind): `bits` of the security bits come from a nonce ground between the FRI commit phase and the query
 * phase; fri_queries is recomputed with ms_num_queries_grind.  Call before msh_stark_prove / msh_stark_verify*; prover and verifier must agree on `bits`.  Prover:
 * seed = 32 challenge bytes behind the last round's root, the nonce's 8 little-endian bytes are absorbed (they travel in arthur), then the query positions are drawn.
 * Verifier: the same steps; a nonce that fails pow_ok rejects with a `why` naming the proof of work.  0 bits (the default): nothing is drawn or absorbed.
 * Returns what ms_num_queries_grind returns. */
int msh_stark_set_grinding(msh_stark* h, uint32_t bits);
/* the nonce of the last proof: MS_OK, MS_ERR_STATE when that proof was made without grinding */
int msh_proof_pow_nonce(const msh_stark* h, uint64_t* nonce);
/* pow_ok(D, seed, nonce, bits) of ministark.h with the hasher behind msh_hash: 1, 0, or -1 for an unknown digest id or bits > 64 */
int msh_pow_check(int digest_id, const uint8_t seed[32], uint64_t nonce, uint32_t bits);
/* Stark::prove (starks.rs:59-169): trace from host memory or already in HBM; transitions as lincombs of trace polynomials */
int msh_stark_prove(msh_stark* h, const uint64_t* trace_host, const void* trace_dev, size_t N, size_t w, int ntrans, const int* tr_k,
                    const uint64_t* tr_scalars, const int* tr_idx, int read_fri_proof);
/* A pipelined caller names the page-locked (ms_pinned_alloc) row-major trace of the proof AFTER the next msh_stark_prove: that call hands it to
 * ms_trace_upload_async right behind its own trace commitment, so the upload overlaps the proof (one-shot: name it again before every prove). */
void msh_stark_next_trace(msh_stark* h, const uint64_t* trace_host, size_t N, size_t w);
size_t msh_proof_arthur(const msh_stark* h, uint8_t* out, size_t cap);
int msh_proof_commits(const msh_stark* h, uint8_t* trace_commit, uint8_t* lde_commit);
size_t msh_proof_evals(const msh_stark* h, uint64_t* out, size_t cap_elems);
size_t msh_proof_fri_roots(const msh_stark* h, uint8_t* out, size_t cap);
/* read_fri_proof of msh_stark_prove: 0 = the FRI proof stays in HBM, 1 = read back before returning, 2 = read back asynchronously
 * (ms_fri_proof_read_async: the bytes travel into the slot's page-locked buffer while the caller goes on, e.g. into the next
 * msh_stark_prove); msh_proof_wait - and every accessor below that touches the blob - waits for them; 3 = the query-phase kernels write
 * the blob straight into the slot's page-locked buffer (ms_fri_query_into), complete on return.
 * The mirror holds TWO proof slots: msh_stark_prove k + 1 reuses the slot of proof k - 1, so proof k stays whole (msh_prev_proof_*) while
 * k + 1 is computed - including a mode-2 blob that is still arriving. */
int msh_proof_wait(const msh_stark* h);
size_t msh_proof_fri_blob(const msh_stark* h, uint8_t* out, size_t cap);
size_t msh_proof_challenges(const msh_stark* h, uint64_t* out, size_t cap_elems);
size_t msh_proof_num_polys(const msh_stark* h);
size_t msh_prev_proof_arthur(const msh_stark* h, uint8_t* out, size_t cap);
size_t msh_prev_proof_fri_roots(const msh_stark* h, uint8_t* out, size_t cap);
size_t msh_prev_proof_fri_blob(const msh_stark* h, uint8_t* out, size_t cap);
/* FNV-1a (64-bit words) over the FRI blob of the last (which = 0) / previous (which = 1) proof, read in place from its page-locked slot */
uint64_t msh_proof_blob_checksum(const msh_stark* h, int which);
/* the same over one 64-bit word per `stride_bytes` plus the last word */
uint64_t msh_proof_blob_sample(const msh_stark* h, int which, size_t stride_bytes);
/* Stark::verify (starks.rs:171-235) on the CPU.  A PARITY MIRROR of the reference's verifier, including what it does NOT bind
 * (INTEGRATION.md "verifier"): 1 accepted, 0 rejected, < 0 malformed. */
int msh_stark_verify(const msh_stark* h, const uint64_t* constrains, size_t c, size_t N, const uint8_t* arthur, size_t arthur_len, const uint8_t* trace_commit,
                     const uint8_t* lde_commit, const uint64_t* evals, size_t nevals, const uint8_t* fri_roots, size_t nroots, const uint8_t* blob, size_t blob_len,
                     int zero_display_empty, char* why, size_t why_cap);
/* MSSP: serialise the last proof (returns the size needed; writes when cap suffices), parse (views into the buffer), verify from bytes */
size_t msh_proof_serialize(const msh_stark* h, uint8_t* out, size_t cap);
int msh_proof_parse(const uint8_t* data, size_t len, msh_proof_view* out);
int msh_stark_verify_mssp(const msh_stark* h, const uint64_t* constrains, size_t c, size_t N, const uint8_t* data, size_t len, int zero_display_empty, char* why, size_t why_cap);
/* FriProof (fri.rs:17-22) from its MSFP bytes: the compiled twin of the Rust shim's FriProof::from_msfp.  windows = rounds - 1; returns the
 * number of (window, query) records (windows * nq; the first `cap` are written to `out`) or -1 if the bytes do not parse exactly. */
int msh_fri_proof_parse(const uint8_t* blob, size_t len, uint32_t e, uint32_t windows, uint32_t nq, msh_fri_query_view* out, size_t cap);
/* The verifying side of the openings by index (ministark.h: ms_tree_open, ms_fri_query_index; build-defined, no reference counterpart).
 * msh_merkle_path_check_index is check_proof made POSITIONAL, on one serialised MerklePath (ic = 2, any lpn, ext in {1, E} limbs per element) of at most `avail`
 * bytes: the path's leaf_index word must be expect_leaf_group * lpn, its leaf_neighbours canonical; at level l the running digest must sit in slot
 * (expect_leaf_group >> l) & 1 - "either half" is not accepted -, the path must be as high as the position needs and end at `root`.  *used receives the path's
 * bytes.  1 accepted, 0 rejected, < 0 a null argument, an unknown digest id or field, ext or lpn out of range. */
int msh_merkle_path_check_index(int digest_id, int field, int ext, size_t lpn, int zero_display_empty, const uint8_t root[32], const uint8_t* path, size_t avail,
                                uint64_t expect_leaf_group, size_t* used);
/* The MSFI blob of ms_fri_query_index against the commit phase: roots rounds * 32 bytes (round 0 first), z (rounds - 1) * E limbs, B (rounds - 1) * 2 * E limbs,
 * alpha (rounds - 1) * E limbs - what ms_fri_deep / ms_fri_fold_commit took and returned -, and the nq betas.  It parses the blob exactly (a header that is not the
 * verifier's E, rounds and nq or names no domain that can be halved rounds - 1 times, a non-canonical limb, a path of another height than its round's, trailing
 * bytes: rejected), checks nfinal <= max(1, D_(R-1) / blowup), checks every path at ITS position (leaf_index = the position, group = position / 2) under its
 * round's root, and per (window, query) the DEEP-adjusted linearity check of Stark::verify's FRI step with y3 = the next window's opened value, for the last window
 * the final polynomial at x3: the line through (x1, y1), (x2, y2) at alpha_i equals y3 (x3 - z_i) + B_i0 + B_i1 alpha_i.  1 accepted, 0 rejected (reason in `why`),
 * < 0 malformed arguments. */
int msh_fri_index_verify(int digest_id, int field, int zero_display_empty, uint64_t blowup, const uint8_t* roots, size_t rounds, const uint64_t* z, const uint64_t* B,
                         const uint64_t* alpha, const uint64_t* betas, size_t nq, const uint8_t* blob, size_t len, char* why, size_t why_cap);
/* The MSFF blob of ms_fri_query_folded (ministark.h: folded FRI, build-defined) against its commit phase: roots rounds * 32 bytes (the R committed rounds, round 0
 * first), alpha rounds * E limbs (alpha_0 .. alpha_(R-1): what ms_fri_fold_folded and ms_fri_fold_final took), the nq betas, a = 2^log_arity.  It trusts no header
 * field: E, k, R and nq must be the verifier's, D_0 a power of two within the field's two-adicity with a^R * blowup <= D_0, nfinal = D_R / blowup exactly, and the
 * blob exactly as long as that header fixes (truncated, or trailing bytes: rejected); a non-canonical limb and a path of another height than its round's are rejected.
 * With b_(0,j) = betas[j] mod D_0, b_(i+1,j) = b_(i,j) mod D_(i+1), per round i and query j it checks the path by msh_merkle_path_check_index's rule (lpn = a,
 * ext = E, leaf group b_(i+1,j)) under round i's root; then for i >= 1 that slot b_(i,j) / D_(i+1) of the opened coset is the fold of round i - 1's coset at
 * alpha_(i-1) - the value at alpha_(i-1) of the polynomial of degree < a through the coset's a values, the coset being x w^t with x = g_(i-1)^(b_(i,j)),
 * w = g_(i-1)^(D_(i-1) / a) -; then that the fold of round R - 1's coset at alpha_(R-1) is the final polynomial at g_R^(b_(R,j)).
 * Round 0's values are bound to nothing by this check alone, as in MSFI: what ties them to a trace is msh_deep_link_verify_folded, over the a LDE rows under each
 * round-0 coset.
 * 1 accepted, 0 rejected (`why` names the step: "header: ..", "round i opening: ..", "round i fold: ..", "final polynomial: .."), < 0 malformed arguments (a null
 * pointer, an unknown digest id or field, rounds outside 1..64, nq outside 1..4096, a blowup that is zero or no power of two, log_arity outside 1..3, an alpha limb that is not canonical). */
int msh_fri_folded_verify(int digest_id, int field, int zero_display_empty, uint64_t blowup, int log_arity, const uint8_t* roots, size_t rounds, const uint64_t* alpha,
                          const uint64_t* betas, size_t nq, const uint8_t* blob, size_t len, char* why, size_t why_cap);
/* The verifying side of the DEEP stage (ministark.h: ms_validity_commit, ms_deep_evals, ms_deep_compose; build-defined, no reference counterpart): the link between
 * FRI's round 0 and the two committed trees.  N rows, L = blowup * N (the FRI blowup is the LDE's), c LDE columns, m chunk columns, `deep` / evals / gamma what the
 * prover's ms_deep_evals / ms_deep_compose took and returned, msfi the blob of ms_fri_query_index for `betas`.  With D_0 from the MSFI header (required: a power of two
 * that divides L, D_0 <= L) and b_j = betas[j] mod D_0, lde_open and val_open are the ms_tree_open outputs of MS_TREE_LDE and MS_TREE_VALIDITY for the 2 nq rows
 * p_j = b_j (L / D_0) and (p_j + L / 2) mod L, in that order per query: the rows under window 0's two positions b_j and (b_j + D_0 / 2) mod D_0.
 * It checks every path positionally under its root (msh_merkle_path_check_index's rule: leaf_index = row * lpn), both blobs consumed exactly; for each row computes
 *   sum_n gamma^n (F_(pt_poly[n])(x) - evals[n]) / (x - z_t(n))   at x = shift g_L^p, F from the opened rows,
 * and requires it to equal the value window 0 of the MSFI opened at the matching position (leaf_neighbours[position & 1] of the query's first or second path); for
 * R = 1 there is no window and it compares with the final polynomial at g_0^position.  It does NOT repeat msh_fri_index_verify (run it on the same MSFI, with the
 * round roots from the transcript) nor the AIR identity at z (msh_air_expected_validity[_ext] against msh_validity_from_chunks): the caller runs those.
 * 1 accepted, 0 rejected (reason in `why`, naming the step: "LDE opening: ..", "validity opening: ..", "DEEP link: ..", "MSFI .."), < 0 malformed arguments. */
int msh_deep_link_verify(int digest_id, int field, int zero_display_empty, uint64_t N, uint64_t blowup, uint64_t shift, uint32_t c, uint32_t m,
                         const uint8_t lde_root[32], const uint8_t val_root[32], const ms_deep* deep, const uint64_t* evals, const uint64_t* gamma,
                         const uint64_t* betas, size_t nq, const uint8_t* msfi, size_t msfi_len, const uint8_t* lde_open, size_t lde_len,
                         const uint8_t* val_open, size_t val_len, char* why, size_t why_cap);
/* V(z) from the m = ve * nchunks chunk evaluations (chunk column k * ve + l at chunk_evals + (k * ve + l) * E, E limbs each) by the identity of ms_validity_commit,
 *   V(z) = sum_k z^(kN) sum_l u_l V_(k,l)(z):  the value to compare with msh_air_expected_validity[_ext].  ve in {1, E}.  MS_OK, or MS_ERR_ARG (null, ve, a limb >= p). */
int msh_validity_from_chunks(int field, uint32_t ve, uint32_t nchunks, uint64_t N, const uint64_t* z, const uint64_t* chunk_evals, uint64_t* out);
/* D(data) by this library's own host implementation of an ms_digest_id (SHA-256, BLAKE2s-256, BLAKE3 with its chunk tree, Keccak-256, SHA3-256: any length): 0, -1 for an unknown id (3 is unassigned) */
int msh_hash(int digest_id, const uint8_t* data, size_t len, uint8_t out[32]);
/* The verifying side of ms_mix_terms (ministark.h; build-defined, no reference counterpart): the value validity(z) must have at an extension point z (E limbs),
 *   (sum_t r^t C_t(z)) * prod_{k=1..nexempt} (z - w^(N-k)) / (z^N - 1),  C_t(z) = sum_m coef_m * prod_f opened[k(row_f)][poly_f],
 * from the same CSR program and the opened values opened[k][j] = P_j(w^rows[k] z): E limbs each, row k at opened + k * row_stride (u64 words), polynomial j at
 * + j * E - with rows[k] the offsets the program touches, the output of ms_eval_ext at the points w^rows[k] z is this layout with row_stride = (c + 1) * E.
 * Writes E limbs to out.  MS_OK; MS_ERR_ARG for a null argument, a malformed program (the conditions of ms_mix_terms; a polynomial index >= npolys) or a
 * non-canonical element; MS_ERR_OUT_OF_RANGE when the program uses a row that `rows` does not list; MS_ERR_SHAPE when z^N = 1. */
int msh_terms_expected_validity(int field, uint64_t r, int ncons, const uint32_t* term_begin, const uint64_t* coef, const uint32_t* fac_begin, const uint32_t* fac_poly,
                                const uint32_t* fac_row, int nexempt, uint64_t N, const uint64_t* z, int nrows, const uint32_t* rows, const uint64_t* opened,
                                size_t row_stride, uint32_t npolys, uint64_t* out);
/* The verifying side of ms_mix_air (ministark.h; build-defined): the value validity(z) must have at an extension point z,
 *   sum_t r^t C_t(z) Z_t(z) / (z^N - 1)  +  sum_b r^(ncons+b) (opened[row 0][bnd_poly[b]] - bnd_val[b]) / (z - w^bnd_row[b]),
 * from the same ms_air program and opened values laid out as for msh_terms_expected_validity.  A periodic factor K_k(w^row z) is evaluated here and needs no
 * opening; the boundary quotients are computed from the row-0 opening P_j(z).  Writes E limbs to out.  MS_OK; MS_ERR_ARG for a null argument, a malformed
 * program (the conditions of ms_mix_air; a polynomial index >= npolys) or a non-canonical element; MS_ERR_OUT_OF_RANGE when the program uses a row that `rows`
 * does not list (row 0 included when nbound > 0); MS_ERR_SHAPE when z^N = 1. */
int msh_air_expected_validity(int field, uint64_t r, const ms_air* air, uint64_t N, const uint64_t* z, int nrows, const uint32_t* rows, const uint64_t* opened,
                              size_t row_stride, uint32_t npolys, uint64_t* out);
/* The verifying side of ms_mix_air_ext: the same value with r in the extension (E canonical limbs), its powers taken there.  Everything else as above; a null r
 * or a limb >= p is MS_ERR_ARG.  r = (r0, 0, ..) gives msh_air_expected_validity(r0). */
int msh_air_expected_validity_ext(int field, const uint64_t* r /* E limbs */, const ms_air* air, uint64_t N, const uint64_t* z, int nrows, const uint32_t* rows,
                                  const uint64_t* opened, size_t row_stride, uint32_t npolys, uint64_t* out);
/* ---- LINKED PROOFS: MSLP v1 (build-defined; the sound counterpart of msh_stark_prove / MSSP, which keep the reference's unlinked flow byte for byte) ----------------
 * THE STATEMENT a linked proof claims: there are w polynomials of degree < N, committed under the LDE root, that satisfy `air` - its transition constraints,
 * exemption sets, periodic columns and boundary values are the public input.  The constraint polynomials are the trace columns (c = w; no ms_polys_lincomb
 * transitions).  Running columns are not part of THIS flow: their challenges have to follow a commitment to the main columns' LDE - the staged commitment of MSLP v2,
 * below.  The raw-trace root is computed because ms_trace_commit is how the trace gets in; it is absorbed first
 * and BINDS NOTHING - no opening of that tree is part of the proof.
 * The handle's configuration supplies field, digest, blowup, the rounds (fri_rounds = 0), fri_queries and the grinding bits (msh_stark_set_grinding).  The linked proof
 * lives in a slot of its own: msh_stark_prove, MSSP and the two MSFP slots are untouched.
 *
 * msh_air_encode: the canonical bytes of an AIR program, little-endian: u32 'MSAR' (0x5241534D) | u32 version 1 | u32 ncons, nterms, nfacs, nexempt, nperiodic,
 * nperval, nbound, array_bytes (the eight counts: nterms = term_begin[ncons], nfacs = fac_begin[nterms], nexempt = ex_begin[ncons], nperval = per_begin[nperiodic],
 * array_bytes = the bytes that follow) | the arrays in the order of the ms_air struct: term_begin, coef, fac_begin, fac_poly, fac_row, ex_begin, ex_row, per_begin
 * (the single word 0 when nperiodic = 0), per_val, bnd_poly, bnd_row, bnd_val - u32 arrays as u32, u64 arrays as u64.  The counts fix every array's length, so two
 * programs that differ in any entry encode differently.  Returns the size (writes when cap suffices), 0 for a null or malformed program (a needed array missing, CSR
 * offsets not starting at 0 or decreasing, a limit of ms_mix_air on the counts exceeded).
 * msh_air_rows: the row offsets the verifying side needs opened - those of the program's factors, and row 0 when there are boundary constraints - ascending, the C
 * twin of mini_stark_amd.air_rows.  Returns their number (the first `cap` are written), MS_ERR_ARG for a malformed program.
 *
 * TRANSCRIPT: the Transcript hash chain with the domain separator domsep + "/linked/v1" (a linked and an unlinked transcript never coincide), in this order:
 *   1. absorb the statement: the u64 words field, digest id, N, w, blowup, R, nq, grinding bits; then msh_air_encode(air).  (The statement does not travel.)
 *   2. absorb the trace root; draw shift (one base-field scalar), REDRAWN while msh_linked_shift_ok is 0: shift == 0 or shift^L == 1, the coset meeting the trace
 *      domain - probability about 2^-8 for BabyBear at the headline size, so the redraw is part of the protocol on both sides, not an error path.
 *   3. ms_interpolate, ms_lde_commit(blowup, shift, lpn = w); absorb the LDE root.
 *   4. draw r (E limbs); ms_mix_air_ext.  MS_ERR_SHAPE comes back as is: the trace violates the AIR.
 *   5. ms_validity_commit(m), m = E * VL / N; absorb the validity root.
 *   6. draw z (E limbs), REDRAWN while msh_linked_z_ok is 0: every limb above limb 0 zero, z in the base field (this makes ms_deep_compose's MS_ERR_SHAPE
 *      unreachable).  The points are z * w^row for row in msh_air_rows(air), row 0 first (added if the program does not name it); more than 8: MS_ERR_ARG.  Every
 *      point opens all c columns, the point of row 0 the m chunk columns too.  ms_deep_evals; absorb the evaluations.
 *   7. draw gamma (E limbs); ms_deep_compose.
 *   8. ms_fri_begin(blowup, R); absorb round 0's root (the unlinked flow never does).  Per round: draw z_i, ms_fri_deep, absorb B, draw alpha_i,
 *      ms_fri_fold_commit, absorb the root.
 *   9. grind exactly as msh_stark_prove: 32 challenge bytes as seed, the nonce's 8 little-endian bytes absorbed.
 *  10. draw nq = fri_queries betas, 8 challenge bytes each; ms_query_linked.
 * MSLP v1, little-endian:
 *   u32 'MSLP' (0x504C534D) | u32 version 1 | u32 E | u32 c | u32 m | u32 npts | u32 R | u32 nq | u32 grinding bits | u64 N | u64 blowup | u64 len(arthur) | u64 len(MSLQ)
 *   arthur   everything the prover absorbed after the statement, in order: trace root, LDE root, validity root, evaluations, round 0's root, per round B and root, nonce
 *   MSLQ     the blob of ms_query_linked (ministark.h)
 * msh_stark_prove_linked returns the stage's code on failure (MS_ERR_ARG for a malformed program or shape, MS_ERR_SHAPE for a trace that violates the AIR) and leaves
 * the slot empty; msh_linked_proof returns the size of the last linked proof (0: none) and writes it when cap suffices.
 * msh_stark_verify_linked compares EVERY header field with what it computes from its own configuration, air, N, w and fri_rounds (none is trusted), requires the
 * lengths to fit exactly with no trailing bytes and every limb canonical, replays the transcript from the arthur bytes with both redraw rules, then runs in this order
 * the proof of work, the AIR identity at z (msh_air_expected_validity_ext on the opened evaluations against msh_validity_from_chunks), msh_fri_index_verify on the
 * MSFI section with the roots, z_i, B_i, alpha_i of the replay and its own betas, and msh_deep_link_verify on the three sections.  1 accepted; 0 rejected, `why`
 * naming the step: "header: ..", "transcript: ..", "proof of work: ..", "AIR identity: ..", "FRI: .." (msh_fri_index_verify's reason behind it), or
 * msh_deep_link_verify's own "LDE opening: ..", "validity opening: ..", "DEEP link: ..", "MSFI .."; < 0 malformed arguments.
 * The Python mirror writes the same bytes (mini_stark_amd.stark.Stark.prove_air). */
int msh_stark_prove_linked(msh_stark* h, const uint64_t* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, uint32_t fri_rounds /* 0: the configuration's */);
size_t msh_linked_proof(const msh_stark* h, uint8_t* out, size_t cap);
int msh_stark_verify_linked(const msh_stark* h, const ms_air* air, size_t N, size_t w, uint32_t fri_rounds, const uint8_t* data, size_t len, int zero_display_empty,
                            char* why, size_t why_cap);
size_t msh_air_encode(const ms_air* air, uint8_t* out, size_t cap);
int msh_air_rows(const ms_air* air, uint32_t* rows, int cap);
/* ---- LINKED PROOFS WITH RUNNING COLUMNS: MSLP v2 (build-defined) -----------------------------------------------------------------------------------------------------
 * A v2 proof carries permutation and lookup arguments: running columns whose challenges are drawn BEHIND the commitment to the main columns, built by
 * ms_aux_running_staged and committed in a second LDE tree by ms_lde_commit_stage (ministark.h).  THE STATEMENT: there are w polynomials of degree < N, committed under
 * the stage-0 LDE root, that satisfy `air` (a program over the w trace columns, at least one constraint) and the nargs arguments.
 *
 * msh_aux_arg: one argument with SYMBOLIC challenges.  A proof draws nch challenges ch[0 .. nch) in K (nch in 1..8).  The arrays are those of ms_aux with base-field
 * values (one u64 each) and a selector beside every value: 0 "times 1", k "times ch[k - 1]".  The column's ext is always E.  Instantiating a descriptor with drawn
 * challenges gives the ms_aux of ms_aux_running_staged.
 * msh_aux_encode: the canonical bytes, little-endian: u32 'MSAX' (0x5841534D) | u32 version 1 | u32 nargs | u32 nch, then per argument u32 op, nfrac, nterms |
 * form_begin (2 nfrac + 1 u32) | term_col, term_ch (nterms u32 each) | form_ch (2 nfrac u32) | term_coef (nterms u64) | form_const (2 nfrac u64).  The counts fix every
 * length.  Returns the size (writes when cap suffices), 0 for a malformed descriptor: a null array, a selector > nch, a value >= p, nch outside 1..8, more than 16 limb
 * columns (nargs * E), any limit of ms_aux_running (op, nfrac, form_begin, 16 terms per form).  A column >= w is refused by the drivers, which know w.
 *
 * msh_air_prog: a growable copy of an ms_air program (msh_air_prog_new: NULL for a malformed one; msh_air_prog_air: the program as it stands, valid until the next
 * call on the object).  msh_aux_constraints: the C twin of mini_stark_amd.aux_constraints - for an instantiated ms_aux (ext = E) it appends the transition constraint
 * cleared of denominators, expanded limb by limb (terms in the order of their sorted monomials), with no exemption, and the boundary z(w^0) = identity, as constraints
 * over the polynomials first_poly .. first_poly + E - 1: msh_air_encode of the result is the bytes of the Python function's.  MS_ERR_ARG when the expansion exceeds
 * ms_mix_air's limits (8 factors per term, 65536 terms, 4096 constraints); the program is then unchanged.
 *
 * msh_deep_link_verify_staged: msh_deep_link_verify with two LDE trees - per row F_j comes from the stage-0 row (c0 elements, under lde_root) for j < c0 and from the
 * staged row (c1 elements, under stg_root) for c0 <= j < c0 + c1; the chunk columns are j >= c0 + c1.  Both blobs are consumed exactly, paths checked positionally
 * under their own roots; the additional reason prefix is "staged opening: ..".
 *
 * TRANSCRIPT, domain separator domsep + "/linked/v2":
 *   1. absorb the statement: the u64 words field, digest id, N, w, blowup, R, nq, grinding bits, nargs, nch; then msh_air_encode(air); then msh_aux_encode(args).
 *   2. absorb the trace root; draw shift with v1's redraw rule.
 *   3. ms_interpolate, ms_lde_commit(blowup, shift, lpn = w); absorb the stage-0 root.
 *   4. draw ch[0 .. nch), E limbs each; instantiate every argument and call ms_aux_running_staged once per argument, in order.  A zero denominator (MS_ERR_SHAPE,
 *      probability about N / |K|) is returned as it is: there is no redraw rule.  A `final` that is not the identity - the argument does not hold - is MS_ERR_SHAPE too.
 *   5. ms_lde_commit_stage(lpn = c1 = nargs * E); absorb the staged root.
 *   6. v1's steps 4-10 on the combined program - air plus msh_aux_constraints of every argument, argument k at first_poly = w + k E - with c = w + c1 columns: r,
 *      ms_mix_air_ext, ms_validity_commit, z, ms_deep_evals, gamma, ms_deep_compose, the FRI commit phase with round 0's root absorbed, grinding, betas, ms_query_linked
 *      (the staged layout, MSLS).  The points are msh_air_rows of the combined program; every point opens all c columns.
 * MSLP v2, little-endian:
 *   u32 'MSLP' | 2 | E | c0 | c1 | m | npts | R | nq | grinding bits | nargs | nch | u64 N | blowup | len(arthur) | len(MSLS)
 *   arthur (v1's, with the staged root behind the stage-0 root) | the MSLS blob
 * msh_stark_prove_linked_aux returns the stage's code on failure and leaves the slot empty; msh_linked_proof returns whichever linked proof was made last.
 * msh_stark_verify_linked_aux trusts no header field: it compares what the statement fixes, replays the transcript (both redraws, the challenge draw), rebuilds the
 * combined program from its own statement and the challenges it drew, compares what that program fixes (m, npts, len(arthur); the MSLS lengths must fit exactly), then
 * runs in order the proof of work, the AIR identity at z, msh_fri_index_verify and msh_deep_link_verify_staged.  `why` prefixes: v1's, plus "staged opening: ".  A v1
 * verifier given v2 bytes answers "header: ..", and so does a v2 verifier given v1 bytes.  The Python mirror writes the same bytes (Stark.prove_air(.., aux=(args, nch))). */
typedef struct msh_aux_arg {
  uint32_t op, nfrac;
  const uint32_t* form_begin;   /* 2 nfrac + 1 */
  const uint32_t* term_col;     /* nterms: a trace column, < w */
  const uint64_t* term_coef;    /* nterms base-field values */
  const uint32_t* term_ch;      /* nterms selectors */
  const uint64_t* form_const;   /* 2 nfrac base-field values */
  const uint32_t* form_ch;      /* 2 nfrac selectors */
} msh_aux_arg;
typedef struct msh_air_prog msh_air_prog;
size_t msh_aux_encode(int field, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, uint8_t* out, size_t cap);
msh_air_prog* msh_air_prog_new(const ms_air* base);
void msh_air_prog_free(msh_air_prog* prog);
const ms_air* msh_air_prog_air(msh_air_prog* prog);
int msh_aux_constraints(msh_air_prog* prog, int field, const ms_aux* aux /* ext = E */, uint32_t first_poly);
int msh_deep_link_verify_staged(int digest_id, int field, int zero_display_empty, uint64_t N, uint64_t blowup, uint64_t shift, uint32_t c0, uint32_t c1, uint32_t m,
                                const uint8_t lde_root[32], const uint8_t stg_root[32], const uint8_t val_root[32], const ms_deep* deep, const uint64_t* evals,
                                const uint64_t* gamma, const uint64_t* betas, size_t nq, const uint8_t* msfi, size_t msfi_len, const uint8_t* lde_open, size_t lde_len,
                                const uint8_t* stg_open, size_t stg_len, const uint8_t* val_open, size_t val_len, char* why, size_t why_cap);
int msh_stark_prove_linked_aux(msh_stark* h, const uint64_t* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const msh_aux_arg* args,
                               uint32_t nargs, uint32_t nch, uint32_t fri_rounds /* 0: the configuration's */);
int msh_stark_verify_linked_aux(const msh_stark* h, const ms_air* air, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, size_t N, size_t w, uint32_t fri_rounds,
                                const uint8_t* data, size_t len, int zero_display_empty, char* why, size_t why_cap);
/* ---- THE LINK OF A FOLDED FRI TO COSET-GROUPED ROW TREES (build-defined) ------------------------------------------------------------------------------------------------
 * msh_deep_link_verify_folded: what msh_deep_link_verify[_staged] is to an MSFI, for the MSFF of a folded FRI at arity a = 2^log_arity over row trees committed by
 * ms_lde_commit_coset, ms_lde_commit_stage_coset and ms_validity_commit_coset at the same log_arity (ministark.h).  c0 LDE columns, c1 staged columns (stg_root NULL iff
 * c1 = 0; stg_open is then not read), m chunk columns; deep / evals / gamma as for msh_deep_link_verify; msff the blob of ms_fri_query_folded for `betas`; the three
 * opening sections those of ms_query_linked_folded.  D_0 comes from the MSFF header: a power of two that divides L = blowup * N, a <= D_0 <= L.  With s = L / D_0,
 * D_1 = D_0 / a and q_j = (betas[j] mod D_0) mod D_1 every row path is checked positionally under its root (msh_merkle_path_check_index with lpn = a * c, leaf group
 * q_j s) and each section must be consumed exactly.  For EVERY t < a, at x = shift g_L^(q_j s + t L / a), it recomputes
 *   sum_n gamma^n (F_(pt_poly[n])(x) - evals[n]) / (x - z_t(n)),   F_n from slot col * a + t of the proper tree's leaf group,
 * and requires it to equal slot t (E limbs) of round 0's path for query j in the MSFF: all a slots feed the fold, so all a slots are bound.  It does NOT repeat
 * msh_fri_folded_verify (run it on the same MSFF) nor the AIR identity at z.  1 accepted, 0 rejected (`why` names the step: "LDE opening: ..", "staged opening: ..",
 * "validity opening: ..", "DEEP link: ..", "MSFF .."), < 0 malformed arguments. */
int msh_deep_link_verify_folded(int digest_id, int field, int zero_display_empty, uint64_t N, uint64_t blowup, uint64_t shift, int log_arity, uint32_t c0, uint32_t c1,
                                uint32_t m, const uint8_t lde_root[32], const uint8_t stg_root[32] /* NULL iff c1 = 0 */, const uint8_t val_root[32], const ms_deep* deep,
                                const uint64_t* evals, const uint64_t* gamma, const uint64_t* betas, size_t nq, const uint8_t* msff, size_t msff_len, const uint8_t* lde_open,
                                size_t lde_len, const uint8_t* stg_open, size_t stg_len, const uint8_t* val_open, size_t val_len, char* why, size_t why_cap);
/* ---- LINKED PROOFS OVER A FOLDED FRI: MSLP v3 (build-defined) --------------------------------------------------------------------------------------------------------
 * A v3 proof is a v2 proof (v1 when nargs = 0: args NULL, nch 0) whose three row commitments are the `_coset` ones at k = log_arity and whose FRI is the folded one at
 * arity a = 2^k, R = fri_folds folds (0: floor(log2 N / k)).  THE STATEMENT is v2's.
 * TRANSCRIPT, domain separator domsep + "/linked/v3" - v2's steps with these changes:
 *   1. the statement words are field, digest id, N, w, blowup, k, R, nq, grinding bits, nargs, nch; msh_air_encode(air) follows, then msh_aux_encode(args) when nargs > 0.
 *   2. ms_lde_commit_coset, (nargs > 0: the challenge draw, ms_aux_running_staged per argument,) ms_lde_commit_stage_coset, ms_validity_commit_coset, all at k.
 *   3. ms_fri_begin_folded(blowup, k): absorb root 0; for i < R - 1 draw alpha_i, ms_fri_fold_folded, absorb root i + 1; draw alpha_(R-1), ms_fri_fold_final, absorb the
 *      nfinal * E limbs of the final polynomial as u64 little-endian.
 *   4. grind as v1; draw nq = fri_queries betas; ms_query_linked_folded.
 * A stage's MS_ERR_SHAPE is returned as it is - a trace that violates the AIR, an argument that does not hold, a DEEP polynomial so short that R folds do not fit - and
 * the slot is then left empty.
 * MSLP v3, little-endian:
 *   u32 'MSLP' | 3 | E | k | c0 | c1 | m | npts | R | nq | grinding bits | nargs | nch | u64 N | blowup | D_0 | len(arthur) | len(MSLF)
 *   arthur: trace root, LDE root, staged root (nargs > 0), validity root, evaluations, the R round roots, the final polynomial, nonce | the MSLF blob (ministark.h)
 * msh_stark_verify_linked_folded trusts no header field: it compares everything the statement and its own rebuilt program fix; D_0 must be the MSFF's own, a power of two
 * that divides L, and >= a^R * blowup; lengths must fit exactly, with no trailing bytes, and every limb must be canonical; it replays the transcript with both redraw
 * rules and requires the final polynomial in arthur to equal the one in the MSFF ("transcript: .."); then it runs, in order, the proof of work, the AIR identity at z,
 * msh_fri_folded_verify and msh_deep_link_verify_folded.  `why` prefixes: v2's.  A v1 or v2 verifier given v3 bytes answers "header: ..", and so does a v3 verifier
 * given v1 or v2 bytes.  The proof goes into the linked slot (msh_linked_proof).  The Python mirror writes the same bytes (Stark.prove_air(.., log_arity=k)).
 * Measured (tools/linked_folded_bench.py, profiles/linked_folded.json; one paired run on one MI355X, Goldilocks, 2^20 rows, six trace columns, blowup 8, 2 queries, one context, legs alternated x 5): a v1 linked proof 11.30 ms (9.39 ms of kernel time, 221 launches); v3 at arity 2 / 4 / 8 (R = 20 / 10 / 6) 9.36 / 7.02 / 6.31 ms (7.77 / 5.66 / 5.05 ms, 186 / 121 / 96 launches): 0.83 / 0.62 / 0.56 of v1.  Inner hashing 2.87 ms in v1 against 2.70 / 1.42 / 0.97 ms, leaf hashing 2.51 against 2.76 / 1.98 / 1.85 ms.  Proof bytes 83 060 against 41 052 / 23 772 / 18 364; with 32 queries 1 300 340 against 639 132 / 367 452 / 281 404.  Only the paired ratios of this run mean anything. */
int msh_stark_prove_linked_folded(msh_stark* h, const uint64_t* trace_host, const void* trace_dev, size_t N, size_t w, const ms_air* air, const msh_aux_arg* args /* NULL iff nargs = 0 */,
                                  uint32_t nargs, uint32_t nch, int log_arity, uint32_t fri_folds /* 0: floor(log2 N / log_arity) */);
int msh_stark_verify_linked_folded(const msh_stark* h, const ms_air* air, const msh_aux_arg* args, uint32_t nargs, uint32_t nch, size_t N, size_t w, int log_arity,
                                   uint32_t fri_folds, const uint8_t* data, size_t len, int zero_display_empty, char* why, size_t why_cap);
/* the two redraw rules, for a caller that keeps its own transcript: 1 the draw stands, 0 draw again, < 0 an unknown field or a null z */
int msh_linked_shift_ok(int field, uint64_t L, uint64_t shift);
int msh_linked_z_ok(int field, const uint64_t* z /* E limbs */);
/* synthetic trace of the build-defined degree-3 wide AIR (ms_mix_cubic): col_j[i+1] = col_j[i] col_{j+1}[i] col_{j+2}[i] + s_j col_{j+3}[i]; length x w row-major, w scalars */
int msh_cubic_rows(uint64_t p, size_t length, size_t w, uint64_t seed, uint64_t* out, uint64_t* scalars);
/* synthetic Fibonacci-AIR trace of the benchmark workload (N x 3 row-major) */
int msh_fibonacci_rows(uint64_t p, size_t length, size_t steps, uint64_t secret_b, uint64_t pad_seed, uint64_t* out);
#ifdef __cplusplus
}
#endif
#endif
