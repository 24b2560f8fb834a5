/* ministark.h — C ABI of the MI355X-native backend for mini-stark's
 * low-degree-extension + FRI + Merkle proving path.
 *
 * The reference (alv-around/mini-stark, Rust on arkworks) has no FFI; the seams
 * this ABI sits behind are `Stark::prove` (src/starks.rs:59-169), `Fri::prove`
 * (src/fri.rs:53-189), the `Tree` trait (src/merkle.rs:8-30) and the arkworks
 * calls they make.  One function per transcript-delimited stage, so the
 * Fiat–Shamir transcript (nimue) stays with the caller: every challenge is an
 * INPUT and every commitment / opened value an OUTPUT.  INTEGRATION.md shows the
 * Rust `extern "C"` block and the patched `prove` that binds these symbols.
 *
 * Conventions
 *  - Field elements cross the boundary as canonical little-endian u64 limbs
 *    (`Fp::into_bigint()`), also for BabyBear (the reference stores one u64
 *    limb for both fields, src/field.rs:47,76).  Extension elements are E
 *    consecutive limbs: Goldilocks Fp2 = (c0, c1); BabyBear Fp4 =
 *    (c0.c0, c0.c1, c1.c0, c1.c1)  (src/field.rs:50-109).
 *  - Digests are 32 raw bytes of the context's `D` (`Hash<D>`, src/lib.rs:13): SHA-256 (MS_DIGEST_SHA256, `D = Sha256`, the
 *    default), BLAKE2s-256 (MS_DIGEST_BLAKE2S256, `D = Blake2s256`, with MS_FLAG_DIGEST_BLAKE2S), BLAKE3 (MS_DIGEST_BLAKE3,
 *    `D = blake3::Hasher`, with MS_FLAG_DIGEST_BLAKE3), Keccak-256 (MS_DIGEST_KECCAK256, `D = sha3::Keccak256`, with
 *    MS_FLAG_DIGEST_KECCAK256: the hash the EVM has as an opcode) or SHA3-256 (MS_DIGEST_SHA3_256, `D = sha3::Sha3_256`, with
 *    MS_FLAG_DIGEST_SHA3_256).  Every digest the library handles is 32 bytes, so roots, nodes, Merkle paths and the proof layouts
 *    are the same for all of them.
 *  - Every function returns MS_OK or a negative ms_status; nothing unwinds.
 *    Conditions on which the reference panics/asserts map to MS_ERR_SHAPE
 *    (src/merkle.rs:93-104, src/air.rs:23-26,53-54, src/starks.rs:317-320);
 *    src/error.rs:13-21 maps to MS_ERR_LEAF_NOT_FOUND / MS_ERR_OUT_OF_RANGE.
 *  - Blocking calls; one ms_ctx per host thread and per GPU (the reference is
 *    single-threaded, `Stark::prove(&self)`); not thread-safe.
 *  - Host buffers are caller-owned and only read/written during the call.
 *    Large intermediates (polynomials, LDE, trees, FRI rounds) stay in HBM
 *    inside the context until the next proof or ms_destroy.
 */
#ifndef MINISTARK_H
#define MINISTARK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ms_ctx ms_ctx;

typedef enum { MS_FIELD_GOLDILOCKS = 0, MS_FIELD_BABYBEAR = 1 } ms_field; /* src/field.rs:36-76 */

typedef enum {
  MS_OK = 0,
  MS_ERR_SHAPE = -1,          /* reference assert!/panic */
  MS_ERR_LEAF_NOT_FOUND = -2, /* MerkleProofError::LeafNotFound, src/error.rs:15-18 */
  MS_ERR_OUT_OF_RANGE = -3,   /* MerkleProofError::OutOfRangeError, src/error.rs:19-21 */
  MS_ERR_STATE = -4,          /* stage called out of order */
  MS_ERR_ARG = -5,            /* null pointer, non-canonical element, unsupported parameter */
  MS_ERR_HIP = -6,            /* HIP runtime failure; see ms_last_error */
  MS_ERR_NOMEM = -7
} ms_status;

/* flags for ms_create */
#define MS_FLAG_ZERO_DISPLAY_EMPTY 0x1u /* ark-ff Display prints ZERO as "" (default behaviour of ark-ff 0.5.0) */
#define MS_FLAG_TRACE_MONT64 0x2u       /* ms_trace_commit* input is arkworks memory: Montgomery form x*2^64 mod p, one u64 limb
                                          (`Fp<MontBackend<_,1>,1>`, src/field.rs:47,76); everything else stays canonical */
#define MS_FLAG_LATENCY 0x4u            /* this context proves ALONE on its GPU and the caller wants the shortest proof, not the most proofs: independent chains of
                                         * a stage (a FRI round's coefficient side and evaluation side) run on two streams, and the calling thread SPINS on a
                                         * page-locked word the stage's last kernel stores behind its results instead of blocking in the stream synchronisation
                                         * (4-5 us less per transcript round trip, 44 of them per proof; a stage longer than 2 ms falls back to the blocking wait).
                                         * With several contexts in flight it costs throughput (the side streams compete for HIP's few hardware queues: -15 % at
                                         * 8 in flight; every proving thread burns a core while it waits): leave it off there. */
#define MS_FLAG_DIGEST_BLAKE2S 0x8u      /* every commitment of the context (trace, LDE, FRI rounds, the Merkle entry points) hashes with BLAKE2s-256 (RFC 7693, unkeyed:
                                         * RustCrypto `blake2::Blake2s256`) instead of SHA-256: the reference's `D` type argument.  One proof sharded over ranks stays
                                         * SHA-256 only: ms_set_shard / ms_set_shard_rccl return MS_ERR_ARG on such a context. */
#define MS_FLAG_DIGEST_BLAKE3 0x10u      /* the same with BLAKE3 (unkeyed hash mode, 32-byte output: the `blake3` crate's `Hasher`, which implements the `digest` traits behind its
                                         * `traits-preview` feature).  Excludes MS_FLAG_DIGEST_BLAKE2S: ms_create returns MS_ERR_ARG when both are set.  A hashed message
                                         * (a leaf group's decimal text, or the children of an inner node) may be at most 16 KiB under this digest: a commitment whose
                                         * shape allows more returns MS_ERR_ARG.  Sharded proofs: as for BLAKE2s, MS_ERR_ARG from ms_set_shard / ms_set_shard_rccl. */
#define MS_FLAG_DIGEST_KECCAK256 0x20u   /* the same with Keccak-256: the Keccak-f[1600] sponge, rate 136 bytes, with the ORIGINAL Keccak padding (domain byte 0x01) as Ethereum
                                         * uses it (`sha3::Keccak256`).  A sponge has no message-length limit.  Sharded proofs: MS_ERR_ARG, as for the BLAKE digests. */
#define MS_FLAG_DIGEST_SHA3_256 0x40u    /* the same sponge with the FIPS 202 padding (domain byte 0x06): SHA3-256 (`sha3::Sha3_256`).
                                         * A context has ONE digest: ms_create returns MS_ERR_ARG when more than one of the four MS_FLAG_DIGEST_* flags is set. */
#define MS_FLAGS_DEFAULT MS_FLAG_ZERO_DISPLAY_EMPTY
/* Id 3 is unassigned on purpose and stays so: ms_digest never returns it and msh_hash refuses it (the Keccak family starts at 4). */
typedef enum { MS_DIGEST_SHA256 = 0, MS_DIGEST_BLAKE2S256 = 1, MS_DIGEST_BLAKE3 = 2, MS_DIGEST_KECCAK256 = 4, MS_DIGEST_SHA3_256 = 5 } ms_digest_id;

/* ---- context ------------------------------------------------------------ */
int ms_create(ms_ctx** out, int device, ms_field field, uint32_t flags);
void ms_destroy(ms_ctx* ctx);
const char* ms_last_error(const ms_ctx* ctx);
int ms_ext_degree(const ms_ctx* ctx);             /* 2 (Goldilocks) / 4 (BabyBear): StarkField::Extension */
int ms_digest(const ms_ctx* ctx);                 /* ms_digest_id: what the context commits with */
/* Streams.  A context enqueues all its work on ONE stream: its own (created by ms_create, hipStreamNonBlocking) or a caller-owned hipStream_t.
 *   ms_set_stream(ctx, s)   from now on the context works on `s`; NULL (0) selects the context's OWN stream.  HIP's null stream - PyTorch's default stream, whose
 *                           handle is 0 - can therefore not be named: a caller on it creates a stream and orders the two with an event.
 *   ordering at the switch  ms_set_stream is a hand-over point: everything the context enqueued before the call happens before everything it enqueues after it.  The
 *                           stream being left is drained inside the call (the calling thread waits for it, for the side stream of MS_FLAG_LATENCY and for a sharded
 *                           context's communication stream), so it must still exist then: if draining fails, the call returns MS_ERR_HIP and the context is on the
 *                           new stream all the same.  A caller's own work on the NEW stream is ordered by that stream as usual.  Naming the stream the context is
 *                           on already costs nothing.
 *   unsynchronised returns  EXACTLY these return with launches still in flight: ms_interpolate, ms_mix, ms_polys_lincomb (with MS_LAZY_LINCOMB=0; by default it
 *                           launches nothing) and ms_bench_lde.  Every other entry point returns with the context's stream idle: it has waited for what it hands to
 *                           the host, and the ones whose last launch comes behind that wait - ms_mix_cubic, ms_mix_terms, ms_mix_air, ms_mix_air_ext,
 *                           ms_aux_running_staged, ms_polys_append - synchronise once more behind it.  (Under MS_FLAG_LATENCY a stage's results are home when its
 *                           last kernel has stored them, a moment before the kernel retires.)  ms_fri_proof_read_async is asynchronous by design, on a copy stream of
 *                           the context's own, until ms_fri_proof_wait.  The effects of the four are ordered before every later call on the context, across
 *                           ms_set_stream too; a caller that needs them FINISHED - to time them - calls ms_synchronize, or records an event on ms_stream(ctx).
 *                           Before destroying a stream it lent, a caller ALWAYS moves the context off it (ms_set_stream drains it) or calls ms_synchronize.
 *                           ms_trace_upload_async queues a copy-engine transfer and touches no stream.
 *   caller's buffers        are only read or written during the call that takes them (device pointers too: ms_trace_commit_device reads `trace` on the context's
 *                           stream, behind whatever the caller enqueued there, and has finished reading when it returns).
 *   ms_synchronize(ctx)     waits for the stream the context is on NOW (after ms_set_stream: the new one; the one left was drained by the switch).
 *   ms_stream(ctx)          the hipStream_t the context is on now: the caller's, or the context's own (valid until ms_destroy).  For events and for work the caller
 *                           orders behind an unsynchronised return; NULL for a null ctx.
 * ms_destroy with work in flight on a caller's stream: call ms_synchronize first. */
int ms_set_stream(ms_ctx* ctx, void* hip_stream);
int ms_synchronize(ms_ctx* ctx);
void* ms_stream(const ms_ctx* ctx);
/* page-locked host memory for the boundary's bulk transfers (the trace going in, the FRI proof coming out): copies to and from
 * it are DMA transfers that overlap with kernels of other contexts.  NULL on failure. */
void* ms_pinned_alloc(size_t bytes);
void ms_pinned_free(void* p);

/* ---- one proof sharded over the GPUs of a node (no reference counterpart) ----
 * One process per GPU, every rank calls the SAME stage functions with the SAME inputs and gets the same
 * outputs.  Coefficient-domain work is replicated; the evaluation-domain work of every large commitment
 * (coset LDE / FRI codeword, leaf hashing, Merkle subtree) is partitioned: rank k evaluates and hashes the
 * leaf groups j = k (mod world) (a union of cosets of the evaluation domain: no data moves), then
 *   ALL_TO_ALL   of leaf digests  -> rank r owns the contiguous leaves [r*M/world, (r+1)*M/world) and builds that subtree,
 *   ALL_GATHER   of the `world` subtree roots -> every rank finishes the top log2(world) levels.
 * The query phase locates leaves by value on every rank (ALL_REDUCE_MIN of the global index: first match wins,
 * quirk Q7) and assembles the Merkle paths from their owners (ALL_REDUCE_SUM over disjoint bytes).
 * The library calls `fn` at those points with the payload in the caller-provided device buffers:
 *   ALL_TO_ALL         send = world chunks of `bytes` (chunk p goes to rank p), recv = world chunks (chunk p from rank p)
 *   ALL_GATHER         send = `bytes`, recv = world * `bytes` in rank order
 *   ALL_REDUCE_MIN_U64 / ALL_REDUCE_SUM_U8   in place on send, `bytes` in total
 *   ALL_TO_ALL_SLICE   one slice of a commitment's digest all-to-all (large commitments are hashed in MS_SHARD_SLICES slices so that the digests of a
 *                      slice travel while the next one is hashed): peer p's piece is the `bytes` at offset + p * stride of BOTH buffers, with
 *                      (offset, stride) from ms_shard_slice_layout(ctx, ..) inside the callback
 * The library has synchronised its stream before the call; `fn` returns 0 once the result is visible to the device.
 * Commitments with fewer than MS_SHARD_MIN_LEAVES (env, default 32768) leaf groups stay replicated.
 * world must be a power of two; world = 1 switches sharding off.  ms_lde_read / ms_fri_round_codeword_read
 * are not available for sharded commitments (each rank holds its part only). */
typedef enum { MS_XCHG_ALL_TO_ALL = 0, MS_XCHG_ALL_GATHER = 1, MS_XCHG_ALL_REDUCE_MIN_U64 = 2, MS_XCHG_ALL_REDUCE_SUM_U8 = 3, MS_XCHG_ALL_TO_ALL_SLICE = 4,
               MS_XCHG_GATHER = 5 } ms_xchg_op;
typedef int (*ms_exchange_fn)(void* user, int op, size_t bytes);
int ms_set_shard(ms_ctx* ctx, int rank, int world, void* d_send, void* d_recv, size_t cap_bytes, ms_exchange_fn fn, void* user);
int ms_shard_slice_layout(ms_ctx* ctx, size_t* offset, size_t* stride);
/* The production form: the library runs the four collectives itself with RCCL (ncclSend/ncclRecv in one group, ncclAllGather,
 * ncclAllReduce) ON THE CONTEXT'S STREAM - stream-ordered with the kernels on both sides, no stream synchronisation, no host
 * callback - and owns the two exchange buffers (`cap_bytes` each: 32 * leaf groups of the largest commitment / world + 4 MiB).
 * Rank 0 obtains `unique_id` (ncclGetUniqueId) with ms_rccl_unique_id and hands the 128 bytes to every rank through whatever
 * channel the caller has (bench.py: a torch.distributed broadcast); every rank then calls ms_set_shard_rccl (collective:
 * ncclCommInitRank).  librccl.so is bound at run time (dlopen; env MS_RCCL_LIB overrides the name): MS_ERR_HIP if it is absent.
 * ms_set_shard above stays as the seam for callers without RCCL (the gloo tests on the kernel-emulation build). */
int ms_rccl_unique_id(uint8_t out[128]);
int ms_set_shard_rccl(ms_ctx* ctx, int rank, int world, const uint8_t unique_id[128], size_t cap_bytes);
/* (tests: with env MS_SHARD_WORLD1=1 at ms_create, ms_set_shard / ms_set_shard_rccl accept world = 1 WITH buffers / a unique id and run the sharded code paths on that one
 * rank - every exchange a transfer to itself - so that the sharded kernels and, through ms_set_shard_rccl, the RCCL calls execute through whole proofs on one GPU.) */
/* the four collectives on a ONE-rank RCCL communicator with known payloads: checks the run-time binding (symbols, enums, the
 * by-value ncclUniqueId) and the stream ordering on a single GPU */
int ms_rccl_selftest(ms_ctx* ctx);
/* collective calls [0..3] and bytes sent [4..7] by this rank so far, per ms_xchg_op (the gather to rank 0 is counted with the all-gathers) */
int ms_shard_stats(ms_ctx* ctx, uint64_t out[8]);
/* r04 - the coefficient-domain work of a sharded proof is partitioned too (env MS_SHARD_DIST=0: replicated as before): the raw-trace tree by contiguous
 * leaf ranges (every rank holds the trace; only the subtree roots travel), and for every FRI round whose commitment is sharded the round polynomial BY
 * COEFFICIENT RANGE - rank k holds the coefficients [k*S, (k+1)*S), S = domain / (blowup * world): the fold is local, the DEEP quotient's suffix sums take
 * the sum over the higher ranks as carry-in (ALL_GATHER of one aggregate per rank), even(z) / odd(z) and the DEEP-ALI values of ms_eval_ext are Horner
 * combinations of the ranks' partial sums (ALL_GATHER), the trimmed length rides on the subtree-root ALL_GATHER.  The query phase computes every quotient
 * polynomial by coefficient range as well and ALL_GATHERs the ranks' slices of the proof - or, with ms_shard_proof_on_root(ctx, 1), GATHERs them to rank 0 only
 * (MS_XCHG_GATHER: send = `bytes`, rank 0's recv = world * `bytes` in rank order): ms_fri_proof_size is then 0 on the other ranks.  INTT, the constraint
 * polynomials, the mix and the commitments below MS_SHARD_MIN_LEAVES stay replicated. */
int ms_shard_proof_on_root(ms_ctx* ctx, int on);
int ms_shard_proof_is_elsewhere(const ms_ctx* ctx); /* 1 on a rank != 0 whose finished proof was assembled on rank 0 (ms_shard_proof_on_root) */
/* 1 if FRI round `round` of the current proof is worked on by coefficient range (its polynomial distributed over the ranks), 0 if it is replicated */
int ms_shard_round_is_distributed(ms_ctx* ctx, int round);

/* ---- src/util.rs:4-44, src/starks.rs:268-332 (host-only config math) ----- */
int ms_is_power_of_two(uint64_t n);
long ms_logarithm_of_two_k(uint64_t n, uint64_t base); /* -1: not a power of 2, -2: not a power of base */
uint64_t ms_ceil_log2_k(uint64_t n, uint64_t base);
int ms_num_queries(ms_field f, uint64_t security_bits, uint64_t blowup, uint64_t steps,
                   uint64_t* linking_queries, uint64_t* fri_queries_per_round); /* starks.rs:312-332 */
uint64_t ms_root_of_unity(ms_field f, uint64_t n); /* Radix2EvaluationDomain::new(n).group_gen  (TraceTable::omega, air.rs:75) */

/* ---- Stark::prove stages (src/starks.rs:59-169) --------------------------- */
/* 1.1  MerkleTree::new(trace.get_data(), lpn) -> root.  starks.rs:68-73, air.rs:15-59.
 *      `trace` is the N x w row-major matrix (N a power of two).  Also uploads the trace. */
int ms_trace_commit(ms_ctx* ctx, const uint64_t* trace_rowmajor, size_t N, size_t w, size_t lpn, uint8_t root[32]);
/*      Same, for a trace already resident in HBM (device pointer, same layout).  Elements must be canonical (< p) like the
 *      host path's; the range check runs inside the transposing kernel and the call returns MS_ERR_ARG if any element is >= p. */
int ms_trace_commit_device(ms_ctx* ctx, const void* d_trace_rowmajor, size_t N, size_t w, size_t lpn, uint8_t root[32]);
/* Optional prefetch of the NEXT proof's trace (r05): queues the copy of a page-locked (ms_pinned_alloc) row-major N x w trace into the device buffer the proof in
 * flight does not use, on an SDMA engine, and returns at once; the ms_trace_commit that later names the same pointer and shape finds the trace on the device instead
 * of waiting for the transfer.  Callable any time after the previous ms_trace_commit has returned - typically right behind it, so that the ~24 MiB travel while
 * the current proof computes.  A hint: pageable memory, MS_UPLOAD=hip or a busy engine queue nothing (MS_OK all the same) and ms_trace_commit uploads as before.
 * `trace` must stay valid and unchanged until that ms_trace_commit returns; one prefetch in flight per context (a second one waits for the first). */
int ms_trace_upload_async(ms_ctx* ctx, const uint64_t* trace_rowmajor, size_t N, size_t w);
/* BUILD-DEFINED, no reference counterpart: a column that depends on a verifier challenge - the running product of a permutation argument or the running sum of a
 * LogUp lookup - computed on the GPU from the committed trace.  Between ms_trace_commit[_device] (the trace root is in the caller's transcript, so the challenges
 * in the coefficients may depend on it; the column values are still in HBM) and ms_interpolate (which transforms them in place).
 *   K = Fp for ext = 1, otherwise the context's extension (ext = ms_ext_degree).  T_j[i] = row i of committed trace column j, canonical (MS_FLAG_TRACE_MONT64 has
 *   been undone by the transpose).  N rows, w columns.
 *   form f at row i     a_f(i) = form_const[f] + sum_{m in form_begin[f] .. form_begin[f+1]-1} term_coef[m] * T_{term_col[m]}[i]                    (in K)
 *   s_i                 sum_{k < nfrac} a_{2k}(i) / a_{2k+1}(i)  for MS_AUX_SUM,  the product of the same fractions for MS_AUX_PRODUCT
 *   the column          z_0 = the identity (0 for SUM, 1 for PRODUCT),  z_{i+1} = z_i o s_i for 0 <= i < N-1   (o: + for SUM, * for PRODUCT)
 *   final_out           z_{N-1} o s_{N-1}.  If it equals the identity the recurrence also holds from row N-1 back to row 0, and the caller's transition
 *                       constraint needs no exemption.
 * Limb l of the column becomes column w + ms_aux_count_before + l of the context and ms_aux_count grows by ext.  ms_interpolate then transforms w + ms_aux_count
 * columns and ms_polys_count is that number afterwards; ms_polys_lincomb, ms_lde_commit, ms_mix_*, ms_eval_ext and ms_poly_read treat the new columns like any
 * other (they are materialised columns, never lazy ones).  ms_trace_commit resets the count.  Several calls per proof are allowed, up to 16 limb columns in all.
 * With ms_aux_count == 0 nothing that existed before this stage changes by a bit.  column_out, when not NULL, receives the column row-major (N * ext limbs).
 * The recurrence and z_0 are ordinary constraints of ms_mix_air (mini_stark_amd.aux_constraints writes them out); msh_air_expected_validity checks them on the
 * verifying side.
 * SOUNDNESS.  ext = 1 puts the challenges in Fp: the argument is then only |Fp|-sound - what the base-field `r` of the mix stages gives today - which for BabyBear
 * is 31 bits: use ext = 4 there, and draw the composition challenge from the extension as well (ms_mix_air_ext below).  Binding the trace columns of the LDE tree to the trace root stays the caller's linking step, as before.
 *   MS_ERR_STATE  no committed trace; ms_interpolate already called for this trace; a context with sharding on (ms_set_shard* with world > 1, or MS_SHARD_WORLD1).
 *   MS_ERR_ARG    a null argument (column_out may be null, final_out may not); op > 1; ext not in {1, ms_ext_degree}; nfrac outside 1..4; form_begin not starting at 0 or
 *                 decreasing; more than 16 terms in a form; a column >= w; a non-canonical limb; more than 16 limb columns in all.
 *   MS_ERR_SHAPE  a denominator is zero on some row: the caller draws another challenge.  Decided on the device; the flag word rides back with final_out.
 *   MS_ERR_NOMEM / MS_ERR_HIP as everywhere.
 * After any refusal or failure the context is as if the call had not been made: the count is unchanged, a following valid call gives what a fresh context gives, and
 * proving without aux columns gives the usual proof.  Everything except the zero denominator is decided before anything is launched.  Tests: tests/test_aux_*.py. */
#define MS_AUX_SUM 0u      /* z_{i+1} = z_i + s_i, z_0 = 0  (LogUp)            */
#define MS_AUX_PRODUCT 1u  /* z_{i+1} = z_i * s_i, z_0 = 1  (grand product)    */
typedef struct ms_aux {
  uint32_t op;                 /* MS_AUX_SUM / MS_AUX_PRODUCT */
  uint32_t ext;                /* 1: column and coefficients in the base field; ms_ext_degree(ctx): in the extension (ext limbs per element, limb order as everywhere in this header) */
  uint32_t nfrac;              /* 1..4 fractions per row */
  const uint32_t* form_begin;  /* 2*nfrac + 1, starts at 0, does not decrease: form 2k is the numerator of fraction k, form 2k+1 its denominator; at most 16 terms per form */
  const uint32_t* term_col;    /* nterms: a TRACE column, < w */
  const uint64_t* term_coef;   /* nterms * ext limbs, canonical */
  const uint64_t* form_const;  /* 2*nfrac * ext limbs, canonical */
} ms_aux;
int ms_aux_running(ms_ctx* ctx, const ms_aux* aux, uint64_t* final_out /* ext limbs */, uint64_t* column_out /* NULL, or N*ext limbs, row-major */);
int ms_aux_count(const ms_ctx* ctx);   /* limb columns appended since the last ms_trace_commit */
/* BUILD-DEFINED: the same column, built AFTER the main columns are committed - the first half of the staged LDE commitment (ms_lde_commit_stage below).  In a proof
 * whose statement is bound by the LDE root, the challenges of a permutation or lookup argument must be drawn behind that root; ms_aux_running is over by then.
 * Same descriptor, same argument checks (term_col < w names TRACE columns: the polynomials 0 .. w-1; the limit of 16 limb columns counts the columns of both entry
 * points since ms_trace_commit), same MS_ERR_SHAPE for a zero denominator.
 *   valid        while an unsharded LDE tree is live (ms_lde_commit, and no ms_polys_* / ms_bench_lde since), before ms_lde_commit_stage for that tree, and while no
 *                validity polynomial exists (no mix stage since ms_trace_commit: it lies behind the polynomials, where the new ones go).  Otherwise MS_ERR_STATE;
 *                MS_ERR_STATE on a context with sharding on, as ms_tree_open.
 *   definition   final_out and column_out are exactly what ms_aux_running returns for the same descriptor on the same trace, and the ext new polynomials - indices
 *                ms_polys_count_before .. + ext - 1, materialised - are what ms_interpolate makes of that column.  ms_polys_count grows by ext, ms_aux_staged_count too.
 *   how          the trace polynomials the forms name are evaluated on the trace domain again (one forward size-N transform per maximal run of named columns, into a
 *                scratch buffer), ms_aux_running's launches run over that scratch, one inverse transform of the ext columns writes the polynomials.
 * The LDE tree, the LDE matrix, MS_TREE_LDE openings and ms_lde_read of the c0 committed columns are untouched.  While ms_aux_staged_count != 0 the new polynomials are
 * in no tree: ms_mix, ms_mix_cubic, ms_mix_terms, ms_mix_air, ms_mix_air_ext and ms_validity_commit return MS_ERR_STATE ("uncommitted staged columns");
 * ms_air_check, ms_poly_read, ms_tree_open of the trees that exist, ms_polys_lincomb / ms_polys_append (which kill the LDE as always) and a full ms_lde_commit (all
 * columns in one tree, as always; the stage is cleared) work.  After any refusal or failure the context is as if the call had not been made; everything but the zero
 * denominator is decided before the first launch.  Tests: tests/test_staged_*.py. */
int ms_aux_running_staged(ms_ctx* ctx, const ms_aux* aux, uint64_t* final_out /* ext limbs */, uint64_t* column_out /* NULL, or N*ext limbs, row-major */);
int ms_aux_staged_count(const ms_ctx* ctx);   /* limb columns ms_aux_running_staged appended and no tree covers yet: 0 after ms_lde_commit_stage, ms_lde_commit, ms_trace_commit */
/* 1.2a TraceTable::get_trace_polys: per-column INTT.  air.rs:147-160. */
int ms_interpolate(ms_ctx* ctx);
/* 1.2b constraint polynomial appended as sum_t scalars[t] * poly[idx[t]] (the
 *      closures of tests/e2e_goldilocks.rs:48-59 are such combinations), or
 *      uploaded verbatim (N canonical coefficients).  air.rs:127-144. */
int ms_polys_lincomb(ms_ctx* ctx, const uint64_t* scalars, const int* idx, int k);
int ms_polys_append(ms_ctx* ctx, const uint64_t* coeffs, size_t n);
int ms_polys_count(const ms_ctx* ctx);
int ms_poly_read(ms_ctx* ctx, int i, uint64_t* out /* N */);
/* 1.2c coset LDE of every constraint polynomial over Radix2(blowup*N).get_coset(shift)
 *      and MerkleTree::new over the L x c row-major LDE matrix.  starks.rs:80-95. */
int ms_lde_commit(ms_ctx* ctx, size_t blowup, uint64_t shift, size_t lpn, uint8_t root[32]);
/* BUILD-DEFINED: the second half of the staged commitment.  With c0 = the columns of the live ms_lde_commit, c1 = ms_aux_staged_count > 0 (else MS_ERR_STATE): the c1
 * pending polynomials are evaluated on the SAME coset (blowup, shift, L of that ms_lde_commit) into the columns c0 .. c0 + c1 - 1 of the LDE matrix, a SECOND tree is
 * built over the L x c1 row-major matrix of those columns alone (lpn checked as by ms_lde_commit, against L * c1 leaves) and its root returned.  Afterwards the mix
 * stages, ms_deep_*, ms_lde_read and ms_eval_ext see c0 + c1 columns; ms_tree_open(MS_TREE_LDE) goes on opening rows of c0 elements under the stage-0 root, and
 * ms_tree_open(MS_TREE_LDE_STAGED) opens rows of c1.  One stage per ms_lde_commit: a second call, and ms_aux_running_staged after it, return MS_ERR_STATE.  Whatever
 * kills the LDE tree kills the staged tree with it.  MS_ERR_STATE on a context with sharding on; MS_ERR_ARG for a null root; MS_ERR_SHAPE as ms_lde_commit for lpn.
 * After a refusal or failure the context is as if the call had not been made (the LDE matrix may have moved to a larger buffer, with its columns). */
int ms_lde_commit_stage(ms_ctx* ctx, size_t lpn, uint8_t root[32]);
int ms_lde_read(ms_ctx* ctx, uint64_t* out_rowmajor /* L*c; c = c0 + c1 once a stage is committed */);
/* ---- coset-grouped row trees (BUILD-DEFINED) ---------------------------------------------------------------------------------------------------------------
 * ms_lde_commit_coset, ms_lde_commit_stage_coset and ms_validity_commit_coset are ms_lde_commit, ms_lde_commit_stage and ms_validity_commit in every respect but the
 * tree: the transforms, the matrix in device memory, ms_lde_read, the state they set and the state they kill are the plain calls'.  With k = log_arity in 1..3 and
 * a = 2^k the tree has L / a leaf groups; group j holds, for col = 0 .. c - 1 and then t = 0 .. a - 1, column col of row j + t L / a - element col * a + t of the group
 * - where c is the number of columns of that tree (c0, c1, or the m chunk columns).  These are the LDE rows under one coset of the folded FRI's round 0
 * (ms_fri_begin_folded with the same k), so a query of a linked proof opens ONE path per tree.  Leaves are hashed as every row leaf is: one limb per element, ic = 2,
 * the context's digest and zero_as_empty; lpn = a * c.  The context remembers k per tree: ms_tree_open on such a tree opens leaf group index < L / a, with
 * leaf_index = index * a * c and the a * c values in hashed order; a later plain commit makes the tree plain again.  ms_query_linked answers MS_ERR_STATE on coset trees
 * (they do not hold one row per leaf group); ms_query_linked_folded is their query phase.
 * Refusals, all decided before anything is launched, after which the context is as if the call had not been made: MS_ERR_ARG log_arity outside 1..3; MS_ERR_SHAPE
 * L < 2a; MS_ERR_STATE a context with sharding on; MS_ERR_STATE (ms_lde_commit_coset) an LDE that would have virtual linear columns - the view has a * c "columns", the
 * specification table c, and linked proofs never have such columns; MS_ERR_STATE (ms_lde_commit_stage_coset) a live LDE tree that is not a coset tree of the same k.
 * BLAKE3: a leaf message above 1024 bytes runs the multi-chunk leaf kernels, one that may exceed 16 KiB is MS_ERR_ARG, as for every leaf group.
 * Not supported: sharded contexts, virtual columns under coset leaves.  Measured inside whole proofs only: MSLP v3 in ministark_host.h. */
int ms_lde_commit_coset(ms_ctx* ctx, size_t blowup, uint64_t shift, int log_arity, uint8_t root[32]);
int ms_lde_commit_stage_coset(ms_ctx* ctx, int log_arity, uint8_t root[32]);
int ms_validity_commit_coset(ms_ctx* ctx, int log_arity, uint8_t root[32]);
/* 1.3  validity = sum_i r^i f_i (remainder of divide_by_vanishing_poly; quirk Q1).  starks.rs:108-119. */
int ms_mix(ms_ctx* ctx, uint64_t r);
int ms_validity_read(ms_ctx* ctx, uint64_t* out /* ms_validity_len(ctx): N, 2N after ms_mix_cubic, VL after ms_mix_terms / ms_mix_air; times ms_validity_ext(ctx) limbs after ms_mix_air_ext */);
/* BUILD-DEFINED, no reference counterpart (BASELINE configs[4] "degree-3 constraints"; the reference cannot express them: its validity polynomial is the
 * remainder of divide_by_vanishing_poly, starks.rs:118-119, quirk Q1).  In place of ms_mix, with the TRUE quotient:
 *   C_t(x) = P_j(w x) - P_a(x) P_b(x) P_c(x) - s_t P_d(x)         spec[t] = {j, a, b, c, d} (polynomial indices), w = the trace domain's generator
 *   validity(x) = (sum_t r^t C_t(x)) (x - w^(N-1)) / (x^N - 1)     2N coefficients; MS_ERR_SHAPE if the division is not exact (a row 0..N-2 violates a constraint)
 * Evaluated on the LDE domain of the preceding ms_lde_commit (blowup >= 4), interpolated back.  ms_eval_ext / ms_validity_read / ms_fri_begin then work on the
 * 2N-coefficient validity polynomial.  Checked against a big-integer restatement in the tests; self-verified at full size. */
int ms_mix_cubic(ms_ctx* ctx, uint64_t r, const int* spec /* [ncons][5] */, const uint64_t* s /* [ncons] */, int ncons);
/* BUILD-DEFINED, no reference counterpart: polynomial transition constraints of ANY degree, in place of ms_mix / ms_mix_cubic, with the TRUE quotient.  The
 * constraint system is a sum of monomials over the polynomials the context holds (trace columns and whatever ms_polys_lincomb / ms_polys_append added: indices
 * < ms_polys_count), each factor at a row offset; w = the trace domain's generator:
 *   C_t(x)      = sum_{m in terms(t)} coef_m * prod_{f in factors(m)} P_{poly_f}(w^{row_f} x)          (a term without factors is the constant coef_m)
 *   validity(x) = (sum_t r^t C_t(x)) * prod_{k=1..nexempt} (x - w^(N-k)) / (x^N - 1)
 * i.e. every constraint must hold on the rows 0 .. N-1-nexempt; the last `nexempt` rows are exempt for ALL constraints.  Boundary constraints and per-constraint
 * exemptions are not part of this stage (ms_mix_air below has them).  The program is passed as CSR arrays: the terms of constraint t are term_begin[t] .. term_begin[t+1]-1, the factors of
 * term m are fac_begin[m] .. fac_begin[m+1]-1 (both arrays start at 0 and do not decrease).
 * With d = the most factors of any term, VL = N * next_pow2(max(1, d - 1)) - or, when nexempt > d - 1, next_pow2 of the ceil(((d - 1) N - d + nexempt + 1) / N)
 * slots the quotient's (d - 1) N - d + nexempt + 1 coefficients then need: afterwards ms_validity_len is VL, the validity polynomial has VL coefficients (zero
 * above its degree) and ms_validity_read / ms_eval_ext / ms_fri_begin .. ms_fri_query work on it as after ms_mix_cubic.  Evaluated pointwise on the LDE domain of
 * the preceding ms_lde_commit (L = blowup * N points), interpolated back.
 *   MS_ERR_STATE  called before ms_lde_commit; the LDE of the context is sharded over ranks.
 *   MS_ERR_ARG    a null array; ncons outside 1..4096; more than 65536 terms; a term with more than 8 factors; no term with a factor (d = 0); term_begin / fac_begin
 *                 not starting at 0 or decreasing; a polynomial index >= ms_polys_count; a row offset >= N; a coefficient or r >= p; nexempt outside 0..16.
 *   MS_ERR_SHAPE  the LDE domain cannot decide exactness: needs d (N - 1) + nexempt < L and VL + N <= L (for d = 3, nexempt = 1: blowup >= 4);
 *                 the LDE coset meets the trace domain (shift^N is a blowup-th root of unity);
 *                 the division is not exact: a constraint does not hold on a non-exempt row.
 * Everything but the last is decided before anything is launched; after any refusal the context is usable as if the call had not been made (a validity
 * polynomial of an earlier ms_mix on the same LDE may have to be recomputed).  Checked against a big-integer restatement of this definition, bit for bit
 * against ms_mix_cubic on the specs that entry can express, and by the DEEP-ALI identity at out-of-domain points (tests/test_terms_*.py);
 * msh_terms_expected_validity (ministark_host.h) is the verifying side's evaluation of the same program. */
int ms_mix_terms(ms_ctx* ctx, uint64_t r, int ncons, const uint32_t* term_begin /* ncons + 1 */, const uint64_t* coef /* nterms, canonical */,
                 const uint32_t* fac_begin /* nterms + 1 */, const uint32_t* fac_poly /* nfacs: polynomial index */,
                 const uint32_t* fac_row /* nfacs: row offset, 0 <= row < N */, int nexempt /* 0..16 */);
/* BUILD-DEFINED, no reference counterpart: ms_mix_terms completed to an AIR - an exemption set per transition constraint, periodic columns (public values that
 * repeat with a power-of-two period: round constants, selectors) and boundary constraints.  w = the generator of the N-row trace domain, P_0 .. P_{c-1} the
 * polynomials of the committed LDE (c = ms_polys_count at the preceding ms_lde_commit), L = blowup * N.
 *   periodic column k   period q_k = per_begin[k+1] - per_begin[k], a power of two, 1 <= q_k <= min(N, 256), the q_k summing to at most 4096;
 *                       K_k(x) = Q_k(x^(N/q_k)) with Q_k the polynomial of degree < q_k through Q_k((w^(N/q_k))^i) = per_val[per_begin[k] + i]: K_k(w^i) = value[i mod q_k].
 *                       The factor (MS_AIR_PERIODIC | k, row) is K_k(w^row x); for degrees it counts like a trace column (degree <= N - 1).
 *   transition t        C_t(x) = sum_m coef_m prod_f factor_f(x) as in ms_mix_terms; must vanish on every row outside its exemption set X_t =
 *                       ex_row[ex_begin[t] .. ex_begin[t+1]).  Z_t(x) = prod_{rho in X_t} (x - w^rho), e_t = |X_t|, d_t = the most factors of any of its terms.
 *   boundary b          P_{bnd_poly[b]}(w^{bnd_row[b]}) = bnd_val[b].
 *   validity(x) = sum_t r^t C_t(x) Z_t(x) / (x^N - 1)  +  sum_b r^(ncons+b) (P_{bnd_poly[b]}(x) - bnd_val[b]) / (x - w^{bnd_row[b]})
 * With nq = max(max_t (d_t (N - 1) + e_t - N + 1), N - 1 if nbound > 0, 1): VL = N * next_pow2(ceil(nq / N)).  Afterwards ms_validity_len is VL and ms_validity_read /
 * ms_eval_ext / ms_fri_begin .. ms_fri_query work on the polynomial exactly as after ms_mix_terms.  A program ms_mix_terms can express (every X_t the last nexempt
 * rows, nothing else) gives the same VL and the same outputs bit for bit (for N >= d; below that ms_mix_terms rounds VL up to d - 1 slots).
 *   MS_ERR_STATE  called before ms_lde_commit; the LDE of the context is sharded over ranks.
 *   MS_ERR_ARG    air or an array that is needed is null; r, a coefficient, a periodic value or a boundary value >= p; a limit named here exceeded; the malformed-CSR
 *                 conditions of ms_mix_terms (including "no term has a factor"); a period that is no power of two or exceeds min(N, 256); a periodic index >= nperiodic;
 *                 per_begin not starting at 0; ex_begin not starting at 0 or decreasing; an exempt row >= N or named twice in one set; more than 32 DISTINCT exemption sets; more than 16
 *                 distinct boundary rows; a boundary polynomial >= c or row >= N.
 *   MS_ERR_SHAPE  the LDE domain cannot decide exactness: needs max_t (d_t (N - 1) + e_t) < L, 2N - 2 < L when nbound > 0, and VL + N <= L;
 *                 the LDE coset meets the trace domain; the divisions are not exact: a transition constraint fails on a non-exempt row or a boundary value is wrong.
 * Everything but the last is decided before anything is launched; after any refusal the context is usable as if the call had not been made.
 * msh_air_expected_validity (ministark_host.h) is the verifying side's evaluation of the same program.  Tests: tests/test_air_*.py. */
#define MS_AIR_PERIODIC 0x80000000u
typedef struct ms_air {
  uint32_t ncons;                      /* 1..4096 transition constraints */
  const uint32_t* term_begin;          /* ncons + 1 | exactly the CSR program of ms_mix_terms, except that  */
  const uint64_t* coef;                /* nterms    | fac_poly[f] may be MS_AIR_PERIODIC | k (periodic      */
  const uint32_t* fac_begin;           /* nterms+1  | column k) in place of a polynomial index              */
  const uint32_t* fac_poly;            /* nfacs */
  const uint32_t* fac_row;             /* nfacs, 0 <= row < N */
  const uint32_t* ex_begin;            /* ncons + 1: constraint t is exempt on the rows ex_row[ex_begin[t] .. ex_begin[t+1]) */
  const uint32_t* ex_row;              /* distinct within a constraint, < N, at most 16 per constraint; may be NULL when ex_begin[ncons] == 0 */
  uint32_t nperiodic;                  /* 0..64 */
  const uint32_t* per_begin;           /* nperiodic + 1: column k has period q_k = per_begin[k+1] - per_begin[k] */
  const uint64_t* per_val;             /* its q_k values, canonical */
  uint32_t nbound;                     /* 0..4096 boundary constraints */
  const uint32_t* bnd_poly;            /* < c */
  const uint32_t* bnd_row;             /* < N; at most 16 distinct rows over all boundary constraints */
  const uint64_t* bnd_val;             /* canonical */
} ms_air;
int ms_mix_air(ms_ctx* ctx, uint64_t r, const ms_air* air);
/* BUILD-DEFINED: ms_mix_air with the combiner r in the extension K (Fp2 for Goldilocks, Fp4 for BabyBear): r = E = ms_ext_degree canonical limbs.  Same program,
 * same formula, the powers of r taken in K:
 *   validity(x) = sum_t r^t C_t(x) Z_t(x) / (x^N - 1)  +  sum_b r^(ncons+b) (P_j(x) - v_b) / (x - w^rho_b)
 * a polynomial with coefficients in K; limb l of coefficient k is sum_t (r^t)_l * q_{t,k}, q_t the base-field quotient of constraint t.  A trace that breaks a
 * constraint passes the combination with probability about (ncons + nbound) / |K| instead of / |Fp| (31 bits for BabyBear).  VL, the MS_ERR_ARG and the MS_ERR_SHAPE
 * conditions are ms_mix_air's ("the division is exact": every limb plane of the size-L interpolant has at most VL coefficients); additionally
 *   MS_ERR_ARG    r null or a limb >= p.
 *   MS_ERR_STATE  a context with sharding on (ms_set_shard* with world > 1, or MS_SHARD_WORLD1), as for ms_aux_running.
 * After any refusal the context is as if the call had not been made.  Afterwards ms_validity_len is VL (in coefficients) and ms_validity_ext is E:
 *   ms_validity_read  writes VL * E limbs, the limbs of one coefficient consecutive (as ms_fri_round_poly_read);
 *   ms_eval_ext       out[t][c] = validity(z_t) = sum_k v_k z_t^k with v_k in K, the output shape unchanged;
 *   ms_fri_begin      round 0's polynomial is the validity polynomial itself, all E limbs live (no extend_poly zero-fill), trimmed to the longest limb; the
 *                     domain rule (deg + 1) * blowup is unchanged, and so is everything behind ms_fri_begin.
 * r = (r0, 0, ..) gives ms_mix_air(r0)'s polynomial in limb 0 and zero limbs above it, and the same DEEP-ALI values, FRI roots and MSFP bytes.  A later ms_mix,
 * ms_mix_cubic, ms_mix_terms or ms_mix_air replaces the polynomial and ms_validity_ext is 1 again; ms_polys_* and ms_trace_commit clear it.
 * msh_air_expected_validity_ext (ministark_host.h) is the verifying side.  Tests: tests/test_air_ext_*.py. */
int ms_mix_air_ext(ms_ctx* ctx, const uint64_t* r /* E limbs */, const ms_air* air);
int ms_validity_ext(const ms_ctx* ctx);   /* limbs per validity coefficient: 0 no validity polynomial, 1 after ms_mix / _cubic / _terms / _air, E after ms_mix_air_ext */
/* BUILD-DEFINED, diagnostic: WHY a trace is refused.  The ms_air program of ms_mix_air evaluated on the N rows of the trace domain (not on the LDE), one streaming
 * launch.  T_j[i] = P_j(w^i) is the value of column / polynomial j on row i; the factor (j, row) is T_j[(i + row) mod N], the factor (MS_AIR_PERIODIC | k, row) is
 * per_val[per_begin[k] + ((i + row) mod q_k)]; C_t(i) = sum_m coef_m prod_f factor_f(i) in Fp.  Row i VIOLATES constraint t when C_t(i) != 0 and i is not in X_t.
 *   cons_count[t]      the number of violating rows of constraint t                       (ncons words, or NULL)
 *   cons_first_row[t]  the smallest violating row, N when there is none                   (ncons words, or NULL)
 *   bnd_got[b]         T_{bnd_poly[b]}[bnd_row[b]], the value the trace really has: boundary constraint b fails when it differs from bnd_val[b]   (nbound words, or NULL)
 *   *nfail             the transition constraints with cons_count > 0 plus the failing boundary constraints
 * Returns MS_OK whenever the check ran; the verdict is *nfail.  *nfail == 0: the same program goes through ms_mix_air / ms_mix_air_ext on this trace (their
 * domain-size conditions provided); *nfail > 0 is what those stages report as MS_ERR_SHAPE.  Counts and minima do not depend on grid, wave order or launches.
 * Valid from ms_trace_commit[_device] until the next one:
 *   before ms_interpolate  the columns are the w trace columns and the ms_aux_count running columns behind them (indices < c = w + ms_aux_count), read as they stand;
 *   after it (at any later stage: after ms_lde_commit, a refused mix stage, a finished FRI) c = ms_polys_count as it is now, ms_polys_lincomb / ms_polys_append
 *                          polynomials included (lazily defined ones are written out as by ms_poly_read); the c polynomials are evaluated on the trace domain by
 *                          one forward transform into a scratch buffer of c * N elements, which the same kernel reads.
 *   MS_ERR_STATE  no committed trace; a context with sharding on (as for ms_aux_running and ms_mix_air_ext).
 *   MS_ERR_ARG    air or nfail null; every MS_ERR_ARG condition of ms_mix_air, with c as above.  It needs no LDE: there is no MS_ERR_SHAPE.
 * Everything is decided before anything is launched.  The context is unchanged whether the call succeeds, refuses or fails: polynomials, LDE, tree, validity
 * polynomial, ms_validity_ext and the FRI state are untouched, and a proof with checks inserted anywhere is byte-identical to one without.
 * Tests: tests/test_air_check_*.py (tests/pyref_air_check.py restates the definitions). */
int ms_air_check(ms_ctx* ctx, const ms_air* air, uint64_t* nfail, uint64_t* cons_count /* ncons, or NULL */, uint64_t* cons_first_row /* ncons, or NULL */,
                 uint64_t* bnd_got /* nbound, or NULL */);
size_t ms_validity_len(const ms_ctx* ctx);
/* 2.   DEEP-ALI: out[t][i] = f_i(z_t) for the c constraint polys, out[t][c] = validity(z_t);
 *      z: q*E limbs, out: q*(c+1)*E limbs.  starks.rs:124-151, field.rs:23-32. */
int ms_eval_ext(ms_ctx* ctx, const uint64_t* z, int q, uint64_t* out);

/* ---- Fri::prove stages (src/fri.rs:53-189) -------------------------------- */
/* commit phase, round 0: FriRound::new(extend(validity), (deg+1)*blowup).  fri.rs:73-82, 314-352.
 * (root0 is returned for inspection; the reference never writes it to the transcript.) */
int ms_fri_begin(ms_ctx* ctx, size_t blowup, size_t rounds, uint8_t root0[32]);
/* z -> B = [even(z), odd(z)] (2*E limbs).  fri.rs:89-94, 354-359. */
int ms_fri_deep(ms_ctx* ctx, const uint64_t* z, uint64_t* B);
/* alpha -> fold, DEEP quotient (folded - B(alpha))/(x - z), next FriRound, root.  fri.rs:96-109. */
int ms_fri_fold_commit(ms_ctx* ctx, const uint64_t* alpha, uint8_t root[32]);
int ms_fri_round_info(ms_ctx* ctx, int round, uint64_t* ncoef, uint64_t* domain_size);
int ms_fri_round_poly_read(ms_ctx* ctx, int round, uint64_t* out /* ncoef*E */);
int ms_fri_round_codeword_read(ms_ctx* ctx, int round, uint64_t* out /* D*E */);
/* query phase for `nq` betas (already converted from challenge bytes to u64, fri.rs:121-126).
 * Builds the serialised FriProof ("MSFP" layout below) in HBM.  fri.rs:115-189. */
int ms_fri_query(ms_ctx* ctx, const uint64_t* betas, int nq);
size_t ms_fri_proof_size(const ms_ctx* ctx);
int ms_fri_proof_read(ms_ctx* ctx, uint8_t* out);
/* The same read-back without blocking: the copy runs on the context's own copy stream behind the query phase and `out` (page-locked:
 * ms_pinned_alloc) is complete once ms_fri_proof_wait returns; the next proof's stages may be issued meanwhile - the next
 * ms_fri_query orders itself behind the copy on the device.  One read-back in flight per context. */
int ms_fri_proof_read_async(ms_ctx* ctx, uint8_t* out);
int ms_fri_proof_wait(ms_ctx* ctx);
/* how the last read-back of this context travelled: 1 = an SDMA copy engine through the HSA runtime (hsa_amd_memory_async_copy_on_engine, forced onto the engine:
 * never a blit kernel; the default for ms_fri_proof_read_async when the HSA runtime binds), 0 = the HIP runtime's copy (hipMemcpyAsync; env MS_READBACK=hip, the
 * blocking ms_fri_proof_read, or the fall-back when the engine refused the copy). */
int ms_io_engine(const ms_ctx* ctx);
/* which HSA runtime the copy engines were bound through: the path of the libhsa-runtime64 ALREADY mapped into the process (the one HIP itself runs on; the library
 * never loads a runtime of its own), "" while none is bound.  A profiled or otherwise mixed-runtime run can be recognised in its records by this. */
const char* ms_io_runtime_path(void);
/* Failure semantics of the engine copies (upload and read-back alike): an engine that refuses a copy -> this context uses the HIP runtime's copies from then on; a copy
 * the engine reports as FAILED -> done again through the HIP runtime, the call succeeds if that does; a copy that does not COMPLETE within 20 s (env
 * MS_SDMA_TIMEOUT_S) -> MS_ERR_HIP, and the context is POISONED: the engine may still be accessing the caller's buffer and the device blob, so every later entry
 * point returns MS_ERR_STATE (ms_last_error says why), nothing is reused, and only ms_destroy is valid - it waits for the transfer without limit, then frees.
 * The caller must keep its buffer alive until ms_destroy has returned. */
/* ms_fri_query with the FriProof written WHERE IT IS READ: the query-phase kernels store the MSFP blob straight into `out` - page-locked
 * host memory from ms_pinned_alloc (mapped into the device's address space) or device memory - of `cap` bytes; no read-back copy.  The
 * blob is complete when the call returns.  *len receives the blob size; with cap smaller than that nothing is computed and MS_ERR_ARG is
 * returned (out = NULL, cap = 0: size query, MS_OK).  One buffer per proof in flight on the caller's side: the library keeps no reference to
 * `out` after the call.  ms_fri_proof_read* do not apply to such a proof (MS_ERR_STATE). */
int ms_fri_query_into(ms_ctx* ctx, const uint64_t* betas, int nq, uint8_t* out, size_t cap, size_t* len);
/* MSFP layout — for each window (previous, round) in order, for each beta in order:
 *     6*E u64   x1 y1 x2 y2 x3 y3                      (FriProof.points,    fri.rs:148-154)
 *     u64 qlen, qlen*E u64 quotient coefficients       (FriProof.quotients, fri.rs:159-167)
 *     MerklePath(y1), MerklePath(y2)                   (FriProof.queries,   fri.rs:170-172)
 * MerklePath = u64 leaf_index | lpn*E u64 leaf_neighbours | u64 nlevels | nlevels*ic*32 bytes
 *              (merkle.rs:272-298; leaf located BY VALUE, first match, quirk Q7). */

/* ---- Merkle openings BY INDEX (BUILD-DEFINED; the reference opens by value only and never opens the trace or the LDE tree) ------------------------------------
 * ms_tree_open writes the MerklePaths (layout above, ic = 2) of n leaf groups of one of the trees the context holds, concatenated in request order, to `out`.
 * index[k] is a LEAF-GROUP index: the tree's leaf k hashes the lpn consecutive elements [index * lpn, (index + 1) * lpn) of the committed vector (for the trace and
 * the LDE tree committed with lpn = the number of columns that is row `index`; for a FRI round tree, lpn = 2, it is the codeword positions 2 index and 2 index + 1).
 * The path's leaf_index word is index[k] * lpn, its leaf_neighbours are the group's lpn elements (E limbs each for a FRI tree, one otherwise).  A linear LDE column
 * that is never written to memory is opened with the value that was hashed.  Duplicate and unsorted indices are allowed.  Every path of one call has the same size;
 * *len receives n times that.  out = NULL with cap = 0 is a size query (MS_OK, nothing launched); cap < *len returns MS_ERR_ARG and computes nothing.
 *   MS_TREE_TRACE  valid from ms_trace_commit[_device] until ms_interpolate: the rows are transformed in place there, afterwards the call returns MS_ERR_STATE
 *                  (the tree covers the w trace columns; running columns of ms_aux_running are not in it).
 *   MS_TREE_LDE    valid from ms_lde_commit until the next ms_trace_commit, ms_polys_lincomb / ms_polys_append, ms_bench_lde or ms_lde_commit.
 *   MS_TREE_VALIDITY  the tree of ms_validity_commit (below), opened exactly as MS_TREE_LDE: row `index`, m one-limb neighbours.  Valid while that tree lives.
 *   MS_TREE_LDE_STAGED  the tree of ms_lde_commit_stage, opened exactly as MS_TREE_LDE: row `index`, c1 one-limb neighbours, leaf_index = index * lpn.  MS_ERR_STATE
 *                  while no staged tree lives.
 *   MS_TREE_FRI    round < the rounds committed so far, from ms_fri_begin on (until the next mix stage or trace).  `round` is 0 for the other trees.
 * Errors, all decided before anything is launched (ONE launch per call, on the context's stream; the call returns with the bytes in `out`):
 *   MS_ERR_ARG           null index or len; n outside 1..65536; an unknown tree id; round out of range; out = NULL with cap != 0; cap too small.
 *   MS_ERR_OUT_OF_RANGE  an index at or above the number of leaf groups.
 *   MS_ERR_STATE         the tree does not exist (yet, or any more); a context with sharding on (ms_set_shard* with world > 1, or MS_SHARD_WORLD1), as ms_aux_running.
 * The context is unchanged: a proof with such calls between its stages comes out byte for byte as without them. */
typedef enum { MS_TREE_TRACE = 0, MS_TREE_LDE = 1, MS_TREE_FRI = 2, MS_TREE_VALIDITY = 4, MS_TREE_LDE_STAGED = 5 } ms_tree_id;   /* 3 stays unassigned: it has always been refused as an unknown id (MS_ERR_ARG), and callers may rely on that */
int ms_tree_open(ms_ctx* ctx, int tree, int round /* MS_TREE_FRI only, else 0 */, const uint64_t* index, size_t n, uint8_t* out, size_t cap, size_t* len);
/* The COMPACT query phase: what ms_fri_query opens by value, opened by position, and nothing else.  Valid wherever ms_fri_query is (after the commit phase, before or
 * after ms_fri_query, any number of times); it leaves the FRI state, the MSFP blob and a later ms_fri_query's bytes untouched.  MS_ERR_STATE on a context with sharding
 * on.  With R rounds and D_i the domain size of round i (ms_fri_round_info; D_(i+1) = D_i / 2):
 *   b_(0,j) = betas[j] mod D_0 - a plain modulus: quirk Q6's `>` (a beta equal to D_0 stays D_0 in ms_fri_query) is NOT carried over - and b_(i+1,j) = b_(i,j) mod D_(i+1).
 *   Window i (0 <= i < R - 1), query j opens the positions b = b_(i,j) and (b + D_i / 2) mod D_i of round i's codeword in round i's tree.
 *   x1 = g_i^b, x2 = -x1, x3 = x1^2 are the verifier's to compute; they are not shipped.
 * MSFI layout, u64 little-endian words:
 *   'MSFI' (0x4946534D) | E | R | nq | D_0 | nfinal            nfinal = the last round's ncoef
 *   nfinal * E limbs                                            the last round's polynomial, in the clear
 *   for each window in order, for each beta in order:  MerklePath(first position), MerklePath(second position)
 * A path's leaf_index word is the opened POSITION (as in MSFP, where it is the position found by value: for a codeword of distinct values the two blobs' paths are
 * the same bytes); its group is position / 2 and the opened value y is leaf_neighbours[position & 1].  y3 of window i is not shipped: it is window i + 1's y1 of the
 * same query, and for the last window the final polynomial at x3.  No points, no quotients.  R = 1: header and final polynomial only.
 * What it binds (msh_fri_index_verify, ministark_host.h): every opened value to its position under the round's root, each window's fold to the next window's opened
 * value, the last fold to the final polynomial, and the final polynomial's length to D_(R-1) / blowup.  Not bound here, as in MSFP: round 0's root to the LDE tree -
 * that is the DEEP stage's part (ms_validity_commit / ms_deep_compose below, msh_deep_link_verify on the verifying side).
 * One launch whatever R and nq (openings and final polynomial together); no pass over any codeword or polynomial.  nq outside 1..4096: MS_ERR_ARG.  Size query and
 * cap rule as ms_tree_open.
 * Measured (tools/fri_index_bench.py, profiles/fri_index.json; one paired run on one MI355X, Goldilocks, 2^20 rows, blowup 8, 23 rounds, 2 queries, both phases behind
 * the same commit phase): ms_fri_query 0.370 ms per call with the blob left in HBM - 14 launches, 0.346 ms of kernel time, 67 180 512 bytes (22.2 ms with the read-back);
 * ms_fri_query_index 0.052 ms per call with the bytes at the caller - 1 launch, 0.0062 ms of kernel time, 69 040 bytes; one ms_tree_open of 64 LDE rows 0.039 ms. */
int ms_fri_query_index(ms_ctx* ctx, const uint64_t* betas, int nq, uint8_t* out, size_t cap, size_t* len);

/* ---- the composition commitment and the DEEP stage (BUILD-DEFINED; the reference runs FRI on the validity polynomial alone and ties it to nothing) -----------------
 * Notation: N rows, c = ms_polys_count at the preceding ms_lde_commit, L = blowup * N, shift and g_L the LDE coset's shift and generator, K the context's extension of
 * E limbs, ve = ms_validity_ext and VL = ms_validity_len after the mix stage, m = ve * VL / N.  All four entry points run on the context's stream and return
 * MS_ERR_STATE on a context with sharding on (ms_set_shard* with world > 1, or MS_SHARD_WORLD1), as ms_aux_running and ms_tree_open do.
 *
 * ms_validity_commit commits to the validity polynomial BEFORE the caller draws z.  The polynomial's ve limb planes of VL base-field coefficients are cut into VL / N
 * chunks of N coefficients each: chunk column k * ve + l holds the coefficients [kN, (k+1)N) of plane l, so that
 *   V(x) = sum_k x^(kN) sum_l u_l V_(k,l)(x)            u_l the l-th basis element of K in this header's limb order
 * (msh_validity_from_chunks, ministark_host.h, is this identity on the verifying side).  The stage evaluates the m chunk columns on the coset the LDE tree covers (L
 * points each), builds a Merkle tree with the context's digest over the L x m row-major matrix (lpn must equal m, one row per leaf group as for the LDE tree; ic = 2)
 * and returns the root.  The chunk LDE and the nodes stay in HBM; ms_tree_open(MS_TREE_VALIDITY) opens rows of it.  Valid after any mix stage (ms_mix .. ms_mix_air_ext)
 * on a context with a committed LDE; the tree lives until the next mix stage, ms_polys_*, ms_lde_commit or ms_trace_commit.
 *   MS_ERR_STATE  before a mix stage; no committed LDE.      MS_ERR_ARG  a null root; lpn != m; under BLAKE3 a row whose message may exceed 16 KiB (as everywhere).
 * The validity polynomial, ms_validity_*, ms_eval_ext and a following ms_fri_begin are unchanged by the call.
 *
 * ms_deep describes the openings: npts points (the verifier's z and its shifts z * w^row, computed by the caller) and, per point, the committed polynomials opened
 * there.  F_j for j < c is polynomial j of the LDE tree, F_(c + j') for j' < m chunk column j' of the validity tree.  Entry n is position n of pt_poly; point t owns
 * the entries pt_begin[t] .. pt_begin[t+1] - 1.  Both functions below are valid from ms_validity_commit until that tree dies.
 * ms_deep_evals writes F_(pt_poly[n])(z_t) in entry order, E limbs each: what the caller sends to the verifier.  It is the evaluation path of ms_eval_ext over views
 * of the coefficient storage and changes nothing in the context (a polynomial ms_polys_lincomb defined lazily is written out first, as by ms_poly_read).
 * ms_deep_compose builds, with gamma^n the n-th power in K,
 *   A_t(x) = sum_(n in point t) gamma^n F_(pt_poly[n])(x)          N coefficients in K
 *   D(x)   = sum_t (A_t(x) - A_t(z_t)) / (x - z_t)                 degree <= N - 2
 *   D'(y)  = D(shift * y)                                          coefficient k times shift^k
 * and installs D' as the context's DEEP polynomial: N coefficients of E limbs, zero above its degree, in a buffer of its own (ms_deep_len: N while it is installed, else
 * 0).  The library needs no claimed evaluations: the remainders A_t(z_t) fall out of the divisions.  Launches: ONE streaming pass forms every A_t (each column
 * coefficient loaded once, however many points name the column), the divisions are the synthetic-division scans of the FRI quotient with the npts jobs of a level
 * in one launch (2 levels - 1 launches: levels = 1 up to 2048 coefficients, 2 up to 2^22, 3 beyond), one launch sums the quotients and scales by shift^k:
 * 1 + (2 levels - 1) + 1 launches, 3 / 5 / 7.  A second ms_deep_compose replaces the polynomial; whatever kills the validity tree clears it.
 * While a DEEP polynomial is installed, ms_fri_begin starts round 0 from D' in place of the validity polynomial (all E limbs live, trimmed by the usual degree scan,
 * the domain rule (deg + 1) * blowup unchanged).  Everything behind it - ms_fri_deep, ms_fri_fold_commit, ms_fri_query, ms_fri_query_index, ms_tree_open(MS_TREE_FRI),
 * ms_grind - is untouched, and without ms_deep_compose ms_fri_begin and every blob are byte for byte what they were.  With the FRI blowup equal to the LDE's,
 * D_0 = next_pow2(ncoef * blowup) <= L and round-0 position b is LDE row b * (L / D_0): D'(g_0^b) = D(shift * g_L^(b L / D_0)).
 *   MS_ERR_STATE  no validity tree.
 *   MS_ERR_ARG    a null argument; npts outside 1..8; pt_begin not starting at 0 or decreasing; a point without entries; more than 8192 entries; an index >= c + m;
 *                 a limb >= p.
 *   MS_ERR_SHAPE  some z_t lies in the LDE coset (z_t^L = shift^L): the verifier would divide by zero at one of its rows.
 * All decided before anything is launched; after any refusal the context is as if the call had not been made.
 * WHAT THIS BINDS (msh_deep_link_verify, ministark_host.h): at every FRI query position, the value round 0's tree opens to the rows the LDE tree and the validity tree
 * open there and to the claimed evaluations - so the low-degree test speaks about the committed polynomials, the claimed evaluations are theirs, and V was fixed
 * before z.  WHAT IT LEAVES TO THE CALLER: the transcript order (trace root, LDE root, r, validity root, z, evaluations, gamma, the FRI rounds - each challenge drawn
 * after what it must not depend on); the AIR identity at z (msh_air_expected_validity[_ext] against msh_validity_from_chunks); msh_fri_index_verify on the same MSFI;
 * and linking the trace tree to the LDE tree's trace columns, as before.  Tests: tests/test_deep_*.py (tests/pyref_deep.py restates the definitions). */
typedef struct ms_deep {
  uint32_t npts;              /* 1..8 points */
  const uint64_t* z;          /* npts * E limbs, canonical: the verifier's z and its shifts z*w^row, computed by the caller */
  const uint32_t* pt_begin;   /* npts + 1, starts at 0, does not decrease, at most 8192 entries in all */
  const uint32_t* pt_poly;    /* entry n: F index. j < c: polynomial j of the LDE tree; c + j', j' < m: chunk column j' of the validity tree */
} ms_deep;
int ms_validity_commit(ms_ctx* ctx, size_t lpn, uint8_t root[32]);
int ms_deep_evals(ms_ctx* ctx, const ms_deep* deep, uint64_t* evals /* entries * E limbs: F_{pt_poly[n]}(z_t), entry order */);
int ms_deep_compose(ms_ctx* ctx, const ms_deep* deep, const uint64_t* gamma /* E limbs */);
int ms_deep_len(const ms_ctx* ctx);   /* 0, or N once a DEEP polynomial is installed */
/* The WHOLE query phase of a linked proof in one call and ONE launch: what ms_fri_query_index(betas), ms_tree_open(MS_TREE_LDE) and ms_tree_open(MS_TREE_VALIDITY) at
 * the rows under round 0's positions return, in one blob - one job upload, one launch, one read-back, one stream synchronisation in place of three of each.
 * Valid when the FRI commit phase is finished, a DEEP polynomial is installed (ms_deep_len != 0, so the validity tree lives), both row trees hold one row per leaf
 * group, and round 0's domain satisfies D_0 | L, D_0 <= L (ms_fri_begin with the LDE's blowup); otherwise MS_ERR_STATE.  MS_ERR_STATE on a context with sharding on, as
 * ms_tree_open.  MS_ERR_ARG, the size query (out = NULL, cap = 0) and the cap rule as ms_fri_query_index: null betas or len, out = NULL with cap != 0, nq outside
 * 1..4096, cap too small (*len is set).  Everything is decided before anything is launched, and the context is unchanged: a later ms_fri_query, ms_fri_query_index or
 * ms_tree_open returns the bytes it returns without the call.
 * MSLQ layout, u64 little-endian words:
 *   'MSLQ' (0x514C534D) | len_msfi | len_lde | len_val          the three sections' lengths in bytes
 *   MSFI blob           exactly the bytes ms_fri_query_index(betas) returns (its own header included)
 *   LDE openings        exactly the bytes ms_tree_open(MS_TREE_LDE, 0, rows) returns
 *   validity openings   exactly the bytes ms_tree_open(MS_TREE_VALIDITY, 0, rows) returns
 * rows: the 2 * nq rows msh_deep_link_verify expects - with b_j = betas[j] mod D_0 and p_j = b_j * (L / D_0), query j contributes p_j, then (p_j + L / 2) mod L, in
 * query order.  The equality with the three calls is the definition (tests/test_linked_*.py hold the bytes to it).  A virtual linear LDE column opens with the value
 * that was hashed, as in ms_tree_open.  Not measured on the device yet (tools/linked_bench.py, profiles/linked.json).
 * With a live staged tree (ms_lde_commit_stage) the call writes the STAGED layout instead - still one job table, one launch, one read-back, one synchronisation; it
 * also needs the staged tree to hold one row per leaf group (lpn = c1), else MS_ERR_STATE.  Without a staged tree the bytes are the ones above.
 *   'MSLS' (0x534C534D) | len_msfi | len_lde | len_stg | len_val
 *   MSFI blob | ms_tree_open(MS_TREE_LDE, 0, rows) | ms_tree_open(MS_TREE_LDE_STAGED, 0, rows) | ms_tree_open(MS_TREE_VALIDITY, 0, rows)       the same rows */
int ms_query_linked(ms_ctx* ctx, const uint64_t* betas, int nq, uint8_t* out, size_t cap, size_t* len);

/* ---- folded FRI: arity 2, 4 or 8, one coset per leaf, one path per round (BUILD-DEFINED; the reference folds by 2, with a DEEP quotient in every round) ------------
 * Arity a = 2^k, k = log_arity in {1, 2, 3}, fixed for one FRI; K the context's extension of E limbs.  Round i has the codeword c_i on the subgroup <g_i> of size D_i
 * in natural order, c_i[b] at g_i^b, g_i = ms_root_of_unity(field, D_i); D_(i+1) = D_i / a, g_(i+1) = g_i^a.  The domain is unshifted, as ms_fri_begin's is.
 *   Round 0   is ms_fri_begin's: the polynomial is D' while a DEEP polynomial is installed, otherwise the validity polynomial (all E limbs live after ms_mix_air_ext,
 *             else limb 0), trimmed by the usual degree scan; D_0 = next_pow2(ncoef * blowup); c_0 its transform at size D_0.
 *   Fold      for b < D_(i+1), x = g_i^b, w = g_i^(D_i / a): P the polynomial of degree < a over K with P(x w^t) = c_i[b + t D_(i+1)], t < a; c_(i+1)[b] = P(alpha_i),
 *             for any alpha_i in K.  (The split f(X) = sum_s X^s f_s(X^a) folded as sum_s alpha^s f_s.)
 *   Trees     round i's tree has D_i / a leaf groups; group j holds c_i[j + t D_(i+1)], t = 0 .. a - 1, in that order, E limbs each, hashed as every FRI leaf is
 *             (ic = 2, the context's digest and zero_as_empty).  The two, four or eight points of a fold share ONE leaf.
 *   Schedule  with R >= 1 folds the rounds 0 .. R - 1 are committed; c_R is not: its inverse transform, the final polynomial, is shipped in the clear with exactly
 *             nfinal = D_R / blowup coefficients.  Hence a^R <= D_0 / blowup.  Transcript order (the caller's): root 0, alpha_0, root 1, .., root R - 1, alpha_(R-1),
 *             final polynomial, (grind,) betas - one host round trip per round.
 *   Positions b_(0,j) = betas[j] mod D_0, b_(i+1,j) = b_(i,j) mod D_(i+1).  In round i query j opens the single leaf group b_(i+1,j): the coset that holds position
 *             b_(i,j), in its slot b_(i,j) / D_(i+1).
 * ms_fri_begin_folded is valid exactly where ms_fri_begin is and puts the FRI state into FOLDED MODE.  MS_ERR_ARG: log_arity outside 1..3, a null root, a blowup that
 * is zero or no power of two.  MS_ERR_SHAPE: D_0 above the field's two-adicity, or D_0 < a * blowup (no fold possible).  MS_ERR_STATE: no validity polynomial, or a
 * context with sharding on (as ms_tree_open).
 * ms_fri_fold_folded(alpha, root) folds the last committed round at alpha (E canonical limbs) and commits the result as the next round: one launch of the fold kernel
 * and the tree over the coset view - no coefficient side, no scan, no side stream.  It needs D_(i+1) >= a * blowup, so that a final fold stays possible: else
 * MS_ERR_SHAPE.
 * ms_fri_fold_final(alpha, coeffs, cap, n) folds once more, into a codeword that is not committed, inverse-transforms it and writes the nfinal * E limbs of the final
 * polynomial (coefficient-major) to coeffs; *n = nfinal.  cap counts u64 words.  Size query: coeffs = NULL with cap = 0 sets *n and computes nothing; cap below
 * nfinal * E: MS_ERR_ARG with *n set.  A coefficient at or above nfinal that is not zero: MS_ERR_SHAPE - round 0 was not of the degree its domain assumes; the call
 * may be repeated.  The polynomial stays on the device for the query phase.  After it, ms_fri_fold_folded and a second ms_fri_fold_final return MS_ERR_STATE.
 * ms_fri_query_folded is valid after ms_fri_fold_final, any number of times, and leaves the context unchanged: ONE launch, R * nq openings and the final polynomial.
 * nq outside 1..4096: MS_ERR_ARG.  Size query and cap rule as ms_fri_query_index.  MSFF layout, u64 little-endian words:
 *   'MSFF' (0x4646534D) | E | k | R | nq | D_0 | nfinal
 *   nfinal * E limbs                                                  the final polynomial
 *   for round i = 0 .. R - 1, for query j in order:                   MerklePath of leaf group b_(i+1,j) of round i
 * Each path is, by definition, the bytes ms_tree_open(MS_TREE_FRI, i, [b_(i+1,j)]) returns.  Verifying side: msh_fri_folded_verify (ministark_host.h).  Round 0's
 * values are bound to nothing by the MSFF alone, as in MSFI: ms_query_linked_folded and msh_deep_link_verify_folded bind them to the coset row trees.
 * Mode rules.  In folded mode ms_fri_deep, ms_fri_fold_commit, ms_fri_query[_into], ms_fri_proof_read[_async], ms_fri_proof_wait, ms_fri_query_index, ms_query_linked
 * and ms_fri_round_poly_read return MS_ERR_STATE (ms_fri_proof_size is 0); outside it the three fold and query calls above do.  Either ms_fri_begin* starts afresh,
 * and whatever clears the FRI state (a mix stage, ms_trace_commit, ms_set_shard) clears the mode with it.  In folded mode ms_fri_round_info(i) reports D_i and, as
 * ncoef, the bound D_i / blowup; ms_fri_round_codeword_read(i) reads the committed rounds; ms_tree_open(MS_TREE_FRI, i, index) opens leaf group `index`: lpn = a,
 * leaf_index = index * a, the a * E limbs of the coset as leaf_neighbours.  ms_grind is independent of all this.  Every refusal is decided before anything is launched
 * on the FRI state: after one the context is as if the call had not been made.  Without these calls every other entry point, blob and proof is byte for byte what it
 * was.
 * Measured (tools/fri_folded_bench.py, profiles/fri_folded.json; one paired run on one MI355X, Goldilocks, 2^20 rows, blowup 8, D_0 = 2^23, one context, phases
 * alternated): ms_fri_begin .. ms_fri_fold_commit (23 rounds, 45 host round trips) 4.54 ms per commit phase, 4.23 ms of kernel time; folded at arity 2 / 4 / 8
 * (R = 20 / 10 / 6; 21 / 11 / 7 round trips) 3.30 / 1.66 / 1.27 ms, 3.40 / 1.72 / 1.29 ms of kernel time.  Blob for 2 queries: MSFI 69 040 bytes, MSFF 33 992 /
 * 17 032 / 11 448; for 32 queries 1 103 920 against 542 792 / 271 432 / 181 368.  ms_fri_query_folded: one launch, 0.03-0.08 ms per call. */
int ms_fri_begin_folded(ms_ctx* ctx, size_t blowup, int log_arity, uint8_t root0[32]);
int ms_fri_fold_folded(ms_ctx* ctx, const uint64_t* alpha /* E limbs */, uint8_t root[32]);              /* commits round i + 1 */
int ms_fri_fold_final(ms_ctx* ctx, const uint64_t* alpha, uint64_t* coeffs, size_t cap /* u64 words */, size_t* n /* nfinal */);
int ms_fri_query_folded(ms_ctx* ctx, const uint64_t* betas, int nq, uint8_t* out, size_t cap, size_t* len);

/* The WHOLE query phase of a linked proof over a folded FRI (MSLP v3, ministark_host.h) in one call and ONE launch: one job table, one launch of R * nq + (2 or 3) * nq
 * openings plus the final polynomial's workgroups, one read-back, one stream synchronisation.  Valid when the context is in folded mode with ms_fri_fold_final behind
 * it, a DEEP polynomial is installed, D_0 <= L and D_0 | L, and the LDE tree, the validity tree and a live staged tree are coset trees whose k is the FRI's; otherwise
 * MS_ERR_STATE (also on a context with sharding on).  Argument rules, size query and cap rule as ms_fri_query_folded; the context is unchanged.
 * With s = L / D_0 and q_j = (betas[j] mod D_0) mod D_1, query j opens leaf group q_j * s of every row tree: round 0's coset {q_j + t D_1} lies over the LDE rows
 * q_j s + t L / a.  MSLF layout, u64 little-endian words:
 *   'MSLF' (0x464C534D) | len_msff | len_lde | len_stg (0 without a staged tree) | len_val
 *   MSFF blob            exactly the bytes ms_fri_query_folded(betas) returns
 *   LDE openings         exactly the bytes ms_tree_open(MS_TREE_LDE, 0, groups) returns
 *   staged openings      exactly the bytes ms_tree_open(MS_TREE_LDE_STAGED, 0, groups) returns, or nothing
 *   validity openings    exactly the bytes ms_tree_open(MS_TREE_VALIDITY, 0, groups) returns
 * The equality with the separate calls is the definition.  Verifying side: msh_deep_link_verify_folded binds all a slots of round 0's openings to the row trees. */
int ms_query_linked_folded(ms_ctx* ctx, const uint64_t* betas, int nq, uint8_t* out, size_t cap, size_t* len);

/* ---- proof-of-work grinding (BUILD-DEFINED; the reference has no counterpart) ---------------------------------------------------------------------------------
 * Between the last ms_fri_fold_commit and ms_fri_query a prover may spend `bits` bits of work on a nonce, and draw that many bits of security fewer from the FRI
 * queries (ms_num_queries_grind).  The transcript stays with the caller: the library is given a seed and returns the nonce.
 *   pow_ok(D, seed, nonce, bits):
 *     d    = D(seed[0..32] || nonce as 8 little-endian bytes)            a message of 40 bytes; D the context's digest (ms_digest: 0, 1, 2, 4 or 5)
 *     head = d[0..8] read as a big-endian integer
 *     true iff head < 2^(64 - bits): the digest starts with at least `bits` zero bits in byte order, most significant bit first.  bits = 0 always holds.
 * ms_grind writes the SMALLEST n in [start, start + limit) with pow_ok(D, seed, n, bits) to *nonce and returns MS_OK - the same n whatever the grid, the split into
 * launches or the scheduling - or returns MS_ERR_OUT_OF_RANGE when there is none and leaves *nonce untouched.  MS_ERR_ARG: a null pointer, bits >
 * MS_GRIND_MAX_BITS, limit == 0, start + limit > 2^64 - 1.  Valid in any state of the context: it needs no proof and changes none (a proof that grinds between
 * its last ms_fri_fold_commit and ms_fri_query comes out as it would without the call).  It runs on the context's stream.  A sharded context grinds like any other:
 * every rank computes the same nonce, nothing is exchanged.  No launch covers more than MS_GRIND_LAUNCH_MAX nonces (env, read at ms_create; default 2^30); env
 * MS_GRIND_GRID sets the workgroups of a launch (default: by the device's compute units). */
#define MS_GRIND_MAX_BITS 40u
int ms_grind(ms_ctx* ctx, const uint8_t seed[32], uint32_t bits, uint64_t start, uint64_t limit, uint64_t* nonce);
/* ms_num_queries with `grinding_bits` of the security taken by the proof of work: constrain_queries as ms_num_queries' linking_queries, fri_queries =
 * max(1, ceil(((security_bits - grinding_bits) / log2(2 / (1 + rho))) / rounds)).  MS_ERR_SHAPE for security_bits < 20 (as ms_num_queries), MS_ERR_ARG for
 * grinding_bits > min(security_bits, MS_GRIND_MAX_BITS).  grinding_bits = 0: ms_num_queries, value for value. */
int ms_num_queries_grind(ms_field f, uint64_t security_bits, uint64_t grinding_bits, uint64_t blowup, uint64_t steps,
                         uint64_t* constrain_queries, uint64_t* fri_queries);

/* ---- Tree trait (src/merkle.rs:8-30) on its own -------------------------- */
/* MerkleTree::new over `leaf_num` elements of `ext` limbs each; writes all nodes
 * (level-major, root last) if nodes_out != NULL.  ext in {1, E}. */
int ms_merkle_commit(ms_ctx* ctx, const uint64_t* leafs, size_t leaf_num, int ext, size_t lpn, size_t ic,
                     uint8_t* nodes_out, size_t nodes_cap, size_t* nnodes, uint8_t root[32]);

/* MerkleTree::generate_proof(&leaf) (src/merkle.rs:272-288): builds the tree, locates `leaf` (ext limbs) BY VALUE,
 * first match (merkle.rs:216-225), and writes the serialised MerklePath (layout above) to path_out.
 * inner_children is 2 (get_parent_idx, merkle.rs:203, is only right for binary trees — DESIGN.md quirk Q14).
 * *path_len receives the path size; MS_ERR_LEAF_NOT_FOUND if the value is not a leaf. */
int ms_merkle_prove(ms_ctx* ctx, const uint64_t* leafs, size_t leaf_num, int ext, size_t lpn, const uint64_t* leaf,
                    uint8_t* path_out, size_t cap, size_t* path_len);

/* ---- standalone transforms (NTT micro-benchmark + parity tests) ---------- */
/* `batch` vectors of n elements each, contiguous; natural order in and out. */
int ms_ntt(ms_ctx* ctx, uint64_t* data, size_t n, size_t batch, int inverse);
/* out[b][i] = P_b(shift * g_L^i): coeffs [batch][ncoef] -> out [batch][L]. */
int ms_coset_lde(ms_ctx* ctx, const uint64_t* coeffs, size_t ncoef, size_t batch, uint64_t shift, uint64_t* out, size_t L);
/* device-resident benchmark entry: runs the LDE stage of the current session again
 * (no host copies); used by bench.py to time the NTT kernels in isolation. */
int ms_bench_lde(ms_ctx* ctx, size_t blowup, uint64_t shift);
/* measurement aid: between begin/end every kernel launch is bracketed by HIP events on the
 * launching stream; end() writes a JSON object {kernel: {launches, ms, alg_bytes}} (build-defined,
 * no reference counterpart). */
/* diagnostic: out[i] = a[i] (op) b[i] computed ON THE DEVICE with the arithmetic class the NTT tiles use (Goldilocks: the exec-masked
 * inline-asm class GLM, whose gfx950 wait states are managed by hand and which no CPU build can execute; BabyBear: BB) - so that a
 * test can compare every operation with big-integer arithmetic on directed edge values.  a, b canonical.  op: 0 add, 1 sub, 2 mul,
 * 3 mul by the table form of b (mul_tw(a, to_tw(b))), 4 a * 2^32, 5 a * 2^64, 6 a * 2^(b mod 96) through the compile-time shift
 * chains of the butterflies (Goldilocks only), 7 fold: a + (b mod 2^31) * 2^64 mod p (Goldilocks only), 8 / 9 / 10 a * 2^24 / 2^48 / 2^72 and
 * 11 a * 2^(12 (b mod 8)): the multiplier-free products by 8th and 16th roots of unity of the FRI fold (GL::mul_pow2; Goldilocks only).  No reference counterpart.
 *
 * `op` = operation | class << 8.  Class 0 is as above (GLM / BB).  Goldilocks also takes class 1 = GL (compare + select: every kernel outside the NTT),
 * 2 = GLT (sign bits through v_bitop3_b32: the two-sub-round tiles), 3 = GLM; BabyBear takes class 0 only.  Operations 0-7 run under every Goldilocks class
 * that has them: GL has no mul_x32 / mul_x64 / fold_small, so class 1 refuses 4, 5 and 7, and its operation 6 is GL::mul_pow2<b mod 96>, every shift of it.
 * Further operations:
 *   12  reduce128(lo = a, hi = b) on RAW 64-bit words (no canonical check; any 128-bit value), Goldilocks classes 1 and 2 only
 *   13  a * 2^(b mod 96) through the round-1 shift form (msntt::gl_mul_pow2_v1), Goldilocks
 *   14  1 / a (Goldilocks: the addition chain gl_inv_chain; BabyBear: f_inv); 0 -> 0
 *   15  BabyBear: the table form of a RUN-TIME value, out = mul_tw(a, tw_of(b)) | from_tw(tw_of(a)) << 32  (= a b | a << 32)
 * and on extension elements (E = ms_ext_degree consecutive limbs per element, n counts limbs and is a multiple of E, a and b canonical):
 *   32  e_mul   33  e_mul_tw(a, e_to_tw(b))   34  e_add   35  e_sub   36  e_mul_base(a, b.c[0])
 *   37  BabyBear: e_mul on Fp2, every Fp4 operand read as two Fp2 values   38  BabyBear: e_mul_nr4(a) on the same pairs (b unused)
 * Operations 8-11, 13, 14 and 32-36 are GL's own code: Goldilocks class 0 or 1.  Every other combination of field, class and operation, and an n that
 * is no multiple of E for an operation >= 32, returns MS_ERR_ARG before anything is launched. */
int ms_arith_selftest(ms_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ms_profile_begin(ms_ctx* ctx);
int ms_profile_end(ms_ctx* ctx, char* json_out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
