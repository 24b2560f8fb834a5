"""Host-side mirror of the reference's prover API for the accelerated path.

Same names and argument meaning as the reference (`StarkConfig::new`,
`Stark::prove`, `TraceTable`, `StarkProof`, `FriProof` — src/starks.rs:21-57,
238-333, src/air.rs:63-161, src/fri.rs:17-30), sequencing the C-ABI stage
functions of include/ministark.h exactly where `Stark::prove`
(src/starks.rs:59-169) and `Fri::commit_phase/query_phase` (src/fri.rs:64-189)
call arkworks and `MerkleTree::new`.  All arithmetic runs on the GPU inside
libministark.so; this file only moves challenges and commitments between the
transcript and the library.

Transcript: the reference uses nimue (`IOPattern`/`Merlin` over
`DigestBridge<Sha256>`, src/fiatshamir.rs) whose source is not available here,
so `Transcript` below is a BUILD-DEFINED hash chain (over the context's digest: SHA-256, BLAKE2s-256, BLAKE3, Keccak-256 or SHA3-256) that follows the
same message ORDER (src/fiatshamir.rs:48-64,100-116) but not nimue's bytes.
A Rust caller keeps nimue and passes the challenges in.
"""
import hashlib
import struct
from dataclasses import dataclass, field as _field
from typing import List

import numpy as np

from ._native import AUX_PRODUCT, aux_constraints, aux_fractions, encode_aux, instantiate_aux
from ._native import Context, MsError, AIR_ARRAYS, air_rows, flatten_air, GOLDILOCKS, BABYBEAR, ERR_SHAPE, ERR_ARG, DIGEST_SHA256, DIGEST_BLAKE2S256, DIGEST_BLAKE3, DIGEST_KECCAK256, DIGEST_SHA3_256

_MODULUS = {GOLDILOCKS: 2**64 - 2**32 + 1, BABYBEAR: 2013265921}


def _blake2s256(data=b""):
    return hashlib.blake2s(data, digest_size=32)


class _Blake3:
    """hashlib has no BLAKE3: a hashlib-shaped object over the C++ host mirror's implementation (msh_hash of libministark_host.so, the whole specification)."""
    name, digest_size, block_size = "blake3", 32, 64

    def __init__(self, data=b""):
        self._data = bytearray(data)

    def update(self, data):
        self._data += data

    def copy(self):
        return _Blake3(self._data)

    def digest(self):
        from .host import hash_bytes   # (host.py imports this module)
        return hash_bytes(DIGEST_BLAKE3, bytes(self._data))

    def hexdigest(self):
        return self.digest().hex()


class _Keccak256(_Blake3):
    """hashlib's sha3_256 is FIPS 202; Keccak-256 with the original padding (Ethereum's) is not in hashlib: the same stand-in over msh_hash."""
    name, digest_size, block_size = "keccak256", 32, 136

    def copy(self):
        return _Keccak256(self._data)

    def digest(self):
        from .host import hash_bytes
        return hash_bytes(DIGEST_KECCAK256, bytes(self._data))


# ms_digest_id -> hash constructor: the D of `DigestBridge<D>` (fiatshamir.rs:23-46) is the D of the commitments
DIGEST_HASH = {DIGEST_SHA256: hashlib.sha256, DIGEST_BLAKE2S256: _blake2s256, DIGEST_BLAKE3: _Blake3, DIGEST_KECCAK256: _Keccak256, DIGEST_SHA3_256: hashlib.sha3_256}


class Transcript:
    """Build-defined Fiat–Shamir sponge (NOT nimue): state' = D(state || tag || data), D = SHA-256 unless `digest` (an ms_digest_id) says BLAKE2s-256, BLAKE3, Keccak-256 or SHA3-256."""

    def __init__(self, domsep: str, digest: int = DIGEST_SHA256):
        self.hash = DIGEST_HASH[digest]
        self.state = self.hash(b"mini-stark_amd/transcript/v0" + domsep.encode()).digest()
        self.prover_bytes = bytearray()  # what nimue calls the transcript ("arthur", starks.rs:160)
        self.ops = []                    # ("absorb", nbytes) / ("squeeze", nbytes): the IOPattern the reference declares (fiatshamir.rs:48-64,100-116)

    def add_bytes(self, data: bytes):
        self.ops.append(("absorb", len(data)))
        self.prover_bytes += data
        self.state = self.hash(self.state + b"A" + data).digest()

    def add_scalars(self, limbs):
        self.add_bytes(b"".join(struct.pack("<Q", int(v)) for v in limbs))

    def challenge_bytes(self, n: int, _scalars=None) -> bytes:
        self.ops.append(("squeeze_scalars", _scalars) if _scalars is not None else ("squeeze_bytes", n))
        out = b""
        ctr = 0
        while len(out) < n:
            out += self.hash(self.state + b"C" + struct.pack("<I", ctr)).digest()
            ctr += 1
        self.state = self.hash(self.state + b"R").digest()
        return out[:n]

    def challenge_scalars(self, count: int, p: int):
        raw = self.challenge_bytes(16 * count, _scalars=count)
        return [int.from_bytes(raw[16 * i:16 * i + 16], "little") % p for i in range(count)]


class TraceTable:
    """src/air.rs:63-161.  `data` is the N x w row-major matrix incl. the padding rows."""

    def __init__(self, ctx: Context, steps: int, registers: int):
        self.ctx, self.steps, self.width = ctx, steps, registers
        self.length = 1
        while self.length < steps + 1:  # Radix2EvaluationDomain::new(steps + 1), air.rs:74
            self.length <<= 1
        self.omega = ctx.root_of_unity(self.length)  # air.rs:75
        self.data = np.zeros((self.length, registers), dtype=np.uint64)
        self.transitions = []  # (scalars, idx) linear combinations of trace polys

    def add_row(self, index, row):  # air.rs:106-112
        assert len(row) == self.width and index < self.steps
        self.data[index] = row

    def add_transition_lincomb(self, scalars, idx):  # closures of tests/e2e_goldilocks.rs:48-59
        self.transitions.append((list(scalars), list(idx)))

    def constrain_number(self):  # air.rs:123-125
        return self.width + len(self.transitions)


@dataclass
class FriProof:  # src/fri.rs:17-22, serialised ("MSFP", include/ministark.h)
    blob: bytes = b""
    device_resident: bool = False


@dataclass
class StarkProof:  # src/starks.rs:21-28
    arthur: bytes
    trace_commit: bytes
    constrain_trace_commit: bytes
    constrain_queries: np.ndarray  # [q][c][E]
    validity_queries: np.ndarray   # [q][E]
    fri_proof: FriProof
    fri_roots: List[bytes] = _field(default_factory=list)

    # ---- wire format "MSSP" (build-defined: the reference derives no Serialize for StarkProof/FriProof/MerklePath)
    #   u32 magic 'MSSP' | u32 version 1 | u32 E | u32 c | u32 q | u32 rounds | u64 len(arthur) | u64 len(fri blob)
    #   trace_commit[32] | constrain_trace_commit[32] | constrain_queries q*c*E u64 | validity_queries q*E u64
    #   fri_roots rounds*32 (round 0 first; not part of the reference's StarkProof: round 0's root never reaches the transcript)
    #   arthur bytes | FriProof in the MSFP layout of include/ministark.h            (all little-endian)
    def to_bytes(self) -> bytes:
        cq = np.ascontiguousarray(self.constrain_queries, dtype="<u8")
        vq = np.ascontiguousarray(self.validity_queries, dtype="<u8")
        q, c, e = cq.shape
        if self.fri_proof.device_resident:
            raise ValueError("the FRI proof was left in HBM (read_fri_proof=False): nothing to serialise")
        head = struct.pack("<4sIIIIIQQ", b"MSSP", 1, e, c, q, len(self.fri_roots), len(self.arthur), len(self.fri_proof.blob))
        return b"".join([head, self.trace_commit, self.constrain_trace_commit, cq.tobytes(), vq.tobytes(), b"".join(self.fri_roots), self.arthur, self.fri_proof.blob])

    @staticmethod
    def from_bytes(data: bytes) -> "StarkProof":
        hs = struct.calcsize("<4sIIIIIQQ")
        magic, ver, e, c, q, rounds, la, lb = struct.unpack_from("<4sIIIIIQQ", data, 0)
        if magic != b"MSSP" or ver != 1:
            raise ValueError("not an MSSP v1 proof")
        need = hs + 64 + 8 * q * (c + 1) * e + 32 * rounds + la + lb
        if len(data) != need:
            raise ValueError(f"MSSP proof has {len(data)} bytes, header says {need}")
        pos = hs
        tc, lc = data[pos:pos + 32], data[pos + 32:pos + 64]; pos += 64
        cq = np.frombuffer(data, dtype="<u8", count=q * c * e, offset=pos).reshape(q, c, e).copy(); pos += 8 * q * c * e
        vq = np.frombuffer(data, dtype="<u8", count=q * e, offset=pos).reshape(q, e).copy(); pos += 8 * q * e
        roots = [data[pos + 32 * i:pos + 32 * i + 32] for i in range(rounds)]; pos += 32 * rounds
        arthur = data[pos:pos + la]; pos += la
        return StarkProof(arthur, tc, lc, cq, vq, FriProof(data[pos:pos + lb], device_resident=False), roots)


def encode_air(air) -> bytes:
    """msh_air_encode (include/ministark_host.h) in Python: the canonical bytes of an AIR program, from a flatten_air dict or the tuple (constraints, exempt,
    periodic, boundary): 'MSAR' | version 1 | the eight counts | the arrays in the order of the ms_air struct, little-endian."""
    if not isinstance(air, dict):
        air = flatten_air(*air)
    arr = {k: np.ascontiguousarray(air[k], dtype=t).astype("<u4" if t is np.uint32 else "<u8") for k, t in AIR_ARRAYS}
    ncons, nperiodic, nbound = int(air["ncons"]), int(air["nperiodic"]), int(air["nbound"])
    if nperiodic == 0:
        arr["per_begin"], arr["per_val"] = np.zeros(1, dtype="<u4"), np.zeros(0, dtype="<u8")
    body = b"".join(arr[k].tobytes() for k, _ in AIR_ARRAYS)
    nterms, nfacs = int(arr["term_begin"][ncons]), arr["fac_poly"].size
    return struct.pack("<10I", 0x5241534D, 1, ncons, nterms, nfacs, arr["ex_row"].size, nperiodic, arr["per_val"].size, nbound, len(body)) + body


@dataclass
class LinkedProof:
    """A linked proof, MSLP v1 (include/ministark_host.h): the header's counts, the prover's transcript bytes and the MSLQ blob of Context.query_linked."""
    e: int
    c: int
    m: int
    npts: int
    rounds: int
    nq: int
    grinding_bits: int
    N: int
    blowup: int
    arthur: bytes
    mslq: bytes

    _HEAD = "<4s8I4Q"

    def to_bytes(self) -> bytes:
        return struct.pack(self._HEAD, b"MSLP", 1, self.e, self.c, self.m, self.npts, self.rounds, self.nq, self.grinding_bits, self.N, self.blowup,
                           len(self.arthur), len(self.mslq)) + self.arthur + self.mslq

    @staticmethod
    def from_bytes(data: bytes) -> "LinkedProof":
        hs = struct.calcsize(LinkedProof._HEAD)
        if len(data) < hs:
            raise ValueError("not an MSLP v1 proof")
        magic, ver, e, c, m, npts, rounds, nq, gb, N, blowup, la, lq = struct.unpack_from(LinkedProof._HEAD, data, 0)
        if magic != b"MSLP" or ver != 1:
            raise ValueError("not an MSLP v1 proof")
        if len(data) != hs + la + lq:
            raise ValueError(f"MSLP proof has {len(data)} bytes, header says {hs + la + lq}")
        return LinkedProof(e, c, m, npts, rounds, nq, gb, N, blowup, bytes(data[hs:hs + la]), bytes(data[hs + la:]))


@dataclass
class LinkedProofV2:
    """A linked proof with running columns, MSLP v2 (include/ministark_host.h): the header's counts, the transcript bytes and the MSLS blob of Context.query_linked."""
    e: int
    c0: int
    c1: int
    m: int
    npts: int
    rounds: int
    nq: int
    grinding_bits: int
    nargs: int
    nch: int
    N: int
    blowup: int
    arthur: bytes
    msls: bytes

    _HEAD = "<4s11I4Q"

    def to_bytes(self) -> bytes:
        return struct.pack(self._HEAD, b"MSLP", 2, self.e, self.c0, self.c1, self.m, self.npts, self.rounds, self.nq, self.grinding_bits, self.nargs, self.nch, self.N,
                           self.blowup, len(self.arthur), len(self.msls)) + self.arthur + self.msls


@dataclass
class LinkedProofV3:
    """A linked proof over a folded FRI and coset-grouped row trees, MSLP v3 (include/ministark_host.h): the header's counts, the transcript bytes and the MSLF blob
    of Context.query_linked_folded."""
    e: int
    log_arity: int
    c0: int
    c1: int
    m: int
    npts: int
    folds: int
    nq: int
    grinding_bits: int
    nargs: int
    nch: int
    N: int
    blowup: int
    D0: int
    arthur: bytes
    mslf: bytes

    _HEAD = "<4s12I5Q"

    def to_bytes(self) -> bytes:
        return struct.pack(self._HEAD, b"MSLP", 3, self.e, self.log_arity, self.c0, self.c1, self.m, self.npts, self.folds, self.nq, self.grinding_bits, self.nargs, self.nch,
                           self.N, self.blowup, self.D0, len(self.arthur), len(self.mslf)) + self.arthur + self.mslf


def unflatten_air(air):
    """(constraints, exempt, periodic, boundary) as lists from a flatten_air dict"""
    tb, fb, eb = [int(x) for x in air["term_begin"]], [int(x) for x in air["fac_begin"]], [int(x) for x in air["ex_begin"]]
    cons = [[(int(air["coef"][m]), [(int(air["fac_poly"][f]), int(air["fac_row"][f])) for f in range(fb[m], fb[m + 1])]) for m in range(tb[t], tb[t + 1])]
            for t in range(int(air["ncons"]))]
    exempt = [[int(air["ex_row"][k]) for k in range(eb[t], eb[t + 1])] for t in range(int(air["ncons"]))]
    pb = [int(x) for x in air["per_begin"]] if int(air["nperiodic"]) else [0]
    periodic = [[int(air["per_val"][k]) for k in range(pb[q], pb[q + 1])] for q in range(int(air["nperiodic"]))]
    boundary = [(int(air["bnd_poly"][b]), int(air["bnd_row"][b]), int(air["bnd_val"][b])) for b in range(int(air["nbound"]))]
    return cons, exempt, periodic, boundary


class StarkConfig:
    """src/starks.rs:238-333."""

    def __init__(self, ctx: Context, security_bits: int, blowup_factor: int, steps: int, trace_columns: int, grinding_bits: int = 0):
        """grinding_bits (build-defined, default 0: the reference's proof byte for byte): that many of the security bits come from a proof of work between the
        FRI commit phase and the query phase (Context.grind) instead of from FRI queries; its nonce travels in `arthur`."""
        if grinding_bits:
            rc, cq, fq = ctx.num_queries_grind(security_bits, grinding_bits, blowup_factor, steps)
        else:
            rc, cq, fq = ctx.num_queries(security_bits, blowup_factor, steps)  # starks.rs:274-275, 312-332
        if rc == ERR_ARG:
            raise MsError(rc, "STARK Config: grinding bits exceed the security bits or MS_GRIND_MAX_BITS")
        if rc != 0:
            raise MsError(rc, "STARK Config: security bits has to be at least 20")  # starks.rs:317-320
        self.ctx = ctx
        self.grinding_bits = grinding_bits
        self.security_bits, self.blowup_factor, self.steps = security_bits, blowup_factor, steps
        self.constrain_queries, self.fri_queries = cq, fq
        self.degree = steps - 1                                        # starks.rs:276
        self.rounds = ctx.ceil_log2_k(steps * blowup_factor + 1, 2)    # starks.rs:277
        self.trace_columns = trace_columns                             # merkle_config.leafs_per_node, starks.rs:297-302
        self.domsep = "\U0001F43A"                                     # starks.rs:307


class Stark:
    def __init__(self, config: StarkConfig):
        self.cfg = config

    def prove(self, trace: TraceTable, trace_device_ptr=None, read_fri_proof=True) -> StarkProof:
        """src/starks.rs:59-169.  `trace_device_ptr`: the same matrix already resident in HBM."""
        cfg, ctx = self.cfg, self.cfg.ctx
        p, e = _MODULUS[ctx.field], ctx.e
        t = Transcript(cfg.domsep, ctx.digest)
        # 1.1 commit to the raw trace (starks.rs:68-73)
        if trace_device_ptr is not None:
            rc, trace_commit = ctx.trace_commit_device(trace_device_ptr, trace.length, trace.width, cfg.trace_columns)
        else:
            rc, trace_commit = ctx.trace_commit(trace.data, cfg.trace_columns)
        ctx.check(rc)
        t.add_bytes(trace_commit)
        # 1.2 coset LDE of the constraint polynomials + commit (starks.rs:80-95)
        (shift,) = t.challenge_scalars(1, p)
        shift = shift or 1
        ctx.check(ctx.interpolate())
        for sc, idx in trace.transitions:
            ctx.check(ctx.polys_lincomb(sc, idx))
        rc, lde_commit = ctx.lde_commit(cfg.blowup_factor, shift, cfg.trace_columns)
        ctx.check(rc)
        t.add_bytes(lde_commit)
        # 1.3 mix (starks.rs:108-119)
        (r,) = t.challenge_scalars(1, p)
        ctx.check(ctx.mix(r))
        # 2. DEEP-ALI queries (starks.rs:124-151)
        z = t.challenge_scalars(cfg.constrain_queries * e, p)
        rc, ev = ctx.eval_ext(z)
        ctx.check(rc)
        c = ctx.polys_count()
        # 3. FRI (starks.rs:155-156 -> fri.rs:53-62)
        roots = []
        rc, root0 = ctx.fri_begin(cfg.blowup_factor, cfg.rounds)  # fri.rs:73-82
        ctx.check(rc)
        roots.append(root0)
        for _ in range(1, cfg.rounds):                            # fri.rs:85-110
            zq = t.challenge_scalars(e, p)
            rc, B = ctx.fri_deep(zq)
            ctx.check(rc)
            t.add_scalars(B)
            alpha = t.challenge_scalars(e, p)
            rc, root = ctx.fri_fold_commit(alpha)
            ctx.check(rc)
            t.add_bytes(root)
            roots.append(root)
        self.last_pow = None
        if cfg.grinding_bits:                                     # build-defined: the proof of work, behind the last commitment and in front of the query positions
            seed = t.challenge_bytes(32)
            rc, nonce = ctx.grind(seed, cfg.grinding_bits)
            ctx.check(rc)
            t.add_bytes(struct.pack("<Q", nonce))
            self.last_pow = (seed, nonce)
        raw = t.challenge_bytes(8 * cfg.fri_queries)              # fri.rs:121-126
        betas = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(cfg.fri_queries)]
        rc, blob = ctx.fri_query(betas, read=read_fri_proof)
        ctx.check(rc)
        self.last_challenges = dict(shift=shift, r=r, z=z, betas=betas)
        self.last_transcript_ops = list(t.ops)
        return StarkProof(bytes(t.prover_bytes), trace_commit, lde_commit, ev[:, :c, :], ev[:, c, :],
                          FriProof(blob or b"", device_resident=not read_fri_proof), roots)


    # ---- linked proofs (build-defined; MSLP v1, v2, v3; transcript order and redraw rules: include/ministark_host.h) ---------------
    def prove_air(self, trace, air, fri_rounds: int = 0, aux=None, forced_challenges=None, log_arity: int = 0, fri_folds: int = 0):
        """msh_stark_prove_linked driven from Python: the same stages, the same transcript, the same bytes.  trace: the N x w matrix; air: a flatten_air dict or the
        tuple (constraints, exempt, periodic, boundary).  The statement: there are w polynomials of degree < N, committed under the LDE root, that satisfy `air`.
        Raises MsError(ERR_SHAPE) for a trace that violates the program.
        aux = (args, nch): a proof with running columns, MSLP v2 (msh_stark_prove_linked_aux) - args flatten_aux_arg dicts whose selectors name nch challenges;
        returns a LinkedProofV2.  forced_challenges (tests only): the columns are built from these instead of the transcript's.
        log_arity = k in 1..3: MSLP v3 (msh_stark_prove_linked_folded) - the folded FRI at arity 2^k over coset-grouped row trees, with or without aux; fri_folds = 0
        means floor(log2 N / k) folds; returns a LinkedProofV3.
        One driver for the three versions: it branches where the table above prove_linked in host/stark_host.cpp says they differ, and nowhere else."""
        cfg, ctx = self.cfg, self.cfg.ctx
        field, p, e = ctx.field, _MODULUS[ctx.field], ctx.e
        k, version = log_arity, 3 if log_arity else 1 if aux is None else 2
        args, nch = aux if aux else ([], 0)
        staged = version == 2 or bool(args)                       # running columns: challenges, a staged root, the combined program
        if not isinstance(air, dict):
            air = flatten_air(*air)
        data = np.ascontiguousarray(trace.data if isinstance(trace, TraceTable) else trace, dtype=np.uint64)
        N, w = data.shape
        blowup, L = cfg.blowup_factor, N * cfg.blowup_factor
        if k and (k not in (1, 2, 3) or (not args and nch)):
            raise MsError(ERR_ARG, "prove_air: log_arity outside 1..3, or challenges without arguments")
        R = (fri_folds or (N.bit_length() - 1) // k) if k else fri_rounds or cfg.rounds
        nq, gb = cfg.fri_queries, cfg.grinding_bits
        # the statement: its words, msh_air_encode(air), msh_aux_encode(args) where there are running columns
        t = Transcript(cfg.domsep + "/linked/v%d" % version, ctx.digest)
        words = [field, ctx.digest, N, w, blowup] + ([k] if k else []) + [R, nq, gb] + ([len(args), nch] if version > 1 else [])
        t.add_bytes(struct.pack("<%dQ" % len(words), *words))
        t.add_bytes(encode_air(air))
        if staged:
            t.add_bytes(encode_aux(args, nch))
        t.prover_bytes = bytearray()                              # the statement is the verifier's own: it does not travel
        rc, root = ctx.trace_commit(data, w)                      # the raw-trace root: absorbed first, binds nothing
        ctx.check(rc)
        t.add_bytes(root)
        (shift,) = t.challenge_scalars(1, p)
        while shift == 0 or pow(shift, L, p) == 1:                # the coset must not meet the trace domain: part of the protocol on both sides
            (shift,) = t.challenge_scalars(1, p)
        ctx.check(ctx.interpolate())
        rc, root = ctx.lde_commit_coset(blowup, shift, k) if k else ctx.lde_commit(blowup, shift, w)
        ctx.check(rc)
        t.add_bytes(root)
        ch, prog = [], air
        if staged:
            flat = t.challenge_scalars(nch * e, p)                # the arguments' challenges follow the commitment to the main columns
            ch = [tuple(int(v) for v in flat[j * e:(j + 1) * e]) for j in range(nch)]
            used = ch if forced_challenges is None or k else [tuple(c) for c in forced_challenges]   # (v2's tests force them; v3 never took them)
            cons, exempt, periodic, boundary = unflatten_air(air)
            for j, arg in enumerate(args):
                inst = instantiate_aux(field, arg, used)          # (forced challenges: column AND constraints are the forger's, so the mix stage accepts them)
                rc, final, _ = ctx.aux_running_staged(inst["op"], inst, e)
                ctx.check(rc)                                     # ERR_SHAPE: a zero denominator
                if tuple(final) != ((1 if inst["op"] == AUX_PRODUCT else 0),) + (0,) * (e - 1):
                    raise MsError(ERR_SHAPE, "prove_air: an argument does not hold (final is not the identity)")
                c2, e2, b2 = aux_constraints(field, inst["op"], aux_fractions(inst), e, w + j * e)
                cons, exempt, boundary = cons + c2, exempt + e2, boundary + b2
            rc, root = ctx.lde_commit_stage_coset(k) if k else ctx.lde_commit_stage(len(args) * e)
            ctx.check(rc)
            t.add_bytes(root)
            prog = flatten_air(cons, exempt, periodic, boundary)
        c1 = len(args) * e
        c = w + c1
        r = t.challenge_scalars(e, p)
        ctx.check(ctx.mix_air_ext(r, prog))
        m = e * ctx.validity_len() // N
        rc, root = ctx.validity_commit_coset(k) if k else ctx.validity_commit(m)
        ctx.check(rc)
        t.add_bytes(root)
        z = t.challenge_scalars(e, p)
        while not any(z[1:]):                                     # z outside the base field
            z = t.challenge_scalars(e, p)
        rows = sorted({0} | {int(x) for x in np.asarray(prog["fac_row"]).reshape(-1)})
        if len(rows) > 8:
            raise MsError(ERR_ARG, "prove_air: the program touches more than 8 row offsets")
        omega = ctx.root_of_unity(N)
        pts = [[v * pow(omega, row, p) % p for v in z] for row in rows]
        lists = [list(range(c)) + (list(range(c, c + m)) if j == 0 else []) for j in range(len(rows))]
        rc, ev = ctx.deep_evals(pts, lists)
        ctx.check(rc)
        t.add_scalars(ev.reshape(-1))
        gamma = t.challenge_scalars(e, p)
        ctx.check(ctx.deep_compose(pts, lists, gamma))
        rc, root = ctx.fri_begin_folded(blowup, k) if k else ctx.fri_begin(blowup, R)
        ctx.check(rc)
        t.add_bytes(root)                                         # round 0's root is in the transcript
        if k:                                                     # the folded commit phase: R - 1 x (alpha, root), alpha, the final polynomial
            D0 = ctx.fri_round_info(0)[1]
            for _ in range(R - 1):
                rc, root = ctx.fri_fold_folded(t.challenge_scalars(e, p))
                ctx.check(rc)                                     # ERR_SHAPE: the DEEP polynomial is so short that R folds do not fit
                t.add_bytes(root)
            rc, fin = ctx.fri_fold_final(t.challenge_scalars(e, p))
            ctx.check(rc)
            t.add_scalars(np.asarray(fin, dtype=np.uint64).reshape(-1))
        else:                                                     # the plain commit phase: R - 1 x (z, B, alpha, root)
            for _ in range(1, R):
                zq = t.challenge_scalars(e, p)
                rc, B = ctx.fri_deep(zq)
                ctx.check(rc)
                t.add_scalars(B)
                alpha = t.challenge_scalars(e, p)
                rc, root = ctx.fri_fold_commit(alpha)
                ctx.check(rc)
                t.add_bytes(root)
        if gb:
            rc, nonce = ctx.grind(t.challenge_bytes(32), gb)
            ctx.check(rc)
            t.add_bytes(struct.pack("<Q", nonce))
        raw = t.challenge_bytes(8 * nq)
        betas = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(nq)]
        self.last_challenges = dict(shift=shift, r=r, z=z, gamma=gamma, betas=betas, **(dict(ch=ch) if version > 1 else {}))
        arthur = bytes(t.prover_bytes)
        if version == 1:
            return LinkedProof(e, w, m, len(rows), R, nq, gb, N, blowup, arthur, ctx.query_linked(betas))
        if version == 2:
            return LinkedProofV2(e, w, c1, m, len(rows), R, nq, gb, len(args), nch, N, blowup, arthur, ctx.query_linked(betas))
        return LinkedProofV3(e, k, w, c1, m, len(rows), R, nq, gb, len(args), nch, N, blowup, D0, arthur, ctx.query_linked_folded(betas))

    def verify_air(self, data, air, N: int, w: int, fri_rounds: int = 0, zero_display_empty: bool = True, aux=None, log_arity: int = 0, fri_folds: int = 0) -> bool:
        """msh_stark_verify_linked on MSLP bytes (or a LinkedProof) under this configuration.  True / False, the reason of a rejection - naming the step - in
        `self.last_verify_error`; raises MsError on malformed arguments."""
        from .host import HostStark   # (host.py imports this module)
        cfg = self.cfg
        hs = HostStark(cfg.ctx, cfg.security_bits, cfg.blowup_factor, cfg.steps, cfg.trace_columns, cfg.grinding_bits)
        data = data if isinstance(data, (bytes, bytearray)) else data.to_bytes()
        if log_arity:
            rc, self.last_verify_error = hs.verify_linked_folded(data, air, N, w, log_arity, aux[0] if aux else [], aux[1] if aux else 0, fri_folds, zero_display_empty)
        elif aux is not None:
            rc, self.last_verify_error = hs.verify_linked_aux(data, air, aux[0], aux[1], N, w, fri_rounds, zero_display_empty)
        else:
            rc, self.last_verify_error = hs.verify_linked(data, air, N, w, fri_rounds, zero_display_empty)
        if rc < 0:
            raise MsError(rc, self.last_verify_error)
        return rc == 1


def fibonacci_air(ctx: Context, steps: int, secret_b: int = 2, pad_seed: int = 0x5EED) -> TraceTable:
    """The Fibonacci AIR of tests/e2e_goldilocks.rs:20-63 (w = 3, three transition closures)."""
    p = _MODULUS[ctx.field]
    tt = TraceTable(ctx, steps, 3)
    try:   # C helper of the host mirror (16 s -> 0.1 s at 2^24 rows); same values as synthetic.fibonacci_rows (tests/test_host_mirror.py)
        from .host import fibonacci_rows_native, host_library_path
        import os
        if not os.path.exists(host_library_path()):
            raise ImportError
        tt.data[:] = fibonacci_rows_native(p, tt.length, steps, secret_b, pad_seed)
    except (ImportError, OSError):
        from .synthetic import fibonacci_rows
        tt.data[:] = fibonacci_rows(p, tt.length, steps, secret_b, pad_seed)
    m1 = p - 1
    tt.add_transition_lincomb([tt.omega, m1], [0, 1])      # e2e_goldilocks.rs:48-51
    tt.add_transition_lincomb([tt.omega, m1], [0, 1])      # e2e_goldilocks.rs:53-56 (identical, quirk Q2)
    tt.add_transition_lincomb([1, m1, m1], [2, 0, 1])      # e2e_goldilocks.rs:57-59
    return tt
