"""ctypes binding of the C++ host mirror (mini-stark_amd/host/stark_host.cpp: ministark::StarkConfig /
Stark::prove / Transcript above the C ABI).  libministark_host.so contains no arithmetic: it calls the
ms_* stage functions of whichever libministark build the Context was created from."""
import ctypes as C
import os
import subprocess

import numpy as np

from ._native import Context, MsError, air_struct, flatten_air, flatten_terms
from .stark import FriProof, StarkProof

_HERE = os.path.dirname(os.path.abspath(__file__))
_HOST = None


def host_library_path():
    return os.path.join(_HERE, "libministark_host.so")


def build_host_library(force=False):
    so, src = host_library_path(), os.path.join(_HERE, "host", "stark_host.cpp")
    inc = os.path.join(os.path.dirname(_HERE), "include")
    deps = [src, os.path.join(inc, "ministark.h"), os.path.join(inc, "ministark_host.h"), os.path.join(_HERE, "csrc", "field.hpp"), os.path.join(_HERE, "csrc", "rt.hpp")]
    if not force and os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(d) for d in deps):
        return so
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return so


def _host():
    global _HOST
    if _HOST is None:
        path = host_library_path()
        if not os.path.exists(path):
            raise MsError(-6, f"{path} not found: run __graft_entry__.build()")
        from . import _native
        if not _native._LIBS:      # the mirror resolves ms_* against the libministark build loaded before it: the product's own, unless a test loaded the emulation build
            _native.load_library()
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        L.msh_stark_new.restype = C.c_void_p
        for n in ("msh_proof_arthur", "msh_proof_evals", "msh_proof_fri_roots", "msh_proof_fri_blob", "msh_proof_challenges", "msh_proof_num_polys", "msh_proof_serialize",
                  "msh_linked_proof", "msh_air_encode", "msh_aux_encode",
                  "msh_prev_proof_arthur", "msh_prev_proof_fri_roots", "msh_prev_proof_fri_blob"):
            getattr(L, n).restype = C.c_size_t
        L.msh_proof_blob_checksum.restype = C.c_uint64
        L.msh_proof_blob_sample.restype = C.c_uint64
        L.msh_hash.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p]
        L.msh_hash.restype = C.c_int
        L.msh_air_prog_new.restype = C.c_void_p
        L.msh_air_prog_new.argtypes = [C.c_void_p]
        L.msh_air_prog_air.restype = C.c_void_p
        L.msh_air_prog_air.argtypes = [C.c_void_p]
        L.msh_air_prog_free.argtypes = [C.c_void_p]
        _HOST = L
    return _HOST


def hash_bytes(digest_id: int, data: bytes) -> bytes:
    """D(data) for an ms_digest_id by the C++ mirror's own host hashes (msh_hash): SHA-256, BLAKE2s-256, BLAKE3, Keccak-256, SHA3-256 (any length)."""
    out = C.create_string_buffer(32)
    if _host().msh_hash(int(digest_id), bytes(data), len(data), out) != 0:
        raise MsError(-5, f"msh_hash: unknown digest id {digest_id}")
    return out.raw


def pow_check(digest_id: int, seed: bytes, nonce: int, bits: int) -> bool:
    """msh_pow_check: pow_ok(D, seed, nonce, bits) of include/ministark.h - D(seed || nonce as 8 little-endian bytes) starts with `bits` zero bits."""
    H = _host()
    H.msh_pow_check.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint32]
    rc = H.msh_pow_check(int(digest_id), bytes(seed), int(nonce), int(bits))
    if rc < 0 or len(seed) != 32:
        raise MsError(-5, f"msh_pow_check: unknown digest id {digest_id}, a seed that is not 32 bytes, or more than 64 bits")
    return rc == 1


def merkle_path_check_index(digest_id, field, ext, lpn, zero_display_empty, root, path, expect_leaf_group):
    """msh_merkle_path_check_index: the positional check of ONE serialised MerklePath at the head of `path` (ms_tree_open / ms_fri_query_index; ministark_host.h).
    Returns (rc, bytes used): rc 1 accepted, 0 rejected, < 0 malformed arguments."""
    H = _host()
    H.msh_merkle_path_check_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_size_t)]
    used = C.c_size_t(0)
    rc = H.msh_merkle_path_check_index(int(digest_id), int(field), int(ext), int(lpn), 1 if zero_display_empty else 0, bytes(root), bytes(path), len(path),
                                       int(expect_leaf_group), C.byref(used))
    return rc, int(used.value)


def fri_index_verify(digest_id, field, zero_display_empty, blowup, roots, z, B, alpha, betas, blob):
    """msh_fri_index_verify: the MSFI blob of Context.fri_query_index against the commit phase.  roots: the R round roots (32 bytes each); z, alpha: R - 1 elements of E
    limbs; B: R - 1 pairs of elements; betas: the query values.  Returns (rc, why): rc 1 accepted, 0 rejected, < 0 malformed arguments."""
    H = _host()
    u64p = C.POINTER(C.c_uint64)
    H.msh_fri_index_verify.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_char_p, C.c_size_t, u64p, u64p, u64p, u64p, C.c_size_t, C.c_char_p, C.c_size_t,
                                       C.c_char_p, C.c_size_t]
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))   # noqa: E731
    zz, bb, aa, be = arr(z), arr(B), arr(alpha), arr(betas)
    ptr = lambda a: a.ctypes.data_as(u64p) if a.size else None   # noqa: E731
    why = C.create_string_buffer(512)
    rc = H.msh_fri_index_verify(int(digest_id), int(field), 1 if zero_display_empty else 0, int(blowup), b"".join(bytes(r) for r in roots), len(roots), ptr(zz), ptr(bb),
                                ptr(aa), ptr(be), be.size, bytes(blob), len(blob), why, 512)
    return rc, why.value.decode()


def fri_folded_verify(digest_id, field, zero_display_empty, blowup, log_arity, roots, alpha, betas, blob):
    """msh_fri_folded_verify: the MSFF blob of Context.fri_query_folded against the commit phase.  roots: the R committed rounds' roots (32 bytes each); alpha: the R
    fold challenges of E limbs (the last one ms_fri_fold_final's); betas: the query values.  Returns (rc, why): rc 1 accepted, 0 rejected, < 0 malformed arguments."""
    H = _host()
    u64p = C.POINTER(C.c_uint64)
    H.msh_fri_folded_verify.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t, C.c_char_p, C.c_size_t,
                                        C.c_char_p, C.c_size_t]
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))   # noqa: E731
    aa, be = arr(alpha), arr(betas)
    ptr = lambda a: a.ctypes.data_as(u64p) if a.size else None   # noqa: E731
    why = C.create_string_buffer(512)
    rc = H.msh_fri_folded_verify(int(digest_id), int(field), 1 if zero_display_empty else 0, int(blowup), int(log_arity), b"".join(bytes(r) for r in roots), len(roots),
                                 ptr(aa), ptr(be), be.size, bytes(blob), len(blob), why, 512)
    return rc, why.value.decode()


def deep_link_verify(digest_id, field, zero_display_empty, N, blowup, shift, c, m, lde_root, val_root, z, lists, evals, gamma, betas, msfi, lde_open, val_open):
    """msh_deep_link_verify: FRI's round 0 (the MSFI blob) against the LDE tree and the validity tree.  z / lists as for Context.deep_evals, evals its output, gamma the
    challenge of Context.deep_compose; lde_open / val_open: Context.tree_open of TREE_LDE / TREE_VALIDITY at the rows of window 0's positions (ministark_host.h).
    Returns (rc, why): rc 1 accepted, 0 rejected, < 0 malformed arguments."""
    from ._native import deep_struct
    H = _host()
    u64p = C.POINTER(C.c_uint64)
    H.msh_deep_link_verify.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, u64p, u64p,
                                       u64p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))   # noqa: E731
    s, _keep = deep_struct(z, lists)
    ev, gg, be = arr(evals), arr(gamma), arr(betas)
    why = C.create_string_buffer(512)
    rc = H.msh_deep_link_verify(int(digest_id), int(field), 1 if zero_display_empty else 0, int(N), int(blowup), int(shift), int(c), int(m), bytes(lde_root), bytes(val_root),
                                C.addressof(s), ev.ctypes.data_as(u64p), gg.ctypes.data_as(u64p), be.ctypes.data_as(u64p), be.size, bytes(msfi), len(msfi),
                                bytes(lde_open), len(lde_open), bytes(val_open), len(val_open), why, 512)
    return rc, why.value.decode()


def deep_link_verify_folded(digest_id, field, zero_display_empty, N, blowup, shift, log_arity, c0, c1, m, lde_root, stg_root, val_root, z, lists, evals, gamma, betas,
                            msff, lde_open, stg_open, val_open):
    """msh_deep_link_verify_folded: round 0 of a folded FRI (the MSFF blob) against the coset-grouped LDE, staged and validity trees - every slot of every opened coset.
    stg_root is None and stg_open empty iff c1 = 0; the three opening sections are those of Context.query_linked_folded (ministark_host.h).
    Returns (rc, why): rc 1 accepted, 0 rejected, < 0 malformed arguments."""
    from ._native import deep_struct
    H = _host()
    u64p = C.POINTER(C.c_uint64)
    H.msh_deep_link_verify_folded.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p,
                                              C.c_char_p, C.c_void_p, u64p, u64p, u64p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                              C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))   # noqa: E731
    s, _keep = deep_struct(z, lists)
    ev, gg, be = arr(evals), arr(gamma), arr(betas)
    why = C.create_string_buffer(512)
    rc = H.msh_deep_link_verify_folded(int(digest_id), int(field), 1 if zero_display_empty else 0, int(N), int(blowup), int(shift), int(log_arity), int(c0), int(c1), int(m),
                                       bytes(lde_root), None if stg_root is None else bytes(stg_root), bytes(val_root), C.addressof(s), ev.ctypes.data_as(u64p),
                                       gg.ctypes.data_as(u64p), be.ctypes.data_as(u64p), be.size, bytes(msff), len(msff), bytes(lde_open), len(lde_open),
                                       bytes(stg_open), len(stg_open), bytes(val_open), len(val_open), why, 512)
    return rc, why.value.decode()


def validity_from_chunks(field, ve, N, z, chunk_evals):
    """msh_validity_from_chunks: V(z) from the evaluations of the m = ve * nchunks chunk columns ([m][E] limbs, chunk column k * ve + l at index k * ve + l).
    Returns (status, E limbs)."""
    u64p = C.POINTER(C.c_uint64)
    zz = np.ascontiguousarray(np.asarray(z, dtype=np.uint64).reshape(-1))
    ce = np.ascontiguousarray(np.asarray(chunk_evals, dtype=np.uint64).reshape(-1))
    out = np.zeros(zz.size, dtype=np.uint64)
    nchunks = ce.size // (zz.size * int(ve))
    rc = _host().msh_validity_from_chunks(C.c_int(field), C.c_uint32(int(ve)), C.c_uint32(nchunks), C.c_uint64(int(N)), zz.ctypes.data_as(u64p), ce.ctypes.data_as(u64p),
                                          out.ctypes.data_as(u64p))
    return rc, out


def terms_expected_validity(field, r, constraints, nexempt, N, z, rows, opened, npolys=None):
    """msh_terms_expected_validity: the value validity(z) must have after ms_mix_terms, from the opened values.  `constraints` as for Context.mix_terms (or the CSR
    5-tuple); `rows` the row offsets opened, `opened[k]` = the ms_eval_ext output at w^rows[k] z ([c + 1][E], or [c][E] with npolys = c).  Returns (status, E limbs)."""
    csr = constraints if isinstance(constraints, tuple) and len(constraints) == 5 and isinstance(constraints[0], np.ndarray) else flatten_terms(constraints)
    tb, cf, fb, fp, fr = csr
    zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1)
    e = zz.size
    op = np.ascontiguousarray(opened, dtype=np.uint64)
    rw = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    op = op.reshape(max(1, rw.size), -1)
    if npolys is None:
        npolys = op.shape[1] // e - 1          # the last entry of an ms_eval_ext row is the validity polynomial's value
    out = np.zeros(e, dtype=np.uint64)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = _host().msh_terms_expected_validity(C.c_int(field), C.c_uint64(r), C.c_int(len(tb) - 1), tb.ctypes.data_as(u32p), cf.ctypes.data_as(u64p), fb.ctypes.data_as(u32p),
                                             fp.ctypes.data_as(u32p), fr.ctypes.data_as(u32p), C.c_int(nexempt), C.c_uint64(N), zz.ctypes.data_as(u64p), C.c_int(rw.size),
                                             rw.ctypes.data_as(u32p), op.ctypes.data_as(u64p), C.c_size_t(op.shape[1]), C.c_uint32(npolys), out.ctypes.data_as(u64p))
    return rc, out


def air_expected_validity(field, r, air, N, z, rows, opened, npolys=None):
    """msh_air_expected_validity: the value validity(z) must have after ms_mix_air, from the opened values.  `air` = a flatten_air dict, or the tuple (constraints,
    exempt, periodic, boundary) of Context.mix_air; `rows` the row offsets opened (air_rows: row 0 too when there are boundary constraints), `opened[k]` = the
    ms_eval_ext output at w^rows[k] z ([c + 1][E], or [c][E] with npolys = c).  Returns (status, E limbs)."""
    if not isinstance(air, dict):
        air = flatten_air(*air)
    s, _keep = air_struct(air)
    zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1)
    e = zz.size
    op = np.ascontiguousarray(opened, dtype=np.uint64)
    rw = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    op = op.reshape(max(1, rw.size), -1)
    if npolys is None:
        npolys = op.shape[1] // e - 1          # the last entry of an ms_eval_ext row is the validity polynomial's value
    out = np.zeros(e, dtype=np.uint64)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = _host().msh_air_expected_validity(C.c_int(field), C.c_uint64(r), C.byref(s), C.c_uint64(N), zz.ctypes.data_as(u64p), C.c_int(rw.size), rw.ctypes.data_as(u32p),
                                           op.ctypes.data_as(u64p), C.c_size_t(op.shape[1]), C.c_uint32(npolys), out.ctypes.data_as(u64p))
    return rc, out


def air_expected_validity_ext(field, r, air, N, z, rows, opened, npolys=None):
    """msh_air_expected_validity_ext: air_expected_validity after ms_mix_air_ext, r = the E limbs of the combiner."""
    if not isinstance(air, dict):
        air = flatten_air(*air)
    s, _keep = air_struct(air)
    zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1)
    e = zz.size
    rr = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1)
    if rr.size != e:
        raise ValueError(f"air_expected_validity_ext: r has {rr.size} limbs, z has {e}")
    op = np.ascontiguousarray(opened, dtype=np.uint64)
    rw = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    op = op.reshape(max(1, rw.size), -1)
    if npolys is None:
        npolys = op.shape[1] // e - 1          # the last entry of an ms_eval_ext row is the validity polynomial's value
    out = np.zeros(e, dtype=np.uint64)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = _host().msh_air_expected_validity_ext(C.c_int(field), rr.ctypes.data_as(u64p), C.byref(s), C.c_uint64(N), zz.ctypes.data_as(u64p), C.c_int(rw.size),
                                               rw.ctypes.data_as(u32p), op.ctypes.data_as(u64p), C.c_size_t(op.shape[1]), C.c_uint32(npolys), out.ctypes.data_as(u64p))
    return rc, out


def _air(air):
    """(MsAir, keep-alive arrays) from a flatten_air dict or the tuple (constraints, exempt, periodic, boundary)"""
    return air_struct(air if isinstance(air, dict) else flatten_air(*air))


def air_encode(air) -> bytes:
    """msh_air_encode: the canonical bytes of an AIR program (what a linked proof's statement absorbs); b"" for a malformed program."""
    H = _host()
    s, _keep = _air(air)
    n = H.msh_air_encode(C.byref(s), None, C.c_size_t(0))
    buf = (C.c_uint8 * max(1, n))()
    H.msh_air_encode(C.byref(s), buf, C.c_size_t(n))
    return bytes(buf[:n])


class MshAuxArg(C.Structure):
    """msh_aux_arg of include/ministark_host.h"""
    _fields_ = [("op", C.c_uint32), ("nfrac", C.c_uint32), ("form_begin", C.POINTER(C.c_uint32)), ("term_col", C.POINTER(C.c_uint32)), ("term_coef", C.POINTER(C.c_uint64)),
                ("term_ch", C.POINTER(C.c_uint32)), ("form_const", C.POINTER(C.c_uint64)), ("form_ch", C.POINTER(C.c_uint32))]


def aux_args_struct(args):
    """(an array of msh_aux_arg, what it points into) from flatten_aux_arg dicts; an entry that is None becomes a NULL pointer"""
    from ._native import AUX_ARG_ARRAYS
    arr = (MshAuxArg * max(1, len(args)))()
    keep = []
    for k, a in enumerate(args):
        arr[k].op, arr[k].nfrac = int(a["op"]), int(a["nfrac"])
        for name, t in AUX_ARG_ARRAYS:
            if a.get(name) is not None:
                v = np.ascontiguousarray(a[name], dtype=t)
                keep.append(v)
                setattr(arr[k], name, v.ctypes.data_as(C.POINTER(C.c_uint64 if t is np.uint64 else C.c_uint32)))
    return arr, keep


def aux_encode(field, args, nch) -> bytes:
    """msh_aux_encode: the canonical bytes of the arguments of a linked proof with running columns; b"" for a malformed descriptor."""
    H = _host()
    arr, _keep = aux_args_struct(args)
    n = H.msh_aux_encode(C.c_int(field), arr, C.c_uint32(len(args)), C.c_uint32(nch), None, C.c_size_t(0))
    buf = (C.c_uint8 * max(1, n))()
    H.msh_aux_encode(C.c_int(field), arr, C.c_uint32(len(args)), C.c_uint32(nch), buf, C.c_size_t(n))
    return bytes(buf[:n])


def aux_constraints_native(field, air, auxes, first_poly):
    """msh_aux_constraints: `air` with the constraints of every flatten_aux dict of `auxes` appended, argument k over the polynomials first_poly + k E ..; returns
    (rc of the first refusal or 0, msh_air_encode of the program as it stands)"""
    from ._native import aux_struct
    H = _host()
    s, _keep = _air(air)
    g = H.msh_air_prog_new(C.byref(s))
    if not g:
        raise MsError(-5, "msh_air_prog_new: malformed program")
    try:
        rc = 0
        for k, aux in enumerate(auxes):
            a, _k2 = aux_struct(aux)
            rc = H.msh_aux_constraints(C.c_void_p(g), C.c_int(field), C.byref(a), C.c_uint32(first_poly + k * int(aux["ext"])))
            if rc:
                break
        view = C.c_void_p(H.msh_air_prog_air(C.c_void_p(g)))
        n = H.msh_air_encode(view, None, C.c_size_t(0))
        buf = (C.c_uint8 * max(1, n))()
        H.msh_air_encode(view, buf, C.c_size_t(n))
        return rc, bytes(buf[:n])
    finally:
        H.msh_air_prog_free(C.c_void_p(g))


def air_rows_native(air):
    """msh_air_rows: the row offsets the verifying side of an AIR program needs opened, ascending - the C twin of mini_stark_amd.air_rows."""
    s, _keep = _air(air)
    rows = (C.c_uint32 * 65536)()
    n = _host().msh_air_rows(C.byref(s), rows, C.c_int(65536))
    if n < 0:
        raise MsError(n, "msh_air_rows: malformed program")
    return [int(rows[k]) for k in range(n)]


def linked_shift_ok(field, L, shift) -> bool:
    """msh_linked_shift_ok: the linked transcript keeps a drawn shift unless it is 0 or shift^L == 1 (then it draws again)."""
    return _host().msh_linked_shift_ok(C.c_int(field), C.c_uint64(L), C.c_uint64(shift)) == 1


def linked_z_ok(field, z) -> bool:
    """msh_linked_z_ok: the linked transcript keeps a drawn z unless every limb above limb 0 is zero (then it draws again)."""
    zz = np.ascontiguousarray(z, dtype=np.uint64)
    return _host().msh_linked_z_ok(C.c_int(field), zz.ctypes.data_as(C.POINTER(C.c_uint64))) == 1


class HostStark:
    """StarkConfig::new + Stark::new + Stark::prove + Stark::verify (src/starks.rs:268-310, 40-57, 59-169, 171-235) in C++."""

    def __init__(self, ctx: Context, security_bits: int, blowup_factor: int, steps: int, trace_columns: int, grinding_bits: int = 0):
        self.H, self.ctx = _host(), ctx
        err = C.c_int(0)
        self.h = C.c_void_p(self.H.msh_stark_new(ctx.h, C.c_int(ctx.field), C.c_uint64(security_bits), C.c_uint64(blowup_factor), C.c_uint64(steps),
                                                 C.c_uint64(trace_columns), C.byref(err)))
        if not self.h.value:
            raise MsError(err.value, "STARK Config: security bits has to be at least 20")
        self.grinding_bits = grinding_bits
        if grinding_bits:   # (0: msh_stark_set_grinding is not called at all - the handle is what it always was)
            rc = self.H.msh_stark_set_grinding(self.h, C.c_uint32(grinding_bits))
            if rc != 0:
                raise MsError(rc, "STARK Config: grinding bits exceed the security bits or MS_GRIND_MAX_BITS")
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.H.msh_stark_config(self.h, C.byref(a), C.byref(b), C.byref(c))
        self.rounds, self.constrain_queries, self.fri_queries = a.value, b.value, c.value

    def __del__(self):
        try:
            if self.h is not None and self.h.value:
                self.H.msh_stark_free(self.h)
                self.h = None
        except Exception:
            pass

    def prove_raw(self, trace, trace_device_ptr=None, read_fri_proof=True):
        """Runs the proof; returns the status code only (the bench loop).  read_fri_proof: False (the FRI proof stays in HBM), True (blocking
        read-back), "async" (read-back on the copy stream; wait_proof() completes it), "into" (the query-phase kernels write the blob straight
        into the slot's page-locked buffer: ms_fri_query_into)."""
        if not hasattr(trace, "_lin"):
            k = np.array([len(i) for _, i in trace.transitions], dtype=np.int32)
            sc = np.array([v for s, _ in trace.transitions for v in s], dtype=np.uint64)
            ix = np.array([v for _, i in trace.transitions for v in i], dtype=np.int32)
            trace._lin = (k, sc, ix)
        k, sc, ix = trace._lin
        host_ptr = None if trace_device_ptr is not None else trace.data.ctypes.data_as(C.POINTER(C.c_uint64))
        return self.H.msh_stark_prove(self.h, host_ptr, C.c_void_p(trace_device_ptr), C.c_size_t(trace.length), C.c_size_t(trace.width), C.c_int(len(k)),
                                      k.ctypes.data_as(C.POINTER(C.c_int)), sc.ctypes.data_as(C.POINTER(C.c_uint64)), ix.ctypes.data_as(C.POINTER(C.c_int)),
                                      C.c_int({"async": 2, "into": 3}.get(read_fri_proof, 1 if read_fri_proof else 0)))

    def pow_nonce(self):
        """msh_proof_pow_nonce: the proof-of-work nonce of the last proof (grinding_bits > 0), None for a proof made without grinding."""
        n = C.c_uint64(0)
        return int(n.value) if self.H.msh_proof_pow_nonce(self.h, C.byref(n)) == 0 else None

    def next_trace(self, host_ptr, N, w):
        """msh_stark_next_trace: the page-locked trace of the proof after the next prove_raw - that call prefetches it (ms_trace_upload_async)."""
        self.H.msh_stark_next_trace(self.h, C.c_void_p(host_ptr), C.c_size_t(N), C.c_size_t(w))

    def blob_checksum(self, which=0):
        """FNV-1a over the FRI blob of the last (0) / previous (1) proof, read in place from its page-locked slot (msh_proof_blob_checksum)."""
        return int(self.H.msh_proof_blob_checksum(self.h, C.c_int(which)))

    def blob_sample(self, which=0, stride_bytes=4096):
        """FNV-1a over one word per `stride_bytes` of the blob (+ the last word): touches every page without reading all of it."""
        return int(self.H.msh_proof_blob_sample(self.h, C.c_int(which), C.c_size_t(stride_bytes)))

    def prev_fri_blob(self) -> bytes:
        """The FRI blob of the proof BEFORE the last one: the mirror keeps two proof slots, so it stays whole while the next proof is computed."""
        return self._bytes(self.H.msh_prev_proof_fri_blob)

    def wait_proof(self):
        """Completes an asynchronous read-back (read_fri_proof="async": the FRI proof travels into the mirror's page-locked buffer while
        the next proof is already being computed)."""
        return self.H.msh_proof_wait(self.h)

    def _bytes(self, fn):
        n = fn(self.h, None, C.c_size_t(0))
        buf = (C.c_uint8 * max(1, n))()
        fn(self.h, buf, C.c_size_t(n))
        return bytes(buf[:n])

    def last_proof(self, read_fri_proof=True) -> StarkProof:
        e = self.ctx.e
        tc, lc = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        self.H.msh_proof_commits(self.h, tc, lc)
        c = int(self.H.msh_proof_num_polys(self.h))
        n = self.H.msh_proof_evals(self.h, None, C.c_size_t(0))
        ev = np.zeros(max(1, n), dtype=np.uint64)
        self.H.msh_proof_evals(self.h, ev.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(n))
        ev = ev[:n].reshape(-1, c + 1, e)
        roots = self._bytes(self.H.msh_proof_fri_roots)
        n = self.H.msh_proof_challenges(self.h, None, C.c_size_t(0))
        ch = np.zeros(max(1, n), dtype=np.uint64)
        self.H.msh_proof_challenges(self.h, ch.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(n))
        self.last_challenges = ch[:n]
        blob = self._bytes(self.H.msh_proof_fri_blob) if read_fri_proof else b""
        return StarkProof(self._bytes(self.H.msh_proof_arthur), bytes(tc), bytes(lc), ev[:, :c, :], ev[:, c, :],
                          FriProof(blob, device_resident=not read_fri_proof), [roots[i:i + 32] for i in range(0, len(roots), 32)])

    def derive_constrains(self, trace):
        """TraceTable::derive_constrains (src/air.rs:127-144) for the verifier's copy of the AIR: the c constraint polynomials
        in coefficient form, [c][N] canonical u64 (computed on the GPU: INTT of the trace columns + the transition closures)."""
        ctx = self.ctx
        rc, _ = ctx.trace_commit(trace.data, trace.constrain_number())
        ctx.check(rc)
        ctx.check(ctx.interpolate())
        for sc, idx in trace.transitions:
            ctx.check(ctx.polys_lincomb(sc, idx))
        return np.stack([ctx.poly_read(i) for i in range(ctx.polys_count())])

    def verify(self, constrains, proof: StarkProof, zero_display_empty=True) -> bool:
        """Stark::verify (src/starks.rs:171-235, with Fri::verify src/fri.rs:191-290 and MerkleRoot::check_proof
        src/merkle.rs:312-338) on the CPU, as in the reference.  Returns True/False; the reason of a rejection is in
        `self.last_verify_error`.  Raises MsError on malformed input.
        A PARITY MIRROR of the reference's verifier, NOT a sound verifier: like the reference it takes round 0's root from the proof
        (it never enters the transcript), does not tie y3 of a window to the next window, does not check the last round polynomial
        and only degree-bounds the shipped quotients.  True means "the reference would accept" (INTEGRATION.md section 8)."""
        cs = np.ascontiguousarray(constrains, dtype=np.uint64)
        c, N = cs.shape
        ev = np.ascontiguousarray(np.concatenate([np.asarray(proof.constrain_queries, dtype=np.uint64).reshape(-1, c, self.ctx.e),
                                                  np.asarray(proof.validity_queries, dtype=np.uint64).reshape(-1, 1, self.ctx.e)], axis=1))
        roots = b"".join(proof.fri_roots)
        blob = proof.fri_proof.blob
        why = C.create_string_buffer(512)
        u8p = C.POINTER(C.c_uint8)

        def b(x):
            return C.cast(C.create_string_buffer(bytes(x), max(1, len(x))), u8p)
        self.H.msh_stark_verify.restype = C.c_int
        rc = self.H.msh_stark_verify(self.h, cs.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(c), C.c_size_t(N), b(proof.arthur), C.c_size_t(len(proof.arthur)),
                                     b(proof.trace_commit), b(proof.constrain_trace_commit), ev.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(ev.size),
                                     b(roots), C.c_size_t(len(proof.fri_roots)), b(blob), C.c_size_t(len(blob)), C.c_int(1 if zero_display_empty else 0), why, C.c_size_t(512))
        self.last_verify_error = why.value.decode()
        if rc < 0:
            raise MsError(rc, self.last_verify_error)
        return rc == 1

    def proof_bytes(self) -> bytes:
        """msh_proof_serialize: the last proof in the MSSP wire format (include/ministark_host.h), written by the C++ mirror."""
        n = self.H.msh_proof_serialize(self.h, None, C.c_size_t(0))
        if n == 0:
            raise MsError(-4, "no proof to serialise (none proved yet, or its FRI proof was left in HBM)")
        buf = (C.c_uint8 * n)()
        assert self.H.msh_proof_serialize(self.h, buf, C.c_size_t(n)) == n
        return bytes(buf)

    def verify_bytes(self, constrains, data: bytes, zero_display_empty=True) -> bool:
        """msh_stark_verify_mssp: Stark::verify straight from the wire format."""
        cs = np.ascontiguousarray(constrains, dtype=np.uint64)
        c, N = cs.shape
        why = C.create_string_buffer(512)
        self.H.msh_stark_verify_mssp.restype = C.c_int
        rc = self.H.msh_stark_verify_mssp(self.h, cs.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(c), C.c_size_t(N), data, C.c_size_t(len(data)),
                                          C.c_int(1 if zero_display_empty else 0), why, C.c_size_t(512))
        self.last_verify_error = why.value.decode()
        if rc < 0:
            raise MsError(rc, self.last_verify_error)
        return rc == 1

    def prove(self, trace, trace_device_ptr=None, read_fri_proof=True) -> StarkProof:
        self.ctx.check(self.prove_raw(trace, trace_device_ptr, read_fri_proof))
        return self.last_proof(read_fri_proof)

    # ---- linked proofs (MSLP v1; include/ministark_host.h) ----
    def prove_linked(self, trace, air, fri_rounds=0, trace_device_ptr=None) -> int:
        """msh_stark_prove_linked: the status code (ERR_SHAPE: the trace violates the program).  trace: the N x w matrix (or its shape (N, w) with
        trace_device_ptr); air: a flatten_air dict or the tuple (constraints, exempt, periodic, boundary)."""
        s, _keep = _air(air)
        if trace_device_ptr is not None:
            N, w = trace
            host_ptr = None
        else:
            t = np.ascontiguousarray(trace, dtype=np.uint64)
            N, w = t.shape
            host_ptr = t.ctypes.data_as(C.POINTER(C.c_uint64))
        return self.H.msh_stark_prove_linked(self.h, host_ptr, C.c_void_p(trace_device_ptr), C.c_size_t(N), C.c_size_t(w), C.byref(s), C.c_uint32(fri_rounds))

    def prove_linked_aux(self, trace, air, args, nch, fri_rounds=0) -> int:
        """msh_stark_prove_linked_aux (MSLP v2): air over the w trace columns, args flatten_aux_arg dicts with selectors into nch challenges"""
        s, _keep = _air(air)
        arr, _keep2 = aux_args_struct(args)
        t = np.ascontiguousarray(trace, dtype=np.uint64)
        N, w = t.shape
        return self.H.msh_stark_prove_linked_aux(self.h, t.ctypes.data_as(C.POINTER(C.c_uint64)), None, C.c_size_t(N), C.c_size_t(w), C.byref(s), arr, C.c_uint32(len(args)),
                                                 C.c_uint32(nch), C.c_uint32(fri_rounds))

    def verify_linked_aux(self, data, air, args, nch, N, w, fri_rounds=0, zero_display_empty=True):
        """msh_stark_verify_linked_aux: (rc, why) as verify_linked"""
        s, _keep = _air(air)
        arr, _keep2 = aux_args_struct(args)
        why = C.create_string_buffer(512)
        data = bytes(data)
        rc = self.H.msh_stark_verify_linked_aux(self.h, C.byref(s), arr, C.c_uint32(len(args)), C.c_uint32(nch), C.c_size_t(N), C.c_size_t(w), C.c_uint32(fri_rounds), data,
                                                C.c_size_t(len(data)), C.c_int(1 if zero_display_empty else 0), why, C.c_size_t(512))
        return rc, why.value.decode()

    def prove_linked_folded(self, trace, air, log_arity, args=(), nch=0, fri_folds=0) -> int:
        """msh_stark_prove_linked_folded (MSLP v3): the folded FRI at arity 2^log_arity over coset-grouped row trees; args: flatten_aux_arg dicts ([]: no running columns)"""
        s, _keep = _air(air)
        arr, _keep2 = aux_args_struct(args)
        t = np.ascontiguousarray(trace, dtype=np.uint64)
        N, w = t.shape
        return self.H.msh_stark_prove_linked_folded(self.h, t.ctypes.data_as(C.POINTER(C.c_uint64)), None, C.c_size_t(N), C.c_size_t(w), C.byref(s), arr if len(args) else None,
                                                    C.c_uint32(len(args)), C.c_uint32(nch), C.c_int(log_arity), C.c_uint32(fri_folds))

    def verify_linked_folded(self, data, air, N, w, log_arity, args=(), nch=0, fri_folds=0, zero_display_empty=True):
        """msh_stark_verify_linked_folded: (rc, why) as verify_linked"""
        s, _keep = _air(air)
        arr, _keep2 = aux_args_struct(args)
        why = C.create_string_buffer(512)
        data = bytes(data)
        rc = self.H.msh_stark_verify_linked_folded(self.h, C.byref(s), arr if len(args) else None, C.c_uint32(len(args)), C.c_uint32(nch), C.c_size_t(N), C.c_size_t(w),
                                                   C.c_int(log_arity), C.c_uint32(fri_folds), data, C.c_size_t(len(data)), C.c_int(1 if zero_display_empty else 0), why,
                                                   C.c_size_t(512))
        return rc, why.value.decode()

    def linked_proof(self) -> bytes:
        """msh_linked_proof: the MSLP bytes of the last linked proof (b"": none)."""
        return self._bytes(self.H.msh_linked_proof)

    def verify_linked(self, data, air, N, w, fri_rounds=0, zero_display_empty=True):
        """msh_stark_verify_linked: (rc, why) - 1 accepted, 0 rejected with `why` naming the step, < 0 malformed arguments."""
        s, _keep = _air(air)
        why = C.create_string_buffer(512)
        data = bytes(data)
        rc = self.H.msh_stark_verify_linked(self.h, C.byref(s), C.c_size_t(N), C.c_size_t(w), C.c_uint32(fri_rounds), data, C.c_size_t(len(data)),
                                            C.c_int(1 if zero_display_empty else 0), why, C.c_size_t(512))
        return rc, why.value.decode()


def fibonacci_rows_native(p, length, steps, secret_b=2, pad_seed=0x5EED):
    """msh_fibonacci_rows: the benchmark's synthetic trace in C (same values as mini_stark_amd.synthetic.fibonacci_rows; the Python
    loop takes ~1 us per row, 16 s at 2^24 rows)."""
    out = np.empty((length, 3), dtype=np.uint64)
    rc = _host().msh_fibonacci_rows(C.c_uint64(p), C.c_size_t(length), C.c_size_t(steps), C.c_uint64(secret_b), C.c_uint64(pad_seed), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise MsError(rc, "msh_fibonacci_rows")
    return out


def cubic_rows_native(p, length, w, seed=9):
    """msh_cubic_rows: the synthetic trace of the build-defined degree-3 wide AIR (same values as tests/parity_cases.py:cubic_trace) and its w scalars."""
    out = np.empty((length, w), dtype=np.uint64)
    sc = np.empty(w, dtype=np.uint64)
    rc = _host().msh_cubic_rows(C.c_uint64(p), C.c_size_t(length), C.c_size_t(w), C.c_uint64(seed), out.ctypes.data_as(C.POINTER(C.c_uint64)), sc.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise MsError(rc, "msh_cubic_rows")
    return out, sc
