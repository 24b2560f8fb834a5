"""ctypes binding of include/ministark.h (libministark.so, HIP/gfx950).

Plumbing only: numpy arrays in, numpy arrays / bytes out.  The library is the
product; if it is missing or fails to load this module raises — there is no CPU
fallback (tests may pass an explicit `lib_path` to exercise the CPU *emulation
build of the same kernel code*, tests/emu, which the product never loads).
"""
import ctypes as C
import os
import subprocess

import numpy as np

GOLDILOCKS, BABYBEAR = 0, 1
FLAG_ZERO_DISPLAY_EMPTY = 1
FLAG_TRACE_MONT64 = 2
FLAG_LATENCY = 4   # the context proves alone on its GPU: independent chains of a stage on two streams (costs throughput with several contexts in flight)
FLAG_DIGEST_BLAKE2S = 8   # D = Blake2s256 for every commitment of the context (default: SHA-256)
FLAG_DIGEST_BLAKE3 = 0x10   # D = BLAKE3 (excludes FLAG_DIGEST_BLAKE2S)
FLAG_DIGEST_KECCAK256 = 0x20   # D = Keccak-256 (original padding: Ethereum's); a context takes at most one FLAG_DIGEST_* flag
FLAG_DIGEST_SHA3_256 = 0x40   # D = SHA3-256 (FIPS 202)
DIGEST_SHA256, DIGEST_BLAKE2S256, DIGEST_BLAKE3 = 0, 1, 2   # ms_digest_id
DIGEST_KECCAK256, DIGEST_SHA3_256 = 4, 5   # (3 is unassigned)
TREE_TRACE, TREE_LDE, TREE_FRI, TREE_VALIDITY = 0, 1, 2, 4   # ms_tree_id (3 is unassigned)
TREE_LDE_STAGED = 5                                          # the tree of ms_lde_commit_stage
OK, ERR_SHAPE, ERR_LEAF_NOT_FOUND, ERR_OUT_OF_RANGE, ERR_STATE, ERR_ARG, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7

_HERE = os.path.dirname(os.path.abspath(__file__))
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)
_LIBS = {}


class MsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ministark error {code}: {msg}")
        self.code = code


def library_path():
    """The product library; MS_LIB_PATH names another build of it (same-box A/Bs of compile-time variants: tools/ab.sh)."""
    return os.environ.get("MS_LIB_PATH") or os.path.join(_HERE, "libministark.so")


def build_library(force=False):
    """hipcc cross-compile for gfx950 (works without a GPU): `make` in csrc/, one object per translation unit, side by side."""
    so = library_path()
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    jobs = str(max(1, min(8, len(os.sched_getaffinity(0)))))
    subprocess.check_call(["make", "-C", csrc, "-j", jobs], stdout=subprocess.DEVNULL)   # (no-op when up to date)
    return so


def load_library(path=None):
    path = path or library_path()   # the product loads its own in-tree HIP build only (tests pass the emulation build explicitly)
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise MsError(ERR_HIP, f"{path} not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)  # the C++ host mirror (libministark_host.so) resolves ms_* against it
    L.ms_last_error.restype = C.c_char_p
    L.ms_last_error.argtypes = [C.c_void_p]
    L.ms_fri_proof_size.restype = C.c_size_t
    L.ms_fri_proof_size.argtypes = [C.c_void_p]
    L.ms_root_of_unity.restype = C.c_uint64
    L.ms_ceil_log2_k.restype = C.c_uint64
    L.ms_logarithm_of_two_k.restype = C.c_long
    if hasattr(L, "ms_stream"):   # (a library built before the symbol existed: MS_LIB_PATH naming an older build)
        L.ms_stream.restype = C.c_void_p
        L.ms_stream.argtypes = [C.c_void_p]
    if hasattr(L, "ms_fri_begin_folded"):   # folded FRI (likewise absent from an older build)
        L.ms_fri_begin_folded.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint8 * 32)]
        L.ms_fri_fold_folded.argtypes = [C.c_void_p, _u64p, C.POINTER(C.c_uint8 * 32)]
        L.ms_fri_fold_final.argtypes = [C.c_void_p, _u64p, _u64p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ms_fri_query_folded.argtypes = [C.c_void_p, _u64p, C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "ms_query_linked_folded"):   # coset-grouped row trees and the v3 query phase (likewise)
        L.ms_lde_commit_coset.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(C.c_uint8 * 32)]
        L.ms_lde_commit_stage_coset.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8 * 32)]
        L.ms_validity_commit_coset.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8 * 32)]
        L.ms_query_linked_folded.argtypes = [C.c_void_p, _u64p, C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    _LIBS[path] = L
    return L


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_size_t)  # ms_exchange_fn
XCHG_ALL_TO_ALL, XCHG_ALL_GATHER, XCHG_ALL_REDUCE_MIN_U64, XCHG_ALL_REDUCE_SUM_U8 = 0, 1, 2, 3


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(_u64p)


def flatten_terms(constraints):
    """The CSR arrays of ms_mix_terms from `constraints` = [[(coef, [(poly, row), ...]), ...], ...] (one list of terms per constraint; a term with an empty
    factor list is a constant): (term_begin, coef, fac_begin, fac_poly, fac_row) as contiguous numpy arrays."""
    term_begin, coef, fac_begin, fac_poly, fac_row = [0], [], [0], [], []
    for terms in constraints:
        for c, factors in terms:
            coef.append(int(c))
            for poly, row in factors:
                fac_poly.append(int(poly))
                fac_row.append(int(row))
            fac_begin.append(len(fac_poly))
        term_begin.append(len(coef))
    return (np.array(term_begin, dtype=np.uint32), np.array(coef, dtype=np.uint64), np.array(fac_begin, dtype=np.uint32),
            np.array(fac_poly, dtype=np.uint32), np.array(fac_row, dtype=np.uint32))


def terms_rows(constraints):
    """The row offsets a term program touches, ascending: the verifier needs P_j(w^k z) for every such k, i.e. ms_eval_ext at the points w^k z."""
    return sorted({int(row) for terms in constraints for _, factors in terms for _, row in factors})


AIR_PERIODIC = 0x80000000   # MS_AIR_PERIODIC: fac_poly = AIR_PERIODIC | k names periodic column k


class MsAir(C.Structure):
    """ms_air (include/ministark.h)"""
    _u32p = C.POINTER(C.c_uint32)
    _fields_ = [("ncons", C.c_uint32), ("term_begin", _u32p), ("coef", _u64p), ("fac_begin", _u32p), ("fac_poly", _u32p), ("fac_row", _u32p),
                ("ex_begin", _u32p), ("ex_row", _u32p), ("nperiodic", C.c_uint32), ("per_begin", _u32p), ("per_val", _u64p),
                ("nbound", C.c_uint32), ("bnd_poly", _u32p), ("bnd_row", _u32p), ("bnd_val", _u64p)]


AIR_ARRAYS = (("term_begin", np.uint32), ("coef", np.uint64), ("fac_begin", np.uint32), ("fac_poly", np.uint32), ("fac_row", np.uint32), ("ex_begin", np.uint32),
              ("ex_row", np.uint32), ("per_begin", np.uint32), ("per_val", np.uint64), ("bnd_poly", np.uint32), ("bnd_row", np.uint32), ("bnd_val", np.uint64))


def flatten_air(constraints, exempt=None, periodic=(), boundary=()):
    """The arrays of an ms_air as a dict of contiguous numpy arrays (the names of the struct's fields, plus the counts ncons / nperiodic / nbound):
    constraints = [[(coef, [(poly, row), ...]), ...], ...] with poly = AIR_PERIODIC | k for periodic column k; exempt = one row list per constraint (None: no
    row is exempt); periodic = a list of value lists; boundary = [(poly, row, value), ...]."""
    tb, cf, fb, fp, fr = flatten_terms(constraints)
    exempt = [[] for _ in constraints] if exempt is None else [list(rows) for rows in exempt]
    if len(exempt) != len(constraints):
        raise ValueError("flatten_air: one exemption row list per constraint")
    ex_begin, per_begin = [0], [0]
    for rows in exempt:
        ex_begin.append(ex_begin[-1] + len(rows))
    for vals in periodic:
        per_begin.append(per_begin[-1] + len(vals))
    return {"ncons": len(constraints), "term_begin": tb, "coef": cf, "fac_begin": fb, "fac_poly": fp, "fac_row": fr,
            "ex_begin": np.array(ex_begin, dtype=np.uint32), "ex_row": np.array([int(k) for rows in exempt for k in rows], dtype=np.uint32),
            "nperiodic": len(periodic), "per_begin": np.array(per_begin, dtype=np.uint32), "per_val": np.array([int(v) for vals in periodic for v in vals], dtype=np.uint64),
            "nbound": len(boundary), "bnd_poly": np.array([int(b[0]) for b in boundary], dtype=np.uint32), "bnd_row": np.array([int(b[1]) for b in boundary], dtype=np.uint32),
            "bnd_val": np.array([int(b[2]) for b in boundary], dtype=np.uint64)}


def air_struct(air):
    """(MsAir, the arrays it points into - keep them alive while the struct is in use) from a flatten_air dict; an entry that is None becomes a NULL pointer"""
    keep = {k: (None if air.get(k) is None else np.ascontiguousarray(air[k], dtype=t)) for k, t in AIR_ARRAYS}
    s = MsAir()
    s.ncons, s.nperiodic, s.nbound = int(air["ncons"]), int(air["nperiodic"]), int(air["nbound"])
    for k, t in AIR_ARRAYS:
        if keep[k] is not None:   # (an empty numpy array still has a valid, non-null data pointer)
            setattr(s, k, keep[k].ctypes.data_as(_u64p if t is np.uint64 else C.POINTER(C.c_uint32)))
    return s, keep


def air_rows(constraints, boundary=()):
    """The row offsets the verifying side of an AIR program needs opened, ascending: those of its factors, and row 0 when there are boundary constraints (their
    quotients are evaluated from P_j(z))."""
    rows = {int(row) for terms in constraints for _, factors in terms for _, row in factors}
    if len(boundary):
        rows.add(0)
    return sorted(rows)


class MsDeep(C.Structure):
    """ms_deep (include/ministark.h)"""
    _fields_ = [("npts", C.c_uint32), ("z", _u64p), ("pt_begin", C.POINTER(C.c_uint32)), ("pt_poly", C.POINTER(C.c_uint32))]


def deep_struct(z, lists, npts=None):
    """(MsDeep, the arrays it points into - keep them alive while the struct is in use): z = the points' limbs (npts * E of them, any nesting), lists = one list of F
    indices per point (F index j < c: polynomial j of the LDE tree; c + j': chunk column j' of the validity tree).  A list entry that is None leaves that array NULL;
    `lists` may also be the (pt_begin, pt_poly) arrays themselves; npts overrides the count (the refusal tests)."""
    keep = {"z": None if z is None else np.ascontiguousarray(np.asarray(z, dtype=np.uint64).reshape(-1))}
    if isinstance(lists, tuple):
        pb, pp = lists
        n = (len(pb) - 1) if pb is not None else 0
    else:
        n = len(lists)
        pb = np.cumsum([0] + [len(x) for x in lists])
        pp = [int(j) for x in lists for j in x]
    keep["pt_begin"] = None if pb is None else np.ascontiguousarray(pb, dtype=np.uint32)
    keep["pt_poly"] = None if pp is None else np.ascontiguousarray(pp, dtype=np.uint32)
    s = MsDeep()
    s.npts = int(n if npts is None else npts)
    if keep["z"] is not None:
        s.z = keep["z"].ctypes.data_as(_u64p)
    for k in ("pt_begin", "pt_poly"):
        if keep[k] is not None:
            setattr(s, k, keep[k].ctypes.data_as(C.POINTER(C.c_uint32)))
    return s, keep


AUX_SUM, AUX_PRODUCT = 0, 1   # MS_AUX_SUM / MS_AUX_PRODUCT


class MsAux(C.Structure):
    """ms_aux (include/ministark.h)"""
    _u32p = C.POINTER(C.c_uint32)
    _fields_ = [("op", C.c_uint32), ("ext", C.c_uint32), ("nfrac", C.c_uint32), ("form_begin", _u32p), ("term_col", _u32p), ("term_coef", _u64p), ("form_const", _u64p)]


def _limbs(v, ext):
    """an element of K as `ext` ints: an int for ext = 1, an ext-tuple otherwise"""
    if ext == 1 and not isinstance(v, (tuple, list)):
        return [int(v)]
    v = [int(x) for x in v]
    if len(v) != ext:
        raise ValueError(f"an element of {ext} limbs expected")
    return v


def flatten_aux(op, fractions, ext=1):
    """The arrays of an ms_aux as a dict (the names of the struct's fields) from fractions = [((const, [(col, coef), ...]), (const, [(col, coef), ...])), ...]: numerator
    and denominator of every fraction as affine forms over the trace columns; const / coef are ints for ext = 1 and ext-tuples otherwise."""
    form_begin, term_col, term_coef, form_const = [0], [], [], []
    for frac in fractions:
        if len(frac) != 2:
            raise ValueError("flatten_aux: a fraction is a (numerator, denominator) pair of forms")
        for const, terms in frac:
            form_const += _limbs(const, ext)
            for col, coef in terms:
                term_col.append(int(col))
                term_coef += _limbs(coef, ext)
            form_begin.append(len(term_col))
    return {"op": int(op), "ext": int(ext), "nfrac": len(fractions), "form_begin": np.array(form_begin, dtype=np.uint32), "term_col": np.array(term_col, dtype=np.uint32),
            "term_coef": np.array(term_coef, dtype=np.uint64), "form_const": np.array(form_const, dtype=np.uint64)}


AUX_ARRAYS = (("form_begin", np.uint32), ("term_col", np.uint32), ("term_coef", np.uint64), ("form_const", np.uint64))


def aux_struct(aux):
    """(MsAux, the arrays it points into) from a flatten_aux dict; an entry that is None becomes a NULL pointer"""
    keep = {k: (None if aux.get(k) is None else np.ascontiguousarray(aux[k], dtype=t)) for k, t in AUX_ARRAYS}
    s = MsAux()
    s.op, s.ext, s.nfrac = int(aux["op"]), int(aux["ext"]), int(aux["nfrac"])
    for k, t in AUX_ARRAYS:
        if keep[k] is not None:
            setattr(s, k, keep[k].ctypes.data_as(_u64p if t is np.uint64 else C.POINTER(C.c_uint32)))
    return s, keep


_MODULUS = {GOLDILOCKS: 2**64 - 2**32 + 1, BABYBEAR: 2013265921}

# ---- arguments with symbolic challenges (msh_aux_arg, include/ministark_host.h): the statement of a linked proof with running columns
AUX_ARG_ARRAYS = (("form_begin", np.uint32), ("term_col", np.uint32), ("term_coef", np.uint64), ("term_ch", np.uint32), ("form_const", np.uint64), ("form_ch", np.uint32))


def flatten_aux_arg(op, fractions):
    """The arrays of an msh_aux_arg as a dict from fractions = [(numerator, denominator), ...], a form being ((const, sel), [(col, coef, sel), ...]): base-field
    values with a selector each - 0: times 1, k: times the proof's challenge ch[k - 1]."""
    form_begin, term_col, term_coef, term_ch, form_const, form_ch = [0], [], [], [], [], []
    for frac in fractions:
        if len(frac) != 2:
            raise ValueError("flatten_aux_arg: a fraction is a (numerator, denominator) pair of forms")
        for (const, sel), terms in frac:
            form_const.append(int(const)); form_ch.append(int(sel))
            for col, coef, tsel in terms:
                term_col.append(int(col)); term_coef.append(int(coef)); term_ch.append(int(tsel))
            form_begin.append(len(term_col))
    vals = dict(form_begin=form_begin, term_col=term_col, term_coef=term_coef, term_ch=term_ch, form_const=form_const, form_ch=form_ch)
    out = {"op": int(op), "nfrac": len(fractions)}
    out.update({k: np.array(vals[k], dtype=t) for k, t in AUX_ARG_ARRAYS})
    return out


def instantiate_aux(field, arg, ch):
    """The flatten_aux dict (ext = E) of a flatten_aux_arg dict with the challenges ch (E-tuples) in place: value * ch[sel - 1], or the base-field value itself."""
    p, e = _MODULUS[field], _EXT[field]

    def limbs(value, sel):
        return [int(value) * int(x) % p for x in ch[int(sel) - 1]] if int(sel) else [int(value)] + [0] * (e - 1)
    coef = [x for v, sel in zip(arg["term_coef"], arg["term_ch"]) for x in limbs(v, sel)]
    const = [x for v, sel in zip(arg["form_const"], arg["form_ch"]) for x in limbs(v, sel)]
    return {"op": int(arg["op"]), "ext": e, "nfrac": int(arg["nfrac"]), "form_begin": np.array(arg["form_begin"], dtype=np.uint32),
            "term_col": np.array(arg["term_col"], dtype=np.uint32), "term_coef": np.array(coef, dtype=np.uint64), "form_const": np.array(const, dtype=np.uint64)}


def aux_fractions(aux):
    """the fractions of a flatten_aux dict (ext > 1), in the format flatten_aux and aux_constraints take"""
    e, fb = int(aux["ext"]), [int(x) for x in aux["form_begin"]]
    k = lambda a, i: tuple(int(x) for x in a[i * e:(i + 1) * e])   # noqa: E731
    forms = [(k(aux["form_const"], f), [(int(aux["term_col"][m]), k(aux["term_coef"], m)) for m in range(fb[f], fb[f + 1])]) for f in range(2 * int(aux["nfrac"]))]
    return [(forms[2 * i], forms[2 * i + 1]) for i in range(int(aux["nfrac"]))]


def encode_aux(args, nch) -> bytes:
    """msh_aux_encode in Python: 'MSAX' | version 1 | nargs | nch, then per argument op, nfrac, nterms | form_begin | term_col | term_ch | form_ch | term_coef | form_const"""
    import struct
    out = struct.pack("<4I", 0x5841534D, 1, len(args), int(nch))
    for a in args:
        arr = {k: np.ascontiguousarray(a[k], dtype=t).astype("<u4" if t is np.uint32 else "<u8") for k, t in AUX_ARG_ARRAYS}
        out += struct.pack("<3I", int(a["op"]), int(a["nfrac"]), arr["term_col"].size)
        out += b"".join(arr[k].tobytes() for k in ("form_begin", "term_col", "term_ch", "form_ch", "term_coef", "form_const"))
    return out


_EXT = {GOLDILOCKS: 2, BABYBEAR: 4}
_NR2 = {GOLDILOCKS: 7, BABYBEAR: 11}       # Fp2 = Fp[u] / (u^2 - NR2)
_NR4 = (2013265910, 1)                     # Fp4 = Fp2[v] / (v^2 - (2013265910 + u))  (BabyBear)


def _tower_mul(field, ext, a, b):
    """a * b in K (tuples of `ext` limbs; the towers of csrc/field.hpp)"""
    p = _MODULUS[field]
    if ext == 1:
        return (a[0] * b[0] % p,)
    nr = _NR2[field]

    def m2(x, y):
        return ((x[0] * y[0] + nr * x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)
    if ext == 2:
        return m2(a, b)
    a0, a1, b0, b1 = a[:2], a[2:], b[:2], b[2:]
    lo, t = m2(a0, b0), m2(_NR4, m2(a1, b1))
    x, y = m2(a0, b1), m2(a1, b0)
    return ((lo[0] + t[0]) % p, (lo[1] + t[1]) % p, (x[0] + y[0]) % p, (x[1] + y[1]) % p)


def aux_constraints(field, op, fractions, ext, first_poly, exempt_last=False, N=None):
    """The constraints a column of Context.aux_running satisfies, as (constraints, exempt, boundary) in the formats Context.mix_air takes.  The column's limbs are the
    polynomials first_poly .. first_poly + ext - 1; the forms of `fractions` (as for aux_running) are over the trace columns, whose polynomials keep their indices.
    Transition, cleared of denominators, with z' = z(w x):
        AUX_PRODUCT   z' * prod_k den_k - z * prod_k num_k
        AUX_SUM       (z' - z) * prod_k den_k - sum_k num_k * prod_{j != k} den_j
    For ext > 1 this identity in K is expanded into one base-field constraint per limb over the limb columns, by a symbolic product (monomial -> coefficient in K).
    Boundary: z(w^0) = the identity, limb by limb.  exempt_last: the transition constraints are exempt on row N - 1 (needed when `final` is not the identity; pass N).
    ValueError when the expansion exceeds ms_mix_air's limits (8 factors per term, 65536 terms)."""
    p = _MODULUS[field]
    if ext not in (1, _EXT[field]):
        raise ValueError("aux_constraints: ext must be 1 or the field's extension degree")
    if exempt_last and N is None:
        raise ValueError("aux_constraints: exempt_last needs the number of rows N")
    unit = lambda l: tuple(1 if i == l else 0 for i in range(ext))   # noqa: E731

    def padd(a, b, sign=1):
        out = dict(a)
        for mono, c in b.items():
            out[mono] = tuple((x + sign * y) % p for x, y in zip(out.get(mono, (0,) * ext), c))
        return out

    def pmul(a, b):
        out = {}
        for ma, ca in a.items():
            for mb, cb in b.items():
                mono = tuple(sorted(ma + mb))
                if len(mono) > 8:
                    raise ValueError("aux_constraints: a term with more than 8 factors (ms_mix_air's limit)")
                c = _tower_mul(field, ext, ca, cb)
                out[mono] = tuple((x + y) % p for x, y in zip(out.get(mono, (0,) * ext), c))
            if len(out) * ext > 65536:
                raise ValueError("aux_constraints: more than 65536 terms (ms_mix_air's limit)")
        return out

    def form(f):
        const, terms = f
        out = {(): tuple(v % p for v in _limbs(const, ext))}
        for col, coef in terms:
            out = padd(out, {((int(col), 0),): tuple(v % p for v in _limbs(coef, ext))})
        return out
    z = {((first_poly + l, 0),): unit(l) for l in range(ext)}
    zn = {((first_poly + l, 1),): unit(l) for l in range(ext)}
    one = {(): unit(0)}
    nums, dens = [form(fr[0]) for fr in fractions], [form(fr[1]) for fr in fractions]
    den_all = one
    for d in dens:
        den_all = pmul(den_all, d)
    if op == AUX_PRODUCT:
        num_all = one
        for n_ in nums:
            num_all = pmul(num_all, n_)
        expr = padd(pmul(zn, den_all), pmul(z, num_all), -1)
    elif op == AUX_SUM:
        expr = pmul(padd(zn, z, -1), den_all)
        for k, n_ in enumerate(nums):
            t = n_
            for j, d in enumerate(dens):
                if j != k:
                    t = pmul(t, d)
            expr = padd(expr, t, -1)
    else:
        raise ValueError("aux_constraints: op must be AUX_SUM or AUX_PRODUCT")
    constraints = []
    for l in range(ext):
        terms = [(c[l], list(mono)) for mono, c in sorted(expr.items()) if c[l]]
        if not any(factors for _, factors in terms):
            raise ValueError("aux_constraints: a limb's constraint has no term with a factor")
        constraints.append(terms)
    if sum(len(t) for t in constraints) > 65536:
        raise ValueError("aux_constraints: more than 65536 terms (ms_mix_air's limit)")
    exempt = [[N - 1] if exempt_last else [] for _ in range(ext)]
    boundary = [(first_poly + l, 0, 1 if (op == AUX_PRODUCT and l == 0) else 0) for l in range(ext)]
    return constraints, exempt, boundary


class Context:
    """One ms_ctx: a prover session on one GPU (include/ministark.h)."""

    def __init__(self, field=GOLDILOCKS, device=0, flags=FLAG_ZERO_DISPLAY_EMPTY, lib_path=None):
        self.L = load_library(lib_path)
        self.field = field
        h = C.c_void_p()
        rc = self.L.ms_create(C.byref(h), C.c_int(device), C.c_int(field), C.c_uint32(flags))
        if rc != 0:
            raise MsError(rc, "ms_create failed (no usable GPU / HIP runtime?)")
        self.h = h
        self.e = self.L.ms_ext_degree(self.h)
        # what the context commits with (ms_digest).  A library built before the symbol existed (MS_LIB_PATH naming an older build) knows SHA-256 only
        self.digest = int(self.L.ms_digest(self.h)) if hasattr(self.L, "ms_digest") else DIGEST_SHA256
        if (flags & FLAG_DIGEST_BLAKE2S) and self.digest != DIGEST_BLAKE2S256:
            self.close()
            raise MsError(ERR_ARG, "FLAG_DIGEST_BLAKE2S: this build of the library has no BLAKE2s-256 kernels")
        if (flags & FLAG_DIGEST_BLAKE3) and self.digest != DIGEST_BLAKE3:
            self.close()
            raise MsError(ERR_ARG, "FLAG_DIGEST_BLAKE3: this build of the library has no BLAKE3 kernels")
        for flag, want, name in ((FLAG_DIGEST_KECCAK256, DIGEST_KECCAK256, "KECCAK256"), (FLAG_DIGEST_SHA3_256, DIGEST_SHA3_256, "SHA3_256")):
            if (flags & flag) and self.digest != want:
                self.close()
                raise MsError(ERR_ARG, f"FLAG_DIGEST_{name}: this build of the library has no Keccak kernels")
        self.N = self.w = self.Lsize = 0

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.ms_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return (self.L.ms_last_error(self.h) or b"").decode()

    def check(self, rc):
        if rc != 0:
            raise MsError(rc, self.last_error())

    # ---- host-only config math -------------------------------------------------
    def root_of_unity(self, n):
        return int(self.L.ms_root_of_unity(C.c_int(self.field), C.c_uint64(n)))

    def ceil_log2_k(self, n, base=2):
        return int(self.L.ms_ceil_log2_k(C.c_uint64(n), C.c_uint64(base)))

    def num_queries(self, security_bits, blowup, steps):
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.ms_num_queries(C.c_int(self.field), C.c_uint64(security_bits), C.c_uint64(blowup), C.c_uint64(steps), C.byref(a), C.byref(b))
        return rc, a.value, b.value

    def num_queries_grind(self, security_bits, grinding_bits, blowup, steps):
        """ms_num_queries_grind: (rc, constrain_queries, fri_queries) with `grinding_bits` of the security taken by the proof of work (0: num_queries)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.ms_num_queries_grind(C.c_int(self.field), C.c_uint64(security_bits), C.c_uint64(grinding_bits), C.c_uint64(blowup), C.c_uint64(steps),
                                         C.byref(a), C.byref(b))
        return rc, a.value, b.value

    def grind(self, seed, bits, start=0, limit=2**64 - 1):
        """ms_grind (BUILD-DEFINED proof of work; include/ministark.h): (rc, nonce) with nonce the smallest n in [start, start + limit) whose digest
        D(seed || n as 8 little-endian bytes) starts with `bits` zero bits, D the context's digest; (ERR_OUT_OF_RANGE, None) when the range holds none."""
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("grind: a seed of 32 bytes expected")
        out = C.c_uint64(0)
        rc = self.L.ms_grind(self.h, (C.c_uint8 * 32).from_buffer_copy(seed), C.c_uint32(bits), C.c_uint64(start), C.c_uint64(limit), C.byref(out))
        return (rc, None) if rc != 0 else (0, int(out.value))

    def arith_selftest(self, op, a, b, cls=0):
        """ms_arith_selftest: a (op) b element-wise ON THE DEVICE with arithmetic class `cls` (0: the class of the NTT tiles; Goldilocks 1 GL, 2 GLT, 3 GLM);
        operations >= 32 take extension elements as consecutive limbs (ops and classes: include/ministark.h).  Raises MsError on a refusal."""
        op = int(op) | int(cls) << 8
        a, pa = _u64(a)
        b, pb = _u64(b)
        out = np.zeros(len(a), dtype=np.uint64)
        self.check(self.L.ms_arith_selftest(self.h, C.c_int(op), pa, pb, out.ctypes.data_as(_u64p), C.c_size_t(len(a))))
        return out

    def set_stream(self, hip_stream_ptr):
        """ms_set_stream: from now on the context enqueues its work on the caller's hipStream_t (`torch.cuda.Stream.cuda_stream`); 0 / None selects the context's OWN
        stream - so HIP's null stream, torch's default stream (handle 0), cannot be named: create a stream and order it with an event.  A hand-over point: whatever the
        context enqueued before the call happens before whatever it enqueues after it; the stream being left is drained inside the call, so it must still exist (if
        draining fails, MsError is raised and the context is on the new stream all the same).  Exactly interpolate, mix, polys_lincomb (MS_LAZY_LINCOMB=0) and bench_lde
        return with launches in flight; every other entry point returns with the stream idle.  The four are ordered before every later call, across a switch too;
        synchronize() waits for them - call it, or move the context away, before destroying a stream that was lent."""
        self.check(self.L.ms_set_stream(self.h, C.c_void_p(hip_stream_ptr or None)))

    def stream(self):
        """ms_stream: the handle of the stream the context is on now - the caller's, or its own (`torch.cuda.ExternalStream(ctx.stream())` records events on it)."""
        return int(self.L.ms_stream(self.h) or 0)

    def synchronize(self):
        """ms_synchronize: waits for the stream the context is on now."""
        self.check(self.L.ms_synchronize(self.h))

    def set_shard(self, rank, world, send_ptr, recv_ptr, cap_bytes, callback):
        """ms_set_shard: one proof over `world` ranks.  `callback(op, nbytes) -> int` runs the collective on the exchange
        buffers (mini_stark_amd.dist.ShardExchange does it with torch.distributed)."""
        self._xchg_cb = EXCHANGE_FN(lambda user, op, nbytes: int(callback(int(op), int(nbytes)))) if callback is not None else EXCHANGE_FN(0)
        self.L.ms_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, EXCHANGE_FN, C.c_void_p]
        self.check(self.L.ms_set_shard(self.h, rank, world, send_ptr, recv_ptr, cap_bytes, self._xchg_cb, None))

    def rccl_unique_id(self) -> bytes:
        """ms_rccl_unique_id: the 128-byte ncclUniqueId rank 0 hands to every rank (any channel) before set_shard_rccl."""
        buf = (C.c_uint8 * 128)()
        rc = self.L.ms_rccl_unique_id(buf)
        if rc != 0:
            raise MsError(rc, "RCCL is not available (librccl.so could not be loaded)")
        return bytes(buf)

    def set_shard_rccl(self, rank, world, unique_id: bytes, cap_bytes: int):
        """ms_set_shard_rccl: one proof over `world` ranks, the collectives run by the library itself with RCCL on its stream."""
        self.L.ms_set_shard_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        self.check(self.L.ms_set_shard_rccl(self.h, rank, world, unique_id, cap_bytes))

    def shard_proof_on_root(self, on=True):
        """ms_shard_proof_on_root: a sharded proof's FRI blob is assembled on rank 0 only (the other ranks send their slices and hold no proof)."""
        self.check(self.L.ms_shard_proof_on_root(self.h, C.c_int(1 if on else 0)))

    def shard_stats(self):
        out = (C.c_uint64 * 8)()
        self.check(self.L.ms_shard_stats(self.h, out))
        return [int(v) for v in out]

    # ---- Stark::prove stages ---------------------------------------------------
    def trace_commit(self, trace, lpn):
        t = np.ascontiguousarray(trace, dtype=np.uint64)
        N, w = t.shape
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_trace_commit(self.h, t.ctypes.data_as(_u64p), C.c_size_t(N), C.c_size_t(w), C.c_size_t(lpn), root)
        if rc == 0:
            self.N, self.w = N, w
        return rc, bytes(root)

    def trace_commit_ptr(self, host_ptr, N, w, lpn):
        """ms_trace_commit on a raw host pointer (page-locked memory from pinned_alloc: the trace then travels on an SDMA engine)."""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_trace_commit(self.h, C.c_void_p(host_ptr), C.c_size_t(N), C.c_size_t(w), C.c_size_t(lpn), root)
        if rc == 0:
            self.N, self.w = N, w
        return rc, bytes(root)

    def trace_upload_async(self, host_ptr, N, w):
        """ms_trace_upload_async: prefetch of the NEXT proof's page-locked trace while the current proof computes (a hint; MS_OK also when nothing was queued)."""
        return self.L.ms_trace_upload_async(self.h, C.c_void_p(host_ptr), C.c_size_t(N), C.c_size_t(w))

    def pinned_alloc(self, nbytes):
        self.L.ms_pinned_alloc.restype = C.c_void_p
        return self.L.ms_pinned_alloc(C.c_size_t(nbytes))

    def pinned_free(self, ptr):
        self.L.ms_pinned_free.argtypes = [C.c_void_p]
        self.L.ms_pinned_free(C.c_void_p(ptr))

    def io_runtime_path(self):
        self.L.ms_io_runtime_path.restype = C.c_char_p
        return (self.L.ms_io_runtime_path() or b"").decode()

    def trace_commit_device(self, dev_ptr, N, w, lpn):
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_trace_commit_device(self.h, C.c_void_p(dev_ptr), C.c_size_t(N), C.c_size_t(w), C.c_size_t(lpn), root)
        if rc == 0:
            self.N, self.w = N, w
        return rc, bytes(root)

    def aux_running(self, op, fractions, ext=1, read=False):
        """ms_aux_running (BUILD-DEFINED running product / running sum of fractions of affine forms over the committed trace; include/ministark.h), between trace_commit
        and interpolate: fractions as for flatten_aux, or a flatten_aux dict.  Returns (rc, final, column or None): final an int for ext = 1 and an ext-tuple otherwise,
        column (read=True) an (N, ext) array."""
        aux = fractions if isinstance(fractions, dict) else flatten_aux(op, fractions, ext)
        s, _keep = aux_struct(aux)
        e = int(aux["ext"])
        fin = np.zeros(max(1, e), dtype=np.uint64)
        col = np.zeros((self.N, e), dtype=np.uint64) if read else None
        rc = self.L.ms_aux_running(self.h, C.byref(s), fin.ctypes.data_as(_u64p), col.ctypes.data_as(_u64p) if read else None)
        if rc != 0:
            return rc, None, None
        return 0, (int(fin[0]) if e == 1 else tuple(int(v) for v in fin)), col

    def aux_running_staged(self, op, fractions, ext=1, read=False):
        """ms_aux_running_staged: aux_running's column built while the LDE tree of the main columns is live (after lde_commit, before lde_commit_stage and any mix
        stage); the limbs become the last `ext` polynomials.  Arguments and result as aux_running."""
        aux = fractions if isinstance(fractions, dict) else flatten_aux(op, fractions, ext)
        s, _keep = aux_struct(aux)
        e = int(aux["ext"])
        fin = np.zeros(max(1, e), dtype=np.uint64)
        col = np.zeros((self.N, e), dtype=np.uint64) if read else None
        rc = self.L.ms_aux_running_staged(self.h, C.byref(s), fin.ctypes.data_as(_u64p), col.ctypes.data_as(_u64p) if read else None)
        if rc != 0:
            return rc, None, None
        return 0, (int(fin[0]) if e == 1 else tuple(int(v) for v in fin)), col

    def aux_staged_count(self):
        return self.L.ms_aux_staged_count(self.h)

    def lde_commit_stage(self, lpn):
        """ms_lde_commit_stage: the staged columns evaluated behind the LDE's columns and committed in a second tree -> (rc, root)"""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_lde_commit_stage(self.h, C.c_size_t(lpn), root)
        return rc, bytes(root)

    def lde_commit_stage_coset(self, log_arity):
        """ms_lde_commit_stage_coset: ms_lde_commit_stage with the second tree over coset leaf groups (the live LDE tree's own log_arity) -> (rc, root)"""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_lde_commit_stage_coset(self.h, C.c_int(log_arity), root)
        return rc, bytes(root)

    def aux_count(self):
        return self.L.ms_aux_count(self.h)

    def interpolate(self):
        return self.L.ms_interpolate(self.h)

    def polys_lincomb(self, scalars, idx):
        s, sp = _u64(scalars)
        i = np.ascontiguousarray(idx, dtype=np.int32)
        return self.L.ms_polys_lincomb(self.h, sp, i.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(len(i)))

    def polys_append(self, coeffs):
        c, cp = _u64(coeffs)
        return self.L.ms_polys_append(self.h, cp, C.c_size_t(c.size))

    def polys_count(self):
        return self.L.ms_polys_count(self.h)

    def poly_read(self, i):
        out = np.zeros(self.N, dtype=np.uint64)
        self.check(self.L.ms_poly_read(self.h, C.c_int(i), out.ctypes.data_as(_u64p)))
        return out

    def lde_commit(self, blowup, shift, lpn):
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_lde_commit(self.h, C.c_size_t(blowup), C.c_uint64(shift), C.c_size_t(lpn), root)
        if rc == 0:
            self.Lsize = self.N * blowup
        return rc, bytes(root)

    def lde_commit_coset(self, blowup, shift, log_arity):
        """ms_lde_commit_coset: ms_lde_commit with the tree over L / 2^log_arity coset leaf groups (group j: the rows j + t L / a, column-major) -> (rc, root)"""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_lde_commit_coset(self.h, C.c_size_t(blowup), C.c_uint64(shift), C.c_int(log_arity), root)
        if rc == 0:
            self.Lsize = self.N * blowup
        return rc, bytes(root)

    def bench_lde(self, blowup, shift):
        return self.L.ms_bench_lde(self.h, C.c_size_t(blowup), C.c_uint64(shift))

    def lde_read(self):
        out = np.zeros((self.Lsize, self.polys_count() - self.aux_staged_count()), dtype=np.uint64)   # (staged columns are in the matrix once their stage is committed)
        self.check(self.L.ms_lde_read(self.h, out.ctypes.data_as(_u64p)))
        return out

    def mix(self, r):
        return self.L.ms_mix(self.h, C.c_uint64(r))

    def mix_cubic(self, r, spec, scalars):
        """ms_mix_cubic (BUILD-DEFINED degree-3 composition with the true quotient; include/ministark.h): spec = [(j, a, b, c, d), ...]."""
        sp = np.ascontiguousarray(spec, dtype=np.int32).reshape(-1, 5)
        sc, scp = _u64(scalars)
        return self.L.ms_mix_cubic(self.h, C.c_uint64(r), sp.ctypes.data_as(C.POINTER(C.c_int)), scp, C.c_int(len(sp)))

    def mix_terms(self, r, constraints, nexempt):
        """ms_mix_terms (BUILD-DEFINED composition of any degree with the true quotient; include/ministark.h): constraints = [[(coef, [(poly, row), ...]), ...], ...],
        or the CSR arrays themselves (the 5-tuple flatten_terms returns)."""
        csr = constraints if isinstance(constraints, tuple) and len(constraints) == 5 and isinstance(constraints[0], np.ndarray) else flatten_terms(constraints)
        tb, cf, fb, fp, fr = csr
        u32p = C.POINTER(C.c_uint32)
        # (an empty numpy array still has a valid, non-null data pointer)
        return self.L.ms_mix_terms(self.h, C.c_uint64(r), C.c_int(len(tb) - 1), tb.ctypes.data_as(u32p), cf.ctypes.data_as(_u64p), fb.ctypes.data_as(u32p),
                                   fp.ctypes.data_as(u32p), fr.ctypes.data_as(u32p), C.c_int(nexempt))

    def mix_air(self, r, constraints, exempt=None, periodic=(), boundary=()):
        """ms_mix_air (BUILD-DEFINED AIR composition with the true quotients; include/ministark.h): constraints as for mix_terms with AIR_PERIODIC | k naming periodic
        column k, exempt = one row list per constraint, periodic = a list of value lists, boundary = [(poly, row, value), ...]; or a flatten_air dict as `constraints`."""
        air = constraints if isinstance(constraints, dict) else flatten_air(constraints, exempt, periodic, boundary)
        s, _keep = air_struct(air)
        return self.L.ms_mix_air(self.h, C.c_uint64(r), C.byref(s))

    def mix_air_ext(self, r, constraints, exempt=None, periodic=(), boundary=()):
        """ms_mix_air_ext: mix_air with the combiner in the extension field, r = a sequence of E = ext_degree limbs (None passes a null pointer).  Afterwards
        validity_ext() is E and validity_read() has the shape (VL, E)."""
        air = constraints if isinstance(constraints, dict) else flatten_air(constraints, exempt, periodic, boundary)
        s, _keep = air_struct(air)
        if r is None:
            return self.L.ms_mix_air_ext(self.h, None, C.byref(s))
        rr, rp = _u64(r)
        if rr.size != self.e:
            raise ValueError(f"mix_air_ext: r has {rr.size} limbs, the extension has {self.e}")
        return self.L.ms_mix_air_ext(self.h, rp, C.byref(s))

    def air_check(self, constraints, exempt=None, periodic=(), boundary=()):
        """ms_air_check (BUILD-DEFINED, diagnostic; include/ministark.h): the program of mix_air - same arguments, or a flatten_air dict - evaluated on the rows of the
        trace domain, valid from trace_commit on.  Returns (rc, report); report (None when rc != 0) is a dict: nfail; count and first_row (uint64 arrays of ncons:
        violating rows per constraint, the smallest one or N); bnd_got (the value the trace has at every boundary cell); bnd_fail (indices of the boundary constraints whose
        value differs); first (the (row, constraint) pair smallest by row, then by constraint, or None); ok (nfail == 0)."""
        air = constraints if isinstance(constraints, dict) else flatten_air(constraints, exempt, periodic, boundary)
        s, keep = air_struct(air)
        ncons, nbound = int(air["ncons"]), int(air["nbound"])
        nfail = C.c_uint64(0)
        count, first_row, got = (np.zeros(max(1, n), dtype=np.uint64) for n in (ncons, ncons, nbound))
        rc = self.L.ms_air_check(self.h, C.byref(s), C.byref(nfail), count.ctypes.data_as(_u64p), first_row.ctypes.data_as(_u64p), got.ctypes.data_as(_u64p))
        if rc != 0:
            return rc, None
        count, first_row, got = count[:ncons], first_row[:ncons], got[:nbound]
        bad = [(int(first_row[t]), t) for t in range(ncons) if count[t]]
        return 0, {"nfail": int(nfail.value), "count": count, "first_row": first_row, "bnd_got": got,
                   "bnd_fail": [b for b in range(nbound) if int(got[b]) != int(keep["bnd_val"][b])], "first": min(bad) if bad else None, "ok": nfail.value == 0}

    def validity_ext(self):
        """ms_validity_ext: limbs per coefficient of the validity polynomial (0: none; 1; E after mix_air_ext)."""
        return int(self.L.ms_validity_ext(self.h))

    def validity_len(self):
        """ms_validity_len: coefficients of the validity polynomial after the mix stage (VL)."""
        self.L.ms_validity_len.restype = C.c_size_t
        return int(self.L.ms_validity_len(self.h))

    def validity_read(self):
        self.L.ms_validity_len.restype = C.c_size_t
        vl, ve = int(self.L.ms_validity_len(self.h)) or self.N, max(1, self.validity_ext())
        out = np.zeros(vl * ve, dtype=np.uint64)
        self.check(self.L.ms_validity_read(self.h, out.ctypes.data_as(_u64p)))
        return out.reshape(vl, ve) if ve > 1 else out

    def eval_ext(self, z):
        z, zp = _u64(z)
        q = z.size // self.e
        out = np.zeros((q, self.polys_count() + 1, self.e), dtype=np.uint64)
        rc = self.L.ms_eval_ext(self.h, zp, C.c_int(q), out.ctypes.data_as(_u64p))
        return rc, out

    # ---- Fri::prove stages -------------------------------------------------------
    def fri_begin(self, blowup, rounds):
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_fri_begin(self.h, C.c_size_t(blowup), C.c_size_t(rounds), root)
        return rc, bytes(root)

    def fri_deep(self, z):
        z, zp = _u64(z)
        B = np.zeros(2 * self.e, dtype=np.uint64)
        rc = self.L.ms_fri_deep(self.h, zp, B.ctypes.data_as(_u64p))
        return rc, B

    def fri_fold_commit(self, alpha):
        a, ap = _u64(alpha)
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_fri_fold_commit(self.h, ap, root)
        return rc, bytes(root)

    def fri_round_info(self, r):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(self.L.ms_fri_round_info(self.h, C.c_int(r), C.byref(a), C.byref(b)))
        return a.value, b.value

    def fri_round_poly(self, r):
        n, _ = self.fri_round_info(r)
        out = np.zeros((n, self.e), dtype=np.uint64)
        if n:
            self.check(self.L.ms_fri_round_poly_read(self.h, C.c_int(r), out.ctypes.data_as(_u64p)))
        return out

    def fri_round_codeword(self, r):
        _, D = self.fri_round_info(r)
        out = np.zeros((D, self.e), dtype=np.uint64)
        self.check(self.L.ms_fri_round_codeword_read(self.h, C.c_int(r), out.ctypes.data_as(_u64p)))
        return out

    def fri_query(self, betas, read=True):
        b, bp = _u64(betas)
        rc = self.L.ms_fri_query(self.h, bp, C.c_int(b.size))
        if rc != 0 or not read:
            return rc, None
        return 0, self.fri_proof_read()

    def fri_proof_size(self):
        return int(self.L.ms_fri_proof_size(self.h))

    def fri_proof_read(self):
        n = self.fri_proof_size()
        if n == 0 and self.L.ms_shard_proof_is_elsewhere(self.h) == 1:
            return b""       # ms_shard_proof_on_root: this rank sent its slices to rank 0 and holds no proof
        buf = np.zeros(max(1, n), dtype=np.uint8)
        self.check(self.L.ms_fri_proof_read(self.h, buf.ctypes.data_as(_u8p)))
        return buf[:n].tobytes()

    # ---- openings by index (BUILD-DEFINED; include/ministark.h) -----------------------
    def _sized_bytes(self, call):
        """the size query of an entry point with (out, cap, len) arguments, then the call itself: bytes, or MsError"""
        n = C.c_size_t(0)
        self.check(call(None, C.c_size_t(0), C.byref(n)))
        buf = np.zeros(max(1, n.value), dtype=np.uint8)
        self.check(call(buf.ctypes.data_as(_u8p), C.c_size_t(n.value), C.byref(n)))
        return buf[: n.value].tobytes()

    def tree_open(self, tree, indices, round=0) -> bytes:
        """ms_tree_open: the MerklePaths of the leaf groups `indices` of TREE_TRACE / TREE_LDE / TREE_FRI (round `round`), concatenated in request order."""
        ix, ip = _u64(indices)
        return self._sized_bytes(lambda out, cap, n: self.L.ms_tree_open(self.h, C.c_int(tree), C.c_int(round), ip, C.c_size_t(ix.size), out, cap, n))

    def fri_query_index(self, betas) -> bytes:
        """ms_fri_query_index: the compact query phase, the MSFI blob (openings by position, the last round's polynomial in the clear)."""
        b, bp = _u64(betas)
        return self._sized_bytes(lambda out, cap, n: self.L.ms_fri_query_index(self.h, bp, C.c_int(b.size), out, cap, n))

    # ---- folded FRI: arity 2, 4 or 8, one coset per leaf group (BUILD-DEFINED; include/ministark.h) -----------------------
    def fri_begin_folded(self, blowup, log_arity):
        """ms_fri_begin_folded: (rc, root of round 0's coset-leaf tree); the FRI state is in folded mode from here on."""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_fri_begin_folded(self.h, C.c_size_t(blowup), C.c_int(log_arity), root)
        return rc, bytes(root)

    def fri_fold_folded(self, alpha):
        """ms_fri_fold_folded: folds the last committed round at alpha (E limbs) and commits the result: (rc, root)."""
        a, ap = _u64(alpha)
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_fri_fold_folded(self.h, ap, root)
        return rc, bytes(root)

    def fri_fold_final(self, alpha):
        """ms_fri_fold_final: the last fold, not committed: (rc, its polynomial as (nfinal, E) limbs - None unless rc == 0)."""
        a, ap = _u64(alpha)
        n = C.c_size_t(0)
        rc = self.L.ms_fri_fold_final(self.h, ap, None, C.c_size_t(0), C.byref(n))
        if rc != 0:
            return rc, None
        out = np.zeros((n.value, self.e), dtype=np.uint64)
        rc = self.L.ms_fri_fold_final(self.h, ap, out.ctypes.data_as(_u64p), C.c_size_t(out.size), C.byref(n))
        return rc, (out if rc == 0 else None)

    def fri_query_folded(self, betas) -> bytes:
        """ms_fri_query_folded: the MSFF blob - the final polynomial and one opened coset per round and query."""
        b, bp = _u64(betas)
        return self._sized_bytes(lambda out, cap, n: self.L.ms_fri_query_folded(self.h, bp, C.c_int(b.size), out, cap, n))

    # ---- the composition commitment and the DEEP stage (BUILD-DEFINED; include/ministark.h) -----------------------
    def validity_commit(self, lpn):
        """ms_validity_commit: (rc, root) of the tree over the chunk columns of the validity polynomial on the LDE coset; lpn = validity_ext * validity_len / N."""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_validity_commit(self.h, C.c_size_t(lpn), root)
        return rc, bytes(root)

    def validity_commit_coset(self, log_arity):
        """ms_validity_commit_coset: ms_validity_commit with the tree over coset leaf groups -> (rc, root)"""
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_validity_commit_coset(self.h, C.c_int(log_arity), root)
        return rc, bytes(root)

    def deep_evals(self, z, lists):
        """ms_deep_evals: (rc, evals) with evals[n] = F_{pt_poly[n]}(z_t), E limbs each, in entry order (deep_struct describes z and lists)."""
        s, keep = deep_struct(z, lists)
        n = 0 if keep["pt_poly"] is None else keep["pt_poly"].size
        out = np.zeros((max(1, n), self.e), dtype=np.uint64)
        rc = self.L.ms_deep_evals(self.h, C.byref(s), out.ctypes.data_as(_u64p))
        return rc, out[:n]

    def deep_compose(self, z, lists, gamma):
        """ms_deep_compose: installs the DEEP polynomial D' of the openings (z, lists) under the challenge gamma (E limbs; None passes a null pointer)."""
        s, _keep = deep_struct(z, lists)
        if gamma is None:
            return self.L.ms_deep_compose(self.h, C.byref(s), None)
        g, gp = _u64(gamma)
        if g.size != self.e:
            raise ValueError(f"deep_compose: gamma has {g.size} limbs, the extension has {self.e}")
        return self.L.ms_deep_compose(self.h, C.byref(s), gp)

    def deep_len(self):
        """ms_deep_len: N while a DEEP polynomial is installed, else 0."""
        return int(self.L.ms_deep_len(self.h))

    def query_linked(self, betas) -> bytes:
        """ms_query_linked: the whole query phase of a linked proof in one launch, the MSLQ blob (MSFI, then the LDE and validity rows under round 0's positions)."""
        b, bp = _u64(betas)
        return self._sized_bytes(lambda out, cap, n: self.L.ms_query_linked(self.h, bp, C.c_int(b.size), out, cap, n))

    def query_linked_folded(self, betas) -> bytes:
        """ms_query_linked_folded: the whole query phase of a linked proof over a folded FRI in one launch, the MSLF blob (MSFF, then one coset leaf group per query
        of the LDE, staged and validity trees)."""
        b, bp = _u64(betas)
        return self._sized_bytes(lambda out, cap, n: self.L.ms_query_linked_folded(self.h, bp, C.c_int(b.size), out, cap, n))

    # ---- standalone ----------------------------------------------------------------
    def merkle_commit(self, leafs, ext=1, lpn=2, ic=2):
        a, p = _u64(leafs)
        leaf_num = a.size // ext
        cap = max(1, 2 * leaf_num)
        nodes = np.zeros((cap, 32), dtype=np.uint8)
        nn = C.c_size_t(0)
        root = (C.c_uint8 * 32)()
        rc = self.L.ms_merkle_commit(self.h, p, C.c_size_t(leaf_num), C.c_int(ext), C.c_size_t(lpn), C.c_size_t(ic),
                                     nodes.ctypes.data_as(_u8p), C.c_size_t(cap), C.byref(nn), root)
        if rc != 0:
            return rc, None, None
        return 0, nodes[: nn.value].copy(), bytes(root)

    def merkle_prove(self, leafs, leaf, ext=1, lpn=2):
        a, p = _u64(leafs)
        l, lp = _u64(leaf)
        leaf_num = a.size // ext
        cap = 64 + lpn * ext * 8 + 64 * 64
        buf = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = self.L.ms_merkle_prove(self.h, p, C.c_size_t(leaf_num), C.c_int(ext), C.c_size_t(lpn), lp, buf.ctypes.data_as(_u8p), C.c_size_t(cap), C.byref(n))
        return (rc, None) if rc != 0 else (0, buf[: n.value].tobytes())

    def ntt(self, data, inverse=False):
        a = np.array(data, dtype=np.uint64)
        shape = a.shape
        a = np.ascontiguousarray(a.reshape(-1, shape[-1]))
        rc = self.L.ms_ntt(self.h, a.ctypes.data_as(_u64p), C.c_size_t(a.shape[1]), C.c_size_t(a.shape[0]), C.c_int(1 if inverse else 0))
        return rc, a.reshape(shape)

    def coset_lde(self, coeffs, shift, L):
        c = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.uint64)))
        out = np.zeros((c.shape[0], L), dtype=np.uint64)
        rc = self.L.ms_coset_lde(self.h, c.ctypes.data_as(_u64p), C.c_size_t(c.shape[1]), C.c_size_t(c.shape[0]), C.c_uint64(shift),
                                 out.ctypes.data_as(_u64p), C.c_size_t(L))
        return rc, out
