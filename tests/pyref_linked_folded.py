"""Coset-grouped row trees, ms_query_linked_folded (the MSLF blob) and the link between a folded FRI's round 0 and those trees (msh_deep_link_verify_folded;
include/ministark.h, include/ministark_host.h - build-defined, no reference counterpart), restated with big integers and numpy index arithmetic.  The trees come from
pyref_open.tree_nodes over the leaf groups' elements IN HASHED ORDER: group j of a tree over an (L, c) matrix holds, for col = 0 .. c - 1 and then t = 0 .. a - 1,
column col of row j + t L / a - element col * a + t."""
import struct

import numpy as np

import pyref
import pyref_fri_folded as rf
import pyref_open as ro

MAGIC = int.from_bytes(b"MSLF", "little")


def coset_values(mat, k):
    """(L, c) matrix -> the committed vector of its coset tree, (L * c, 1): leaf group j at [j * a * c, (j + 1) * a * c), lpn = a * c"""
    m = np.ascontiguousarray(mat, dtype=np.uint64)
    L, c = m.shape
    a = 1 << k
    assert L % a == 0 and L // a >= 2
    g = m.reshape(a, L // a, c)                       # g[t, j, col] = mat[j + t L / a, col]
    return np.ascontiguousarray(g.transpose(1, 2, 0)).reshape(-1, 1)   # [j, col, t]


def coset_values_slow(mat, k):
    """the same vector by the definition's own loops (small shapes: holds coset_values to the text)"""
    L, c, a = len(mat), len(mat[0]), 1 << k
    return [[int(mat[j + t * (L // a)][col])] for j in range(L // a) for col in range(c) for t in range(a)]


def coset_tree(digest, mat, k):
    """(values, lpn, nodes) of the coset tree over `mat`: nodes level-major, the L / a leaf digests first, root last"""
    v = coset_values(mat, k)
    lpn = (1 << k) * np.asarray(mat).shape[1]
    return v, lpn, ro.tree_nodes(digest, v, 1, lpn)


def groups(betas, D0, L, k):
    """the leaf group query j opens in every row tree: q_j * s with q_j = (beta mod D_0) mod D_1 and s = L / D_0"""
    assert D0 <= L and L % D0 == 0
    return [int(b) % D0 % (D0 >> k) * (L // D0) for b in betas]


def mslf(msff, lde_open, stg_open, val_open):
    return struct.pack("<5Q", MAGIC, len(msff), len(lde_open), len(stg_open), len(val_open)) + msff + lde_open + stg_open + val_open


def split_mslf(blob):
    """(msff, lde openings, staged openings, validity openings), or None when the bytes are not exactly header + the four sections"""
    if len(blob) < 40:
        return None
    magic, a, b, c, d = struct.unpack_from("<5Q", blob, 0)
    if magic != MAGIC or 40 + a + b + c + d != len(blob):
        return None
    o = 40
    return blob[o:o + a], blob[o + a:o + a + b], blob[o + a + b:o + a + b + c], blob[o + a + b + c:]


# ---------------------------------------------------------------- msh_deep_link_verify_folded
def link_verify(field, digest, zero_as_empty, N, blowup, shift, k, c0, c1, m, lde_root, stg_root, val_root, zs, lists, evals, gamma, betas, msff, lde_open, stg_open, val_open):
    """(accepted, step): step one of "LDE opening", "staged opening", "validity opening", "DEEP link", "MSFF".  zs: the points (limb tuples), lists[t]: the column
    indices named at point t (index < c0 + c1: an LDE column; above: a validity chunk), evals: one limb tuple per entry in entry order"""
    f = pyref.FIELDS[field]
    p, e = f["p"], f["ext"]
    T = pyref.Tower(field, e)
    a, L, nq = 1 << k, N * blowup, len(betas)
    if len(msff) < 56:
        return False, "MSFF"
    magic, E, kk, R, nqh, D0, nfinal = struct.unpack_from("<7Q", msff, 0)
    if magic != rf.MAGIC or E != e or kk != k or nqh != nq or R < 1 or R > 64:
        return False, "MSFF"
    if D0 < a or D0 & (D0 - 1) or D0 > L or L % D0:
        return False, "MSFF"
    s = L // D0
    D1 = D0 >> k
    h0 = D1.bit_length() - 1
    psize = 16 + a * e * 8 + 64 * h0
    base = 56 + nfinal * e * 8
    if nfinal > D0 or len(msff) < base + nq * psize:
        return False, "MSFF"
    q = [int(b) % D0 % D1 for b in betas]
    rows = {}
    for name, blob, c, root in (("LDE opening", lde_open, c0, lde_root), ("staged opening", stg_open, c1, stg_root), ("validity opening", val_open, m, val_root)):
        if c == 0:
            if blob or root is not None:
                return False, name
            continue
        pos = 0
        for j in range(nq):
            ok, used = ro.check_path_index(digest, p, 1, a * c, zero_as_empty, root, blob[pos:], q[j] * s)
            if not ok:
                return False, name
            rows[name, j] = struct.unpack_from("<%dQ" % (a * c), blob, pos + 8)
            pos += used
        if pos != len(blob):
            return False, name
    gL = pyref.root_of_unity(field, L)
    gam = tuple(gamma)
    for j in range(nq):
        at = base + j * psize
        slots = struct.unpack_from("<%dQ" % (a * e), msff, at + 8)
        if struct.unpack_from("<Q", msff, at)[0] != q[j] * a or any(x >= p for x in slots):
            return False, "MSFF"
        for t in range(a):
            x = shift * pow(gL, q[j] * s + t * (L // a), p) % p
            acc, gp, n = T.zero(), T.one(), 0
            for pt, cols in enumerate(lists):
                den = T.sub(T.from_base(x), tuple(zs[pt]))
                if den == T.zero():
                    return False, "DEEP link"
                inv = T.inv(den)
                for col in cols:
                    if col < c0:
                        v = rows["LDE opening", j][col * a + t]
                    elif col < c0 + c1:
                        v = rows["staged opening", j][(col - c0) * a + t]
                    else:
                        v = rows["validity opening", j][(col - c0 - c1) * a + t]
                    acc = T.add(acc, T.mul(gp, T.mul(T.sub(T.from_base(v), tuple(evals[n])), inv)))
                    gp = T.mul(gp, gam)
                    n += 1
            if tuple(acc) != tuple(slots[t * e:(t + 1) * e]):
                return False, "DEEP link"
    return True, ""
