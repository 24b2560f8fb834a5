"""The composition commitment and the DEEP stage (ms_validity_commit, ms_deep_evals, ms_deep_compose, msh_deep_link_verify, msh_validity_from_chunks;
include/ministark.h, include/ministark_host.h - build-defined, no reference counterpart) restated with big integers from their definitions:

  chunk column k * ve + l  = the coefficients [kN, (k+1)N) of limb plane l of the validity polynomial;   V(x) = sum_k x^(kN) sum_l u_l V_(k,l)(x)
  A_t(x) = sum_(n in point t) gamma^n F_(pt_poly[n])(x),  D(x) = sum_t (A_t(x) - A_t(z_t)) / (x - z_t),  D'(y) = D(shift y)
  the link: at row p = b (L / D_0), x = shift g_L^p:  sum_n gamma^n (F_n(x) - eval_n) / (x - z_t(n))  ==  the value round 0 opened at position b.

Field arithmetic: pyref.Tower over Python integers; trees and paths: pyref_open.  Nothing here is derived from the C++."""
import struct

import numpy as np

import pyref
import pyref_open as ro
from common import MODULUS, EXT


def tower(field):
    return pyref.Tower(field, EXT[field])


def chunk_columns(val, ve, N):
    """val: the validity polynomial as VL coefficients (ints for ve = 1, limb tuples for ve > 1) -> the m = ve * VL / N chunk columns, N base-field integers each"""
    rows = [(int(c),) if ve == 1 else tuple(int(x) for x in c) for c in val]
    assert len(rows) % N == 0 and all(len(r) == ve for r in rows)
    return [[rows[k * N + i][l] for i in range(N)] for k in range(len(rows) // N) for l in range(ve)]


def chunk_lde(field, cols, shift, L):
    """the L x m row-major matrix of the chunk columns on shift * <g_L>"""
    ev = [pyref.coset_eval(field, c, shift, L) for c in cols]
    return np.array([[ev[j][i] for j in range(len(cols))] for i in range(L)], dtype=np.uint64)


def horner_base(T, coeffs, z):
    """sum_k c_k z^k for base-field coefficients and z in K"""
    acc = T.zero()
    for c in reversed(coeffs):
        acc = T.add(T.mul(acc, z), T.from_base(c))
    return acc


def deep_evals(field, F, zs, lists):
    """F: the c + m coefficient columns; -> F_(pt_poly[n])(z_t) in entry order"""
    T = tower(field)
    return [horner_base(T, F[j], tuple(zs[t])) for t, lst in enumerate(lists) for j in lst]


def validity_from_chunks(field, ve, N, z, chunk_evals):
    """V(z) from the m chunk evaluations (elements of K)"""
    T = tower(field)
    zN = T.pow(tuple(z), N)
    acc, zk = T.zero(), T.one()
    for k in range(len(chunk_evals) // ve):
        for l in range(ve):
            u = tuple(1 if i == l else 0 for i in range(T.e))
            acc = T.add(acc, T.mul(zk, T.mul(u, tuple(chunk_evals[k * ve + l]))))
        zk = T.mul(zk, zN)
    return acc


def deep_poly(field, F, zs, lists, gamma, shift, N):
    """D' as N coefficients of K (zero above its degree)"""
    T, p = tower(field), MODULUS[field]
    D = [T.zero()] * N
    gp = T.one()
    for t, lst in enumerate(lists):
        A = [T.zero()] * N
        for j in lst:
            A = [T.add(a, tuple(g * c % p for g in gp)) for a, c in zip(A, F[j])]
            gp = T.mul(gp, tuple(gamma))
        # synthetic division by (x - z_t): q_(N-2) = a_(N-1), q_(k-1) = a_k + z q_k; the remainder a_0 + z q_0 is A_t(z_t) and is dropped
        q, carry = [T.zero()] * N, T.zero()
        for k in range(N - 1, 0, -1):
            carry = T.add(A[k], T.mul(carry, tuple(zs[t])))
            q[k - 1] = carry
        D = [T.add(a, b) for a, b in zip(D, q)]
    return [tuple(x * pow(shift, k, p) % p for x in D[k]) for k in range(N)]


def composition_at(field, values, evals, zs, lists, gamma, x):
    """sum_n gamma^n (F_n(x) - eval_n) / (x - z_t(n)) from the opened values[j] = F_j(x) (base field)"""
    T = tower(field)
    acc, gp, n = T.zero(), T.one(), 0
    for t, lst in enumerate(lists):
        inv = T.inv(T.sub(T.from_base(x), tuple(zs[t])))
        for j in lst:
            acc = T.add(acc, T.mul(gp, T.mul(T.sub(T.from_base(values[j]), tuple(evals[n])), inv)))
            gp = T.mul(gp, tuple(gamma))
            n += 1
    return acc


def link_rows(betas, D0, L):
    """the 2 nq rows of both trees the link verifier wants opened, in its order"""
    step = L // D0
    out = []
    for b in betas:
        b = int(b) % D0
        out += [b * step, ((b + D0 // 2) % D0) * step]
    return out


def link_verify(field, digest, zae, N, blowup, shift, c, m, lde_root, val_root, zs, lists, evals, gamma, betas, msfi, lde_open, val_open):
    """(accepted, the step that refused: "" / "msfi" / "lde" / "validity" / "link")"""
    T, p, e = tower(field), MODULUS[field], EXT[field]
    L = N * blowup
    try:
        hd, fin, paths = ro.msfi_parse(msfi, e)
    except (AssertionError, struct.error):
        return False, "msfi"
    R, nq, D0 = hd[2], hd[3], hd[4]
    if nq != len(betas) or D0 < 1 or D0 & (D0 - 1) or D0 > L or L % D0:
        return False, "msfi"
    gL, g0 = pyref.root_of_unity(field, L), pyref.root_of_unity(field, D0)
    lpos = vpos = 0
    for j, b in enumerate(betas):
        b = int(b) % D0
        for s, pos in enumerate((b, (b + D0 // 2) % D0)):
            row = pos * (L // D0)
            ok, used = ro.check_path_index(digest, p, 1, c, zae, lde_root, lde_open[lpos:], row)
            if not ok:
                return False, "lde"
            lrow = struct.unpack_from("<%dQ" % c, lde_open, lpos + 8)
            lpos += used
            ok, used = ro.check_path_index(digest, p, 1, m, zae, val_root, val_open[vpos:], row)
            if not ok:
                return False, "validity"
            vrow = struct.unpack_from("<%dQ" % m, val_open, vpos + 8)
            vpos += used
            x = shift * pow(gL, row, p) % p
            got = composition_at(field, list(lrow) + list(vrow), evals, zs, lists, gamma, x)
            if R > 1:
                path = paths[0][j][s]
                if struct.unpack_from("<Q", path, 0)[0] != pos:
                    return False, "msfi"
                y = struct.unpack_from("<%dQ" % e, path, 8 + (pos & 1) * e * 8)
            else:
                y, xb = T.zero(), T.from_base(pow(g0, pos, p))
                for cf in reversed(fin):
                    y = T.add(T.mul(y, xb), tuple(cf))
            if tuple(got) != tuple(y):
                return False, "link"
    if lpos != len(lde_open):
        return False, "lde"
    if vpos != len(val_open):
        return False, "validity"
    return True, ""
