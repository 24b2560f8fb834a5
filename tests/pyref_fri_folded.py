"""Folded FRI (ms_fri_begin_folded .. ms_fri_query_folded, msh_fri_folded_verify; include/ministark.h - build-defined, no reference counterpart) restated with big
integers.  Nothing here is shared with the kernel: the fold is written twice, from its two definitions - Lagrange interpolation on the coset, and the coefficient
split f(X) = sum_s X^s f_s(X^a) folded as sum_s alpha^s f_s and evaluated forward -, the trees are pyref_open's (hashlib / pyref_blake3 / pyref_keccak), the blob, a
prover and a verifier follow the header's text.  Field arithmetic: pyref.Tower; an extension element is a tuple of E base limbs, a codeword a list of them.

Round i: codeword c_i on <g_i>, |<g_i>| = D_i, natural order; a = 2^k; D_(i+1) = D_i / a.  Leaf group j of round i's tree: c_i[j + t D_(i+1)], t < a."""
import struct

import numpy as np

import pyref
import pyref_open as ro

MAGIC = int.from_bytes(b"MSFF", "little")


def tower(field):
    return pyref.Tower(field, pyref.FIELDS[field]["ext"])


# ---------------------------------------------------------------- the fold, twice
def fold_lagrange_at(field, T, cw, k, alpha, b):
    """c_(i+1)[b]: P(alpha) for the P of degree < a through (x w^t, c_i[b + t D / a]), x = g^b, w = g^(D / a)"""
    p = T.p
    a, D = 1 << k, len(cw)
    m = D // a
    g = pyref.root_of_unity(field, D)
    xs = [pow(g, b + t * m, p) for t in range(a)]
    acc = T.zero()
    for t in range(a):
        num, den = T.one(), 1
        for u in range(a):
            if u != t:
                num = T.mul(num, T.sub(tuple(alpha), T.from_base(xs[u])))
                den = den * (xs[t] - xs[u]) % p
        acc = T.add(acc, T.mul(T.mul(tuple(cw[b + t * m]), num), T.from_base(pow(den, p - 2, p))))
    return acc


def fold_lagrange(field, cw, k, alpha, outputs=None):
    T = tower(field)
    m = len(cw) >> k
    return [fold_lagrange_at(field, T, cw, k, alpha, b) for b in (range(m) if outputs is None else outputs)]


def _fft(a, w, p):
    """a[i] -> sum_n a[n] w^(n i), radix 2, on integers"""
    n = len(a)
    if n == 1:
        return list(a)
    ev, od = _fft(a[0::2], w * w % p, p), _fft(a[1::2], w * w % p, p)
    out, x, h = [0] * n, 1, n // 2
    for i in range(h):
        t = od[i] * x % p
        out[i], out[i + h] = (ev[i] + t) % p, (ev[i] - t) % p
        x = x * w % p
    return out


def interpolate(field, cw):
    """coefficients (limb tuples) of the polynomial of degree < D with the values cw on <g_D>: the inverse transform, limb by limb (the domain is in the base field)"""
    p, D, e = pyref.FIELDS[field]["p"], len(cw), len(cw[0])
    winv, dinv = pow(pyref.root_of_unity(field, D), p - 2, p), pow(D, p - 2, p)
    limbs = [[v * dinv % p for v in _fft([c[l] for c in cw], winv, p)] for l in range(e)]
    return [tuple(limbs[l][n] for l in range(e)) for n in range(D)]


def evaluate(field, coef, D):
    """values on <g_D> of the polynomial with the D coefficients `coef`"""
    p, e = pyref.FIELDS[field]["p"], len(coef[0])
    limbs = [_fft([c[l] for c in coef], pyref.root_of_unity(field, D), p) for l in range(e)]
    return [tuple(limbs[l][n] for l in range(e)) for n in range(D)]


def fold_split(field, cw, k, alpha):
    """the same codeword from the coefficient side: f = sum_s X^s f_s(X^a), g = sum_s alpha^s f_s, evaluated on <g^a>"""
    T = tower(field)
    a, D = 1 << k, len(cw)
    f = interpolate(field, cw)
    apow = [T.one()]
    for _ in range(a - 1):
        apow.append(T.mul(apow[-1], tuple(alpha)))
    g = []
    for n in range(D // a):
        acc = T.zero()
        for s in range(a):
            acc = T.add(acc, T.mul(apow[s], f[a * n + s]))
        g.append(acc)
    return evaluate(field, g, D // a)


# ---------------------------------------------------------------- trees and blob
def coset_leaves(cw, k):
    """the committed vector in leaf order: group j = c[j + t D / a], t < a -> (D, e) limbs"""
    v = np.array(cw, dtype=np.uint64)
    a = 1 << k
    D, e = v.shape
    return np.ascontiguousarray(v.reshape(a, D // a, e).transpose(1, 0, 2)).reshape(D, e)


def coset_tree(digest, cw, k, zero_as_empty=True):
    lv = coset_leaves(cw, k)
    return lv, ro.tree_nodes(digest, lv, lv.shape[1], 1 << k, zero_as_empty)


def positions(betas, D0, k, R):
    """b[i][j] for i = 0 .. R: b_(0,j) = beta mod D_0, b_(i+1,j) = b_(i,j) mod D_(i+1)"""
    out, b = [], [int(x) % D0 for x in betas]
    out.append(b)
    for i in range(R):
        D = D0 >> (k * (i + 1))
        b = [x % D for x in b]
        out.append(b)
    return out


def msff_blob(e, k, leaves, nodes, final_poly, betas):
    """leaves[i], nodes[i]: coset_tree of round i; final_poly: (nfinal, e) limbs"""
    R, D0 = len(leaves), len(leaves[0])
    fin = np.asarray(final_poly, dtype=np.uint64).reshape(-1, e)
    out = bytearray(struct.pack("<7Q", MAGIC, e, k, R, len(betas), D0, fin.shape[0]))
    for x in fin.reshape(-1).tolist():
        out += struct.pack("<Q", x)
    pos = positions(betas, D0, k, R)
    for i in range(R):
        for grp in pos[i + 1]:
            out += ro.path_at(leaves[i], e, 1 << k, nodes[i], grp)
    return bytes(out)


# ---------------------------------------------------------------- prover
def prove(field, digest, c0, blowup, k, alphas, zero_as_empty=True, trees=True):
    """the commit phase from round 0's codeword (limb tuples): R = len(alphas) folds, the last one not committed.  Returns dict(cws, leaves, nodes, roots, final): the
    final polynomial is the first D_R / blowup coefficients of the last fold's interpolant (a prover that does not look at the rest; `high`: is anything above non-zero)"""
    R = len(alphas)
    cws = [list(c0)]
    for i in range(R):
        cws.append(fold_lagrange(field, cws[-1], k, alphas[i]))
    last = cws.pop()
    coef = interpolate(field, last)
    nfinal = len(last) // blowup
    out = dict(cws=cws, final=coef[:nfinal], high=any(any(c) for c in coef[nfinal:]), leaves=[], nodes=[], roots=[])
    if trees:
        for cw in cws:
            lv, nd = coset_tree(digest, cw, k, zero_as_empty)
            out["leaves"].append(lv); out["nodes"].append(nd); out["roots"].append(bytes(nd[-1]))
    return out


# ---------------------------------------------------------------- verifier
def verify_msff(field, digest, zero_as_empty, blowup, k, roots, alphas, betas, blob):
    """msh_fri_folded_verify with big integers: (accepted, step) - step is "", "header", "round i opening", "round i fold" or "final polynomial".  The order of the
    checks is the header's, the blob's length (which the header fixes), the final polynomial's limbs, every opening round by round, every fold, the final polynomial"""
    f = pyref.FIELDS[field]
    p, e = f["p"], f["ext"]
    T = tower(field)
    R, nq, a = len(roots), len(betas), 1 << k
    if len(blob) < 56:
        return False, "header"
    magic, E, kh, Rh, nqh, D0, nfinal = struct.unpack_from("<7Q", blob, 0)
    if magic != MAGIC or E != e or kh != k or Rh != R or nqh != nq:
        return False, "header"
    if D0 < 1 or D0 & (D0 - 1) or D0 > 1 << f["adicity"] or (D0 >> (k * R)) < blowup or (D0 >> (k * R)) << (k * R) != D0:
        return False, "header"
    DR = D0 >> (k * R)
    if nfinal != DR // blowup:
        return False, "header"
    heights = [((D0 >> (k * (i + 1)))).bit_length() - 1 for i in range(R)]
    psize = [16 + a * e * 8 + 64 * h for h in heights]
    if len(blob) != 56 + nfinal * e * 8 + nq * sum(psize):
        return False, "header"
    pos = 56
    fin = [struct.unpack_from("<%dQ" % e, blob, pos + 8 * e * n) for n in range(nfinal)]
    if any(x >= p for c in fin for x in c):
        return False, "final polynomial"
    pos += nfinal * e * 8
    b = positions(betas, D0, k, R)
    cos = {}
    for i in range(R):
        for j in range(nq):
            grp = b[i + 1][j]
            words = struct.unpack_from("<%dQ" % (2 + a * e), blob, pos)
            if words[-1] != heights[i]:
                return False, "round %d opening" % i
            ok, used = ro.check_path_index(digest, p, e, a, zero_as_empty, roots[i], blob[pos:pos + psize[i]], grp)
            if not ok or used != psize[i]:
                return False, "round %d opening" % i
            cos[i, j] = [tuple(words[1 + t * e:1 + (t + 1) * e]) for t in range(a)]
            pos += used
    assert pos == len(blob)

    def folded(i, j):
        """the fold of round i's opened coset at alpha_i: the value at position b_(i+1,j) of round i + 1"""
        D = D0 >> (k * i)
        m, grp = D // a, b[i + 1][j]
        cw = {grp + t * m: cos[i, j][t] for t in range(a)}
        return fold_lagrange_at(field, T, _Sparse(cw, D), k, alphas[i], grp)
    for i in range(1, R):
        Dn = D0 >> (k * (i + 1))
        for j in range(nq):
            if cos[i, j][b[i][j] // Dn] != folded(i - 1, j):
                return False, "round %d fold" % i
    gR = pyref.root_of_unity(field, DR)
    for j in range(nq):
        if pyref.peval(T, fin, T.from_base(pow(gR, b[R][j], p))) != folded(R - 1, j):
            return False, "final polynomial"
    return True, ""


class _Sparse:
    """a codeword of which only one coset is known"""
    def __init__(self, known, D):
        self.known, self.D = known, D

    def __len__(self):
        return self.D

    def __getitem__(self, i):
        return self.known[i]
