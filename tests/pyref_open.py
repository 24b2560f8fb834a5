"""Openings by index (ms_tree_open, ms_fri_query_index; include/ministark.h - build-defined, no reference counterpart) restated with big integers: the MerklePath at
a leaf-group index, the MSFI blob, and the verifying side (msh_merkle_path_check_index, msh_fri_index_verify).  The trees come from the digest files of this directory
(hashlib for SHA-256 / BLAKE2s / SHA3-256, pyref_blake3, pyref_keccak); pyref.merkle_nodes and pyref.PyProver cross-check them on the smallest shapes
(tests/open_cases.py).  Field arithmetic: pyref.Tower.

A MerklePath is  u64 leaf_index | lpn*ext u64 limbs | u64 nlevels | nlevels * 2 * 32 bytes  (ic = 2)."""
import struct

import numpy as np

import pyref
import pyref_blake3
import pyref_digest
import pyref_keccak
from pyref_grind import PURE, SHA256, BLAKE2S, BLAKE3, KECCAK256, SHA3_256

MAGIC = int.from_bytes(b"MSFI", "little")


def tree_nodes(digest, values, ext, lpn, zero_as_empty=True):
    """All nodes of the binary tree over `values` ((leaf_num, ext) canonical limbs), level-major, root last: an (n, 32) uint8 array."""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    if digest == BLAKE3:
        return pyref_blake3.tree_nodes(v, ext, lpn, 2, zero_as_empty)
    if digest == KECCAK256:
        return pyref_keccak.tree_nodes(v, ext, lpn, 2, zero_as_empty, 0x01)
    if digest == SHA3_256:
        return pyref_keccak.tree_nodes_hashlib(v, ext, lpn, 2, zero_as_empty)
    return pyref_digest.tree_nodes(v, ext, lpn, 2, zero_as_empty, digest)


def path_at(values, ext, lpn, nodes, group, leaf_index=None):
    """The MerklePath of leaf group `group`; its leaf_index word is group * lpn unless given (MSFI: the opened position)."""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, ext)
    ngroups = v.shape[0] // lpn
    assert 0 <= group < ngroups and len(nodes) == 2 * ngroups - 1
    out = bytearray(struct.pack("<Q", group * lpn if leaf_index is None else leaf_index))
    for x in v[group * lpn:(group + 1) * lpn].reshape(-1).tolist():
        out += struct.pack("<Q", x)
    nlevels = ngroups.bit_length() - 1
    out += struct.pack("<Q", nlevels)
    off, n, cur = 0, ngroups, group
    for _ in range(nlevels):
        s = cur - cur % 2
        out += bytes(nodes[off + s]) + bytes(nodes[off + s + 1])
        off, n, cur = off + n, n // 2, cur // 2
    return bytes(out)


def path_size(ext, lpn, ngroups):
    return 8 + lpn * ext * 8 + 8 + (ngroups.bit_length() - 1) * 64


def split_paths(blob, ext, lpn):
    """a concatenation of MerklePaths -> the list of their byte strings"""
    out, pos = [], 0
    while pos < len(blob):
        (nlev,) = struct.unpack_from("<Q", blob, pos + 8 + lpn * ext * 8)
        n = 8 + lpn * ext * 8 + 8 + nlev * 64
        out.append(blob[pos:pos + n])
        pos += n
    assert pos == len(blob)
    return out


def check_path_index(digest, p, ext, lpn, zero_as_empty, root, path, group, leaf_index=None):
    """msh_merkle_path_check_index: (accepted, bytes used) for the path at the head of `path`; its leaf_index word must be group * lpn unless another is given (MSFI)"""
    head = 8 + lpn * ext * 8 + 8
    if len(path) < head:
        return False, 0
    words = struct.unpack_from("<%dQ" % (head // 8), path, 0)
    nlev = words[-1]
    if nlev > 64 or len(path) - head < nlev * 64:
        return False, 0
    used = head + nlev * 64
    limbs = words[1:-1]
    if words[0] != (group * lpn if leaf_index is None else leaf_index) or any(x >= p for x in limbs) or (nlev < 64 and group >> nlev):
        return False, used
    msg = "".join(pyref.display(tuple(limbs[i * ext:(i + 1) * ext]), zero_as_empty) for i in range(lpn)).encode()
    H = PURE[digest]
    cur = H(msg)
    for l in range(nlev):
        pair = path[head + 64 * l:head + 64 * l + 64]
        slot = (group >> l) & 1
        if pair[32 * slot:32 * slot + 32] != cur:
            return False, used
        cur = H(pair)
    return cur == bytes(root), used


# ---------------------------------------------------------------- MSFI
def positions(betas, D0, windows):
    """[(first position, second position) per query] per window: b_(0,j) = beta mod D_0, b_(i+1,j) = b_(i,j) mod D_(i+1)"""
    out, b = [], [int(x) for x in betas]
    for i in range(windows):
        D = D0 >> i
        b = [x % D for x in b]
        out.append([(x, (x + D // 2) % D) for x in b])
    return out


def msfi_blob(e, codewords, nodes, final_poly, betas):
    """codewords[i]: (D_i, e) limbs of round i; nodes[i]: its tree (lpn = 2); final_poly: (nfinal, e) limbs of the last round's polynomial"""
    R = len(codewords)
    D0 = len(codewords[0])
    fin = np.ascontiguousarray(final_poly, dtype=np.uint64).reshape(-1, e)
    out = bytearray(struct.pack("<6Q", MAGIC, e, R, len(betas), D0, fin.shape[0]))
    for x in fin.reshape(-1).tolist():
        out += struct.pack("<Q", x)
    for i, row in enumerate(positions(betas, D0, R - 1)):
        assert len(codewords[i]) == D0 >> i
        for pair in row:
            for pos in pair:
                out += path_at(codewords[i], e, 2, nodes[i], pos // 2, leaf_index=pos)
    return bytes(out)


def msfi_parse(blob, e):
    """(header words, final polynomial as limb tuples, paths[window][query][0 / 1] as byte strings); AssertionError when the bytes do not parse exactly"""
    assert len(blob) >= 48
    hd = struct.unpack_from("<6Q", blob, 0)
    magic, E, R, nq, D0, nfinal = hd
    assert magic == MAGIC and E == e and R >= 1 and nq >= 1
    pos = 48
    assert len(blob) - pos >= nfinal * e * 8
    fin = [struct.unpack_from("<%dQ" % e, blob, pos + 8 * e * k) for k in range(nfinal)]
    pos += nfinal * e * 8
    paths = []
    for i in range(R - 1):
        row = []
        for _ in range(nq):
            pair = []
            for _ in range(2):
                assert len(blob) - pos >= 16 + 2 * e * 8
                (nlev,) = struct.unpack_from("<Q", blob, pos + 8 + 2 * e * 8)
                n = 16 + 2 * e * 8 + nlev * 64
                assert nlev <= 64 and len(blob) - pos >= n
                pair.append(blob[pos:pos + n])
                pos += n
            row.append(pair)
        paths.append(row)
    assert pos == len(blob), "trailing bytes"
    return hd, fin, paths


def msfp_paths(blob, e, windows, nq):
    """the MerklePaths inside an MSFP blob (ms_fri_query), as byte strings: [window][query][0 / 1]"""
    pos, out = 0, []
    for _ in range(windows):
        row = []
        for _ in range(nq):
            (qlen,) = struct.unpack_from("<Q", blob, pos + 6 * e * 8)
            pos += (6 * e + 1) * 8 + qlen * e * 8
            pair = []
            for _ in range(2):
                (nlev,) = struct.unpack_from("<Q", blob, pos + 8 + 2 * e * 8)
                n = 16 + 2 * e * 8 + nlev * 64
                pair.append(blob[pos:pos + n])
                pos += n
            row.append(pair)
        out.append(row)
    assert pos == len(blob)
    return out


def verify_msfi(field, digest, zero_as_empty, blowup, roots, zs, Bs, alphas, betas, blob):
    """msh_fri_index_verify with big integers: (accepted, why).  roots: R 32-byte strings; zs, alphas: R - 1 limb tuples; Bs: R - 1 pairs of limb tuples."""
    f = pyref.FIELDS[field]
    p, e = f["p"], f["ext"]
    T = pyref.Tower(field, e)
    R, nq, W = len(roots), len(betas), len(roots) - 1
    if len(blob) < 48:
        return False, "short"
    magic, E, Rh, nqh, D0, nfinal = struct.unpack_from("<6Q", blob, 0)
    if magic != MAGIC or E != e or Rh != R or nqh != nq:
        return False, "header"
    if D0 < 2 or D0 & (D0 - 1) or D0 > 1 << f["adicity"] or (D0 >> W) < 2:
        return False, "domain"
    if nfinal > max(1, (D0 >> W) // blowup):
        return False, "final polynomial too long"
    pos = 48
    if (len(blob) - pos) // 8 < nfinal * e:
        return False, "truncated"
    fin = [struct.unpack_from("<%dQ" % e, blob, pos + 8 * e * k) for k in range(nfinal)]
    if any(x >= p for c in fin for x in c):
        return False, "final polynomial not canonical"
    pos += nfinal * e * 8
    pp = positions(betas, D0, W)
    y = {}
    for i in range(W):
        D = D0 >> i
        for j in range(nq):
            for s in range(2):
                at = pp[i][j][s]
                head = 16 + 2 * e * 8
                if len(blob) - pos < head:
                    return False, "truncated"
                words = struct.unpack_from("<%dQ" % (head // 8), blob, pos)
                if words[0] != at:
                    return False, "leaf_index"
                if words[-1] != (D // 2).bit_length() - 1:
                    return False, "height"
                ok, used = check_path_index(digest, p, e, 2, zero_as_empty, roots[i], blob[pos:], at // 2, leaf_index=at)
                if not ok:
                    return False, "path"
                y[i, j, s] = tuple(words[1 + (at & 1) * e:1 + (at & 1) * e + e])
                pos += used
    if pos != len(blob):
        return False, "trailing bytes"
    for i in range(W):
        D = D0 >> i
        g = pyref.root_of_unity(field, D)
        for j in range(nq):
            x1 = pow(g, pp[i][j][0], p)
            x3 = T.from_base(x1 * x1 % p)
            y1, y2 = y[i, j, 0], y[i, j, 1]
            y3 = y[i + 1, j, 0] if i + 1 < W else pyref.peval(T, fin, x3)
            a = T.mul(T.sub(y2, y1), T.from_base(pow((-2 * x1) % p, p - 2, p)))
            lhs = T.add(T.sub(y1, T.mul(a, T.from_base(x1))), T.mul(a, tuple(alphas[i])))
            deep = T.add(T.mul(y3, T.sub(x3, tuple(zs[i]))), T.add(tuple(Bs[i][0]), T.mul(tuple(Bs[i][1]), tuple(alphas[i]))))
            if lhs != deep:
                return False, "linearity"
    return True, ""
