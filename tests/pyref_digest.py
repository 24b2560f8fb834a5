"""Expected values for the digest tests, from hashlib only (never from the code under test).

`with as_blake2s():` runs tests/pyref.py (merkle_nodes, PyProver) over BLAKE2s-256: pyref reaches its hash through the module attribute `hashlib.sha256`, so it is
handed a stand-in namespace and no copy of the file is needed.  `tree_nodes` is the same tree (src/merkle.rs:81-148) written for numpy input, fast enough for 2^21
leaf groups; `fri_paths` cuts the Merkle paths out of an MSFP blob (include/ministark.h)."""
import contextlib
import hashlib
import struct
import types

import numpy as np

import pyref

SHA256, BLAKE2S = 0, 1   # ms_digest_id


def blake2s256(data=b""):
    return hashlib.blake2s(data, digest_size=32)


HASH = {SHA256: hashlib.sha256, BLAKE2S: blake2s256}


@contextlib.contextmanager
def as_blake2s():
    real = pyref.hashlib
    pyref.hashlib = types.SimpleNamespace(sha256=blake2s256)
    try:
        yield
    finally:
        pyref.hashlib = real


def leaf_messages(values, ext, lpn, zero_as_empty=True):
    """values: canonical limbs, element-major (element f limb k at values[f * ext + k]).  One message per group of lpn elements: arkworks Display of each."""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    s = [str(x) for x in v.tolist()]
    if zero_as_empty:
        s = ["" if x == "0" else x for x in s]
    if ext == 2:
        s = ["QuadExtField(" + a + " + " + b + " * u)" for a, b in zip(s[0::2], s[1::2])]
    elif ext == 4:
        s = ["QuadExtField(QuadExtField(" + a + " + " + b + " * u) + QuadExtField(" + c + " + " + d + " * u) * u)" for a, b, c, d in zip(s[0::4], s[1::4], s[2::4], s[3::4])]
    else:
        assert ext == 1
    assert len(s) % lpn == 0
    return ["".join(s[g:g + lpn]).encode() for g in range(0, len(s), lpn)]


def tree_nodes(values, ext, lpn, ic, zero_as_empty=True, digest=BLAKE2S):
    """All nodes of MerkleTree::new, level-major, root last, as an (n, 32) uint8 array."""
    H = HASH[digest]
    level = [H(m).digest() for m in leaf_messages(values, ext, lpn, zero_as_empty)]
    out = list(level)
    while len(level) > 1:
        assert len(level) % ic == 0
        level = [H(b"".join(level[i:i + ic])).digest() for i in range(0, len(level), ic)]
        out += level
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 32)


def fri_paths(blob, e, windows, nq):
    """MSFP blob -> (records without the path siblings, list of (window, leaf index, [64-byte sibling pair per level]))."""
    pos, plain, paths = 0, [], []
    for i in range(windows):
        for _ in range(nq):
            head = (6 * e + 1) * 8
            (qlen,) = struct.unpack_from("<Q", blob, pos + 6 * e * 8)
            plain.append(blob[pos:pos + head + qlen * e * 8])
            pos += head + qlen * e * 8
            for _ in range(2):
                (idx,) = struct.unpack_from("<Q", blob, pos)
                (nlev,) = struct.unpack_from("<Q", blob, pos + 8 + 2 * e * 8)
                plain.append(blob[pos:pos + 16 + 2 * e * 8])
                pos += 16 + 2 * e * 8
                paths.append((i, idx, [blob[pos + 64 * l:pos + 64 * l + 64] for l in range(nlev)]))
                pos += 64 * nlev
    assert pos == len(blob)
    return plain, paths


def expected_path(nodes, ngroups, idx):
    """The sibling pairs of the binary tree `nodes` (lpn = 2) on the way up from the leaf with element index idx (merkle.rs:241-265)."""
    out, cur, off, n = [], idx // 2, 0, ngroups
    while n > 1:
        s = cur - cur % 2
        out.append(nodes[off + s].tobytes() + nodes[off + s + 1].tobytes())
        off += n
        n //= 2
        cur //= 2
    return out
