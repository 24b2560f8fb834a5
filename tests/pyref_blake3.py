"""BLAKE3 (unkeyed hash mode, 32-byte output) for the tests, independent of the product: nothing here comes from mini-stark_amd.

  blake3(data)          scalar pure Python, the whole specification (chunks of 1024 bytes, the binary tree of chunk chaining values)
  hash_many(messages)   numpy: the compression vectorised over messages of at most one chunk, walked block by block (longer messages go through the scalar code);
                        trees of 2^19 ... 2^21 leaf groups cost seconds
  tree_nodes(...)       MerkleTree::new over BLAKE3 (the counterpart of pyref_digest.tree_nodes)
  as_blake3()           runs tests/pyref.py (merkle_nodes, PyProver) over BLAKE3, as pyref_digest.as_blake2s does for BLAKE2s

Both implementations are pinned by tests/golden/blake3_kats.json (digests of the BLAKE3 C code LLVM ships; tests/golden/gen_blake3_kats.py) in tests/test_blake3_emu.py,
where the batched one is also compared with the scalar one on random messages."""
import contextlib
import json
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pyref
from pyref_digest import leaf_messages, fri_paths, expected_path  # noqa: F401  (digest-independent: message text, MSFP parsing, sibling positions)

BLAKE3 = 2   # ms_digest_id
IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
PERM = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
CHUNK = 1024
M32 = 0xFFFFFFFF
_G_INDEX = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


# ---------------------------------------------------------------------------------------------- scalar
def _compress(cv, m, counter, length, flags):
    """cv: 8 words, m: 16 words -> the first 8 words of the output"""
    v = list(cv) + list(IV[:4]) + [counter & M32, (counter >> 32) & M32, length, flags]
    m = list(m)
    for r in range(7):
        for k, (a, b, c, d) in enumerate(_G_INDEX):
            x, y = m[2 * k], m[2 * k + 1]
            v[a] = (v[a] + v[b] + x) & M32
            t = v[d] ^ v[a]; v[d] = ((t >> 16) | (t << 16)) & M32
            v[c] = (v[c] + v[d]) & M32
            t = v[b] ^ v[c]; v[b] = ((t >> 12) | (t << 20)) & M32
            v[a] = (v[a] + v[b] + y) & M32
            t = v[d] ^ v[a]; v[d] = ((t >> 8) | (t << 24)) & M32
            v[c] = (v[c] + v[d]) & M32
            t = v[b] ^ v[c]; v[b] = ((t >> 7) | (t << 25)) & M32
        m = [m[PERM[i]] for i in range(16)]
    return [v[i] ^ v[i + 8] for i in range(8)]


def _words(block):
    block = block + bytes(64 - len(block))
    return [int.from_bytes(block[4 * i:4 * i + 4], "little") for i in range(16)]


def _chunk_cv(data, counter, root):
    """one chunk (0 ... 1024 bytes; 0 only for the empty message)"""
    cv = list(IV)
    blocks = [data[i:i + 64] for i in range(0, len(data), 64)] or [b""]
    for i, blk in enumerate(blocks):
        last = i + 1 == len(blocks)
        flags = (CHUNK_START if i == 0 else 0) | (CHUNK_END if last else 0) | (ROOT if last and root else 0)
        cv = _compress(cv, _words(blk), counter, len(blk), flags)
    return cv


def _subtree(data, first_chunk, root):
    """chaining value of the subtree over `data` (its chunks are numbered from first_chunk on)"""
    if len(data) <= CHUNK:
        return _chunk_cv(data, first_chunk, root)
    nchunks = (len(data) + CHUNK - 1) // CHUNK
    left = 1
    while 2 * left < nchunks:   # the largest power of two of chunks that leaves the right subtree non-empty
        left *= 2
    l = _subtree(data[:left * CHUNK], first_chunk, False)
    r = _subtree(data[left * CHUNK:], first_chunk + left, False)
    return _compress(IV, l + r, 0, 64, PARENT | (ROOT if root else 0))


def blake3(data=b""):
    return b"".join(w.to_bytes(4, "little") for w in _subtree(bytes(data), 0, True))


class Blake3:
    """hashlib-shaped"""
    name, digest_size, block_size = "blake3", 32, 64

    def __init__(self, data=b""):
        self._data = bytearray(data)

    def update(self, data):
        self._data += data

    def digest(self):
        return blake3(self._data)

    def hexdigest(self):
        return self.digest().hex()


@contextlib.contextmanager
def as_blake3():
    real = pyref.hashlib
    pyref.hashlib = types.SimpleNamespace(sha256=Blake3)
    try:
        yield
    finally:
        pyref.hashlib = real


# ---------------------------------------------------------------------------------------------- numpy, one chunk per message
def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _compress_many(cv, m, length, flags):
    """cv: 8 arrays, m: 16 arrays (uint32, one entry per message), length / flags: uint32 arrays; counter 0"""
    n = cv[0].shape[0]
    v = list(cv) + [np.full(n, IV[i], dtype=np.uint32) for i in range(4)] + [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), length, flags]
    m = list(m)
    for r in range(7):
        for k, (a, b, c, d) in enumerate(_G_INDEX):
            v[a] = v[a] + v[b] + m[2 * k]
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 12)
            v[a] = v[a] + v[b] + m[2 * k + 1]
            v[d] = _rotr(v[d] ^ v[a], 8)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 7)
        m = [m[PERM[i]] for i in range(16)]
    return [v[i] ^ v[i + 8] for i in range(8)]


def _hash_batch(padded, lens):
    """padded: (n, 64 * B) uint8, zero behind each message; lens: (n,) byte counts <= 64 * B and <= 1024 -> (n, 32) uint8"""
    n = padded.shape[0]
    words = np.ascontiguousarray(padded).view("<u4").reshape(n, -1, 16)
    nblocks = np.maximum(1, (lens + 63) // 64)
    cv = [np.full(n, IV[i], dtype=np.uint32) for i in range(8)]
    for b in range(int(nblocks.max())):
        act = np.nonzero(nblocks > b)[0]
        everyone = act.size == n
        last = nblocks[act] == b + 1
        length = np.where(last, lens[act] - 64 * b, 64).astype(np.uint32)
        flags = (np.where(last, CHUNK_END | ROOT, 0) | (CHUNK_START if b == 0 else 0)).astype(np.uint32)
        blk = words[:, b, :] if everyone else words[act, b, :]
        out = _compress_many([c if everyone else c[act] for c in cv], [np.ascontiguousarray(blk[:, i]) for i in range(16)], length, flags)
        for i in range(8):
            if everyone:
                cv[i] = out[i]
            else:
                cv[i][act] = out[i]
    return np.stack(cv, axis=1).astype("<u4").view(np.uint8).reshape(n, 32)


_BATCH = 1 << 14   # messages per compression call: the 40 working arrays stay in cache
_POOL = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))   # (numpy releases the interpreter lock inside its loops)


def _hash_padded(padded, lens):
    n = padded.shape[0]
    if n <= _BATCH:
        return _hash_batch(padded, lens)
    parts = list(_POOL.map(lambda s: _hash_batch(padded[s:s + _BATCH], lens[s:s + _BATCH]), range(0, n, _BATCH)))
    return np.concatenate(parts, axis=0)


def hash_rows(rows):
    """rows: (n, L) uint8, every row one message of L bytes -> (n, 32) uint8"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, L = rows.shape
    if L > CHUNK:
        return np.frombuffer(b"".join(blake3(r.tobytes()) for r in rows), dtype=np.uint8).reshape(n, 32)
    width = max(64, (L + 63) // 64 * 64)
    if width != L:
        padded = np.zeros((n, width), dtype=np.uint8)
        padded[:, :L] = rows
    else:
        padded = rows
    return _hash_padded(padded, np.full(n, L, dtype=np.int64))


def hash_many(messages):
    """messages: a list of bytes -> (n, 32) uint8"""
    n = len(messages)
    lens = np.fromiter((len(m) for m in messages), dtype=np.int64, count=n)
    out = np.empty((n, 32), dtype=np.uint8)
    long = np.nonzero(lens > CHUNK)[0]
    for i in long:
        out[i] = np.frombuffer(blake3(messages[i]), dtype=np.uint8)
    short = np.nonzero(lens <= CHUNK)[0]
    if short.size:
        sl = lens[short]
        width = max(64, int((sl.max() + 63) // 64 * 64))
        flat = np.frombuffer(b"".join(messages[i] for i in short) if long.size else b"".join(messages), dtype=np.uint8)
        starts = np.cumsum(sl) - sl
        padded = np.zeros((short.size, width), dtype=np.uint8)
        row = np.repeat(np.arange(short.size), sl)
        col = np.arange(flat.size) - np.repeat(starts, sl)
        padded[row, col] = flat
        out[short] = _hash_padded(padded, sl)
    return out


def tree_nodes(values, ext, lpn, ic, zero_as_empty=True):
    """All nodes of MerkleTree::new over BLAKE3, level-major, root last, as an (n, 32) uint8 array (pyref_digest.tree_nodes)."""
    level = hash_many(leaf_messages(values, ext, lpn, zero_as_empty))
    out = [level]
    while level.shape[0] > 1:
        assert level.shape[0] % ic == 0
        level = hash_rows(level.reshape(-1, ic * 32))
        out.append(level)
    return np.concatenate(out, axis=0)


def load_kats():
    """[(input bytes, 32-byte digest)] of tests/golden/blake3_kats.json"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blake3_kats.json")) as f:
        recs = json.load(f)["records"]
    out = []
    for r in recs:
        data = bytes(i % 251 for i in range(r["pattern"])) if "pattern" in r else bytes.fromhex(r["hex"])
        out.append((data, bytes.fromhex(r["blake3"])))
    return out
