"""Keccak-256 (original padding, domain suffix 0x01: Ethereum's hash) and SHA3-256 (FIPS 202, suffix 0x06) for the tests, independent of the product: nothing here
comes from mini-stark_amd.  One sponge - Keccak-f[1600], rate 136 bytes, 32 bytes squeezed - with the suffix as a parameter.

  keccak(data, suffix)           scalar pure Python
  hash_many(messages, suffix)    numpy: the permutation vectorised over messages (uint64 lanes), walked block by block; trees of 2^17 ... 2^18 leaf groups cost
                                 a second or two
  tree_nodes(...)                MerkleTree::new over the sponge (the counterpart of pyref_digest.tree_nodes); suffix 0x06 may also be had from hashlib directly
  as_keccak(suffix)              runs tests/pyref.py (merkle_nodes, PyProver) over the sponge, as pyref_digest.as_blake2s does for BLAKE2s

Pinned in keccak_cases.case_pyref_pinned: suffix 0x06 against hashlib.sha3_256, suffix 0x01 against published Keccak-256 digests."""
import contextlib
import hashlib
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pyref
from pyref_digest import leaf_messages, fri_paths, expected_path  # noqa: F401  (digest-independent: message text, MSFP parsing, sibling positions)

KECCAK256, SHA3_256 = 4, 5   # ms_digest_id
SUFFIX = {KECCAK256: 0x01, SHA3_256: 0x06}
RATE = 136
M64 = (1 << 64) - 1
RC = (0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001, 0x8000000080008081, 0x8000000000008009,
      0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003,
      0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008)
# rotation offsets r[x][y] (FIPS 202 table 2) as lane x + 5 y
RHO = (0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14)


# ---------------------------------------------------------------------------------------------- scalar
def _rol(x, n):
    return ((x << n) | (x >> (64 - n))) & M64 if n else x


def _permute(a):
    for r in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for y in range(5):
            for x in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y], RHO[x + 5 * y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & M64 & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] ^= RC[r]
    return a


def keccak(data=b"", suffix=0x01):
    """pad10*1 with the domain suffix: `suffix` behind the message, 0x80 into the last byte of the block (one byte when both meet)"""
    data = bytearray(data)
    pad = RATE - len(data) % RATE
    data += bytes(pad)
    data[-pad] ^= suffix
    data[-1] ^= 0x80
    a = [0] * 25
    for off in range(0, len(data), RATE):
        for i in range(RATE // 8):
            a[i] ^= int.from_bytes(data[off + 8 * i:off + 8 * i + 8], "little")
        a = _permute(a)
    return b"".join(a[i].to_bytes(8, "little") for i in range(4))


class _Sponge:
    """hashlib-shaped"""
    digest_size, block_size, suffix, name = 32, RATE, 0x01, "keccak256"

    def __init__(self, data=b""):
        self._data = bytearray(data)

    def update(self, data):
        self._data += data

    def digest(self):
        return keccak(self._data, self.suffix)

    def hexdigest(self):
        return self.digest().hex()


class Keccak256(_Sponge):
    pass


class Sha3_256(_Sponge):
    suffix, name = 0x06, "sha3_256"


@contextlib.contextmanager
def as_keccak(suffix):
    real = pyref.hashlib
    pyref.hashlib = types.SimpleNamespace(sha256=Keccak256 if suffix == 0x01 else Sha3_256)
    try:
        yield
    finally:
        pyref.hashlib = real


# ---------------------------------------------------------------------------------------------- numpy, vectorised over messages
def _rol_many(x, n):
    return (x << np.uint64(n)) | (x >> np.uint64(64 - n)) if n else x


def _permute_many(a):
    """a: 25 uint64 arrays, one entry per message"""
    for r in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol_many(c[(x + 1) % 5], 1) for x in range(5)]
        b = [None] * 25
        for y in range(5):
            for x in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol_many(a[x + 5 * y] ^ d[x], RHO[x + 5 * y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] = a[0] ^ np.uint64(RC[r])
    return a


def _hash_batch(padded, nblocks):
    """padded: (n, 136 * B) uint8 with the padding in place; nblocks: (n,) blocks per message -> (n, 32) uint8"""
    n = padded.shape[0]
    lanes = np.ascontiguousarray(padded).view("<u8").reshape(n, -1, 17)
    a = [np.zeros(n, dtype=np.uint64) for _ in range(25)]
    for blk in range(int(nblocks.max())):
        act = np.nonzero(nblocks > blk)[0]
        if act.size == n:
            a = _permute_many([a[i] ^ lanes[:, blk, i] if i < 17 else a[i] for i in range(25)])
        else:
            out = _permute_many([a[i][act] ^ lanes[act, blk, i] if i < 17 else a[i][act] for i in range(25)])
            for i in range(25):
                a[i][act] = out[i]
    return np.stack(a[:4], axis=1).astype("<u8").view(np.uint8).reshape(n, 32)


_BATCH = 1 << 13   # messages per permutation call: the working arrays stay in cache
_POOL = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))   # (numpy releases the interpreter lock inside its loops)


def _hash_padded(padded, nblocks):
    n = padded.shape[0]
    if n <= _BATCH:
        return _hash_batch(padded, nblocks)
    parts = list(_POOL.map(lambda s: _hash_batch(padded[s:s + _BATCH], nblocks[s:s + _BATCH]), range(0, n, _BATCH)))
    return np.concatenate(parts, axis=0)


def _pad_in_place(padded, lens, suffix):
    nblocks = lens // RATE + 1
    rows = np.arange(padded.shape[0])
    padded[rows, lens] ^= np.uint8(suffix)
    padded[rows, nblocks * RATE - 1] ^= np.uint8(0x80)
    return nblocks


def hash_rows(rows, suffix):
    """rows: (n, L) uint8, every row one message of L bytes -> (n, 32) uint8"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, L = rows.shape
    padded = np.zeros((n, (L // RATE + 1) * RATE), dtype=np.uint8)
    padded[:, :L] = rows
    return _hash_padded(padded, _pad_in_place(padded, np.full(n, L, dtype=np.int64), suffix))


def hash_many(messages, suffix):
    """messages: a list of bytes -> (n, 32) uint8"""
    n = len(messages)
    lens = np.fromiter((len(m) for m in messages), dtype=np.int64, count=n)
    padded = np.zeros((n, int(lens.max() // RATE + 1) * RATE), dtype=np.uint8)
    flat = np.frombuffer(b"".join(messages), dtype=np.uint8)
    starts = np.cumsum(lens) - lens
    padded[np.repeat(np.arange(n), lens), np.arange(flat.size) - np.repeat(starts, lens)] = flat
    return _hash_padded(padded, _pad_in_place(padded, lens, suffix))


def tree_nodes(values, ext, lpn, ic, zero_as_empty=True, suffix=0x01):
    """All nodes of MerkleTree::new over the sponge, level-major, root last, as an (n, 32) uint8 array (pyref_digest.tree_nodes)."""
    level = hash_many(leaf_messages(values, ext, lpn, zero_as_empty), suffix)
    out = [level]
    while level.shape[0] > 1:
        assert level.shape[0] % ic == 0
        level = hash_rows(level.reshape(-1, ic * 32), suffix)
        out.append(level)
    return np.concatenate(out, axis=0)


def tree_nodes_hashlib(values, ext, lpn, ic, zero_as_empty=True):
    """The SHA3-256 tree by hashlib.sha3_256 alone"""
    H = hashlib.sha3_256
    level = [H(m).digest() for m in leaf_messages(values, ext, lpn, zero_as_empty)]
    out = list(level)
    while len(level) > 1:
        assert len(level) % ic == 0
        level = [H(b"".join(level[i:i + ic])).digest() for i in range(0, len(level), ic)]
        out += level
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 32)
