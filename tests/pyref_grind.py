"""The proof-of-work predicate of include/ministark.h (pow_ok) and ms_grind's answer, restated as a linear search.
    d = D(seed[0..32] || nonce as 8 little-endian bytes), head = d[0..8] as a big-endian integer, pow_ok iff head < 2^(64 - bits)
D by ms_digest_id: hashlib.sha256 (0), hashlib.blake2s(digest_size=32) (1), tests/pyref_blake3.py (2), tests/pyref_keccak.py with the original padding (4),
hashlib.sha3_256 (5).  The searches over the two pure-Python hashes go through their batched (numpy) forms, which the same suites hold to the scalar ones.  Above SLOW_BITS bits the pure-Python BLAKE3 and Keccak-256 are too slow for a search: there the digest comes from host.hash_bytes (msh_hash),
which tests/test_blake3_emu.py and tests/test_keccak_emu.py pin against those two files."""
import functools
import hashlib
import struct

import pyref_blake3
import pyref_keccak

SHA256, BLAKE2S, BLAKE3, KECCAK256, SHA3_256 = 0, 1, 2, 4, 5
DIGESTS = (SHA256, BLAKE2S, BLAKE3, KECCAK256, SHA3_256)
SLOW_BITS = 9
PURE = {SHA256: lambda m: hashlib.sha256(m).digest(), BLAKE2S: lambda m: hashlib.blake2s(m, digest_size=32).digest(), BLAKE3: pyref_blake3.blake3,
        KECCAK256: lambda m: pyref_keccak.keccak(m, 0x01), SHA3_256: lambda m: hashlib.sha3_256(m).digest()}


def seed_of(k):
    return hashlib.sha256(b"ms_grind/%d" % k).digest()


def hasher(digest, bits):
    if bits > SLOW_BITS and digest in (BLAKE3, KECCAK256):
        from mini_stark_amd.host import hash_bytes
        return lambda m: hash_bytes(digest, m)
    return PURE[digest]


def head(h, seed, nonce):
    return int.from_bytes(h(seed + struct.pack("<Q", nonce))[:8], "big")


def pow_ok(digest, seed, nonce, bits, h=None):
    assert len(seed) == 32 and 0 <= bits <= 64
    return head(h or PURE[digest], seed, nonce) < (1 << (64 - bits))


@functools.lru_cache(maxsize=None)
def grind(digest, seed, bits, start=0, limit=2**64 - 1):
    """the smallest n in [start, start + limit) with pow_ok(digest, seed, n, bits), or None"""
    bound = 1 << (64 - bits)
    if bits <= SLOW_BITS and digest in (BLAKE3, KECCAK256):   # the same search, a batch of nonces at a time
        many = pyref_blake3.hash_many if digest == BLAKE3 else (lambda msgs: pyref_keccak.hash_many(msgs, 0x01))
        n, step = start, 64
        while n < start + limit:
            k = min(step, start + limit - n)
            for i, dg in enumerate(many([seed + struct.pack("<Q", n + i) for i in range(k)])):
                if int.from_bytes(dg.tobytes()[:8], "big") < bound:
                    return n + i
            n, step = n + k, min(4 * step, 1024)
        return None
    h = hasher(digest, bits)
    for n in range(start, start + limit):
        if head(h, seed, n) < bound:
            return n
    return None
