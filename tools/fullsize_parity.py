#!/usr/bin/env python3
"""One-off bit-exactness runs at sizes beyond the test-suite's budget: GPU proof vs the CPU oracle (OpenMP over its independent loops).
   python tools/fullsize_parity.py FIELD LOG_ROWS [THREADS [wide | blake2s | blake3 | keccak256 | sha3_256]]
   blake2s: the proof on a BLAKE2s-256 context (MS_FLAG_DIGEST_BLAKE2S) against a SHA-256 context and hashlib trees over every committed vector (tests/digest_cases.py;
   about 25 s of hashlib for the LDE tree of a 2^20-row proof).
   blake3: the same on a BLAKE3 context (MS_FLAG_DIGEST_BLAKE3) against the numpy BLAKE3 of tests/pyref_blake3.py (tests/blake3_cases.py).
   keccak256 / sha3_256: the same on a Keccak-256 / SHA3-256 context against tests/pyref_keccak.py / hashlib.sha3_256 (tests/keccak_cases.py)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import mini_stark_amd as ms
import parity_cases as pc
from oracle import oracle as orc
field, log_n = int(sys.argv[1]), int(sys.argv[2])
orc.set_threads(int(sys.argv[3]) if len(sys.argv) > 3 else 32)
cache = {}
def mk(f, fresh=False):
    if f not in cache: cache[f] = ms.Context(f)
    return cache[f]
t = time.time()
if len(sys.argv) > 4 and sys.argv[4] == "wide":   # BASELINE configs[4] shape: 64 trace columns, c = 128
    pc.case_prove_wide(mk, field, log_n=log_n, w=64)
    print(f"wide AIR (w=64, c=128), field {field}, 2^{log_n} rows, blowup 8: commitments, DEEP values, FRI rounds and FRI proof bit-exact vs the oracle ({time.time() - t:.0f} s)", flush=True)
    sys.exit(0)
if len(sys.argv) > 4 and sys.argv[4] == "blake2s":
    import digest_cases as dc
    dc.case_whole_proof(lambda f, flags, env=None: ms.Context(f, flags=flags), field, log_n, 8)
    print(f"field {field} 2^{log_n} rows, blowup 8, BLAKE2s-256: every root and Merkle path equal to hashlib's, everything else equal to the SHA-256 proof ({time.time() - t:.0f} s)", flush=True)
    sys.exit(0)
if len(sys.argv) > 4 and sys.argv[4] == "blake3":
    import blake3_cases as bc
    bc.case_whole_proof(lambda f, flags, env=None: ms.Context(f, flags=flags), field, log_n, 8)
    print(f"field {field} 2^{log_n} rows, blowup 8, BLAKE3: every root and Merkle path equal to pyref_blake3's, everything else equal to the SHA-256 proof ({time.time() - t:.0f} s)", flush=True)
    sys.exit(0)
if len(sys.argv) > 4 and sys.argv[4] in ("keccak256", "sha3_256"):
    import keccak_cases as kc
    d = 4 if sys.argv[4] == "keccak256" else 5
    kc.case_whole_proof(lambda f, flags, env=None: ms.Context(f, flags=flags), d, field, log_n, 8)
    print(f"field {field} 2^{log_n} rows, blowup 8, {sys.argv[4]}: every root and Merkle path equal to the expected trees', everything else equal to the SHA-256 proof ({time.time() - t:.0f} s)", flush=True)
    sys.exit(0)
pc.case_prove(mk, field, log_n, 8, nq_fri=0, read_big=False)
print(f"field {field} 2^{log_n} rows, blowup 8: every commitment, DEEP value, FRI round and the FRI proof bit-exact vs the oracle ({time.time() - t:.0f} s)", flush=True)
