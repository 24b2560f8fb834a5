#!/usr/bin/env python3
"""Writes tests/golden/blake3_kats.json: BLAKE3 digests from an implementation that is neither this project's nor the tests' - the BLAKE3 C code that LLVM (>= 15)
carries and exports from its shared library (llvm_blake3_hasher_init / _update / _finalize).  Build-machine only: the tests read the JSON, never this script.
   python tests/golden/gen_blake3_kats.py [path/to/libLLVM.so]
Records: {"pattern": n} - the official test-vector input, byte i = i % 251, n bytes - or {"hex": "..."} - the input itself -, each with "blake3": 64 hex digits."""
import ctypes
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169, 8192, 8193,
                   16384, 31744]
EMPTY = "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
ABC = "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85"


def find_library(paths):
    for path in paths:
        try:
            lib = ctypes.CDLL(path)
        except OSError:
            continue
        if all(hasattr(lib, "llvm_blake3_hasher_" + n) for n in ("init", "update", "finalize")):
            return lib, path
    raise SystemExit("no libLLVM*.so exporting llvm_blake3_hasher_* found")


def main():
    paths = sys.argv[1:] or sorted(glob.glob("/usr/lib/x86_64-linux-gnu/libLLVM*.so*") + glob.glob("/usr/lib/llvm-*/lib/libLLVM*.so*"), reverse=True)
    lib, path = find_library(paths)
    for n in ("init", "update", "finalize"):
        getattr(lib, "llvm_blake3_hasher_" + n).restype = None

    def blake3(data, pieces=1):
        state = ctypes.create_string_buffer(4096)   # (the hasher struct is 1912 bytes in BLAKE3 1.3.1)
        lib.llvm_blake3_hasher_init(state)
        step = max(1, (len(data) + pieces - 1) // pieces)
        for i in range(0, len(data), step):
            piece = data[i:i + step]
            lib.llvm_blake3_hasher_update(state, piece, ctypes.c_size_t(len(piece)))
        out = ctypes.create_string_buffer(32)
        lib.llvm_blake3_hasher_finalize(state, out, ctypes.c_size_t(32))
        return out.raw.hex()

    assert blake3(b"") == EMPTY and blake3(b"abc") == ABC, "the library's BLAKE3 does not give the published digests"
    records = []
    for n in PATTERN_LENGTHS:
        data = bytes(i % 251 for i in range(n))
        d = blake3(data)
        assert d == blake3(data, 3) == blake3(data, 7)
        records.append({"pattern": n, "blake3": d})
    records.append({"hex": b"abc".hex(), "blake3": ABC})
    # leaf-style messages: decimal digits and the extension fields' affixes, every length 0 ... 200 and around the chunk boundaries
    text = (b"QuadExtField(18446744069414584320 + 1234567890123456789 * u)" b"2013265920" b"QuadExtField(QuadExtField(7 +  * u) + QuadExtField(2013265920 + 99 * u) * u)"
            b"10000000000000000000" b"31415926535897932384") * 40
    lengths = list(range(0, 201)) + [n + d for n in (1024, 2048, 3072) for d in (-2, -1, 0, 1, 2)]
    for k, n in enumerate(lengths):
        data = text[k % 97:k % 97 + n]
        assert len(data) == n
        records.append({"hex": data.hex(), "blake3": blake3(data)})
    with open(os.path.join(HERE, "blake3_kats.json"), "w") as f:
        json.dump({"source": "BLAKE3 C implementation exported by " + os.path.basename(path), "records": records}, f, indent=0)
        f.write("\n")
    print(len(records), "records from", path)


if __name__ == "__main__":
    main()
