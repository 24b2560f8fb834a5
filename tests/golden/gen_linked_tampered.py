#!/usr/bin/env python3
"""Writes tests/golden/linked_tampered.bin: one linked proof (Goldilocks, SHA-256, the fib program, N = 8, R = 3, 4 grinding bits) made on the emulation build, and the
truncated and tampered copies of tests/linked_cases.py:tampered_fixture with the verdict and the step msh_stark_verify_linked gave for each.  The stand-alone
sanitizer program tests/asan/linked_verify_asan.cpp reads it (tests/asan/Makefile).  Little-endian:
  'MSLF' | u32 version 1 | u32 field, digest, security_bits, blowup, steps, w, grinding_bits, N, fri_rounds | u32 len, msh_air_encode bytes
  u32 len, the proof's MSLP bytes
  u32 ncases | per case: u32 len, name | u32 cut, u32 append, u32 nedits, per edit u32 offset, u32 len, bytes (the proof cut to `cut` bytes, `append` zero bytes behind
  it, the edits written over that) | i32 rc | u32 len, the beginning of `why` up to its first colon
    python3 tests/golden/gen_linked_tampered.py"""
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import mini_stark_amd as ms
    import linked_cases as lc
    from mini_stark_amd.host import build_host_library
    emu = os.path.join(os.path.dirname(HERE), "emu")
    subprocess.check_call(["make", "-C", emu], stdout=subprocess.DEVNULL)
    build_host_library()
    out, cases = lc.fixture_bytes(lambda field, flags, env=None: ms.Context(field, flags=flags, lib_path=os.path.join(emu, "libministark_emu.so")))
    with open(os.path.join(HERE, "linked_tampered.bin"), "wb") as fh:
        fh.write(out)
    print(len(cases), "cases,", len(out), "bytes;", sum(1 for c in cases if c[4] == 1), "accepted")


if __name__ == "__main__":
    main()
