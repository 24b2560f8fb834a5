#!/usr/bin/env python3
"""Writes tests/golden/linked_v3_tampered.bin: one MSLP v3 proof (Goldilocks, SHA-256, the permutation statement with one argument, N = 16, log_arity 2, 4 grinding
bits) made by msh_stark_prove_linked_folded on the emulation build, and the truncated and tampered copies of tests/linked_folded_cases.py:v3_fixture with the verdict
and the step msh_stark_verify_linked_folded gave for each.  The stand-alone sanitizer program tests/asan_linked_v3/linked_v3_asan.cpp reads it.  Little-endian:
  'MSL3' | u32 version 1 | u32 field, digest, security_bits, blowup, steps, w, grinding_bits, N, log_arity, fri_folds, nargs, nch
  u32 len, msh_air_encode bytes | u32 len, msh_aux_encode bytes | u32 len, the proof's MSLP bytes
  u32 ncases | per case: u32 len, name | u32 cut, u32 append, u32 nedits, per edit u32 offset, u32 len, bytes (the proof cut to `cut` bytes, `append` zero bytes behind
  it, the edits written over that) | i32 rc | u32 len, the beginning of `why` up to its first colon
    python3 tests/golden/gen_linked_v3_tampered.py"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import mini_stark_amd as ms
    import linked_folded_cases as lf
    from mini_stark_amd.host import build_host_library
    emu = os.path.join(os.path.dirname(HERE), "emu")
    subprocess.check_call(["make", "-C", emu], stdout=subprocess.DEVNULL)
    build_host_library()
    out, cases = lf.v3_fixture_bytes(lambda field, flags, env=None: ms.Context(field, flags=flags, lib_path=os.path.join(emu, "libministark_emu.so")))
    with open(os.path.join(HERE, "linked_v3_tampered.bin"), "wb") as fh:
        fh.write(out)
    print(len(cases), "cases,", len(out), "bytes;", sum(1 for c in cases if c[4] == 1), "accepted")


if __name__ == "__main__":
    main()
