#!/usr/bin/env python3
"""Writes tests/golden/link_folded_tampered.bin: the inputs of msh_deep_link_verify_folded for one folded linked state (Goldilocks, SHA-256, the permutation statement,
N = 16, blowup 8, log_arity 2, three queries) made on the emulation build, and the truncated and tampered copies of tests/linked_folded_cases.py:link_fixture with the
verdict and the step the verifier gave for each.  The stand-alone sanitizer program tests/asan_link_folded/link_folded_asan.cpp reads it.  Little-endian:
  'MSKF' | u32 version 1 | u32 field, digest, N, blowup, log_arity, c0, c1, m, npts, nentries, nq | u64 shift | pt_begin (npts + 1 u32) | pt_poly (nentries u32)
  z (npts * E u64) | evals (nentries * E u64) | gamma (E u64) | betas (nq u64) | LDE root, staged root, validity root (32 bytes each)
  the four sections, u32 len and bytes each: MSFF, LDE openings, staged openings, validity openings
  u32 ncases | per case: u32 len, name | u32 section (0..3), u32 cut, u32 append, u32 nedits, per edit u32 offset, u32 len, bytes (the section cut to `cut` bytes, `append`
  zero bytes behind it, the edits written over that; the other three sections whole) | i32 rc | u32 len, the beginning of `why` up to its first colon
    python3 tests/golden/gen_link_folded_tampered.py"""
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
    out, cases = lf.link_fixture_bytes(lambda field, flags, env=None: ms.Context(field, flags=flags, lib_path=os.path.join(emu, "libministark_emu.so")))
    with open(os.path.join(HERE, "link_folded_tampered.bin"), "wb") as fh:
        fh.write(out)
    print(len(cases), "cases,", len(out), "bytes;", sum(1 for c in cases if c[5] == 1), "accepted")


if __name__ == "__main__":
    main()
