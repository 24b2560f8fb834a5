#!/usr/bin/env python3
"""Writes tests/golden/linked_verdicts.json: what the three linked-proof drivers and verifiers (MSLP v1, v2, v3) give on the emulation build - per case of
tests/linked_folded_cases.py:verdict_cases the SHA-256 of the proof's bytes, and the whole (rc, why) msh_stark_verify_linked{,_aux,_folded} gives for every tampered
copy: the edit lists of linked_cases.tampered_edits (v1), linked_folded_cases.v2_edits (v2) and linked_folded_cases.v3_edits (v3).
  {"table": [[rc, why], ..], "cases": {name: {"sha256": hex, "verdicts": [index into table, one per edit, in the list's order], "truncations": hex}}}
"truncations" (v2 only): SHA-256 over one line 'rc|why' per truncation length 0 .. len - 1.  tests/test_linked_folded_emu.py regenerates and compares.
    python3 tests/golden/gen_linked_verdicts.py"""
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
    text = lf.linked_verdicts_text(lf.linked_verdicts(lambda field, flags, env=None: ms.Context(field, flags=flags, lib_path=os.path.join(emu, "libministark_emu.so"))))
    with open(os.path.join(HERE, "linked_verdicts.json"), "w") as fh:
        fh.write(text)
    print(text.count('"sha256"'), "cases,", len(text), "bytes")


if __name__ == "__main__":
    main()
