"""What the resource-ownership tests share, on the raw C ABI of the emulation build (tests/emu): the reference's prove sequence stage by stage, the live-resource
counters of the emulated runtime (ms_emu_live) and its three failure hooks."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np

from common import MODULUS, EXT, SplitMix64, fibonacci_trace, fibonacci_closures
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
U64P = C.POINTER(C.c_uint64)
KINDS = ("device buffers", "page-locked buffers", "streams", "events", "copy-engine signals")


def load():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    L = C.CDLL(EMU)
    L.ms_emu_alloc_count.restype = C.c_long
    L.ms_emu_fail_alloc_after.argtypes = [C.c_long]
    L.ms_emu_fail_device_alloc_after.argtypes = [C.c_long]
    L.ms_emu_fail_handle_after.argtypes = [C.c_long]
    L.ms_last_error.restype = C.c_char_p
    L.ms_fri_proof_size.restype = C.c_size_t
    L.ms_fri_proof_size.argtypes = [C.c_void_p]
    L.ms_pinned_alloc.restype = C.c_void_p
    L.ms_pinned_alloc.argtypes = [C.c_size_t]
    L.ms_pinned_free.argtypes = [C.c_void_p]
    gc.collect()   # (a context of an earlier test that is still waiting for the collector would be destroyed in the middle of a balance)
    return L


def live(L):
    """(device buffers, page-locked buffers, streams, events, copy-engine signals) the emulated runtime has handed out and not taken back"""
    out = (C.c_long * 7)()
    L.ms_emu_live(out)
    return tuple(out[:5])


def made(L):
    """(device and page-locked allocations, handle creations) so far"""
    out = (C.c_long * 7)()
    L.ms_emu_live(out)
    return out[5], out[6]


def create(L, field, flags=1):
    h = C.c_void_p()
    rc = L.ms_create(C.byref(h), 0, field, flags)
    return rc, h


def stages(L, h, field, outs=None, N=16, blowup=4, rounds=6, read=True):
    """the reference's prove sequence (Fibonacci AIR) as raw C calls: yields (name, rc); `outs` (a list) collects every output of the proof"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(5)
    root = (C.c_uint8 * 32)()
    t = np.ascontiguousarray(fibonacci_trace(field, N))
    omega = orc.root_of_unity(field, N)

    def keep(*vals):
        if outs is not None:
            outs.extend(bytes(v) for v in vals)
    yield "trace_commit", L.ms_trace_commit(h, t.ctypes.data_as(U64P), C.c_size_t(N), C.c_size_t(3), C.c_size_t(6), root)
    keep(root)
    yield "interpolate", L.ms_interpolate(h)
    for sc, idx in fibonacci_closures(field, N, omega):
        yield "polys_lincomb", L.ms_polys_lincomb(h, (C.c_uint64 * len(sc))(*sc), (C.c_int * len(idx))(*idx), len(sc))
    yield "lde_commit", L.ms_lde_commit(h, C.c_size_t(blowup), C.c_uint64(rng.nonzero(p)), C.c_size_t(6), root)
    keep(root)
    yield "mix", L.ms_mix(h, C.c_uint64(rng.field(p)))
    out = (C.c_uint64 * (7 * e))()
    yield "eval_ext", L.ms_eval_ext(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), 1, out)
    keep(out)
    yield "fri_begin", L.ms_fri_begin(h, C.c_size_t(blowup), C.c_size_t(rounds), root)
    keep(root)
    B = (C.c_uint64 * (2 * e))()
    for _ in range(1, rounds):
        yield "fri_deep", L.ms_fri_deep(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), B)
        yield "fri_fold_commit", L.ms_fri_fold_commit(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), root)
        keep(B, root)
    yield "fri_query", L.ms_fri_query(h, (C.c_uint64 * 2)(3, 77), 2)
    if outs is not None and read:
        blob = (C.c_uint8 * L.ms_fri_proof_size(h))()
        yield "fri_proof_read", L.ms_fri_proof_read(h, blob)
        keep(blob)
    yield "ntt", L.ms_ntt(h, (C.c_uint64 * 64)(*range(64)), C.c_size_t(64), C.c_size_t(1), 0)
    yield "merkle_commit", L.ms_merkle_commit(h, (C.c_uint64 * 16)(*range(16)), C.c_size_t(16), 1, C.c_size_t(2), C.c_size_t(2), None, C.c_size_t(0), None, root)
    keep(root)


def first_failure(gen):
    for name, rc in gen:
        if rc != 0:
            return name, rc
    return None


def standalone_calls(L, h, field):
    """name -> callable returning (rc, output bytes): the entry points that work on buffers of their own"""
    e = EXT[field]
    root = (C.c_uint8 * 32)()

    def ntt():
        d = (C.c_uint64 * 64)(*range(64))
        return L.ms_ntt(h, d, C.c_size_t(64), C.c_size_t(1), 0), bytes(d)

    def coset_lde():
        out = (C.c_uint64 * 64)()
        return L.ms_coset_lde(h, (C.c_uint64 * 16)(*range(1, 17)), C.c_size_t(16), C.c_size_t(1), C.c_uint64(3), out, C.c_size_t(64)), bytes(out)

    def merkle_commit():
        nodes = (C.c_uint8 * (32 * 64))()
        nn = C.c_size_t()
        rc = L.ms_merkle_commit(h, (C.c_uint64 * 64)(*range(64)), C.c_size_t(64), 1, C.c_size_t(2), C.c_size_t(2), nodes, C.c_size_t(64), C.byref(nn), root)
        return rc, bytes(nodes) + bytes(root)

    def merkle_prove():
        out = (C.c_uint8 * 1024)()
        n = C.c_size_t()
        rc = L.ms_merkle_prove(h, (C.c_uint64 * (64 * e))(*range(64 * e)), C.c_size_t(64), e, C.c_size_t(2), (C.c_uint64 * e)(*range(5 * e, 6 * e)), out, C.c_size_t(1024), C.byref(n))
        return rc, bytes(out)

    def arith_selftest():
        out = (C.c_uint64 * 8)()
        return L.ms_arith_selftest(h, 2, (C.c_uint64 * 8)(*range(3, 11)), (C.c_uint64 * 8)(*range(20, 28)), out, C.c_size_t(8)), bytes(out)
    return {"ntt": ntt, "coset_lde": coset_lde, "merkle_commit": merkle_commit, "merkle_prove": merkle_prove, "arith_selftest": arith_selftest}
