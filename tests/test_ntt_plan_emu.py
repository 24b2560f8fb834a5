"""CPU suite: the NTT plan a context builds - its shape and the kernel instance of every pass, both chosen when the plan is built - as the emulation build reports it
(ms_emu_ntt_plan: the shape alone, no table, nothing on the device, so 2^32 points answer as fast as 2^3), against tests/pyref_ntt_plan.py, the restatement of the
rule the library had while every launch chose its instance again.  For both fields, every size up to the two-adicity, every zero-padding factor, both directions,
one and several columns, under every NTT knob the suites and the A/B tools set.  No kernel runs in the enumeration; the last test ties the view to real launches."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mini_stark_amd as ms
import ntt_directed_cases as nd
import pyref_ntt_plan as ref

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
ERR_STATE = -4   # MS_ERR_STATE (include/ministark.h): what a plan whose pass has no kernel instance fails with

CONTEXTS = [{}, {"V2": 0}, {"V2": 2, "V2_REGPASS": 2}, {"V2_REGPASS": 0}, {"FAST": 0}] + \
           [{"KMAX": k, "FAST": f} for k in (5, 7, 8) for f in (0, 1)] + [{"SHARE": 0}, {"COOP_WGS": 8}]
BATCHES = (1, 6)


@pytest.fixture(scope="module")
def build():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@pytest.fixture
def mk(build, monkeypatch):
    """a fresh context of the emulation build created under the given MS_NTT_* knobs (ms_create reads them)"""
    made = []

    def make(field, env):
        for name in ref.knobs():
            monkeypatch.delenv("MS_NTT_" + name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv("MS_NTT_" + name, str(v))
        made.append(ms.Context(field, lib_path=EMU))
        return made[-1]
    yield make
    for ctx in made:
        ctx.close()


def view(ctx, log_n, log_pad, inverse, batch):
    """(status, the plan as ms_emu_ntt_plan writes it)"""
    buf = C.create_string_buffer(4096)
    rc = ctx.L.ms_emu_ntt_plan(ctx.h, C.c_int(log_n), C.c_int(log_pad), C.c_int(1 if inverse else 0), C.c_size_t(batch), buf, C.c_size_t(len(buf)))
    return rc, (json.loads(buf.value.decode()) if rc == 0 else None)


def launched(plan):
    """the instance every pass of the viewed plan launches for the batch the view was asked about"""
    return [ps.get("launches", ps["instance"]) for ps in plan["passes"]]


def pass_kernels(field):
    """Every pass kernel instance the library builds for the field: the kernel symbols of ntt_plan.cpp's device code for gfx950 (`hipcc --cuda-device-only -S`, demangled),
    without ScalePowKernel and CosetFoldKernel.  Inverse transforms are never zero-padded, so the cooperative tiles behind the virtual pass (MODE 2, and MODE 3 with the
    shared tables) exist forwards only; BabyBear's 8-column cooperative tiles are the virtual pass's 8 cosets, so they exist in MODE 2 only."""
    F = ref.FIELD_NAME[field]
    out = set()
    for inv in ("false", "true"):
        out |= {f"msntt::PassKernel<{F}, {inv}, {th}>" for th in (256, 512)}
        out |= {f"msntt::PassKernelK<{F}, {inv}, {k}, {512 if k == 9 else 256}>" for k in (6, 7, 8, 9)}
        out |= {f"msntt::RegPassKernel<{F}, {('GLM', 'BB')[field]}, {inv}, {k}>" for k in (1, 2, 3, 4, 5)}
        for mode in (0, 1) if inv == "true" else (0, 1, 2):
            if field == 0:
                out |= {f"msntt::PassKernel2<GL, {a}, {inv}, {k}, 3, {th}, {ns}, {mode}>" for a, k, th, ns in (("GLT", 7, 256, 2), ("GLM", 8, 256, 3), ("GLM", 9, 512, 3), ("GLM", 10, 512, 3))}
            elif mode == 2:
                out |= {f"msntt::PassKernel2<BB, BB, {inv}, {k}, 3, 256, {3 if k == 10 else 2}, 2>" for k in (7, 8, 9, 10)}
            else:
                out |= {f"msntt::PassKernel2<BB, BB, {inv}, {k}, 4, {512 if k == 10 else 256}, {3 if k == 10 else 2}, {mode}>" for k in (7, 8, 9, 10)}
    if field == 0:
        out.add("msntt::PassKernel2<GL, GLM, false, 10, 3, 512, 3, 3>")
    return out


@pytest.mark.parametrize("field", [0, 1])
def test_plan_view_equals_the_restated_rule(mk, field):
    """Shape and instances for every size, and - what licenses leaving instances out of the library - the instances that the combinations call sites can produce are
    exactly the pass kernels it builds.  Call sites: every one of ntt_run's passes n_in == n for an inverse transform, so inverse is only ever planned with log_pad = 0;
    the combinations with inverse and log_pad > 0 are still held to the restatement, but do not count towards the union."""
    union = set()
    for env in CONTEXTS:
        ctx, kn = mk(field, env), ref.knobs(**env)
        for log_n in range(1, ref.TWO_ADICITY[field] + 1):
            for log_pad in range(4):
                want_shape = ref.shape(field, log_n, log_pad, kn)
                for inverse in (False, True):
                    for batch in BATCHES:
                        what = (field, env, log_n, log_pad, inverse, batch)
                        want = ref.launches(field, log_n, log_pad, inverse, batch, kn)
                        rc, got = view(ctx, log_n, log_pad, inverse, batch)
                        if inverse and log_pad and rc == ERR_STATE:   # (no call site, and the one instance the rule names here that the library leaves out)
                            assert any(w.startswith("msntt::PassKernel2<") and w.endswith((", 2>", ", 3>")) for w in want), (what, want)
                            continue
                        assert rc == 0, (what, rc, ctx.last_error())
                        assert (got["log_r0"], got["log_rho"]) == (want_shape["log_r0"], want_shape["log_rho"]), what
                        assert [(ps["K"], ps["LC"]) for ps in got["passes"]] == [(ps["K"], ps["LC"]) for ps in want_shape["passes"]], what
                        assert launched(got) == want, what
                        for ps in got["passes"]:   # a shared-table alternative: the same instance in MODE 3, and the plain one is what MS_NTT_SHARE=0 launches
                            if "shared" in ps:
                                assert ps["instance"].endswith(", 2>") and ps["shared"] == ps["instance"][:-2] + "3>", what
                                assert ps["launches"] in (ps["instance"], ps["shared"]), what
                        if not (inverse and log_pad):
                            union |= set(launched(got))
    assert union == pass_kernels(field), (sorted(union - pass_kernels(field)), sorted(pass_kernels(field) - union))


def test_view_needs_no_device_memory(mk):
    ctx = mk(0, {})
    L = ctx.L
    before, after = (C.c_long * 7)(), (C.c_long * 7)()
    L.ms_emu_live(C.byref(before))
    rc, plan = view(ctx, 32, 3, False, 6)
    L.ms_emu_live(C.byref(after))
    assert rc == 0 and len(plan["passes"]) >= 3 and list(before) == list(after)   # (nothing handed out, no allocation made)
    assert view(ctx, 33, 0, False, 1)[0] != 0 and view(ctx, 0, 0, False, 1)[0] != 0


@pytest.mark.parametrize("env", [{}, {"V2": 2, "V2_REGPASS": 2}], ids=["default", "regpass-tiles"])
@pytest.mark.parametrize("field", [0, 1])
def test_view_names_what_runs(mk, field, env):
    """transforms and blowup-8 evaluations up to 2^16 points: the instances the view names are the keys of the profile's ntt_pass_variants after running them"""
    ctx = mk(field, env)
    rng = np.random.default_rng(5)
    for log_n in range(1, 17):
        a = rng.integers(0, nd.MODULUS[field], size=(1, 1 << log_n), dtype=np.uint64)
        for inverse in (False, True):
            ran = nd.profiled(ctx, lambda: ctx.check(ctx.ntt(a, inverse=inverse)[0]))
            rc, plan = view(ctx, log_n, 0, inverse, 1)
            assert rc == 0 and set(ran) == set(launched(plan)) and sum(ran.values()) == len(plan["passes"]), (field, env, log_n, inverse, ran, plan)
        if log_n >= 3:
            ran = nd.profiled(ctx, lambda: ctx.check(ctx.coset_lde(a[:, :1 << (log_n - 3)], 7, 1 << log_n)[0]))
            rc, plan = view(ctx, log_n, 3, False, 1)
            assert rc == 0 and set(ran) == set(launched(plan)) and sum(ran.values()) == len(plan["passes"]), (field, env, log_n, "lde", ran, plan)
