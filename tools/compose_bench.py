#!/usr/bin/env python3
"""What the general composition kernel costs against the hard-coded cubic one: the 64-column cubic spec (BASELINE configs[4]) at 2^18 rows, blowup 8, Goldilocks,
through ms_mix_cubic (mspoly::CubicComposeKernel) and through ms_mix_terms (mspoly::ComposeTermsKernel) in ONE process on one GPU, on the SAME committed LDE, the
legs alternated cubic / terms / cubic / ... - only the paired times of one run mean anything.  The compose-kernel times are the per-kernel times of
ms_profile_begin / ms_profile_end (HIP events around every launch): class "mix" for the cubic kernel, "mix_terms" for the general one.  Both stages must give the
same validity polynomial, which is checked before anything is timed.  Writes one JSON line to profiles/mix_terms_vs_cubic.json and prints it.
On a shared GPU box run it under a time limit of its own, chained behind whatever precedes it:
  timeout -k 10 600 python3 tools/compose_bench.py [--passes 8] [--log-rows 18] [--width 64] [--blowup 8] [--out profiles/mix_terms_vs_cubic.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(ctx, stage, key):
    """runs `stage` with every launch bracketed by events; (status, milliseconds of kernel class `key`, launches of it, host milliseconds of the whole call:
    the stage ends behind its one stream synchronisation, so this is what a caller waits)"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    rc = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    prof = json.loads(buf.value.decode())
    return rc, prof[key]["ms"], prof[key]["launches"], call_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="timed legs per stage (alternated), after one untimed leg each")
    ap.add_argument("--log-rows", type=int, default=18)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_terms_vs_cubic.json"))
    args = ap.parse_args()
    import mini_stark_amd as ms
    from mini_stark_amd.host import build_host_library, cubic_rows_native
    build_host_library()
    ctx = ms.Context(ms.GOLDILOCKS)          # raises without a GPU: there is nothing to measure then
    p = (1 << 64) - (1 << 32) + 1
    N, w = 1 << args.log_rows, args.width
    trace, sc = cubic_rows_native(p, N, w)
    spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
    terms = ms.flatten_terms([[(1, [(j, 1)]), (p - 1, [(a, 0), (b, 0), (c, 0)]), ((p - int(s)) % p, [(d, 0)])] for (j, a, b, c, d), s in zip(spec, sc)])
    rc, _ = ctx.trace_commit(trace, w)
    ctx.check(rc)
    ctx.check(ctx.interpolate())
    rc, _ = ctx.lde_commit(args.blowup, 7, w)
    ctx.check(rc)
    r = 0x123456789ABCDEF % p
    legs = {"cubic": (lambda: ctx.mix_cubic(r, spec, sc), "mix"), "terms": (lambda: ctx.mix_terms(r, terms, 1), "mix_terms")}
    # same polynomial from both, and the untimed first legs (code objects, the interpolation's NTT plan)
    outs = {}
    for k, (stage, key) in legs.items():
        rc, _, n, _ = kernel_ms(ctx, stage, key)
        ctx.check(rc)
        assert n == 1, (k, n)
        outs[k] = ctx.validity_read()
    assert (outs["cubic"] == outs["terms"]).all() and outs["cubic"].any(), "ms_mix_terms and ms_mix_cubic disagree"
    times, calls = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.passes):
        for k, (stage, key) in legs.items():
            rc, t, _, call_ms = kernel_ms(ctx, stage, key)
            ctx.check(rc)
            times[k].append(t)
            calls[k].append(call_ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    res = {"metric": "mix_terms_vs_cubic", "workload": f"{w}-column cubic spec, Goldilocks, 2^{args.log_rows} rows, blowup {args.blowup}: one compose launch over the 2^{args.log_rows + args.blowup.bit_length() - 1}-point LDE domain, "
           f"{args.passes} legs per stage, alternated", "unit": "ms per compose kernel (HIP events)", "cubic_compose_ms": med["cubic"], "terms_compose_ms": med["terms"],
           "ratio_terms_over_cubic": med["terms"] / med["cubic"], "cubic_spread": (max(times["cubic"]) - min(times["cubic"])) / med["cubic"],
           "terms_spread": (max(times["terms"]) - min(times["terms"])) / med["terms"], "legs_ms": times, "call_ms_mean": {k: statistics.mean(v) for k, v in calls.items()}, "legs_call_ms": calls,
           "outputs_identical": True, "device": device}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
