#!/usr/bin/env python3
"""What the AIR composition kernel costs against the term kernel it generalises: the 64-column cubic spec (BASELINE configs[4]) at 2^18 rows, blowup 8, Goldilocks,
in ONE process on one GPU, on the SAME committed LDE, the legs alternated A / B / C / A / ... - only the paired times of one run mean anything:
  A  ms_mix_terms (mspoly::ComposeTermsKernel), profile class "mix_terms"
  B  ms_mix_air on the same program (mspoly::ComposeAirKernel: one transition group), class "mix_air"; its outputs are checked bit-equal to A's before anything is timed
  C  B plus 128 boundary constraints: every column at rows 0 and N - 1, the values taken from the trace (two boundary groups, 128 more column loads per point)
The times are the per-kernel times of ms_profile_begin / ms_profile_end (HIP events around every launch).  Also reported: the one launch of class "air_inv" that
builds the boundary inverse table on C's first leg.  Writes one JSON line to profiles/mix_air_vs_terms.json and prints it.
On a shared GPU box run it under a time limit of its own, chained behind whatever precedes it:
  timeout -k 10 600 python3 tools/air_bench.py [--passes 8] [--log-rows 18] [--width 64] [--blowup 8] [--out profiles/mix_air_vs_terms.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profile(ctx, stage):
    """runs `stage` with every launch bracketed by events; (status, the profile, host milliseconds of the whole call: the stage ends behind its one stream
    synchronisation, so this is what a caller waits)"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    rc = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return rc, json.loads(buf.value.decode()), call_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="timed legs per stage (alternated), after one untimed leg each")
    ap.add_argument("--log-rows", type=int, default=18)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_air_vs_terms.json"))
    args = ap.parse_args()
    import mini_stark_amd as ms
    from mini_stark_amd.host import build_host_library, cubic_rows_native
    build_host_library()
    ctx = ms.Context(ms.GOLDILOCKS)          # raises without a GPU: there is nothing to measure then
    p = (1 << 64) - (1 << 32) + 1
    N, w = 1 << args.log_rows, args.width
    trace, sc = cubic_rows_native(p, N, w)
    spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
    cons = [[(1, [(j, 1)]), (p - 1, [(a, 0), (b, 0), (c, 0)]), ((p - int(s)) % p, [(d, 0)])] for (j, a, b, c, d), s in zip(spec, sc)]
    terms = ms.flatten_terms(cons)
    exempt = [[N - 1]] * w
    boundary = [(j, row, int(trace[row, j])) for row in (0, N - 1) for j in range(w)]
    air_b, air_c = ms.flatten_air(cons, exempt), ms.flatten_air(cons, exempt, (), boundary)
    rc, _ = ctx.trace_commit(trace, w)
    ctx.check(rc)
    ctx.check(ctx.interpolate())
    rc, _ = ctx.lde_commit(args.blowup, 7, w)
    ctx.check(rc)
    r = 0x123456789ABCDEF % p
    legs = {"A": (lambda: ctx.mix_terms(r, terms, 1), "mix_terms"), "B": (lambda: ctx.mix_air(r, air_b), "mix_air"), "C": (lambda: ctx.mix_air(r, air_c), "mix_air")}
    # the untimed first legs (code objects, the interpolation's NTT plan, the inverse table), and B's outputs against A's
    outs, inv_ms = {}, None
    for k, (stage, key) in legs.items():
        rc, prof, _ = profile(ctx, stage)
        ctx.check(rc)
        assert prof[key]["launches"] == 1 and prof["air_inv"]["launches"] == (1 if k == "C" else 0), (k, prof[key], prof["air_inv"])
        if k == "C":
            inv_ms = prof["air_inv"]["ms"]
        outs[k] = ctx.validity_read()
    assert outs["A"].size == 2 * N
    assert (outs["A"] == outs["B"]).all() and outs["A"].any(), "ms_mix_air and ms_mix_terms disagree"
    assert (outs["C"] != outs["A"]).any()
    times, calls = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.passes):
        for k, (stage, key) in legs.items():
            rc, prof, call_ms = profile(ctx, stage)
            ctx.check(rc)
            assert prof["air_inv"]["launches"] == 0
            times[k].append(prof[key]["ms"])
            calls[k].append(call_ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    res = {"metric": "mix_air_vs_terms", "workload": f"{w}-column cubic spec, Goldilocks, 2^{args.log_rows} rows, blowup {args.blowup}: one compose launch over the 2^{args.log_rows + args.blowup.bit_length() - 1}-point LDE domain, "
           f"{args.passes} legs per stage, alternated; C = B + {len(boundary)} boundary constraints (every column at rows 0 and N - 1)", "unit": "ms per compose kernel (HIP events)",
           "terms_compose_ms": med["A"], "air_compose_ms": med["B"], "air_boundary_compose_ms": med["C"], "ratio_air_over_terms": med["B"] / med["A"],
           "ratio_air_boundary_over_terms": med["C"] / med["A"], "terms_spread": spread["A"], "air_spread": spread["B"], "air_boundary_spread": spread["C"],
           "b_within_a_spread_plus_0_05": med["B"] / med["A"] <= 1.0 + spread["A"] + 0.05, "air_inv_build_ms": inv_ms, "legs_ms": times, "call_ms_mean": {k: statistics.mean(v) for k, v in calls.items()},
           "legs_call_ms": calls, "outputs_identical": True, "device": device}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
