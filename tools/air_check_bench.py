#!/usr/bin/env python3
"""What the trace-domain check costs against the compose launch of the same program: the 64-column cubic spec (BASELINE configs[4]) at 2^18 rows, blowup 8, once on
Goldilocks and once on BabyBear; per field ONE process on one GPU, two contexts over the same trace (one stopped behind ms_trace_commit, one behind ms_lde_commit),
the legs alternated P / Q / B / P / ... - only the paired times of one run mean anything:
  P  ms_air_check before ms_interpolate: the check launch alone (mspoly::AirCheckKernel), profile class "air_check"
  Q  ms_air_check after ms_lde_commit: one forward transform of the 64 polynomials (class "ntt_pass") plus the same launch
  B  ms_mix_air on the same program: its compose launch over the 2^21-point LDE domain (mspoly::ComposeAirKernel), class "mix_air"
The times are kernel times of ms_profile_begin / ms_profile_end (HIP events around every launch); the whole-call host times are reported beside them.  Before anything
is timed the check must find the trace clean in both states and ms_mix_air must accept it.  By bytes P reads 1 / blowup of what B reads; nothing here holds it to a number.
Writes one JSON line to profiles/air_check.json and prints it.  Without --field each field runs in a child process of its own under its own time limit
(--leg-timeout), the second only if the first ended well; on a shared GPU box run the whole under a limit too:
  timeout -k 10 900 python3 tools/air_check_bench.py [--passes 8] [--log-rows 18] [--width 64] [--blowup 8] [--out profiles/air_check.json]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = {"goldilocks": (0, (1 << 64) - (1 << 32) + 1), "babybear": (1, 15 * (1 << 27) + 1)}


def profile(ctx, stage):
    """runs `stage` with every launch bracketed by events; (its result, the profile, host milliseconds of the whole call)"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    out = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return out, json.loads(buf.value.decode()), call_ms


def one_field(name, args):
    import mini_stark_amd as ms
    from mini_stark_amd.host import build_host_library, cubic_rows_native
    build_host_library()
    fid, p = FIELDS[name]
    N, w = 1 << args.log_rows, args.width
    trace, sc = cubic_rows_native(p, N, w)
    spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
    cons = [[(1, [(j, 1)]), (p - 1, [(a, 0), (b, 0), (c, 0)]), ((p - int(s)) % p, [(d, 0)])] for (j, a, b, c, d), s in zip(spec, sc)]
    air = ms.flatten_air(cons, [[N - 1]] * w)
    early, late = ms.Context(fid), ms.Context(fid)     # raise without a GPU: there is nothing to measure then
    for ctx in (early, late):
        rc, _ = ctx.trace_commit(trace, w)
        ctx.check(rc)
    late.check(late.interpolate())
    rc, _ = late.lde_commit(args.blowup, 7, w)
    late.check(rc)
    r = 0x123456789ABCDEF % p

    def check_on(ctx):
        rc, rep = ctx.air_check(air)
        ctx.check(rc)
        assert rep["ok"] and not rep["count"].any(), "the cubic trace does not satisfy its program"
        return 0
    legs = {"P": (early, lambda: check_on(early)), "Q": (late, lambda: check_on(late)), "B": (late, lambda: late.mix_air(r, air))}

    def kernel_ms(k, prof):
        if k == "B":
            assert prof["mix_air"]["launches"] == 1 and prof["air_check"]["launches"] == 0
            return {"compose": prof["mix_air"]["ms"]}
        assert prof["air_check"]["launches"] in (1, 2) and prof["mix_air"]["launches"] == 0 and (prof["ntt_pass"]["launches"] == 0) == (k == "P"), (k, prof)
        return {"check": prof["air_check"]["ms"], "ntt": prof["ntt_pass"]["ms"]}
    for k, (ctx, stage) in legs.items():               # untimed: code objects, NTT plans, buffers
        rc, prof, _ = profile(ctx, stage)
        ctx.check(rc)
        kernel_ms(k, prof)
    times, calls = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.passes):
        for k, (ctx, stage) in legs.items():
            rc, prof, call_ms = profile(ctx, stage)
            ctx.check(rc)
            times[k].append(kernel_ms(k, prof))
            calls[k].append(call_ms)
    med = lambda k, key: statistics.median(t[key] for t in times[k])   # noqa: E731
    spread = lambda k, key: (max(t[key] for t in times[k]) - min(t[key] for t in times[k])) / med(k, key)   # noqa: E731
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    compose, before, after_chk, after_ntt = med("B", "compose"), med("P", "check"), med("Q", "check"), med("Q", "ntt")
    return {"field": name, "check_before_interpolate_ms": before, "check_after_lde_launch_ms": after_chk, "check_after_lde_ntt_ms": after_ntt,
            "check_after_lde_ms": after_chk + after_ntt, "air_compose_ms": compose, "ratio_check_over_compose": before / compose,
            "ratio_check_after_lde_over_compose": (after_chk + after_ntt) / compose, "check_slower_than_compose": before > compose,
            "check_spread": spread("P", "check"), "check_after_lde_spread": spread("Q", "check"), "compose_spread": spread("B", "compose"),
            "call_ms_median": {k: statistics.median(v) for k, v in calls.items()}, "legs_ms": times, "legs_call_ms": calls, "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="timed legs per stage (alternated), after one untimed leg each")
    ap.add_argument("--log-rows", type=int, default=18)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--field", choices=sorted(FIELDS), help="run this field in this process and print its result (what the parent starts)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a field's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_check.json"))
    args = ap.parse_args()
    if args.field:
        print(json.dumps(one_field(args.field, args)))
        return
    per = {}
    for name in ("goldilocks", "babybear"):    # a fresh child each; the parent never opens the GPU.  A child that fails or runs out of time ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--field", name, "--passes", str(args.passes), "--log-rows", str(args.log_rows), "--width", str(args.width),
               "--blowup", str(args.blowup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.leg_timeout, check=True)
        per[name] = json.loads(done.stdout.decode().strip().splitlines()[-1])
    res = {"metric": "air_check_vs_compose", "workload": f"{args.width}-column cubic spec, 2^{args.log_rows} rows, blowup {args.blowup}: ms_air_check over the 2^{args.log_rows} rows "
           f"(before ms_interpolate; after ms_lde_commit with its forward transform) against ms_mix_air's compose launch over the 2^{args.log_rows + args.blowup.bit_length() - 1}-point "
           f"LDE domain, {args.passes} legs per stage, alternated P / Q / B", "unit": "ms of kernel time (HIP events); call_ms = host time of the whole call", "fields": per}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
