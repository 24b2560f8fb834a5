#!/usr/bin/env python3
"""What the composition challenge in the extension field costs: the 64-column cubic spec (BASELINE configs[4]) at 2^18 rows, blowup 8, once on Goldilocks (K = Fp2)
and once on BabyBear (K = Fp4); per field ONE process on one GPU, the SAME committed LDE, the legs alternated B / D / B / D ... - only the paired times of one run
mean anything:
  B  ms_mix_air (mspoly::ComposeAirKernel), profile class "mix_air"
  D  ms_mix_air_ext on the same program with a full K value of r (mspoly::ComposeAirExtKernel), class "mix_air_ext"; before anything is timed its output on a
     base-field r = (r0, 0, ..) is checked against B's: limb 0 equal, the limbs above it zero
Reported per field: the compose-kernel time per class (ms_profile_begin / ms_profile_end: HIP events around every launch), the whole-call time (D also interpolates
and scales E planes: real cost of the stage), the spreads, and `d_within_e_times_b_plus_b_spread`: the column loads are the same in B and D, and running the base
kernel E times with the limb-l weights would give the same planes, so a D compose time above E x B's median (plus B's spread) means the K accumulation is
structured badly.  Writes one JSON line to profiles/mix_air_ext.json and prints it.
Without --field each field runs in a child process of its own under its own time limit (--leg-timeout), the second only if the first ended well; on a shared GPU
box run the whole under a limit too:
  timeout -k 10 900 python3 tools/air_ext_bench.py [--passes 8] [--log-rows 18] [--width 64] [--blowup 8] [--out profiles/mix_air_ext.json]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = {"goldilocks": (0, (1 << 64) - (1 << 32) + 1, 2), "babybear": (1, 15 * (1 << 27) + 1, 4)}


def profile(ctx, stage):
    """runs `stage` with every launch bracketed by events; (status, the profile, host milliseconds of the whole call)"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    rc = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return rc, json.loads(buf.value.decode()), call_ms


def one_field(name, args):
    import mini_stark_amd as ms
    from mini_stark_amd.host import build_host_library, cubic_rows_native
    build_host_library()
    fid, p, e = FIELDS[name]
    ctx = ms.Context(fid)                     # raises without a GPU: there is nothing to measure then
    assert ctx.e == e
    N, w = 1 << args.log_rows, args.width
    trace, sc = cubic_rows_native(p, N, w)
    spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
    cons = [[(1, [(j, 1)]), (p - 1, [(a, 0), (b, 0), (c, 0)]), ((p - int(s)) % p, [(d, 0)])] for (j, a, b, c, d), s in zip(spec, sc)]
    air = ms.flatten_air(cons, [[N - 1]] * w)
    rc, _ = ctx.trace_commit(trace, w)
    ctx.check(rc)
    ctx.check(ctx.interpolate())
    rc, _ = ctx.lde_commit(args.blowup, 7, w)
    ctx.check(rc)
    r0 = 0x123456789ABCDEF % p
    rk = [(r0 * (l + 3) + l) % p for l in range(e)]
    assert all(rk)
    legs = {"B": (lambda: ctx.mix_air(r0, air), "mix_air"), "D": (lambda: ctx.mix_air_ext(rk, air), "mix_air_ext")}
    # untimed: code objects, the interpolation's NTT plans (batch 1 and batch E), and D on a base-field r against B
    rc, prof, _ = profile(ctx, legs["B"][0])
    ctx.check(rc)
    assert prof["mix_air"]["launches"] == 1 and prof["mix_air_ext"]["launches"] == 0
    out_b = ctx.validity_read()
    rc, prof, _ = profile(ctx, lambda: ctx.mix_air_ext([r0] + [0] * (e - 1), air))
    ctx.check(rc)
    assert prof["mix_air_ext"]["launches"] == 1 and prof["mix_air"]["launches"] == 0
    out_d = ctx.validity_read()
    assert out_b.shape == (2 * N,) and out_d.shape == (2 * N, e) and out_b.any()
    assert (out_d[:, 0] == out_b).all() and not out_d[:, 1:].any(), "ms_mix_air_ext on a base-field r and ms_mix_air disagree"
    rc, _, _ = profile(ctx, legs["D"][0])
    ctx.check(rc)
    full = ctx.validity_read()
    assert all(full[:, l].any() for l in range(e))
    times, calls = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.passes):
        for k, (stage, key) in legs.items():
            rc, prof, call_ms = profile(ctx, stage)
            ctx.check(rc)
            assert prof[key]["launches"] == 1
            times[k].append(prof[key]["ms"])
            calls[k].append(call_ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    cmed = {k: statistics.median(v) for k, v in calls.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    return {"field": name, "ext_degree": e, "air_compose_ms": med["B"], "air_ext_compose_ms": med["D"], "ratio_ext_over_air": med["D"] / med["B"],
            "air_spread": spread["B"], "air_ext_spread": spread["D"], "d_within_e_times_b_plus_b_spread": med["D"] / med["B"] <= e * (1.0 + spread["B"]),
            "air_call_ms": cmed["B"], "air_ext_call_ms": cmed["D"], "call_ratio_ext_over_air": cmed["D"] / cmed["B"],
            "air_call_spread": (max(calls["B"]) - min(calls["B"])) / cmed["B"], "air_ext_call_spread": (max(calls["D"]) - min(calls["D"])) / cmed["D"],
            "legs_ms": times, "legs_call_ms": calls, "base_r_output_identical": True, "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="timed legs per stage (alternated), after the untimed ones")
    ap.add_argument("--log-rows", type=int, default=18)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--field", choices=sorted(FIELDS), help="run this field in this process and print its result (what the parent starts)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a field's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_air_ext.json"))
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
    res = {"metric": "mix_air_ext_vs_air", "workload": f"{args.width}-column cubic spec, 2^{args.log_rows} rows, blowup {args.blowup}: one compose launch over the "
           f"2^{args.log_rows + args.blowup.bit_length() - 1}-point LDE domain, {args.passes} legs per stage, alternated B / D; D = ms_mix_air_ext with a full extension-field r",
           "unit": "ms per compose kernel (HIP events); call_ms = host time of the whole stage call", "fields": per}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
