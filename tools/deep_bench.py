#!/usr/bin/env python3
"""What binding the FRI to the LDE tree costs: ms_validity_commit, ms_deep_evals and ms_deep_compose against ms_lde_commit and ms_eval_ext on the same context, in
the same process, and one whole linked proof against today's unlinked proof.  Two workloads, each field in a child process of its own on one GPU:
  fibonacci   the headline shape: the Fibonacci AIR (3 trace columns + 3 ms_polys_lincomb closures, ms_mix), 2^20 rows, blowup 8         Goldilocks
  cubic       the 64-column cubic spec through ms_mix_air_ext, 2^18 rows, blowup 8                                                       Goldilocks and BabyBear
Legs, alternated L / E / V / D / C / L / ..., kernel times of ms_profile_begin / ms_profile_end (HIP events around every launch), host time of the call beside them:
  L  ms_lde_commit                     E  ms_eval_ext at the opened points
  V  ms_validity_commit                D  ms_deep_evals (every column at every point, the chunk columns at the first)
  C  ms_deep_compose, split into its combine launch (class "deep_combine"), the scans ("suffix_horner") and the scale launch ("deep_scale")
The combine launch's achieved bytes/s is its algorithmic bytes - (c + m) N elements read once + npts E N written, the floor of the pass - over its time; the
streaming classes of leg L that carry byte counts are reported the same way beside it.  Then the whole proof, one alone, linked and unlinked alternated: trace commit
to ms_fri_query_index, the linked one with the three stages and the openings of both trees at the FRI positions.  Only the paired times of one run mean anything
(DESIGN.md 6); nothing here holds the stage to a number.  Writes one JSON line to profiles/deep_compose.json and prints it.  On a shared GPU box run it under a limit:
  timeout -k 10 900 python3 tools/deep_bench.py [--passes 5] [--out profiles/deep_compose.json]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = {"goldilocks": (0, (1 << 64) - (1 << 32) + 1, 2, 8), "babybear": (1, 15 * (1 << 27) + 1, 4, 4)}   # id, p, E, bytes per stored element
RUNS = (("fibonacci", "goldilocks"), ("cubic", "goldilocks"), ("cubic", "babybear"))


def profile(ctx, stage):
    """runs `stage` with every launch bracketed by events; (its result, the profile, host milliseconds of the whole call)"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    out = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return out, json.loads(buf.value.decode()), call_ms


def kernel_classes(prof):
    return {k: v for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}


def one_run(workload, name, args):
    import mini_stark_amd as ms
    from mini_stark_amd.host import build_host_library, cubic_rows_native, fibonacci_rows_native
    build_host_library()
    fid, p, e, elem = FIELDS[name]
    blowup, shift = args.blowup, 7
    if workload == "fibonacci":
        N = 1 << args.log_rows_fibonacci
        trace = fibonacci_rows_native(p, N, N - 1)
    else:
        N = 1 << args.log_rows_cubic
        w = args.width
        trace, sc = cubic_rows_native(p, N, w)
        cons = [[(1, [(j, 1)]), (p - 1, [(j, 0), ((j + 1) % w, 0), ((j + 2) % w, 0)]), ((p - int(s)) % p, [((j + 3) % w, 0)])] for j, s in enumerate(sc)]
        air = ms.flatten_air(cons, [[N - 1]] * w)
    width = trace.shape[1]
    ctx = ms.Context(fid)                     # raises without a GPU: there is nothing to measure then
    omega = ctx.root_of_unity(N)
    r = [(0x123456789ABCDEF + 77 * k) % p for k in range(e)]
    gamma = [(0xFEDCBA987654321 + 31 * k) % p for k in range(e)]
    z = [(0x0F1E2D3C4B5A6978 + 13 * k) % p for k in range(e)]
    zs = [z, [x * omega % p for x in z]]      # z and z w: the rows the programs read
    R = (N * blowup).bit_length() - 1
    betas = [3, 2**40 + 77]
    st = {}

    def to_polys():
        rc, _ = ctx.trace_commit(trace, width)
        ctx.check(rc)
        ctx.check(ctx.interpolate())
        if workload == "fibonacci":
            m1 = p - 1
            for s, idx in (([omega, m1], [0, 1]), ([omega, m1], [0, 1]), ([1, m1, m1], [2, 0, 1])):
                ctx.check(ctx.polys_lincomb(s, idx))
        st["c"] = ctx.polys_count()

    def lde():
        rc, _ = ctx.lde_commit(blowup, shift, st["c"])
        return rc

    def mix():
        return ctx.mix(r[0]) if workload == "fibonacci" else ctx.mix_air_ext(r, air)

    def lists():
        c, m = st["c"], st["m"]
        return [list(range(c + m)), list(range(c))]

    def vcommit():
        ctx.L.ms_validity_len.restype = C.c_size_t
        st["m"] = ctx.validity_ext() * int(ctx.L.ms_validity_len(ctx.h)) // N
        rc, _ = ctx.validity_commit(st["m"])
        return rc
    legs = {"L": lde, "E": lambda: ctx.eval_ext([x for zz in zs for x in zz])[0], "V": vcommit, "D": lambda: ctx.deep_evals(zs, lists())[0],
            "C": lambda: ctx.deep_compose(zs, lists(), gamma)}
    to_polys()
    ctx.check(lde()); ctx.check(mix()); ctx.check(vcommit())
    times, calls, combine, streaming = {k: [] for k in legs}, {k: [] for k in legs}, [], {}
    for it in range(args.passes + 1):         # the first pass is untimed: code objects, plans, buffers
        for k, stage in legs.items():
            rc, prof, call_ms = profile(ctx, stage)
            ctx.check(rc)
            if k == "L":                      # (a new LDE commitment ends the validity tree: the mix stage and the commitment are redone behind it, untimed)
                ctx.check(mix()); ctx.check(vcommit())
            if not it:
                continue
            cls = kernel_classes(prof)
            times[k].append({n: v["ms"] for n, v in cls.items()}); calls[k].append(call_ms)
            if k == "C":
                assert cls["deep_combine"]["launches"] == 1 and cls["deep_scale"]["launches"] == 1, cls
                combine.append(cls["deep_combine"]["alg_bytes"] / (cls["deep_combine"]["ms"] * 1e-3) / 1e9 if cls["deep_combine"]["ms"] > 0 else 0.0)
            if k == "L":
                for n, v in cls.items():
                    if v["alg_bytes"] > 0 and v["ms"] > 0:
                        streaming.setdefault(n, []).append(v["alg_bytes"] / (v["ms"] * 1e-3) / 1e9)
    total = lambda k: statistics.median(sum(t.values()) for t in times[k])   # noqa: E731
    part = lambda k, n: statistics.median(t.get(n, 0.0) for t in times[k])   # noqa: E731
    c, m = st["c"], st["m"]
    floor_bytes = ((c + m) * N + len(zs) * e * N) * elem

    # ---- one whole proof alone, linked against unlinked, alternated
    def proof(linked):
        t0 = time.perf_counter()
        to_polys()
        ctx.check(lde()); ctx.check(mix())
        if linked:
            ctx.check(vcommit())
            rc, _ev = ctx.deep_evals(zs, lists())
            ctx.check(rc)
            ctx.check(ctx.deep_compose(zs, lists(), gamma))
        else:
            ctx.check(ctx.eval_ext([x for zz in zs for x in zz])[0])
        rc, _ = ctx.fri_begin(blowup, R)
        ctx.check(rc)
        for k in range(1, R):
            ctx.check(ctx.fri_deep([(z[0] + k) % p] + z[1:])[0])
            ctx.check(ctx.fri_fold_commit([(gamma[0] + k) % p] + gamma[1:])[0])
        blob = ctx.fri_query_index(betas)
        if linked:
            D0 = ctx.fri_round_info(0)[1]
            L = N * blowup
            rows = [x for b in betas for x in ((b % D0) * (L // D0), ((b % D0 + D0 // 2) % D0) * (L // D0))]
            ctx.tree_open(ms.TREE_LDE, rows); ctx.tree_open(ms.TREE_VALIDITY, rows)
        return (time.perf_counter() - t0) * 1e3, len(blob)
    proof(False); proof(True)
    whole = {"unlinked": [], "linked": []}
    for _ in range(args.passes):
        whole["unlinked"].append(proof(False)[0]); whole["linked"].append(proof(True)[0])
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    return {"workload": workload, "field": name, "rows": N, "blowup": blowup, "c": c, "m": m, "npts": len(zs), "entries": sum(len(x) for x in lists()),
            "lde_commit_ms": total("L"), "eval_ext_ms": total("E"), "validity_commit_ms": total("V"), "deep_evals_ms": total("D"), "deep_compose_ms": total("C"),
            "deep_compose_combine_ms": part("C", "deep_combine"), "deep_compose_scans_ms": part("C", "suffix_horner"), "deep_compose_scale_ms": part("C", "deep_scale"),
            "combine_floor_bytes": floor_bytes, "combine_gb_per_s": statistics.median(combine), "lde_commit_streaming_gb_per_s": {n: statistics.median(v) for n, v in streaming.items()},
            "call_ms_median": {k: statistics.median(v) for k, v in calls.items()}, "proof_unlinked_ms": statistics.median(whole["unlinked"]),
            "proof_linked_ms": statistics.median(whole["linked"]), "proof_ms": whole, "legs_ms": times, "device": device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5, help="timed legs per stage (alternated), after one untimed leg each")
    ap.add_argument("--log-rows-fibonacci", type=int, default=20)
    ap.add_argument("--log-rows-cubic", type=int, default=18)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--run", help="workload:field - run this one in this process and print its result (what the parent starts)")
    ap.add_argument("--leg-timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_compose.json"))
    args = ap.parse_args()
    if args.run:
        workload, name = args.run.split(":")
        print(json.dumps(one_run(workload, name, args)))
        return
    runs = []
    for workload, name in RUNS:               # a fresh child each; the parent never opens the GPU.  A child that fails or runs out of time ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--run", f"{workload}:{name}", "--passes", str(args.passes), "--log-rows-fibonacci", str(args.log_rows_fibonacci),
               "--log-rows-cubic", str(args.log_rows_cubic), "--width", str(args.width), "--blowup", str(args.blowup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.leg_timeout, check=True)
        runs.append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
    res = {"metric": "deep_stage_cost", "workload": f"Fibonacci AIR at 2^{args.log_rows_fibonacci} rows (Goldilocks) and the {args.width}-column cubic spec at 2^{args.log_rows_cubic} rows "
           f"(both fields), blowup {args.blowup}; {args.passes} legs per stage, alternated; one paired run", "unit": "ms of kernel time (HIP events); call_ms and proof_*_ms = host time",
           "runs": runs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
