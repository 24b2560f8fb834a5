#!/usr/bin/env python3
"""The staged LDE commitment on one GPU, in ONE process; prints one JSON line and writes profiles/staged.json.
Shape: Goldilocks, 2^20 rows, blowup 8, 20 security bits, six trace columns - two Fibonacci columns (the main program) and the columns (2, 3), (4, 5) of a
permutation argument - and one Fp2 permutation argument, PRODUCT of (ch0 + T2 + ch1 T3) / (ch0 + T4 + ch1 T5).
  (a) the column.  ms_aux_running_staged (behind ms_interpolate and ms_lde_commit of the six columns) against ms_aux_running (behind ms_trace_commit) for the same
      descriptor: kernel milliseconds and launches of the one call under ms_profile_begin / ms_profile_end, and the host clock around it; legs alternated.  The
      expected difference is the forward transform of the four named columns and the inverse transform of the two new ones.
  (b) ms_lde_commit_stage alone: on a context whose LDE buffer already holds eight columns (warm: no growth copy), and the first call on a fresh context (the
      device-to-device copy of the six committed columns into a larger buffer, and the first allocation of the staged tree's nodes, inside it).
  (c) the proof.  A v2 proof (Stark.prove_air with aux: staged order, two LDE trees) against the UNSTAGED order with the same arithmetic - ms_aux_running early, one
      ms_lde_commit over eight columns, the same combined program, ms_query_linked - both driven from Python with the same fixed challenges for the unstaged leg;
      and msh_stark_prove_linked_aux, the C++ driver of the same v2 proof.  Legs alternated `passes` times, `proofs` proofs per leg.
Only the paired figures of one run mean anything.  It gates nothing.
  python3 tools/staged_bench.py [--log-rows 20] [--proofs 3] [--passes 5] [--out profiles/staged.json] [--lib PATH]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_trace(p, N, seed=7):
    """N x 6: Fibonacci columns a' = b, b' = a + b; columns (2, 3) random, the rows of (4, 5) a permutation of theirs"""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.zeros((N, 6), dtype=np.uint64)
    a, b = 1, 2
    for i in range(N):
        t[i, 0], t[i, 1] = a, b
        a, b = b, (a + b) % p
    t[:, 2:4] = rng.integers(0, p, size=(N, 2), dtype=np.uint64)
    t[:, 4:6] = t[rng.permutation(N), 2:4]
    return t


def main_program(p, N):
    m1 = p - 1
    cons = [[(1, [(0, 1)]), (m1, [(1, 0)])], [(1, [(1, 1)]), (m1, [(0, 0)]), (m1, [(1, 0)])]]
    return cons, [[N - 1], [N - 1]], (), [(0, 0, 1), (1, 0, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--proofs", type=int, default=3, help="proofs (or calls) per leg")
    ap.add_argument("--passes", type=int, default=5, help="legs per variant, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staged.json"))
    ap.add_argument("--lib", default=None, help="another libministark build (the emulation build: a dry run of the tool, its times mean nothing)")
    args = ap.parse_args()
    import mini_stark_amd as ms
    from common import MODULUS, SplitMix64
    from linked_bench import alternate, profile
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import Stark, StarkConfig
    build_host_library()
    field, p, e = ms.GOLDILOCKS, MODULUS[ms.GOLDILOCKS], 2
    N, blowup, w = 1 << args.log_rows, 8, 6
    trace = build_trace(p, N)
    air = main_program(p, N)
    sym = [ms.flatten_aux_arg(ms.AUX_PRODUCT, [(((1, 1), [(2, 1, 0), (3, 1, 2)]), ((1, 1), [(4, 1, 0), (5, 1, 2)]))])]
    nch = 2
    rng = SplitMix64(0x57A6ED)
    ch = [tuple(rng.nonzero(p) for _ in range(e)) for _ in range(nch)]
    inst = ms.instantiate_aux(field, sym[0], ch)
    shift = rng.nonzero(p)
    lib = {"lib_path": args.lib} if args.lib else {}
    mk = lambda: ms.Context(field, flags=ms.FLAG_ZERO_DISPLAY_EMPTY, **lib)   # noqa: E731
    ctx = mk()
    out = {"metric": "staged_bench", "unit": "ms", "one_paired_run": True,
           "workload": f"six trace columns (Fibonacci + one Fp2 permutation argument over two column pairs), Goldilocks, 2^{args.log_rows} rows, blowup {blowup}, "
                       f"20 security bits; one process, legs alternated x {args.passes}"}

    # ---- (a) the column: the one call, behind its own preparation
    def prep_early():
        ctx.check(ctx.trace_commit(trace, w)[0])

    def prep_staged():
        prep_early()
        ctx.check(ctx.interpolate())
        ctx.check(ctx.lde_commit(blowup, shift, w)[0])
    calls = {"ms_aux_running": (prep_early, lambda: ctx.check(ctx.aux_running(inst["op"], inst, e)[0])),
             "ms_aux_running_staged": (prep_staged, lambda: ctx.check(ctx.aux_running_staged(inst["op"], inst, e)[0]))}
    for prep, call in calls.values():                              # every shape twice before anything is timed
        for _ in range(2):
            prep(); call()
    rec = {k: {"host_ms": [], "kernel_ms": [], "launches": None, "by_class": None} for k in calls}
    for _ in range(args.passes):
        for k, (prep, call) in calls.items():
            prep()
            ctx.synchronize()
            t0 = time.perf_counter()
            call()
            rec[k]["host_ms"].append(round((time.perf_counter() - t0) * 1e3, 4))
            prep()
            pr = profile(ctx, call)
            rec[k]["kernel_ms"].append(pr["kernel_ms"]); rec[k]["launches"] = pr["launches"]; rec[k]["by_class"] = pr["by_class"]
    for k in rec:
        rec[k]["host_ms_mean"] = round(statistics.mean(rec[k]["host_ms"]), 4)
        rec[k]["kernel_ms_mean"] = round(statistics.mean(rec[k]["kernel_ms"]), 4)
    rec["kernel_ms_added_by_staging"] = round(rec["ms_aux_running_staged"]["kernel_ms_mean"] - rec["ms_aux_running"]["kernel_ms_mean"], 4)
    out["column"] = rec

    # ---- (b) ms_lde_commit_stage alone
    def stage_once(c):
        c.check(c.trace_commit(trace, w)[0]); c.check(c.interpolate()); c.check(c.lde_commit(blowup, shift, w)[0])
        c.check(c.aux_running_staged(inst["op"], inst, e)[0])
        c.synchronize()
        t0 = time.perf_counter()
        c.check(c.lde_commit_stage(e)[0])
        return (time.perf_counter() - t0) * 1e3
    warm, first = [], []
    stage_once(ctx)                                                # (this context's LDE buffer holds eight columns from here on)
    for _ in range(args.passes):
        warm.append(round(stage_once(ctx), 4))
        fresh = mk()
        fresh.check(fresh.trace_commit(trace, w)[0]); fresh.check(fresh.interpolate()); fresh.check(fresh.lde_commit(blowup, shift, w)[0])   # plans and tables built
        first.append(round(stage_once(fresh), 4))
        fresh.close()
    prep_staged(); ctx.check(ctx.aux_running_staged(inst["op"], inst, e)[0])
    out["lde_commit_stage"] = {"warm_no_growth_copy_ms": warm, "warm_mean_ms": round(statistics.mean(warm), 4),
                               "first_call_with_growth_copy_and_node_allocation_ms": first, "first_mean_ms": round(statistics.mean(first), 4),
                               "growth_copy_bytes": w * N * blowup * 8, "warm_profile": profile(ctx, lambda: ctx.check(ctx.lde_commit_stage(e)[0]))}

    # ---- (c) the proof: staged order against the unstaged order with the same arithmetic
    cfg = StarkConfig(ctx, 20, blowup, N - 1, w)
    st = Stark(cfg)
    hs = HostStark(ctx, 20, blowup, N - 1, w)
    R, nq = cfg.rounds, cfg.fri_queries
    c2, e2, b2 = ms.aux_constraints(field, inst["op"], ms.aux_fractions(inst), e, w)
    prog = ms.flatten_air(air[0] + c2, air[1] + e2, (), list(air[3]) + b2)
    prog_rows = ms.air_rows(air[0] + c2, list(air[3]) + b2)
    omega = ctx.root_of_unity(N)

    def unstaged():
        r2 = SplitMix64(0xBEEF)
        ext = lambda: [r2.nonzero(p) for _ in range(e)]   # noqa: E731
        ctx.check(ctx.trace_commit(trace, w)[0])
        ctx.check(ctx.aux_running(inst["op"], inst, e)[0])
        ctx.check(ctx.interpolate())
        c = w + e
        ctx.check(ctx.lde_commit(blowup, shift, c)[0])
        ctx.check(ctx.mix_air_ext(ext(), prog))
        m = e * ctx.validity_len() // N
        ctx.check(ctx.validity_commit(m)[0])
        z = ext()
        pts = [[v * pow(omega, row, p) % p for v in z] for row in prog_rows]
        lists = [list(range(c)) + (list(range(c, c + m)) if k == 0 else []) for k in range(len(prog_rows))]
        ctx.check(ctx.deep_evals(pts, lists)[0])
        ctx.check(ctx.deep_compose(pts, lists, ext()))
        ctx.check(ctx.fri_begin(blowup, R)[0])
        for _ in range(1, R):
            ctx.check(ctx.fri_deep(ext())[0])
            ctx.check(ctx.fri_fold_commit(ext())[0])
        return ctx.query_linked([r2.next() for _ in range(nq)])
    legs = {"v2_staged_python_driver": lambda: st.prove_air(trace, air, 0, aux=(sym, nch)),
            "unstaged_order_python_driver": unstaged,
            "v2_staged_cpp_driver": lambda: (ctx.check(hs.prove_linked_aux(trace, air, sym, nch)), hs.linked_proof())}
    per = alternate(legs, args.passes, args.proofs)
    proof = {"proofs_per_leg": args.proofs, "rounds": R, "queries": nq, "proof_bytes_v2": len(hs.linked_proof()),
             "legs": {k: {"ms_per_proof": round(statistics.mean(v), 4), "legs_ms": [round(x, 4) for x in v]} for k, v in per.items()}}
    proof["staged_over_unstaged"] = round(proof["legs"]["v2_staged_python_driver"]["ms_per_proof"] / proof["legs"]["unstaged_order_python_driver"]["ms_per_proof"], 4)
    proof["profile_v2"] = profile(ctx, legs["v2_staged_cpp_driver"])
    proof["profile_unstaged"] = profile(ctx, unstaged)
    out["proof"] = proof
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
