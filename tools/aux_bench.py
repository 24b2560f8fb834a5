#!/usr/bin/env python3
"""What the running-column stage (ms_aux_running: running.hpp's tile / carry / apply launches) costs, against a streaming stage over comparable bytes in the same
process: 2^20 rows, Goldilocks, w = 6, on one GPU; only the paired times of one run mean anything:
  A  MS_AUX_PRODUCT, ext = 2, one fraction, three columns per form            (a permutation argument over column triples)
  B  MS_AUX_SUM, ext = 2, two fractions  m / (gamma - t)  -  1 / (gamma - f)   (a LogUp lookup)
  Y  the yardstick: ms_interpolate of the same trace (w columns), profile class "ntt_pass"
Every pass commits the trace (untimed), runs A and B (alternated from pass to pass), commits again and interpolates.  The times are the per-class times of
ms_profile_begin / ms_profile_end (HIP events around every launch) and the host time of the whole call; the bytes per leg are computed from the shapes: per row the
tile launch reads the distinct columns its forms name and writes ext limbs, the apply launch reads and writes ext limbs.  A's column is checked against the
recurrence at 4096 sampled rows before anything is timed.  Writes one JSON line to profiles/aux_running.json and prints it.
On a shared GPU box run it under a time limit of its own, chained behind whatever precedes it:
  timeout -k 10 600 python3 tools/aux_bench.py [--passes 8] [--log-rows 20] [--out profiles/aux_running.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profile(ctx, stage):
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    t0 = time.perf_counter()
    out = stage()
    call_ms = (time.perf_counter() - t0) * 1e3
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return out, json.loads(buf.value.decode()), call_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="timed legs per stage, after one untimed pass")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_running.json"))
    args = ap.parse_args()
    import numpy as np
    import mini_stark_amd as ms
    ctx = ms.Context(ms.GOLDILOCKS)          # raises without a GPU: there is nothing to measure then
    p = (1 << 64) - (1 << 32) + 1
    N, w, ext = 1 << args.log_rows, 6, 2
    rng = np.random.default_rng(20)
    trace = (rng.integers(0, 1 << 63, size=(N, w), dtype=np.uint64) % np.uint64(p)).astype(np.uint64)
    trace[:, 2] = rng.integers(0, 4, size=N, dtype=np.uint64)      # (B's multiplicities: small)
    g = (0x123456789ABCDEF % p, 0xFEDCBA987654321 % p)
    c1, c2, one, m1 = (3, 5), (7, 11), (1, 0), (p - 1, 0)
    frac_a = [((g, [(0, one), (1, c1), (2, c2)]), (g, [(3, one), (4, c1), (5, c2)]))]
    frac_b = [(((0, 0), [(2, one)]), (g, [(0, m1)])), ((m1, []), (g, [(1, m1)]))]
    legs = {"A": ms.flatten_aux(ms.AUX_PRODUCT, frac_a, ext), "B": ms.flatten_aux(ms.AUX_SUM, frac_b, ext)}
    cols = {k: len(set(int(c) for c in a["term_col"])) for k, a in legs.items()}
    nbytes = {k: N * 8 * (cols[k] + ext + 2 * ext) for k in legs}
    commit = lambda: ctx.check(ctx.trace_commit(trace, w)[0])   # noqa: E731

    def aux(k, read=False):
        rc, final, col = ctx.aux_running(0, legs[k], read=read)
        ctx.check(rc)
        return final, col
    # the untimed first pass (code objects, buffers, the NTT plan), and A's column against the recurrence z_{i+1} B_i = z_i A_i at sampled rows
    commit()
    final, col = aux("A", read=True)
    aux("B")
    ctx.check(ctx.interpolate())
    mul = lambda a, b: ((a[0] * b[0] + 7 * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)   # noqa: E731
    form = lambda f, row: tuple((f[0][l] + sum(cf[l] * int(row[c]) for c, cf in f[1])) % p for l in range(2))   # noqa: E731
    assert tuple(int(v) for v in col[0]) == (1, 0)
    for i in [int(v) for v in rng.integers(0, N, size=4096)] + [N - 1]:
        zn = tuple(int(v) for v in col[i + 1]) if i + 1 < N else final
        assert mul(zn, form(frac_a[0][1], trace[i])) == mul(tuple(int(v) for v in col[i]), form(frac_a[0][0], trace[i])), i
    times = {k: [] for k in ("A", "B", "Y")}
    calls = {k: [] for k in ("A", "B", "Y")}
    launches = {}
    for it in range(args.passes):
        commit()
        for k in (("A", "B") if it % 2 == 0 else ("B", "A")):
            _, prof, call_ms = profile(ctx, lambda: aux(k))
            times[k].append(prof["aux_running"]["ms"])
            calls[k].append(call_ms)
            launches[k] = prof["aux_running"]["launches"]
        commit()
        rc, prof, call_ms = profile(ctx, ctx.interpolate)
        ctx.check(rc)
        times["Y"].append(prof["ntt_pass"]["ms"])
        calls["Y"].append(call_ms)
        launches["Y"] = prof["ntt_pass"]["launches"]
        nbytes["Y"] = prof["ntt_pass"]["alg_bytes"]
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "?"
    res = {"metric": "aux_running", "workload": f"Goldilocks, 2^{args.log_rows} rows, w = {w}, ext = {ext}: A = running product of one fraction, three columns per form; "
           f"B = running sum of two fractions (LogUp); Y = ms_interpolate of the same {w} columns; {args.passes} legs each, A / B alternated", "unit": "ms per stage (HIP events, summed over its launches)",
           "product_ms": med["A"], "sum_ms": med["B"], "interpolate_ms": med["Y"], "product_spread": spread["A"], "sum_spread": spread["B"], "interpolate_spread": spread["Y"],
           "launches": launches, "alg_bytes": nbytes, "gb_per_s": {k: nbytes[k] / med[k] / 1e6 for k in med}, "ratio_product_over_interpolate": med["A"] / med["Y"],
           "ratio_sum_over_interpolate": med["B"] / med["Y"], "tile_rows": int(os.environ.get("MS_AUX_TILE", 2048)), "legs_ms": times,
           "call_ms_mean": {k: statistics.mean(v) for k, v in calls.items()}, "legs_call_ms": calls, "column_checked": True, "device": device}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
