"""The NTT plan of a transform and the pass kernel instance every pass launches, restated in plain Python from the rule the library had while the two were
decided in two places: the shape by Ctx::get_plan (passes, K[], LC[], the virtual pass, which generation each pass belongs to), the instance at every launch
by the chain launch_pass -> launch_v2k -> launch_v2 -> launch_v2m -> launch_v2i (beside it launch_reg and launch_fast) out of the pass's PassParams.
tests/test_ntt_plan_emu.py holds the library's plan-time choice (ms_emu_ntt_plan) to this file for every size up to the field's two-adicity.

    shape(field, log_n, log_pad, knobs)                -> {"log_r0", "log_rho", "passes": [{"K", "LC", "v2", "regp"}]}
    launches(field, log_n, log_pad, inverse, batch, knobs) -> the instance name of every pass, as the per-kernel profile spells it; where the chain found the plan and
                                                          the kernel at odds, the integer it returned then (994 .. 999) stands in the name's place
The rule is restated as written, for any number of passes: the library's arrays then held four, so MS_NTT_KMAX=5 had no valid plan above 2^20 points; a plan holds seven now.
Fields: 0 Goldilocks, 1 BabyBear.  n_in, the valid input length, is taken as n >> log_pad: the longest input that log_pad stands for."""
TWO_ADICITY = (32, 27)
ELEMENT_BYTES = (8, 4)
FIELD_NAME = ("GL", "BB")
TILE_LOG_C, MAX_LOG_R, MAX_LOG_RHO = 4, 10, 2


def knobs(**env):
    """the context's NTT knobs as ms_create reads them from MS_NTT_*: knobs(KMAX=5, FAST=0)"""
    k = {"KMAX": 9, "FAST": 1, "V2": 1, "V2_REGPASS": 1, "SHARE": 1, "COOP_WGS": 512}
    for name, v in env.items():
        v = int(v)
        if name == "KMAX":
            if 5 <= v <= MAX_LOG_R:
                k[name] = v
        elif name == "COOP_WGS":
            if 8 <= v <= 65536:
                k[name] = v & ~7
        else:
            k[name] = v
    return k


def split(m, P):
    return [m // P + (1 if i < m % P else 0) for i in range(P)]


def shape(field, log_n, log_pad, kn):
    v2_lc = 3 if field == 0 else 4
    passes = None
    log_r0 = log_rho = 0
    if kn["V2"] >= 1 and log_n >= 14 and log_n > MAX_LOG_R and log_pad in (0, 3):
        m = log_n - log_pad
        P = (m + 9) // 10
        kb = 7 if kn["V2_REGPASS"] == 2 else 10
        if kn["V2_REGPASS"] and 1 <= m - 2 * kb <= 5:
            log_r0 = log_pad
            passes = [{"K": kb, "LC": 3 if log_pad else v2_lc, "v2": True, "regp": False}, {"K": kb, "LC": v2_lc, "v2": True, "regp": False},
                      {"K": m - 2 * kb, "LC": 0, "v2": False, "regp": True}]
        elif P <= 2 and m // P >= 7:
            log_r0 = log_pad
            passes = [{"K": K, "LC": 3 if (i == 0 and log_pad) else v2_lc, "v2": True, "regp": False} for i, K in enumerate(split(m, P))]
    if passes is None:
        if log_n <= MAX_LOG_R:
            Ks = [log_n]
        else:
            best_rho, bestP = 0, 1 << 20
            for lr in range((MAX_LOG_RHO if log_pad else 0) + 1):
                m = log_n - log_pad - lr
                if m < 2:
                    break
                P = (m + kn["KMAX"] - 1) // kn["KMAX"]
                if P < 2 and log_pad == 0:
                    P = 2
                P = max(P, 1)
                if P < bestP:
                    bestP, best_rho = P, lr
            if kn["FAST"] and bestP > 1 and (log_pad == 0 or 22 <= log_n <= 24):
                best_rho = log_pad = 0
                bestP = max((log_n + kn["KMAX"] - 1) // kn["KMAX"], 2)
            log_rho, log_r0 = best_rho, log_pad + best_rho
            Ks = split(log_n - log_r0, bestP)
        passes = [{"K": K, "LC": TILE_LOG_C, "v2": False, "regp": False} for K in Ks]
    return {"log_r0": log_r0, "log_rho": log_rho, "passes": passes}


def coop_grid(kn, work_items, per_cu=2):
    return min(work_items, kn["COOP_WGS"] * per_cu // 2)


def tf(b):
    return "true" if b else "false"


def pass_kernel2(field, inverse, K, LC, mode, pp):
    """launch_v2m's arms, then launch_v2i: the instance's constants, its applicable(), its name"""
    if field == 0 and K in (8, 9) and LC == 3:
        arith, th, nsub = "GLM", 256 if K == 8 else 512, 3
    elif field == 0 and K == 10 and LC == 3:
        arith, th, nsub = "GLM", 512, 3
    elif field == 1 and K == 10:
        arith, th, nsub = "BB", 512 if LC == 4 else 256, 3
    else:
        arith, th, nsub = ("GLT", "BB")[field], 256, 2
    pm = 2 if mode == 3 else mode
    mode_of = 2 if pp["log_r0"] else (0 if pp["log_Rp"] == 0 else 1)
    ok = (pp["log_r"] == K and pp["log_C"] == LC and pp["log_rho"] == 0 and mode_of == pm and (mode != 3 or pp["nbatch"] > 1) and
          ((pp["log_r0"] == 0 and (pp["log_Rp"] == 0 or pp["log_Rp"] >= LC)) or (pp["log_r0"] == LC and pp["log_Rp"] == LC)))
    if not ok:
        return 998
    return "msntt::PassKernel2<%s, %s, %s, %d, %d, %d, %d, %d>" % (FIELD_NAME[field], arith, tf(inverse), K, LC, th, nsub, mode)


def launch_pass(field, inverse, kn, pp, tiles, batch, v2, regp):
    K = pp["log_r"]
    if regp:
        if not 1 <= K <= 5:
            return 994
        vec = 16 // ELEMENT_BYTES[field] if K <= 4 else 1
        ok = (pp["last"] and pp["log_r0"] == 0 and pp["log_rho"] == 0 and pp["log_Rp"] == pp["log_n"] - K and pp["n_in"] >= 1 << pp["log_n"] and
              (1 << pp["log_Rp"]) % vec == 0)
        return "msntt::RegPassKernel<%s, %s, %s, %d>" % (FIELD_NAME[field], ("GLM", "BB")[field], tf(inverse), K) if ok else 995
    if v2:
        if field == 0 and pp["log_C"] != 3:
            return 997
        LC = 3 if pp["log_C"] == 3 else 4
        if not 7 <= K <= 10:
            return 999
        if pp["log_r0"]:
            if LC != 3:
                return 996
            if field == 0 and K == 10 and kn["SHARE"] and batch > 1 and tiles >= coop_grid(kn, tiles * batch) and (tiles & 7) == 0:
                return pass_kernel2(field, inverse, K, LC, 3, pp)
            return pass_kernel2(field, inverse, K, LC, 2, pp)
        return pass_kernel2(field, inverse, K, LC, 0 if pp["log_Rp"] == 0 else 1, pp)
    if kn["FAST"] and pp["log_C"] == TILE_LOG_C and pp["log_r0"] == 0 and (pp["log_Rp"] == 0 or pp["log_Rp"] >= TILE_LOG_C) and 6 <= K <= 9:
        return "msntt::PassKernelK<%s, %s, %d, %d>" % (FIELD_NAME[field], tf(inverse), K, 512 if K == 9 else 256)
    th512 = K >= 9 and pp["log_C"] == TILE_LOG_C
    return "msntt::PassKernel<%s, %s, %d>" % (FIELD_NAME[field], tf(inverse), 512 if th512 else 256)


def launches(field, log_n, log_pad, inverse, batch, kn):
    """ntt_run's loop: the PassParams of every pass out of the plan, and what launch_pass makes of them"""
    sh = shape(field, log_n, log_pad, kn)
    n = 1 << log_n
    P = len(sh["passes"])
    out = []
    log_Rp = sh["log_r0"]
    for k, ps in enumerate(sh["passes"]):
        cols_log = log_n - ps["K"]
        pp = {"log_n": log_n, "log_r": ps["K"], "log_Rp": log_Rp, "log_r0": sh["log_r0"] if k == 0 else 0, "log_rho": sh["log_rho"] if k == 0 else 0,
              "log_C": min(cols_log, ps["LC"]), "last": k == P - 1, "nbatch": batch, "n_in": n >> log_pad if k == 0 else n}
        tiles = (1 << cols_log) >> pp["log_C"]
        out.append(launch_pass(field, inverse, kn, pp, tiles, batch, ps["v2"], ps["regp"]))
        log_Rp += ps["K"]
    return out
