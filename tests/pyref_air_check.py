"""ms_air_check (include/ministark.h; build-defined, diagnostic) restated in Python integers: the ms_air program evaluated on the rows of the trace domain.
    T_j[i]                          the value of column / polynomial j on row i
    factor (j, row)                 T_j[(i + row) mod N]
    factor (PERIODIC | k, row)      periodic[k][(i + row) mod q_k]
    C_t(i)                          sum_m coef_m prod_f factor_f(i)  in Fp
    row i violates constraint t     C_t(i) != 0 and i not in exempt[t]
`cols[j][i]` = T_j[i].  Nothing here knows how the kernel splits the rows."""
PERIODIC = 0x80000000


def constraint_values(p, N, cols, periodic, terms):
    """[C_t(i) for i in range(N)] for one constraint"""
    out = []
    for i in range(N):
        acc = 0
        for coef, factors in terms:
            m = coef % p
            for poly, row in factors:
                if poly & PERIODIC:
                    vals = periodic[poly & ~PERIODIC]
                    m = m * vals[(i + row) % len(vals)] % p
                else:
                    m = m * int(cols[poly][(i + row) % N]) % p
            acc = (acc + m) % p
        out.append(acc)
    return out


def check(p, N, cols, constraints, exempt=None, periodic=(), boundary=()):
    """The report of ms_air_check as Context.air_check returns it, with plain lists: nfail, count, first_row, bnd_got, bnd_fail, first, ok"""
    exempt = [[] for _ in constraints] if exempt is None else exempt
    count, first_row = [], []
    for terms, rows in zip(constraints, exempt):
        skip = {int(r) for r in rows}
        bad = [i for i, v in enumerate(constraint_values(p, N, cols, periodic, terms)) if v and i not in skip]
        count.append(len(bad))
        first_row.append(bad[0] if bad else N)
    bnd_got = [int(cols[poly][row]) for poly, row, _ in boundary]
    bnd_fail = [b for b, (_, _, value) in enumerate(boundary) if bnd_got[b] != int(value)]
    hits = [(first_row[t], t) for t in range(len(constraints)) if count[t]]
    nfail = len(hits) + len(bnd_fail)
    return {"nfail": nfail, "count": count, "first_row": first_row, "bnd_got": bnd_got, "bnd_fail": bnd_fail, "first": min(hits) if hits else None, "ok": nfail == 0}
