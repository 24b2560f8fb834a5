"""Big-integer restatement of ms_mix_air by its DEFINITION (include/ministark.h), in plain Python integers; imports the polynomial helpers of pyref_terms.py and
nothing of the product.

    K_k(x)      = Q_k(x^(N/q_k)),  Q_k of degree < q_k with Q_k((w^(N/q_k))^i) = periodic[k][i]                  (periodic column k: K_k(w^i) = periodic[k][i mod q_k])
    C_t(x)      = sum_{m in terms(t)} coef_m * prod_{f in factors(m)} factor_f(x),   factor = P_poly(w^row x)  or  K_k(w^row x) for poly = PERIODIC | k
    Z_t(x)      = prod_{rho in exempt[t]} (x - w^rho)
    validity(x) = sum_t r^t C_t(x) Z_t(x) / (x^N - 1)  +  sum_b r^(ncons + b) (P_{j_b}(x) - v_b) / (x - w^{rho_b})

Polynomials are coefficient lists, lowest first.  Every division is carried out on its own - constraint by constraint, boundary by boundary - by long division
with the remainder checked, so a trace that satisfies the system only "in the random combination" does not pass.
`constraints` = [[(coef, [(poly, row), ...]), ...], ...], `exempt` = one row list per constraint, `periodic` = a list of value lists, `boundary` = [(poly, row, value), ...]."""
from pyref_terms import check_root, divide_by_vanishing, padd, pmul, shifted

PERIODIC = 0x80000000


def periodic_q(p, omega, N, values):
    """Q of degree < q with Q(eta^i) = values[i], eta = omega^(N/q): the inverse DFT by its definition, the powers of eta^-1 from a table"""
    q = len(values)
    assert q >= 1 and q & (q - 1) == 0 and q <= N and N % q == 0
    eta = pow(omega, N // q, p)
    check_root(p, eta, q)
    qinv, einv = pow(q, -1, p), pow(eta, -1, p)
    tab = [pow(einv, i, p) for i in range(q)]
    return [sum(int(v) * tab[i * m % q] for i, v in enumerate(values)) * qinv % p for m in range(q)]


def periodic_poly(p, omega, N, values):
    """K(x) = Q(x^(N/q)) as N coefficients"""
    q = len(values)
    Q = periodic_q(p, omega, N, values)
    out = [0] * N
    for m, c in enumerate(Q):
        out[m * (N // q)] = c
    return out


def factor_poly(p, omega, N, polys, periodic, poly, row):
    base = periodic_poly(p, omega, N, periodic[poly & ~PERIODIC]) if poly & PERIODIC else polys[poly]
    return shifted(p, omega, base, row)


def constraint_poly(p, omega, N, polys, periodic, terms):
    ct = [0]
    for coef, factors in terms:
        mono = [coef % p]
        for poly, row in factors:
            mono = pmul(p, mono, factor_poly(p, omega, N, polys, periodic, poly, row))
        ct = padd(p, ct, mono)
    return ct


def divide_linear(p, num, a):
    """(quotient, remainder) of num / (x - a), synthetic division from the top"""
    quo, carry = [0] * max(1, len(num) - 1), 0
    for k in range(len(num) - 1, 0, -1):
        carry = (num[k] + carry * a) % p
        quo[k - 1] = carry
    return quo, (num[0] + carry * a) % p


def quotients(p, omega, N, polys, r, constraints, exempt, periodic, boundary):
    """[(quotient, remainder is zero)] of every transition and boundary constraint, already scaled by its power of r"""
    check_root(p, omega, N)
    assert len(exempt) == len(constraints)
    out, rp = [], 1
    for terms, rows in zip(constraints, exempt):
        assert len(set(rows)) == len(rows) and all(0 <= k < N for k in rows)
        num = constraint_poly(p, omega, N, polys, periodic, terms)
        for rho in rows:
            num = pmul(p, num, [(-pow(omega, rho, p)) % p, 1])
        quo, rem = divide_by_vanishing(p, num, N)
        out.append(([rp * v % p for v in quo], not any(rem)))
        rp = rp * r % p
    for poly, row, value in boundary:
        num = list(polys[poly])
        num[0] = (num[0] - value) % p
        quo, rem = divide_linear(p, num, pow(omega, row, p))
        out.append(([rp * v % p for v in quo], rem == 0))
        rp = rp * r % p
    return out


def is_exact(p, omega, N, polys, r, constraints, exempt, periodic=(), boundary=()):
    return all(ok for _, ok in quotients(p, omega, N, polys, r, constraints, exempt, periodic, boundary))


def validity(p, omega, N, polys, r, constraints, exempt, periodic, boundary, length):
    """the validity polynomial as `length` coefficients (zero above its degree); every division must be exact and the sum must fit"""
    acc = [0]
    for quo, ok in quotients(p, omega, N, polys, r, constraints, exempt, periodic, boundary):
        assert ok, "the restatement's own divisions must be exact for a valid trace"
        acc = padd(p, acc, quo)
    while len(acc) > 1 and acc[-1] == 0:
        acc.pop()
    assert len(acc) <= length, (len(acc), length)
    return acc + [0] * (length - len(acc))


def validity_len(N, constraints, exempt, nbound):
    """VL of include/ministark.h: N * next_pow2(ceil(nq / N)), nq = max(max_t (d_t (N - 1) + e_t - N + 1), N - 1 if there are boundary constraints, 1)"""
    nq = max(max(len(factors) for _, factors in terms) * (N - 1) + len(rows) - N + 1 for terms, rows in zip(constraints, exempt) if terms)
    nq = max(nq, N - 1 if nbound else 0, 1)
    v = 1
    while v < -(-nq // N):
        v *= 2
    return N * v


def periodic_at(p, N, Q, x):
    """K(x) = Q(x^(N/q)) at a base-field point, Q from periodic_q"""
    y, acc = pow(x, N // len(Q), p), 0
    for c in reversed(Q):
        acc = (acc * y + c) % p
    return acc
