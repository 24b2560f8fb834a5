"""Big-integer restatement of ms_mix_terms by its DEFINITION (include/ministark.h), in plain Python integers; imports nothing of the product.

    C_t(x)      = sum_{m in terms(t)} coef_m * prod_{f in factors(m)} P_{poly_f}(w^{row_f} x)
    validity(x) = (sum_t r^t C_t(x)) * prod_{k=1..nexempt} (x - w^(N-k)) / (x^N - 1)

Polynomials are coefficient lists, lowest first.  Products are schoolbook, P(w^k x) is the scaling of coefficient i by w^(k i), the division by x^N - 1 is long
division with its own check that the remainder is zero.  `constraints` = [[(coef, [(poly, row), ...]), ...], ...]."""

MODULUS = {0: (1 << 64) - (1 << 32) + 1, 1: (1 << 31) - (1 << 27) + 1}


def check_root(p, omega, N):
    """omega generates the multiplicative subgroup of order N (a power of two)"""
    assert N >= 1 and N & (N - 1) == 0
    assert pow(omega, N, p) == 1 and (N == 1 or pow(omega, N // 2, p) == p - 1)


def interpolate(p, omega, column):
    """coefficients of the polynomial of degree < N with P(omega^i) = column[i]  (the inverse DFT, by the definition: O(N^2))"""
    N = len(column)
    check_root(p, omega, N)
    ninv, winv = pow(N, -1, p), pow(omega, -1, p)
    return [sum(int(v) * pow(winv, i * k, p) for i, v in enumerate(column)) * ninv % p for k in range(N)]


def pmul(p, a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for k, y in enumerate(b):
                out[i + k] = (out[i + k] + x * y) % p
    return out


def padd(p, a, b):
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % p for i in range(n)]


def shifted(p, omega, poly, row):
    """P(omega^row x)"""
    s = pow(omega, row, p)
    out, sp = [], 1
    for c in poly:
        out.append(c * sp % p)
        sp = sp * s % p
    return out


def numerator(p, omega, N, polys, r, constraints, nexempt):
    """(sum_t r^t C_t(x)) * prod_{k=1..nexempt} (x - omega^(N-k))"""
    check_root(p, omega, N)
    mixed, rp = [0], 1
    for terms in constraints:
        ct = [0]
        for coef, factors in terms:
            mono = [coef % p]
            for poly, row in factors:
                mono = pmul(p, mono, shifted(p, omega, polys[poly], row))
            ct = padd(p, ct, mono)
        mixed = padd(p, mixed, [rp * v % p for v in ct])
        rp = rp * r % p
    for k in range(1, nexempt + 1):
        mixed = pmul(p, mixed, [(-pow(omega, N - k, p)) % p, 1])
    return mixed


def divide_by_vanishing(p, num, N):
    """(quotient, remainder) of num / (x^N - 1), long division from the top"""
    rem = list(num)
    quo = [0] * max(1, len(num) - N)
    for k in range(len(num) - 1, N - 1, -1):
        q = rem[k]
        quo[k - N] = q
        rem[k] = 0
        rem[k - N] = (rem[k - N] + q) % p
    return quo, rem[:N]


def is_exact(p, omega, N, polys, r, constraints, nexempt):
    return not any(divide_by_vanishing(p, numerator(p, omega, N, polys, r, constraints, nexempt), N)[1])


def validity(p, omega, N, polys, r, constraints, nexempt, length):
    """the validity polynomial as `length` coefficients (zero above its degree); the division must be exact and the quotient must fit"""
    quo, rem = divide_by_vanishing(p, numerator(p, omega, N, polys, r, constraints, nexempt), N)
    assert not any(rem), "the restatement's own division must be exact for a valid trace"
    while len(quo) > 1 and quo[-1] == 0:
        quo.pop()
    assert len(quo) <= length, (len(quo), length)
    return quo + [0] * (length - len(quo))


def degree(constraints):
    return max(len(factors) for terms in constraints for _, factors in terms)


def validity_len(N, constraints, nexempt):
    """VL of include/ministark.h: N * next_pow2(max(1, d - 1, slots of N the quotient's (d - 1) N - d + nexempt + 1 coefficients need))"""
    d = degree(constraints)
    need = (d - 1) * N - d + nexempt + 1
    slots = max(1, d - 1, -(-need // N))
    v = 1
    while v < slots:
        v *= 2
    return N * v


def horner(p, poly, x):
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + int(c)) % p
    return acc
