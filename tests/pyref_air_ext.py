"""Restatement of ms_mix_air_ext by its DEFINITION (include/ministark.h) in plain Python integers: ms_mix_air's formula with the combiner r in the extension K,

    validity(x) = sum_t r^t C_t(x) Z_t(x) / (x^N - 1)  +  sum_b r^(ncons + b) (P_{j_b}(x) - v_b) / (x - w^{rho_b}),     r^t taken in K.

The per-constraint quotients are base-field polynomials (pyref_air.quotients with r = 1: unscaled, every division carried out and checked on its own); they are
combined limb by limb with the Tower powers of r.  A K-valued polynomial is a list of limb tuples, lowest coefficient first.  Imports nothing of the product."""
import pyref_air as ra
from common import MODULUS, EXT
from pyref import Tower

PERIODIC = ra.PERIODIC


def tower(field):
    return Tower(field, EXT[field])


def validity(field, omega, N, polys, r, constraints, exempt, periodic, boundary, length):
    """`length` coefficients in K (zero above the degree): limb l of coefficient k is sum_t (r^t)_l q_{t,k}"""
    p, T = MODULUS[field], tower(field)
    assert len(r) == T.e
    planes = [[0] * length for _ in range(T.e)]
    rp = T.one()
    for quo, ok in ra.quotients(p, omega, N, polys, 1, constraints, exempt, periodic, boundary):
        assert ok, "the restatement's own divisions must be exact for a valid trace"
        while len(quo) > 1 and quo[-1] == 0:
            quo = quo[:-1]
        assert len(quo) <= length, (len(quo), length)
        for limb, plane in zip(rp, planes):
            if limb:
                for k, v in enumerate(quo):
                    plane[k] = (plane[k] + limb * v) % p
        rp = T.mul(rp, tuple(r))
    return [tuple(plane[k] for plane in planes) for k in range(length)]


def horner_base(T, poly, x):
    """a base-field polynomial at a point of K"""
    acc = T.zero()
    for c in reversed(poly):
        acc = T.add(T.mul(acc, x), T.from_base(int(c)))
    return acc


def horner_ext(T, poly, x):
    """a K-valued polynomial (limb tuples) at a point of K"""
    acc = T.zero()
    for c in reversed(poly):
        acc = T.add(T.mul(acc, x), tuple(int(v) for v in c))
    return acc


def rhs_at(field, omega, N, polys, r, constraints, exempt, periodic, boundary, z):
    """the right-hand side of the defining formula at z in K (z^N != 1), in Tower arithmetic, with inverses in K: independent of any polynomial product"""
    p, T = MODULUS[field], tower(field)
    Q = [ra.periodic_q(p, omega, N, v) for v in periodic]
    seen = {}

    def factor(poly, row):
        if (poly, row) not in seen:
            x = T.mul(z, T.from_base(pow(omega, row, p)))
            if poly & PERIODIC:
                q = Q[poly & ~PERIODIC]
                seen[(poly, row)] = horner_base(T, q, T.pow(x, N // len(q)))
            else:
                seen[(poly, row)] = horner_base(T, polys[poly], x)
        return seen[(poly, row)]
    den = T.sub(T.pow(z, N), T.one())
    assert not T.is_zero(den)
    acc, rp = T.zero(), T.one()
    for terms, rows in zip(constraints, exempt):
        ct = T.zero()
        for coef, factors in terms:
            m = T.from_base(coef)
            for poly, row in factors:
                m = T.mul(m, factor(poly, row))
            ct = T.add(ct, m)
        for rho in rows:
            ct = T.mul(ct, T.sub(z, T.from_base(pow(omega, rho, p))))
        acc = T.add(acc, T.mul(rp, ct))
        rp = T.mul(rp, tuple(r))
    acc = T.mul(acc, T.inv(den))
    for poly, row, value in boundary:
        num = T.sub(factor(poly, 0), T.from_base(value))
        acc = T.add(acc, T.mul(rp, T.mul(num, T.inv(T.sub(z, T.from_base(pow(omega, row, p)))))))
        rp = T.mul(rp, tuple(r))
    return acc
