"""Big-integer restatement of ms_aux_running by its DEFINITION (include/ministark.h), in plain Python integers; imports the tower of pyref.py and nothing of the product.

    a_f(i) = const_f + sum_m coef_m * T_{col_m}[i]                      (in K: tuples of `ext` limbs)
    s_i    = sum_k num_k(i) / den_k(i)   (SUM = 0)   or   prod_k num_k(i) / den_k(i)   (PRODUCT = 1)
    z_0    = identity,  z_{i+1} = z_i o s_i,  final = z_{N-1} o s_{N-1}

`fractions` = [((const, [(col, coef), ...]), (const, [(col, coef), ...])), ...] with const / coef ints for ext = 1 and ext-tuples otherwise; `trace` a list of rows
(or an N x w array).  Two checks: `running` restates the definition row by row with one inversion (Tower.inv) per fraction; `check_recurrence` needs none - with
A_i / B_i the row's fractions on ONE denominator, a column is right iff z_0 is the identity and z_{i+1} B_i = z_i A_i (PRODUCT) or (z_{i+1} - z_i) B_i = A_i (SUM)
for every row, `final` standing for z_N; given B_i != 0 that determines the column.  Both assert that no denominator vanishes."""
from pyref import Tower

SUM, PRODUCT = 0, 1


def _k(T, v):
    return tuple(int(x) % T.p for x in v) if isinstance(v, (tuple, list)) else T.from_base(int(v))


def form_at(T, form, row):
    const, terms = form
    acc = _k(T, const)
    for col, coef in terms:
        v = int(row[col])
        acc = T.add(acc, tuple(c * v % T.p for c in _k(T, coef)))   # (K is a vector space over Fp: a base-field factor scales every limb)
    return acc


def identity(T, op):
    return T.one() if op == PRODUCT else T.zero()


def running(field, ext, op, fractions, trace):
    """(column as a list of N ext-tuples, final)"""
    T = Tower(field, ext)
    z, col = identity(T, op), []
    for row in trace:
        col.append(z)
        s = identity(T, op)
        for num, den in fractions:
            d = form_at(T, den, row)
            assert not T.is_zero(d), "a denominator vanishes: pick the next seed"
            q = T.mul(form_at(T, num, row), T.inv(d))
            s = T.mul(s, q) if op == PRODUCT else T.add(s, q)
        z = T.mul(z, s) if op == PRODUCT else T.add(z, s)
    return col, z


def one_fraction(T, op, fractions, row):
    """(A, B): the row's fractions on one denominator"""
    A, B = None, None
    for num, den in fractions:
        n, d = form_at(T, num, row), form_at(T, den, row)
        assert not T.is_zero(d), "a denominator vanishes: pick the next seed"
        if A is None:
            A, B = n, d
        else:
            A = T.mul(A, n) if op == PRODUCT else T.add(T.mul(A, d), T.mul(n, B))
            B = T.mul(B, d)
    return A, B


def check_recurrence(field, ext, op, fractions, trace, column, final):
    """True iff `column` (N ext-tuples) and `final` are the running column of the definition; no inversions"""
    T = Tower(field, ext)
    N = len(trace)
    if len(column) != N or tuple(column[0]) != identity(T, op):
        return False
    for i, row in enumerate(trace):
        A, B = one_fraction(T, op, fractions, row)
        z, zn = tuple(column[i]), tuple(column[i + 1]) if i + 1 < N else tuple(final)
        if op == PRODUCT:
            ok = T.mul(zn, B) == T.mul(z, A)
        else:
            ok = T.mul(T.sub(zn, z), B) == A
        if not ok:
            return False
    return True
