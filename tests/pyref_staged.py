"""An independent restatement of the staged layout of ms_query_linked (MSLS; include/ministark.h), in plain Python: the bytes of a blob from its four sections, and
the sections of a blob; and of MSLP v2 (include/ministark_host.h): the 'MSAX' encoding, the constraints of an argument, the header and the verifier.  Imports nothing from
the library."""
import struct

MSLS = 0x534C534D   # 'MSLS'
assert MSLS == int.from_bytes(b"MSLS", "little")


def msls(msfi, lde_open, stg_open, val_open):
    """'MSLS' | len_msfi | len_lde | len_stg | len_val, u64 little-endian, then the four sections"""
    return struct.pack("<5Q", MSLS, len(msfi), len(lde_open), len(stg_open), len(val_open)) + msfi + lde_open + stg_open + val_open


def split_msls(blob):
    """(msfi, lde_open, stg_open, val_open), or None unless the header is there and the four lengths fit the blob exactly"""
    if len(blob) < 40:
        return None
    magic, a, b, c, d = struct.unpack_from("<5Q", blob, 0)
    if magic != MSLS or 40 + a + b + c + d != len(blob):
        return None
    o = 40
    out = []
    for n in (a, b, c, d):
        out.append(blob[o:o + n])
        o += n
    return tuple(out)


# ---------------------------------------------------------------- linked proofs with running columns: 'MSAX', MSLP v2 and its verifier (include/ministark_host.h)
import pyref                      # noqa: E402
import pyref_deep as rd           # noqa: E402
import pyref_linked as rl         # noqa: E402
import pyref_open as ro           # noqa: E402
from pyref_grind import pow_ok    # noqa: E402
from common import MODULUS, EXT   # noqa: E402

MSLP2_HEAD = "<4s11I4Q"
DOMSEP = "\U0001F43A/linked/v2"
PREFIX = dict(rl.PREFIX, staged="staged opening: ")
SUM, PRODUCT = 0, 1
ARG_ORDER = ("form_begin", "term_col", "term_ch", "form_ch", "term_coef", "form_const")


def encode_aux(args, nch):
    """msh_aux_encode: 'MSAX' | version 1 | nargs | nch, then per argument op, nfrac, nterms | form_begin | term_col | term_ch | form_ch | term_coef | form_const"""
    out = struct.pack("<4I", int.from_bytes(b"MSAX", "little"), 1, len(args), nch)
    for a in args:
        nterms = len(a["term_col"])
        out += struct.pack("<3I", int(a["op"]), int(a["nfrac"]), nterms)
        for name in ARG_ORDER:
            vals = [int(v) for v in a[name]]
            out += struct.pack("<%d%s" % (len(vals), "Q" if name in ("term_coef", "form_const") else "I"), *vals)
    return out


def instantiate(field, arg, ch):
    """the forms of an argument with the challenges in place: [(const, [(col, coef)])] per form, elements of K as limb tuples"""
    p, e = MODULUS[field], EXT[field]

    def val(v, sel):
        return tuple(int(v) * x % p for x in ch[int(sel) - 1]) if int(sel) else (int(v),) + (0,) * (e - 1)
    fb = [int(x) for x in arg["form_begin"]]
    return [(val(arg["form_const"][f], arg["form_ch"][f]), [(int(arg["term_col"][m]), val(arg["term_coef"][m], arg["term_ch"][m])) for m in range(fb[f], fb[f + 1])])
            for f in range(2 * int(arg["nfrac"]))]


def argument_constraints(field, op, forms, first_poly):
    """the transition constraint of a running column cleared of denominators, as E base-field constraints over the limb polynomials first_poly .., and the boundary
    z(w^0) = identity: polynomials in the variables (poly, row) with coefficients in K, a monomial = the sorted tuple of its variables"""
    p, e, T = MODULUS[field], EXT[field], rd.tower(field)

    def add(a, b, sign=1):
        out = dict(a)
        for mono, c in b.items():
            out[mono] = T.add(out.get(mono, T.zero()), c) if sign > 0 else T.sub(out.get(mono, T.zero()), c)
        return out

    def mul(a, b):
        out = {}
        for ma, ca in a.items():
            for mb, cb in b.items():
                mono = tuple(sorted(ma + mb))
                out[mono] = T.add(out.get(mono, T.zero()), T.mul(ca, cb))
        return out

    def form(f):
        out = {(): tuple(f[0])}
        for col, coef in f[1]:
            out = add(out, {((col, 0),): tuple(coef)})
        return out
    unit = lambda l: tuple(1 if i == l else 0 for i in range(e))   # noqa: E731
    zc = {((first_poly + l, 0),): unit(l) for l in range(e)}
    zn = {((first_poly + l, 1),): unit(l) for l in range(e)}
    nums, dens = [form(f) for f in forms[0::2]], [form(f) for f in forms[1::2]]
    den = {(): unit(0)}
    for d in dens:
        den = mul(den, d)
    if op == PRODUCT:
        num = {(): unit(0)}
        for n in nums:
            num = mul(num, n)
        expr = add(mul(zn, den), mul(zc, num), -1)
    else:
        expr = mul(add(zn, zc, -1), den)
        for k, n in enumerate(nums):
            t = n
            for j, d in enumerate(dens):
                if j != k:
                    t = mul(t, d)
            expr = add(expr, t, -1)
    cons = [[(c[l], list(mono)) for mono, c in sorted(expr.items()) if c[l]] for l in range(e)]
    boundary = [(first_poly + l, 0, 1 if (op == PRODUCT and l == 0) else 0) for l in range(e)]
    return cons, [[] for _ in range(e)], boundary


def combined_program(field, w, air, args, ch):
    cons, exempt, periodic, boundary = air
    cons, exempt, boundary = list(cons), list(exempt if exempt is not None else [[] for _ in cons]), list(boundary)
    for k, a in enumerate(args):
        c2, e2, b2 = argument_constraints(field, int(a["op"]), instantiate(field, a, ch), w + k * EXT[field])
        cons, exempt, boundary = cons + c2, exempt + e2, boundary + b2
    return cons, exempt, periodic, boundary


def parse_mslp2(data):
    """the MSLP v2 header as a dict with the arthur and MSLS bytes, or None when the bytes are shorter than a header or the two lengths do not fit exactly"""
    hs = struct.calcsize(MSLP2_HEAD)
    if len(data) < hs:
        return None
    magic, ver, e, c0, c1, m, npts, R, nq, gb, nargs, nch, N, blowup, la, lq = struct.unpack_from(MSLP2_HEAD, data, 0)
    if hs + la + lq != len(data):
        return None
    return dict(magic=magic, version=ver, e=e, c0=c0, c1=c1, m=m, npts=npts, R=R, nq=nq, gb=gb, nargs=nargs, nch=nch, N=N, blowup=blowup, arthur=data[hs:hs + la],
                msls=data[hs + la:])


def link_verify(field, digest, zae, N, blowup, shift, c0, c1, m, lde_root, stg_root, val_root, zs, lists, evals, gamma, betas, msfi, lde_open, stg_open, val_open):
    """pyref_deep.link_verify with two LDE trees: (accepted, the step that refused: "" / "msfi" / "lde" / "staged" / "validity" / "link")"""
    T, p, e = rd.tower(field), MODULUS[field], EXT[field]
    L = N * blowup
    try:
        hd, fin, paths = ro.msfi_parse(msfi, e)
    except (AssertionError, struct.error):
        return False, "msfi"
    R, nq, D0 = hd[2], hd[3], hd[4]
    if nq != len(betas) or D0 < 1 or D0 & (D0 - 1) or D0 > L or L % D0:
        return False, "msfi"
    gL, g0 = pyref.root_of_unity(field, L), pyref.root_of_unity(field, D0)
    pos3 = [0, 0, 0]
    trees = (("lde", c0, lde_root, lde_open), ("staged", c1, stg_root, stg_open), ("validity", m, val_root, val_open))
    for j, b in enumerate(betas):
        b = int(b) % D0
        for s, pos in enumerate((b, (b + D0 // 2) % D0)):
            row = pos * (L // D0)
            opened = []
            for k, (step, width, root, blob) in enumerate(trees):
                ok, used = ro.check_path_index(digest, p, 1, width, zae, root, blob[pos3[k]:], row)
                if not ok:
                    return False, step
                opened += list(struct.unpack_from("<%dQ" % width, blob, pos3[k] + 8))
                pos3[k] += used
            x = shift * pow(gL, row, p) % p
            got = rd.composition_at(field, opened, evals, zs, lists, gamma, x)
            if R > 1:
                path = paths[0][j][s]
                if struct.unpack_from("<Q", path, 0)[0] != pos:
                    return False, "msfi"
                y = struct.unpack_from("<%dQ" % e, path, 8 + (pos & 1) * e * 8)
            else:
                y, xb = T.zero(), T.from_base(pow(g0, pos, p))
                for cf in reversed(fin):
                    y = T.add(T.mul(y, xb), tuple(cf))
            if tuple(got) != tuple(y):
                return False, "link"
    for k, (step, _w, _r, blob) in enumerate(trees):
        if pos3[k] != len(blob):
            return False, step
    return True, ""


def verify(field, digest, zae, N, w, blowup, R, nq, gb, air, args, nch, data):
    """msh_stark_verify_linked_aux with big integers: (accepted, the step that refused)"""
    p, e, T = MODULUS[field], EXT[field], rd.tower(field)
    L = N * blowup
    c1 = len(args) * e
    c = w + c1
    h = parse_mslp2(data)
    if h is None:
        return False, "header"
    want = dict(magic=b"MSLP", version=2, e=e, c0=w, c1=c1, R=R, nq=nq, gb=gb, nargs=len(args), nch=nch, N=N, blowup=blowup)
    if any(h[k] != v for k, v in want.items()) or len(h["arthur"]) < 64:
        return False, "header"
    t = rl.Transcript(DOMSEP, digest)
    t.absorb(struct.pack("<10Q", field, digest, N, w, blowup, R, nq, gb, len(args), nch))
    t.absorb(rl.encode_air(*air))
    t.absorb(encode_aux(args, nch))
    a, pos = h["arthur"], 0

    def take(n):
        nonlocal pos
        out = a[pos:pos + n]
        pos += n
        t.absorb(out)
        return out
    take(32)
    shift, _ = t.draw_shift(p, L)
    lde_root = take(32)
    flat = t.scalars(nch * e, p)
    ch = [tuple(flat[k * e:(k + 1) * e]) for k in range(nch)]
    prog = combined_program(field, w, air, args, ch)
    m, rows, lists, ne, la = rl.shape(field, N, c, blowup, R, gb, prog)
    if (h["m"], h["npts"], len(h["arthur"])) != (m, len(rows), la + 32):
        return False, "header"
    sec = split_msls(h["msls"])
    if sec is None or any(len(x) % 8 for x in sec):
        return False, "header"
    msfi, lde_open, stg_open, val_open = sec
    stg_root = take(32)
    r = t.scalars(e, p)
    val_root = take(32)
    z = t.draw_z(e, p)
    flat = struct.unpack("<%dQ" % (ne * e), take(ne * e * 8))
    if any(v >= p for v in flat):
        return False, "transcript"
    evals = [tuple(flat[n * e:(n + 1) * e]) for n in range(ne)]
    gamma = tuple(t.scalars(e, p))
    roots, zs, Bs, alphas = [take(32)], [], [], []
    for _ in range(1, R):
        zs.append(tuple(t.scalars(e, p)))
        B = struct.unpack("<%dQ" % (2 * e), take(2 * e * 8))
        Bs.append((B[:e], B[e:]))
        alphas.append(tuple(t.scalars(e, p)))
        roots.append(take(32))
    if any(v >= p for B in Bs for half in B for v in half):
        return False, "transcript"
    if gb:
        seed = t.challenge_bytes(32)
        (nonce,) = struct.unpack("<Q", take(8))
    assert pos == la + 32
    raw = t.challenge_bytes(8 * nq)
    betas = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(nq)]
    if gb and not pow_ok(digest, seed, nonce, gb):
        return False, "pow"
    opened, at = {}, 0
    for k, row in enumerate(rows):
        for j in range(c):
            opened[j, row] = evals[at + j]
        at += len(lists[k])
    if tuple(rl.expected_validity(field, N, r, prog, z, opened)) != tuple(rd.validity_from_chunks(field, e, N, z, evals[c:c + m])):
        return False, "air"
    if not ro.verify_msfi(field, digest, zae, blowup, roots, zs, Bs, alphas, betas, msfi)[0]:
        return False, "fri"
    omega = pyref.root_of_unity(field, N)
    pts = [T.mul(z, T.from_base(pow(omega, row, p))) for row in rows]
    return link_verify(field, digest, zae, N, blowup, shift, w, c1, m, lde_root, stg_root, val_root, pts, lists, evals, gamma, betas, msfi, lde_open, stg_open, val_open)
