"""ms_query_linked (include/ministark.h - build-defined, no reference counterpart) restated in plain Python: the rows a linked proof opens and the MSLQ layout.
Built on pyref_deep / pyref_open, which restate the sections themselves."""
import struct

MSLQ = 0x514C534D   # 'MSLQ'


def link_rows(betas, D0, L):
    """b_j = beta_j mod D_0, p_j = b_j * (L / D_0): query j contributes p_j, then (p_j + L / 2) mod L"""
    out = []
    for beta in betas:
        pj = (int(beta) % D0) * (L // D0)
        out += [pj, (pj + L // 2) % L]
    return out


def mslq(msfi, lde_open, val_open):
    """the MSLQ blob of three sections: 'MSLQ' | len_msfi | len_lde | len_val, u64 little-endian, then the sections"""
    return struct.pack("<4Q", MSLQ, len(msfi), len(lde_open), len(val_open)) + msfi + lde_open + val_open


def split_mslq(blob):
    """(msfi, lde_open, val_open), or None unless the header is there and the three lengths fit the blob exactly"""
    if len(blob) < 32:
        return None
    magic, a, b, c = struct.unpack_from("<4Q", blob, 0)
    if magic != MSLQ or 32 + a + b + c != len(blob):
        return None
    return blob[32:32 + a], blob[32 + a:32 + a + b], blob[32 + a + b:]


# ---------------------------------------------------------------- linked proofs: MSLP v1 (include/ministark_host.h)
import pyref                     # noqa: E402
import pyref_air as ra           # noqa: E402
import pyref_deep as rd          # noqa: E402
import pyref_open as ro          # noqa: E402
from pyref_grind import PURE, pow_ok   # noqa: E402
from common import MODULUS, EXT  # noqa: E402

MSLP_HEAD = "<4s8I4Q"
DOMSEP = "\U0001F43A/linked/v1"
PREFIX = {"header": "header: ", "transcript": "transcript: ", "pow": "proof of work: ", "air": "AIR identity: ", "fri": "FRI: ", "msfi": "MSFI", "lde": "LDE opening: ",
          "validity": "validity opening: ", "link": "DEEP link: "}   # the verifier's step -> how msh_stark_verify_linked's `why` begins


def air_arrays(constraints, exempt=None, periodic=(), boundary=()):
    """the arrays of an ms_air in the order of the struct, as (name, width in bytes, values)"""
    exempt = [[] for _ in constraints] if exempt is None else exempt
    tb, cf, fb, fp, fr, eb, er, pb, pv = [0], [], [0], [], [], [0], [], [0], []
    for terms, rows in zip(constraints, exempt):
        for coef, factors in terms:
            cf.append(int(coef))
            for poly, row in factors:
                fp.append(int(poly)); fr.append(int(row))
            fb.append(len(fp))
        tb.append(len(cf))
        er += [int(x) for x in rows]
        eb.append(len(er))
    for vals in periodic:
        pv += [int(v) for v in vals]
        pb.append(len(pv))
    return [("term_begin", 4, tb), ("coef", 8, cf), ("fac_begin", 4, fb), ("fac_poly", 4, fp), ("fac_row", 4, fr), ("ex_begin", 4, eb), ("ex_row", 4, er),
            ("per_begin", 4, pb), ("per_val", 8, pv), ("bnd_poly", 4, [int(b[0]) for b in boundary]), ("bnd_row", 4, [int(b[1]) for b in boundary]),
            ("bnd_val", 8, [int(b[2]) for b in boundary])]


def encode_air(constraints, exempt=None, periodic=(), boundary=()):
    """msh_air_encode: 'MSAR' | version 1 | ncons nterms nfacs nexempt nperiodic nperval nbound array_bytes | the arrays, little-endian"""
    arrs = dict((n, (w, v)) for n, w, v in air_arrays(constraints, exempt, periodic, boundary))
    body = b"".join(struct.pack("<%d%s" % (len(v), "I" if w == 4 else "Q"), *v) for _, (w, v) in arrs.items())
    counts = [len(constraints), len(arrs["coef"][1]), len(arrs["fac_poly"][1]), len(arrs["ex_row"][1]), len(periodic), len(arrs["per_val"][1]), len(boundary), len(body)]
    return struct.pack("<10I", int.from_bytes(b"MSAR", "little"), 1, *counts) + body


def air_rows(constraints, boundary=()):
    rows = {int(row) for terms in constraints for _, factors in terms for _, row in factors}
    return sorted(rows | ({0} if len(boundary) else set()))


class Transcript:
    """the build-defined hash chain (stark.py, stark_host.cpp) over a plain hash function"""

    def __init__(self, domsep, digest, forced_shifts=()):
        self.H = PURE[digest]
        self.state = self.H(b"mini-stark_amd/transcript/v0" + domsep.encode())
        self.forced_shifts = list(forced_shifts)   # (tests of the redraw rule: what the next single-scalar draws return in place of the chain's values)

    def absorb(self, data):
        self.state = self.H(self.state + b"A" + bytes(data))

    def challenge_bytes(self, n):
        out, ctr = b"", 0
        while len(out) < n:
            out += self.H(self.state + b"C" + struct.pack("<I", ctr))
            ctr += 1
        self.state = self.H(self.state + b"R")
        return out[:n]

    def scalars(self, count, p):
        raw = self.challenge_bytes(16 * count)
        return [int.from_bytes(raw[16 * i:16 * i + 16], "little") % p for i in range(count)]

    def draw_shift(self, p, L):
        """one base-field scalar, redrawn while it is 0 or shift^L == 1; returns (shift, the number of draws)"""
        draws = 0
        while True:
            (s,) = self.scalars(1, p)
            if self.forced_shifts:
                s = self.forced_shifts.pop(0)
            draws += 1
            if shift_ok(p, L, s):
                return s, draws

    def draw_z(self, e, p):
        while True:
            z = self.scalars(e, p)
            if z_ok(z):
                return tuple(z)


def shift_ok(p, L, s):
    return s != 0 and pow(s, L, p) != 1


def z_ok(z):
    return any(int(v) for v in z[1:])


def expected_validity(field, N, r, air, z, opened):
    """the AIR program at z from opened values: opened[(poly, row)] = P_poly(z w^row) as limb tuples (pyref_air_ext.rhs_at with the openings in place of polynomials)"""
    constraints, exempt, periodic, boundary = air
    exempt = [[] for _ in constraints] if exempt is None else exempt
    p, T = MODULUS[field], rd.tower(field)
    omega = pyref.root_of_unity(field, N)
    Q = [ra.periodic_q(p, omega, N, v) for v in periodic]

    def factor(poly, row):
        if poly & ra.PERIODIC:
            q = Q[poly & ~ra.PERIODIC]
            x = T.pow(T.mul(tuple(z), T.from_base(pow(omega, row, p))), N // len(q))
            acc = T.zero()
            for cf in reversed(q):
                acc = T.add(T.mul(acc, x), T.from_base(int(cf)))
            return acc
        return tuple(opened[poly, row])
    den = T.sub(T.pow(tuple(z), N), T.one())
    acc, rp = T.zero(), T.one()
    for terms, rows in zip(constraints, exempt):
        ct = T.zero()
        for coef, factors in terms:
            mm = T.from_base(int(coef))
            for poly, row in factors:
                mm = T.mul(mm, factor(poly, row))
            ct = T.add(ct, mm)
        for rho in rows:
            ct = T.mul(ct, T.sub(tuple(z), T.from_base(pow(omega, rho, p))))
        acc = T.add(acc, T.mul(rp, ct))
        rp = T.mul(rp, tuple(r))
    acc = T.mul(acc, T.inv(den))
    for poly, row, value in boundary:
        num = T.sub(tuple(opened[poly, 0]), T.from_base(int(value)))
        acc = T.add(acc, T.mul(rp, T.mul(num, T.inv(T.sub(tuple(z), T.from_base(pow(omega, row, p)))))))
        rp = T.mul(rp, tuple(r))
    return acc


def shape(field, N, w, blowup, R, gb, air):
    """what prover and verifier derive from the statement: (m, rows, lists, entries, len(arthur))"""
    constraints, exempt, periodic, boundary = air
    exempt = [[] for _ in constraints] if exempt is None else exempt
    e = EXT[field]
    m = e * ra.validity_len(N, constraints, exempt, len(boundary)) // N
    rows = sorted({0} | set(air_rows(constraints, boundary)))
    lists = [list(range(w)) + (list(range(w, w + m)) if k == 0 else []) for k in range(len(rows))]
    ne = sum(len(x) for x in lists)
    return m, rows, lists, ne, 96 + ne * e * 8 + 32 + (R - 1) * (2 * e * 8 + 32) + (8 if gb else 0)


def parse_mslp(data):
    """the MSLP header as a dict with the arthur and MSLQ bytes, or None when the bytes are shorter than a header or the two lengths do not fit exactly"""
    hs = struct.calcsize(MSLP_HEAD)
    if len(data) < hs:
        return None
    magic, ver, e, c, m, npts, R, nq, gb, N, blowup, la, lq = struct.unpack_from(MSLP_HEAD, data, 0)
    if hs + la + lq != len(data):
        return None
    return dict(magic=magic, version=ver, e=e, c=c, m=m, npts=npts, R=R, nq=nq, gb=gb, N=N, blowup=blowup, arthur=data[hs:hs + la], mslq=data[hs + la:])


def verify(field, digest, zae, N, w, blowup, R, nq, gb, air, data, forced_shifts=()):
    """msh_stark_verify_linked with big integers: (accepted, the step that refused: "" / "header" / "transcript" / "pow" / "air" / "fri" / "msfi" / "lde" /
    "validity" / "link").  Everything is the verifier's own: the header is only compared."""
    p, e, T = MODULUS[field], EXT[field], rd.tower(field)
    L = N * blowup
    m, rows, lists, ne, la = shape(field, N, w, blowup, R, gb, air)
    h = parse_mslp(data)
    if h is None:
        return False, "header"
    want = dict(magic=b"MSLP", version=1, e=e, c=w, m=m, npts=len(rows), R=R, nq=nq, gb=gb, N=N, blowup=blowup)
    if any(h[k] != v for k, v in want.items()) or len(h["arthur"]) != la:
        return False, "header"
    sec = split_mslq(h["mslq"])
    if sec is None or any(len(x) % 8 for x in sec):
        return False, "header"
    msfi, lde_open, val_open = sec
    # the transcript
    t = Transcript(DOMSEP, digest, forced_shifts)
    t.absorb(struct.pack("<8Q", field, digest, N, w, blowup, R, nq, gb))
    t.absorb(encode_air(*air))
    a, pos = h["arthur"], 0

    def take(n):
        nonlocal pos
        out = a[pos:pos + n]
        pos += n
        t.absorb(out)
        return out
    take(32)                                             # the raw-trace root: binds nothing
    shift, _ = t.draw_shift(p, L)
    lde_root = take(32)
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
    assert pos == la
    raw = t.challenge_bytes(8 * nq)
    betas = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(nq)]
    # 1. the proof of work
    if gb and not pow_ok(digest, seed, nonce, gb):
        return False, "pow"
    # 2. the AIR identity at z
    opened, at = {}, 0
    for k, row in enumerate(rows):
        for j in range(w):
            opened[j, row] = evals[at + j]
        at += len(lists[k])
    if tuple(expected_validity(field, N, r, air, z, opened)) != tuple(rd.validity_from_chunks(field, e, N, z, evals[w:w + m])):
        return False, "air"
    # 3. FRI on the MSFI section
    if not ro.verify_msfi(field, digest, zae, blowup, roots, zs, Bs, alphas, betas, msfi)[0]:
        return False, "fri"
    # 4. round 0 against the two trees
    omega = pyref.root_of_unity(field, N)
    pts = [T.mul(z, T.from_base(pow(omega, row, p))) for row in rows]
    ok, step = rd.link_verify(field, digest, zae, N, blowup, shift, w, m, lde_root, val_root, pts, lists, evals, gamma, betas, msfi, lde_open, val_open)
    return ok, step
