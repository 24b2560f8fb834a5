"""Cases of ms_query_linked (the whole query phase of a linked proof in one launch, the MSLQ blob; include/ministark.h - build-defined, no reference counterpart),
shared by the emulation suite (tests/test_linked_emu.py) and the GPU suite (tests/test_linked_gpu.py).  The oracle is the definition: the bytes of
ms_fri_query_index, ms_tree_open(MS_TREE_LDE) and ms_tree_open(MS_TREE_VALIDITY) behind the MSLQ header (tests/pyref_linked.py restates the layout and the rows);
every comparison is exact.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import ctypes as C

import numpy as np

import mini_stark_amd as ms
import deep_cases as dc
import open_cases as oc
import pyref_linked as rl
from common import MODULUS, EXT, SplitMix64

SHA, KECCAK = dc.SHA, dc.ro.KECCAK256
ctx_of = oc.ctx_of
_u64p = C.POINTER(C.c_uint64)


def spec_of(name, field, N, seed):
    """the AIR programs of deep_cases by name; `wide`: the cubic program on 65 columns (a leaf group of more than 64 words: every lane of the opening wave loops)"""
    if name == "wide":
        return dc.cubic_spec(field, N, seed=seed, w=65)
    return dc.SPECS[name](field, N, seed=seed)


def build_state(ctx, d, field, name, N=64, blowup=8, R=3, seed=1, stop=None):
    """deep_cases.build_proof up to the end of the commit phase: trace -> LDE -> ms_mix_air_ext -> ms_validity_commit -> ms_deep_compose -> FRI commit phase.
    `stop`: "compose" returns before ms_deep_compose, "begin" after ms_fri_begin alone (R > 1: the commit phase is under way)"""
    p, e = MODULUS[field], EXT[field]
    trace, cons, exempt, periodic, boundary = spec_of(name, field, N, 100 + seed)
    c = trace.shape[1]
    rng = SplitMix64(5000 + seed)
    P = dict(field=field, d=d, N=N, blowup=blowup, c=c, L=N * blowup, R=R, air=(cons, exempt, periodic, boundary))
    P["shift"] = rng.nonzero(p)
    dc.commit(ctx, trace, blowup, P["shift"])
    P["r"] = dc.full_ext(rng, field)
    assert ctx.mix_air_ext(P["r"], cons, exempt, periodic, boundary) == 0, ctx.last_error()
    P["m"] = m = e * dc.vl_of(ctx) // N
    assert ctx.validity_commit(m)[0] == 0, ctx.last_error()
    z = dc.full_ext(rng, field)
    rows = ms.air_rows(cons, boundary)
    P["zs"] = dc.shifted_points(field, z, ctx.root_of_unity(N), rows)
    P["lists"] = [list(range(c)) + (list(range(c, c + m)) if k == 0 else []) for k in range(len(rows))]
    P["gamma"] = dc.full_ext(rng, field)
    if stop == "compose":
        return P
    assert ctx.deep_compose(P["zs"], P["lists"], P["gamma"]) == 0, ctx.last_error()
    if stop == "begin":
        assert ctx.fri_begin(blowup, R)[0] == 0
        return P
    P["S"] = oc.commit_phase(ctx, field, blowup, R, seed=6000 + seed)
    P["D0"] = P["S"]["D0"]
    return P


def raw_linked(ctx, betas, nq, out, cap, want_len=True):
    """ms_query_linked with the arguments as given -> (rc, *len)"""
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.uint64)
    ln = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_query_linked(ctx.h, None if b is None else b.ctypes.data_as(_u64p), C.c_int(nq), out, C.c_size_t(cap), C.byref(ln) if want_len else None)
    return rc, ln.value


def by_definition(ctx, betas, D0, L):
    """header || ms_fri_query_index(betas) || ms_tree_open(LDE, rows) || ms_tree_open(VALIDITY, rows), with the rows of pyref_linked (and of pyref_deep: the rows
    msh_deep_link_verify expects)"""
    rows = rl.link_rows(betas, D0, L)
    assert rows == dc.rd.link_rows(betas, D0, L)
    return rl.mslq(ctx.fri_query_index(betas), ctx.tree_open(ms.TREE_LDE, rows), ctx.tree_open(ms.TREE_VALIDITY, rows))


def beta_sets(D0):
    """nq = 3 and nq = 1: equal betas, a beta equal to D_0, one above 2^63, positions whose partner wraps (b >= D_0 / 2) and does not"""
    return [[D0 // 2 + 1, D0, D0 // 2 + 1], [5 % D0, 2**63 + 12345, D0 - 1], [0], [D0], [2**64 - 1], [D0 // 2]]


# ---------------------------------------------------------------- 1. MSLQ equals its definition
def case_definition(make, d, field, name, R=3, N=64):
    ctx = ctx_of(make, d, field)
    P = build_state(ctx, d, field, name, N=N, R=R)
    D0, L = P["D0"], P["L"]
    assert L % D0 == 0 and D0 <= L
    if name == "constant":
        assert D0 == P["blowup"] < L                     # rows are positions scaled by L / D_0
    for betas in beta_sets(D0):
        want = by_definition(ctx, betas, D0, L)
        got = ctx.query_linked(betas)
        assert got == want
        sec = rl.split_mslq(got)
        assert sec is not None and (R > 1 or len(sec[0]) == 48 + 8 * EXT[field] * ctx.fri_round_info(0)[0])   # R = 1: no windows, header and final polynomial
        assert len(sec[1]) == 2 * len(betas) * dc.ro.path_size(1, P["c"], L) and len(sec[2]) == 2 * len(betas) * dc.ro.path_size(1, P["m"], L)
    if name in ("fib", "cubic") and R >= 3:               # the three sections are deep_cases.build_proof's, which the link verifier accepts
        other = ctx_of(make, d, field)
        Q = dc.build_proof(other, d, field, name, N=N, R=R)
        sec = rl.split_mslq(other.query_linked(Q["betas"]))
        assert sec == (Q["msfi"], Q["lde_open"], Q["val_open"])
        assert dc.link(Q, msfi=sec[0], lde_open=sec[1], val_open=sec[2]) == (1, "", "")


def case_virtual_column(make, d, field):
    """A linked state CAN contain a virtual linear LDE column: ms_mix needs no LDE, so the lincomb columns of open_cases.build_lde (c = 65) are still only hashed when
    ms_validity_commit, ms_deep_compose (which names none of them here) and the commit phase have run.  They open with the value that was hashed."""
    p, e = MODULUS[field], EXT[field]
    ctx = ctx_of(make, d, field)
    N, c = 16, 65
    root, L, lincombs = oc.build_lde(ctx, field, c, N=N)
    assert lincombs == 0                                 # the linear columns are virtual
    rng = SplitMix64(4242)
    assert ctx.mix(rng.nonzero(p)) == 0 and ctx.validity_commit(1)[0] == 0, ctx.last_error()
    zs = dc.shifted_points(field, dc.full_ext(rng, field), ctx.root_of_unity(N), [0, 1])
    assert ctx.deep_compose(zs, [[0, c], [0]], dc.full_ext(rng, field)) == 0, ctx.last_error()
    S = oc.commit_phase(ctx, field, 4, 3, seed=4243)
    betas = [3, S["D0"] - 1, 2**63 + 5]
    got = ctx.query_linked(betas)
    assert got == by_definition(ctx, betas, S["D0"], L)
    lde = ctx.lde_read()                                 # writes the virtual columns out: the opened rows are the rows of the matrix, under the LDE root
    rows = rl.link_rows(betas, S["D0"], L)
    nodes = dc.ro.tree_nodes(d, lde.reshape(-1, 1), 1, c)
    oc.check_paths(ctx, d, field, rl.split_mslq(got)[1], lde.reshape(-1, 1), 1, c, nodes, root, rows)
    assert ctx.query_linked(betas) == got                # ... and the same bytes from the stored columns


# ---------------------------------------------------------------- 2. one launch
def case_one_launch(make, d, field, R, nq):
    ctx = ctx_of(make, d, field)
    P = build_state(ctx, d, field, "fib", R=R)
    betas = [7, P["D0"] + 3, 2**40][:nq]
    blob, prof = oc.profile(ctx, lambda: ctx.query_linked(betas))
    launches = {k: v["launches"] for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    assert launches == {"merkle_path": 1}, launches
    assert blob == by_definition(ctx, betas, P["D0"], P["L"])


# ---------------------------------------------------------------- 3. refusals and invariance
def other_calls(ctx, betas, L):
    """what ms_fri_query, ms_fri_query_index and ms_tree_open return"""
    rows = [0, L - 1, 3]
    return [ctx.fri_query(betas), ctx.fri_query_index(betas), ctx.tree_open(ms.TREE_LDE, rows), ctx.tree_open(ms.TREE_VALIDITY, rows), ctx.tree_open(ms.TREE_FRI, [0, 1], 0)]


def case_refusals(make, d, field):
    N, blowup, R = 64, 8, 3
    betas = [7, 9]
    # states in which the call is refused
    ctx = ctx_of(make, d, field)
    assert raw_linked(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE                       # nothing at all
    build_state(ctx, d, field, "fib", R=R, stop="begin")
    assert raw_linked(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE and "commit phase" in ctx.last_error()   # the commit phase is under way
    ctx = ctx_of(make, d, field)
    build_state(ctx, d, field, "fib", R=R, stop="compose")
    oc.commit_phase(ctx, field, blowup, R, seed=6001)
    assert raw_linked(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE and "DEEP" in ctx.last_error()           # no ms_deep_compose
    without = other_calls(ctx, betas, N * blowup)
    assert raw_linked(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE and other_calls(ctx, betas, N * blowup) == without
    ctx = ctx_of(make, d, field)
    P = build_state(ctx, d, field, "fib", R=R)
    cons, exempt, periodic, boundary = P["air"]
    assert ctx.mix_air_ext(P["r"], cons, exempt, periodic, boundary) == 0               # a mix stage kills the validity tree
    assert raw_linked(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE
    # arguments and the size query, on a valid state; after each the other entry points give what they give on a context that never made the call
    ctx, fresh = ctx_of(make, d, field), ctx_of(make, d, field)
    P = build_state(ctx, d, field, "fib", R=R)
    build_state(fresh, d, field, "fib", R=R)
    L = P["L"]
    want_others = other_calls(fresh, betas, L)
    want = by_definition(fresh, betas, P["D0"], L)
    size = len(want)
    buf = (C.c_uint8 * (size + 8))(*([0xAB] * (size + 8)))
    untouched = bytes(buf)

    def unchanged():
        assert other_calls(ctx, betas, L) == want_others

    assert raw_linked(ctx, betas, 2, None, 0) == (0, size); unchanged()                             # the size query
    assert raw_linked(ctx, betas, 2, buf, size - 1) == (ms.ERR_ARG, size); unchanged()              # one byte short: *len set, nothing computed
    assert raw_linked(ctx, None, 2, buf, size)[0] == ms.ERR_ARG; unchanged()                        # null betas
    assert raw_linked(ctx, betas, 2, buf, size, want_len=False)[0] == ms.ERR_ARG; unchanged()       # null len
    assert raw_linked(ctx, betas, 2, None, size)[0] == ms.ERR_ARG; unchanged()                      # null out with a capacity
    assert raw_linked(ctx, betas, 0, buf, size)[0] == ms.ERR_ARG; unchanged()                       # nq outside 1..4096
    assert raw_linked(ctx, [7] * 4097, 4097, None, 0)[0] == ms.ERR_ARG
    assert raw_linked(ctx, [7] * 4096, 4096, None, 0)[0] == 0; unchanged()
    assert bytes(buf) == untouched
    assert ctx.L.ms_query_linked(None, None, C.c_int(1), None, C.c_size_t(0), None) == ms.ERR_ARG
    assert raw_linked(ctx, betas, 2, buf, size + 8) == (0, size)                                    # a larger buffer: the blob, and nothing behind it
    assert bytes(buf)[:size] == want and bytes(buf)[size:] == untouched[size:]
    unchanged()
    assert ctx.query_linked(betas) == want and ctx.query_linked(betas) == want                      # twice; between and behind the other calls
    unchanged()
    assert ctx.fri_proof_read() == want_others[0][1]                                                # the MSFP blob stays readable


def case_sharded(ctx):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the call, as ms_tree_open does"""
    from mini_stark_amd.dist import LocalShard
    sh = LocalShard(ctx, 4 << 20)
    dc.commit(ctx, dc.fib_spec(0, 64)[0], 4, 3)
    assert ctx.mix(5) == 0
    assert raw_linked(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE and "sharding" in ctx.last_error()
    sh.close()


# ================================================================ linked proofs: MSLP v1 and the drivers (include/ministark_host.h)
import struct   # noqa: E402

from mini_stark_amd import host as mh   # noqa: E402
from mini_stark_amd.stark import LinkedProof, Stark, StarkConfig, encode_air   # noqa: E402

SECURITY_BITS, BLOWUP = 20, 8
HEAD = struct.calcsize(rl.MSLP_HEAD)


def handle(ctx, N, w, gb=0):
    """the msh_stark handle and the Python configuration of one statement shape: steps = N - 1, so the configuration's own rounds end at a domain of two points"""
    return mh.HostStark(ctx, SECURITY_BITS, BLOWUP, N - 1, w, gb), StarkConfig(ctx, SECURITY_BITS, BLOWUP, N - 1, w, gb)


def prove(make, d, field, name, N=8, R=3, gb=0, seed=1):
    """one linked proof by the C++ driver: a dict with everything the verifying sides are given"""
    ctx = ctx_of(make, d, field)
    trace, cons, exempt, periodic, boundary = spec_of(name, field, N, 100 + seed)
    w = trace.shape[1]
    hs, cfg = handle(ctx, N, w, gb)
    air = (cons, exempt, periodic, boundary)
    rc = hs.prove_linked(trace, air, R)
    assert rc == 0, (rc, ctx.last_error())
    Rr = R or hs.rounds
    return dict(ctx=ctx, hs=hs, cfg=cfg, d=d, field=field, N=N, w=w, R=R, Rr=Rr, gb=gb, nq=hs.fri_queries, air=air, trace=trace, data=hs.linked_proof())


def verdicts(P, data=None, air=None, N=None, R=None, hs=None, gb=None, nq=None):
    """(the host library's rc and why, pyref_linked's verdict and step) - which must agree: the same verdict, and `why` beginning as the step's prefix"""
    data = P["data"] if data is None else data
    air, N, hs = air or P["air"], N or P["N"], hs or P["hs"]
    R = P["R"] if R is None else R
    rc, why = hs.verify_linked(data, air, N, P["w"], R)
    ok, step = rl.verify(P["field"], P["d"], True, N, P["w"], BLOWUP, R or hs.rounds, P["nq"] if nq is None else nq, P["gb"] if gb is None else gb, air, data)
    assert rc in (0, 1) and (rc == 1) == ok, (rc, why, step)
    assert (why == "" and step == "") if ok else why.startswith(rl.PREFIX[step]), (why, step)
    return rc, why, step


def rejected(P, data=None, steps=None, **over):
    rc, why, step = verdicts(P, data, **over)
    assert rc == 0 and (steps is None or step in steps), (why, step, steps)
    return step


# ---------------------------------------------------------------- 4. end to end
def case_end_to_end(make, d, field, name, N=8, R=3, gb=0):
    P = prove(make, d, field, name, N=N, R=R, gb=gb)
    data = P["data"]
    assert verdicts(P) == (1, "", "")
    # the Python driver writes the same bytes; the format round-trips
    lp = Stark(P["cfg"]).prove_air(P["trace"], P["air"], R)
    assert lp.to_bytes() == data
    back = LinkedProof.from_bytes(data)
    assert back == lp and back.to_bytes() == data
    h = rl.parse_mslp(data)
    assert h is not None and (h["R"], h["nq"], h["gb"], h["N"], h["c"]) == (P["Rr"], P["nq"], gb, N, P["w"])
    assert rl.split_mslq(h["mslq"]) is not None
    st = Stark(P["cfg"])
    assert st.verify_air(data, P["air"], N, P["w"], R) is True and st.verify_air(lp, P["air"], N, P["w"], R) is True
    assert st.verify_air(data[:-1], P["air"], N, P["w"], R) is False and st.last_verify_error.startswith("header: ")
    # a second proof on the same handle replaces the slot; msh_stark_prove's slots are not touched by either
    assert P["hs"].prove_linked(P["trace"], P["air"], R) == 0 and P["hs"].linked_proof() == data


def case_redraw_rule(field):
    """THE REDRAW OF shift.  A seed whose first drawn shift is redrawn was NOT searched for: at N = 8, blowup 8 a draw is redrawn with probability 2^-25, and a try costs a
    trace tree and a transcript in plain Python (a millisecond at best), so a second of search covers a few hundred of the 2^25 tries it takes.  The rule is tested with
    a FORCED first draw instead: the predicate both C++ sides loop on (msh_linked_shift_ok / msh_linked_z_ok) against pyref_linked's, and pyref_linked's replay."""
    p, e = MODULUS[field], EXT[field]
    L = 64
    gL = dc.pyref.root_of_unity(field, L)
    inside = [1, gL, pow(gL, 3, p), p - 1, pow(gL, L - 1, p)]              # shift^L == 1: the coset would be the subgroup itself
    outside = [2, 3, pow(dc.pyref.root_of_unity(field, 2 * L), 1, p), p - 2]
    for s in [0] + inside:
        assert not mh.linked_shift_ok(field, L, s) and not rl.shift_ok(p, L, s)
    for s in outside:
        assert mh.linked_shift_ok(field, L, s) and rl.shift_ok(p, L, s)
    for z in ([5] + [0] * (e - 1), [0] * e):
        assert not mh.linked_z_ok(field, z) and not rl.z_ok(z)
    for z in ([5] + [0] * (e - 2) + [1], [0, 7] + [0] * (e - 2)):
        assert mh.linked_z_ok(field, z) and rl.z_ok(z)
    free, forced = rl.Transcript(rl.DOMSEP, SHA), rl.Transcript(rl.DOMSEP, SHA, forced_shifts=[inside[2], 0])
    first = free.draw_shift(p, L)
    assert first[1] == 1
    second, third = free.draw_shift(p, L)[0], free.draw_shift(p, L)[0]
    assert forced.draw_shift(p, L) == (third, 3) and forced.state == free.state   # two forced draws are refused, the third - the chain's own - stands


def case_redraw_in_the_verdict(make, field):
    """a verifier whose first draw is refused goes on to the second: the proof, made from the first, is then rejected (the redraw is in the replay)"""
    P = prove(make, SHA, field, "fib")
    gL = dc.pyref.root_of_unity(field, P["N"] * BLOWUP)
    args = (field, SHA, True, P["N"], P["w"], BLOWUP, P["Rr"], P["nq"], 0, P["air"], P["data"])
    assert rl.verify(*args) == (True, "")
    ok, step = rl.verify(*args, forced_shifts=[gL])
    assert not ok and step in ("air", "lde", "link")


# ---------------------------------------------------------------- 5. rejections
def flip(data, at, mask=1):
    return data[:at] + bytes([data[at] ^ mask]) + data[at + 1:]


def put_u64(data, at, v):
    return data[:at] + struct.pack("<Q", v) + data[at + 8:]


def case_rejections(make, d, field, gb=4):
    p, e = MODULUS[field], EXT[field]
    P = prove(make, d, field, "fib", N=8, R=3, gb=gb)
    data, w, N, R = P["data"], P["w"], P["N"], P["Rr"]
    assert verdicts(P) == (1, "", "")
    m, rows, lists, ne, la = rl.shape(field, N, w, BLOWUP, R, gb, P["air"])
    assert len(rows) >= 2
    a0 = HEAD                                                                # arthur
    ev0 = a0 + 96
    fri0 = ev0 + ne * e * 8
    fields = {"trace root": a0 + 5, "LDE root": a0 + 32 + 5, "validity root": a0 + 64 + 5, "evaluation at the first point": ev0, "a chunk's evaluation": ev0 + w * e * 8,
              "evaluation at a later point": ev0 + (w + m) * e * 8, "round 0's root": fri0 + 7, "a B": fri0 + 32, "a round root": fri0 + 32 + 2 * e * 8 + 9,
              "the nonce": a0 + la - 8}
    seen = set()
    for what, at in fields.items():
        seen.add(rejected(P, flip(data, at)))
    assert seen <= {"pow", "air", "fri", "lde", "validity", "link"} and len(seen) >= 2, seen
    # a non-canonical limb: in the claimed evaluations, and in an opened row
    rejected(P, put_u64(data, ev0, p), steps=("transcript",))
    rejected(P, put_u64(data, fri0 + 32, p), steps=("transcript", "pow"))
    q0 = a0 + la                                                             # MSLQ
    l_msfi, l_lde, l_val = struct.unpack_from("<3Q", data, q0 + 8)
    s_msfi, s_lde, s_val = q0 + 32, q0 + 32 + l_msfi, q0 + 32 + l_msfi + l_lde
    rejected(P, put_u64(data, s_lde + 8, p), steps=("lde",))
    # one byte changed in each MSLQ section
    nfinal = struct.unpack_from("<Q", data, s_msfi + 40)[0]
    rejected(P, flip(data, s_msfi + 48), steps=("fri",))                     # the final polynomial
    rejected(P, flip(data, s_msfi + 48 + nfinal * e * 8 + 8), steps=("fri",))   # a value window 0 opened
    rejected(P, flip(data, s_lde + 8), steps=("lde",))
    rejected(P, flip(data, s_val + 8), steps=("validity",))
    rejected(P, flip(data, s_val + l_val - 1), steps=("validity",))
    # the section lengths of the MSLQ header
    rejected(P, put_u64(data, q0 + 24, l_val + 8), steps=("header",))
    rejected(P, put_u64(put_u64(data, q0 + 8, l_msfi + 8), q0 + 16, l_lde - 8), steps=("fri",))      # the sum fits: the sections are cut elsewhere
    rejected(P, put_u64(put_u64(data, q0 + 16, l_lde + 8), q0 + 24, l_val - 8), steps=("lde", "validity"))
    rejected(P, flip(data, q0), steps=("header",))                           # the MSLQ magic
    # every MSLP header field
    for k in range(9):
        rejected(P, flip(data, 4 * k), steps=("header",))
    for k in range(4):
        rejected(P, flip(data, 36 + 8 * k), steps=("header",))
    # truncation by one byte and by one path; trailing bytes - as they are, and with both length words made to fit
    rejected(P, data[:-1], steps=("header",))
    rejected(P, data + bytes(8), steps=("header",))
    pv = dc.ro.path_size(1, m, N * BLOWUP)
    lq = len(data) - q0

    def refit(blob, dv):
        return put_u64(put_u64(blob, q0 + 24, l_val + dv), 36 + 24, lq + dv)
    rejected(P, data[:-pv], steps=("header",))
    rejected(P, refit(data[:-pv], -pv), steps=("validity",))
    rejected(P, refit(data + bytes(8), 8), steps=("validity",))
    rejected(P, data[:HEAD - 1], steps=("header",))
    rejected(P, b"", steps=("header",))
    # another proof's MSLQ: deep_cases.case_splice through the driver
    B = prove(make, d, field, "fib", N=8, R=3, gb=gb, seed=2)
    assert len(B["data"]) == len(data) and B["data"] != data and verdicts(B) == (1, "", "")
    spliced = B["data"][:q0] + data[q0:]
    rejected(B, spliced, steps=("fri",))
    # statement binding: the same proof against a program that differs in one coefficient, in one boundary value
    cons, exempt, periodic, boundary = P["air"]
    cons2 = [list(t) for t in cons]; cons2[0][0] = (2, cons2[0][0][1])
    bnd2 = list(boundary); bnd2[0] = (bnd2[0][0], bnd2[0][1], (bnd2[0][2] + 1) % p)
    rejected(P, air=(cons2, exempt, periodic, boundary), steps=("pow", "air"))
    rejected(P, air=(cons, exempt, periodic, bnd2), steps=("pow", "air"))
    # another fri_rounds, another grinding setting, another N
    rejected(P, R=R + 1, steps=("header",))
    other, _cfg = handle(P["ctx"], N, w, 0 if gb else 4)
    rejected(P, hs=other, gb=other.grinding_bits, nq=other.fri_queries, steps=("header",))
    rejected(P, N=2 * N, steps=("header",))


def apply_edits(base, cut, append, edits):
    """`base` cut to `cut` bytes, `append` zero bytes behind it, then every (offset, bytes) of `edits` written over it"""
    out = bytearray(base[:cut] + bytes(append))
    for at, new in edits:
        out[at:at + len(new)] = new
    return bytes(out)


def tampered_edits(P):
    """[(name, cut, append, edits)]: the truncated and tampered copies of the v1 proof P["data"], as edits of it (apply_edits)"""
    data, field = P["data"], P["field"]
    m, rows, lists, ne, la = rl.shape(field, P["N"], P["w"], BLOWUP, P["Rr"], P["gb"], P["air"])
    q0, n = HEAD + la, len(data)
    l_msfi, l_lde, l_val = struct.unpack_from("<3Q", data, q0 + 8)
    out = [("whole", n, 0, [])]
    out += [("cut to %d" % k, k, 0, []) for k in (0, 1, HEAD - 1, HEAD, HEAD + 40, q0 - 1, q0, q0 + 31, q0 + 32, q0 + 79, q0 + 32 + l_msfi - 8, q0 + 32 + l_msfi, q0 + 32 + l_msfi + 24,
                                                  n - l_val, n - l_val + 16, n - 64, n - 1)]
    out += [("trailing", n, 8, [])]
    out += [("flip %d" % at, n, 0, [(at, bytes([data[at] ^ 0x80]))]) for at in list(range(0, HEAD)) + list(range(q0, q0 + 32 + 48)) + list(range(q0 + 32 + l_msfi, q0 + 32 + l_msfi + 40)) +
            list(range(q0 + 32 + l_msfi + l_lde, q0 + 32 + l_msfi + l_lde + 40)) + list(range(HEAD, q0, 37))]
    big = 2**64 - 1
    for at in (36 + 16, 36 + 24, q0 + 8, q0 + 16, q0 + 24):                   # length words: huge, and off by 8 either way
        for v in (big, big - 7, 2**63, struct.unpack_from("<Q", data, at)[0] + 8, struct.unpack_from("<Q", data, at)[0] - 8):
            out.append(("len@%d=%d" % (at, v), n, 0, [(at, struct.pack("<Q", v))]))
    nlev_lde = q0 + 32 + l_msfi + 8 + P["w"] * 8
    nlev_fri = q0 + 32 + 48 + struct.unpack_from("<Q", data, q0 + 32 + 40)[0] * EXT[field] * 8 + 8 + 2 * EXT[field] * 8
    for at in (nlev_lde, nlev_fri):
        for v in (big, 65, 64, 63, 0):
            out.append(("nlevels@%d=%d" % (at, v), n, 0, [(at, struct.pack("<Q", v))]))
    return out


def tampered_fixture(make, field=0):
    """(the proof's dict, [(name, cut, append, edits, rc, the beginning of why)]): truncated and tampered copies of one proof, as edits of it (apply_edits), with the
    verdict msh_stark_verify_linked gives for each - what the sanitizer program (tests/asan) is fed"""
    P = prove(make, SHA, field, "fib", N=8, R=3, gb=4)
    cases = []
    for name, cut, append, edits in tampered_edits(P):
        rc, why = P["hs"].verify_linked(apply_edits(P["data"], cut, append, edits), P["air"], 8, P["w"], 3)
        cases.append((name, cut, append, edits, rc, why.split(":")[0]))
    return P, cases


def fixture_bytes(make):
    """tests/golden/linked_tampered.bin (layout: tests/golden/gen_linked_tampered.py): the statement, the proof, and per case the edits, the verdict and the step"""
    P, cases = tampered_fixture(make)
    blob = lambda b: struct.pack("<I", len(b)) + b   # noqa: E731
    out = b"MSLF" + struct.pack("<10I", 1, P["field"], P["d"], SECURITY_BITS, BLOWUP, P["N"] - 1, P["w"], P["gb"], P["N"], P["R"]) + blob(mh.air_encode(P["air"]))
    out += blob(P["data"]) + struct.pack("<I", len(cases))
    for name, cut, append, edits, rc, step in cases:
        out += blob(name.encode()) + struct.pack("<3I", cut, append, len(edits)) + b"".join(struct.pack("<I", at) + blob(new) for at, new in edits)
        out += struct.pack("<i", rc) + blob(step.encode())
    return out, cases


# ---------------------------------------------------------------- 6. a false trace
def case_false_trace(make, d, field):
    ctx = ctx_of(make, d, field)
    trace, cons, exempt, periodic, boundary = spec_of("fib", field, 8, 101)
    air = (cons, exempt, periodic, boundary)
    hs, _cfg = handle(ctx, 8, 2)
    bad = trace.copy()
    bad[3, 1] = (int(bad[3, 1]) + 1) % MODULUS[field]
    assert hs.prove_linked(bad, air, 3) == ms.ERR_SHAPE
    assert hs.linked_proof() == b""
    assert hs.prove_linked(trace, air, 3) == 0
    assert hs.verify_linked(hs.linked_proof(), air, 8, 2, 3) == (1, "")
    assert hs.prove_linked(bad, air, 3) == ms.ERR_SHAPE and hs.linked_proof() == b""   # a failed proof leaves no stale bytes behind


# ---------------------------------------------------------------- 7. msh_air_encode / msh_air_rows
def periodic_program(field):
    """a program with two periodic columns and three distinct exemption sets (encoded and listed only: no trace has to satisfy it)"""
    p = MODULUS[field]
    cons = [[(1, [(0, 1)]), (p - 1, [(0, 0), (ms.AIR_PERIODIC | 0, 0)]), (p - 2, [(ms.AIR_PERIODIC | 1, 3)])],
            [(3, [(1, 2), (0, 0), (1, 0)]), (5, [])],
            [(7, [(1, 1)])]]
    return cons, [[7], [6, 7], [0, 5, 7]], [[1, 2], [3, 4, 5, 6]], [(0, 0, 9), (1, 7, 11), (1, 0, 13)]


def case_air_encoding(field):
    p = MODULUS[field]
    programs = [spec_of(name, field, 8, 101)[1:] for name in ("fib", "cubic", "constant")] + [periodic_program(field)]
    for air in programs:
        cons, exempt, periodic, boundary = air
        want = rl.encode_air(*air)
        assert mh.air_encode(air) == want == encode_air(air) and len(want) == 40 + struct.unpack_from("<I", want, 36)[0]
        assert mh.air_rows_native(air) == ms.air_rows(cons, boundary) == rl.air_rows(cons, boundary)
        flat = ms.flatten_air(*air)
        for name in ("coef", "fac_poly", "fac_row", "ex_row", "per_val", "bnd_poly", "bnd_row", "bnd_val"):   # every entry of every value array
            for k in range(len(flat[name])):
                other = dict(flat); other[name] = flat[name].copy(); other[name][k] += 1
                assert mh.air_encode(other) not in (want, b""), (name, k)
                assert encode_air(other) == mh.air_encode(other)
    # the offset arrays: programs with the same value arrays that are cut elsewhere
    cons, exempt, periodic, boundary = periodic_program(field)
    t = cons[0] + cons[1]
    a = ([t[:3], t[3:], cons[2]], exempt, periodic, boundary)
    b = ([t[:2], t[2:], cons[2]], exempt, periodic, boundary)                                            # term_begin
    c = ([[(1, [(0, 1), (0, 0)]), (2, [(1, 0)])]], [[7]], (), ())
    dd = ([[(1, [(0, 1)]), (2, [(0, 0), (1, 0)])]], [[7]], (), ())                                        # fac_begin
    f = (cons, [[7, 6], [7], [0, 5, 7]], periodic, boundary)                                             # ex_begin
    g = (cons, exempt, [[1, 2, 3, 4], [5, 6]], boundary)                                                 # per_begin
    for x, y in ((a, b), (c, dd), ((cons, exempt, periodic, boundary), f), ((cons, exempt, periodic, boundary), g)):
        ex, ey = mh.air_encode(x), mh.air_encode(y)
        assert ex and ey and ex != ey and len(ex) == len(ey) and ex == rl.encode_air(*x) and ey == rl.encode_air(*y)
    # a malformed program: refused, not read
    flat = ms.flatten_air(*programs[0])
    for name in ("term_begin", "coef", "fac_begin", "ex_begin"):
        assert mh.air_encode(dict(flat, **{name: None})) == b""
    assert mh.air_encode(dict(flat, ncons=0)) == b"" and mh.air_encode(dict(flat, ncons=4097)) == b""
