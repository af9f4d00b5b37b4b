"""GPU: the uncompressed-point decoders of the pairing calls held to tests/wire_model.py on the whole table of
tests/wire_cases.py, through every route that reaches one, and the Miller kernel's handling of bad and skipped pairs at the edges
of its lane layout.

Verdicts are known BY CONSTRUCTION, as in tests/test_gpu_bls_verify.py: for pairs (a_i G1, b_i G2) the product of pairings is 1
iff sum a_i b_i == 0 (mod r).  No pairing is computed in Python.  A crafted encoding takes the slot of the table's base point
(11 G1 or 5 G2) in a group built around that scalar, so each class of the model has one verdict:

  same      (the canonical bytes, bit 5 on the leading element)   the verdict of the group as built
  infinity  (every spelling with bit 6 of byte 0)                 the verdict the canonical 0x40 00.. gives in that slot
  bad                                                             PE_BLS_BAD_POINT = 2 for that group, and no other group moves

The decoding kernels, read from the engine code:
  pe_pairing_check, pe_profile_pairing_gt     pairing_run -> k_bls_prepare (its own written-out copy of the decode)
  pe_fast_aggregate_verify                    pe_g1_sum for the key, then verify_pairs_run -> pairing_run -> k_bls_prepare
  pe_batch_verify                             k_bls_batch_settle (wire_load_g1 / wire_load_g2 of wire_points.h) for all three
                                              points; the groups of a failing chunk again through verify_pairs_run -> k_bls_prepare
  pe_batch_fast_aggregate_verify              pe_g1_sum for the key, then as pe_batch_verify
  pe_verify_signatures (message point)        verify_pairs_run -> k_bls_prepare, for the combined check and for the locate pass
  pe_verify_resident (message point)          k_bls_resident_prepare (wire_load_g2): tests/test_gpu_verify_resident.py
  pe_g1_sum, pe_g2_sum                        k_g1_convert, k_g2_convert: no check at all, flags masked (pinned at the end)

How these tests fail, from the decoders' code.  fp_to_mont is a Montgomery product with R^2 < p, so any 384-bit input leaves it
fully reduced: v + k p becomes the Montgomery form of v and passes the curve equation.  fp_is_canonical is therefore the ONLY
thing between the `plus_p` / `plus_kp_max` cases (and `zero_on_curve`) and verdict 1; every other bad case is also off the curve.
  k_bls_prepare without fp_is_canonical(x) in its G1 half: g1:x:plus_p, g1:x:plus_kp_max turn from 2 to the group's own verdict
    in pairing_check[g1] (and g1:point:zero_on_curve to 0 or 1); without (y): g1:y:plus_p, g1:y:plus_kp_max.  In its G2 half,
    without (x): g2:x.c1 and g2:x.c0 (one lane each), :plus_p and :plus_kp_max, in pairing_check[g2],
    fast_aggregate_verify[msg, sig] and verify_signatures; without (y): the same four of g2:y.c1 and g2:y.c0.
  wire_load_g1 / wire_load_g2 (k_bls_batch_settle): the same cases in batch_verify[pk | msg, sig] at chunk 1 -- the group stays
    live, its chunk of one is valid and nothing looks at it again -- and in batch_fast_aggregate_verify[msg, sig].
  wire_load_g2 (k_bls_resident_prepare): the same G2 cases in test_gpu_verify_resident's test_every_wire_case_on_the_message_point.
  The top limb: were role 0's x.c0 or any y left masked, :bit7 / :bit6 / :bit5 of that element would decode to the base point
    (2 -> 1); were x.c1 read in full, g2:x.c1:bit5 would be >= p (1 -> 2) and the GT bytes test would fail with it.
  k_bls_miller: a scan that stopped after its first round would miss the bad pair at index 6, 11 and 12 (2 -> 1 or 0); a flag
    not ORed across the row would lose the pairs whose lane pair is not the row's first (index 5, 11); a skipped pair whose line
    were not set to 1 in a later round would move `without_inf_*` from 1 to 0."""
import numpy as np
import pytest

from oracle import g1, g2
from oracle.g1 import R_ORDER as R
from tests import wire_cases as wc
from tests import wire_model as wm

pytestmark = pytest.mark.gpu
K1, K2 = wc.BASE_K["g1"], wc.BASE_K["g2"]
FULL = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R
VERIFY_VERDICT = {wc.SAME: 1, wm.INFINITY: 0, wm.BAD: 2}      # a group (key, message, signature) valid as built
CASES_PER_CALL = 16
INF1, INF2 = g1.to_bytes96(None), g2.to_bytes192(None)


def _inv(v):
    return pow(v, -1, R)


def _p1(k):
    return g1.to_bytes96(g1.mul(k % R, g1.G) if k % R else None)


def _p2(k):
    return g2.to_bytes192(g2.mul(k % R, g2.G2) if k % R else None)


def _rows(blobs, width):
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(-1, width).copy()


def _chunks(seq, n=CASES_PER_CALL):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


@pytest.fixture(scope="module")
def engine(engine_factory):
    return engine_factory(device=0)


# ------------------------------------------------------------------ pe_pairing_check: the G1 and the G2 side
@pytest.fixture(scope="module")
def pair_groups():
    """Per side the two groups a case is put into, as (G1 bytes, G2 bytes, slot of the crafted point, {class: verdict}), and
    the neighbours.  A: two pairs whose whole sum is 0 (crafted in slot 0).  B: three pairs, the crafted one in the middle and
    the OTHER two summing to 0 -- so an infinity and the point itself give opposite verdicts in A and in B."""
    a1, b0, a0, a2 = FULL, 0x1F2E3D4C5B6A79881122334455667788, R - 1, 0x0123456789ABCDEF0FEDCBA987654321
    out = {}
    # G1 side: the crafted point is K1 G1, paired with b0 G2
    q0 = _p2(b0)
    out["g1"] = [
        ([None, _p1(a1)], [q0, _p2(-K1 * b0 * _inv(a1))], 0, {wc.SAME: 1, wm.INFINITY: 0, wm.BAD: 2}),
        ([_p1(a0), None, _p1(a2)], [_p2(b0 + 1), q0, _p2(-a0 * (b0 + 1) * _inv(a2))], 1, {wc.SAME: 0, wm.INFINITY: 1, wm.BAD: 2}),
    ]
    # G2 side: the crafted point is K2 G2, paired with a0 G1
    p0 = _p1(a0)
    out["g2"] = [
        ([p0, _p1(-a0 * K2 * _inv(b0))], [None, q0], 0, {wc.SAME: 1, wm.INFINITY: 0, wm.BAD: 2}),
        ([_p1(a1), p0, _p1(a2)], [q0, None, _p2(-a1 * b0 * _inv(a2))], 1, {wc.SAME: 0, wm.INFINITY: 1, wm.BAD: 2}),
    ]
    out["valid"] = ([_p1(3), _p1(R - 1)], [_p2(7), _p2(21)], 1)
    out["invalid"] = ([_p1(3), _p1(R - 1)], [_p2(7), _p2(22)], 0)
    return out


def _fill(group, side, enc):
    pts1, pts2, slot, _ = group
    pts1, pts2 = list(pts1), list(pts2)
    (pts1 if side == "g1" else pts2)[slot] = enc
    return pts1, pts2


def _pairing_args(groups):
    a = _rows([p for g in groups for p in g[0]], 96)
    b = _rows([q for g in groups for q in g[1]], 192)
    return a, b, np.cumsum([0] + [len(g[0]) for g in groups]).astype(np.uint32)


@pytest.mark.parametrize("side", ("g1", "g2"))
def test_pairing_check_decodes_every_case(engine, pair_groups, side):
    """k_bls_prepare.  Every case in both groups of its side, a valid or an invalid neighbour after each case."""
    for part in _chunks(wc.cases(side)):
        groups, want, names = [pair_groups["valid"]], [1], ["neighbour"]
        for i, c in enumerate(part):
            for grp in pair_groups[side]:
                groups.append(_fill(grp, side, c.enc))
                want.append(grp[3][c.expect])
                names.append(c.name)
            nb = pair_groups["invalid" if i & 1 else "valid"]
            groups.append(nb)
            want.append(nb[2])
            names.append("neighbour")
        got = engine.pairing_check(*_pairing_args(groups)).tolist()
        print(list(zip(names, got, want)))
        assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]


@pytest.mark.parametrize("side", ("g1", "g2"))
def test_ignored_bits_and_infinity_spellings_give_the_same_gt_bytes(engine, pair_groups, side):
    """pe_profile_pairing_gt: bit 5 on the leading element changes none of the 576 bytes the verdict compares with 1, and every
    spelling of infinity gives the bytes of 0x40 00..  (a masked bit that leaked into x would move every byte)."""
    table = [c for c in wc.cases(side) if c.expect != wm.BAD]
    assert {c.edge for c in table} >= {"bit5", "bit6", "inf_c0", "inf_60", "inf_40_nonzero"}
    ref = {wc.SAME: wc.case(side + ":point:canonical"), wm.INFINITY: wc.case(side + ":point:inf_canonical")}
    for grp in pair_groups[side]:
        groups = [_fill(grp, side, c.enc) for c in table] + [_fill(grp, side, ref[k].enc) for k in (wc.SAME, wm.INFINITY)]
        gt = engine._profile_pairing_gt(*_pairing_args(groups))
        want = {wc.SAME: gt[len(table)].tobytes(), wm.INFINITY: gt[len(table) + 1].tobytes()}
        assert want[wc.SAME] != want[wm.INFINITY]
        one = (1).to_bytes(48, "big") + bytes(528)
        assert (want[wc.SAME] == one) == (grp[3][wc.SAME] == 1) and (want[wm.INFINITY] == one) == (grp[3][wm.INFINITY] == 1)
        for c, row in zip(table, gt):
            assert row.tobytes() == want[c.expect], c.name


# ------------------------------------------------------------------ the verify calls: groups (key, message, signature)
SK = [(0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R for i in range(8)]
CRAFTED_SIGNERS, NEIGHBOUR_SIGNERS = [0, 1, 2], [3, 4]
H_NEIGHBOUR = 7


def _triple(field, key_scalar):
    """(key bytes or None, message, signature) of a valid group with `None` where the crafted point goes: the key K1 G1, the
    message 5 G2 or the signature 5 G2, the other two chosen so that key * message == signature in the exponent."""
    if field == "pk":
        return None, _p2(FULL), _p2(K1 * FULL)
    if field == "msg":
        return _p1(key_scalar), None, _p2(key_scalar * K2)
    return _p1(key_scalar), _p2(K2 * _inv(key_scalar)), None


def _neighbours(key_scalar):
    pk, msg = _p1(key_scalar), _p2(H_NEIGHBOUR)
    return (pk, msg, _p2(key_scalar * H_NEIGHBOUR), 1), (pk, msg, _p2(key_scalar * H_NEIGHBOUR + 1), 0)


def _layout(part, triple, field, valid, invalid):
    """[V, case, V, case, I, case, V, ...]: a valid group on both sides of most cases, an invalid one after every second."""
    slot = {"pk": 0, "msg": 1, "sig": 2}[field]
    groups, want, names = [valid[:3]], [1], ["neighbour"]
    for i, c in enumerate(part):
        t = list(triple)
        t[slot] = c.enc
        groups.append(tuple(t))
        want.append(VERIFY_VERDICT[c.expect])
        names.append(c.name)
        nb = invalid if i & 1 else valid
        groups.append(nb[:3])
        want.append(nb[3])
        names.append("neighbour")
    return groups, want, names


def _scalars(n):
    rng = np.random.default_rng(n)
    return np.array([int(v) | 1 for v in rng.integers(1, 1 << 63, size=n, dtype=np.uint64)], dtype=np.uint64)


def _assert(got, want, names):
    print(list(zip(names, got, want)))
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]


@pytest.mark.parametrize("chunk", (1, None))
@pytest.mark.parametrize("field", ("pk", "msg", "sig"))
def test_batch_verify_decodes_every_case(engine_factory, field, chunk):
    """k_bls_batch_settle (wire_load_g1 for the key, wire_load_g2 for message and signature) settles the crafted group before
    the batch; the invalid neighbours fail the top-level product, so the engine's search (chunk verdicts, then
    verify_pairs_run -> k_bls_prepare on the ORIGINAL bytes of the failing chunks' groups) runs over neighbours of bad groups and
    over the `same` cases: one group to a chunk, and the default chunk."""
    e = engine_factory(device=0)
    if chunk:
        e._profile_batch_set_chunk(chunk)
    a = 0x6F2A9D1C33
    triple = _triple(field, a)
    valid, invalid = _neighbours(a + 1)
    for part in _chunks(wc.cases("g1" if field == "pk" else "g2")):
        groups, want, names = _layout(part, triple, field, valid, invalid)
        pk, msg, sig = (_rows([g[i] for g in groups], w) for i, w in ((0, 96), (1, 192), (2, 192)))
        got = e.batch_verify(pk, msg, sig, _scalars(len(groups))).tolist()
        stats = e._profile_batch_stats()
        _assert(got, want, names)
        assert stats["live"] == want.count(1) + sum(1 for n, w in zip(names, want) if n == "neighbour" and w == 0)
        if 0 in [w for n, w in zip(names, want) if n == "neighbour"]:
            assert stats["fallback_exps"] == stats["chunks"] and stats["rechecked"] >= 1
        if chunk:
            assert stats["c"] == 1 and stats["chunks"] == stats["live"]


@pytest.fixture(scope="module")
def registry(engine_factory):
    e = engine_factory(device=0)
    keys = _rows([_p1(k) for k in SK], 96)
    e.set_validators(np.full(len(SK), 32 * 10 ** 9, dtype=np.uint64), np.ones(len(SK), dtype=np.uint8), keys)
    return e


def _indexed(part, field):
    s, s_nb = sum(SK[i] for i in CRAFTED_SIGNERS) % R, sum(SK[i] for i in NEIGHBOUR_SIGNERS) % R
    valid, invalid = _neighbours(s_nb)
    groups, want, names = _layout(part, _triple(field, s), field, valid, invalid)
    members = [NEIGHBOUR_SIGNERS if n == "neighbour" else CRAFTED_SIGNERS for n in names]
    index = np.array([i for m in members for i in m], dtype=np.uint32)
    off = np.cumsum([0] + [len(m) for m in members]).astype(np.uint32)
    return index, off, _rows([g[1] for g in groups], 192), _rows([g[2] for g in groups], 192), want, names


@pytest.mark.parametrize("field", ("msg", "sig"))
def test_fast_aggregate_verify_decodes_every_case(registry, field):
    """k_bls_prepare, through verify_pairs_run: pair 2g = (the summed key, message), pair 2g + 1 = (-g1, signature)."""
    for part in _chunks(wc.cases("g2")):
        index, off, msgs, sigs, want, names = _indexed(part, field)
        _assert(registry.fast_aggregate_verify(index, off, msgs, sigs).tolist(), want, names)


@pytest.mark.parametrize("field", ("msg", "sig"))
def test_batch_fast_aggregate_verify_decodes_every_case(registry, field):
    """k_bls_batch_settle, then k_bls_prepare for the groups of the chunks the invalid neighbours fail."""
    for part in _chunks(wc.cases("g2")):
        index, off, msgs, sigs, want, names = _indexed(part, field)
        _assert(registry.batch_fast_aggregate_verify(index, off, msgs, sigs, _scalars(len(want))).tolist(), want, names)
        assert registry._profile_batch_stats()["rechecked"] >= 1


def test_verify_signatures_decodes_every_message_point(registry):
    """k_bls_prepare, through verify_pairs_run, twice: the combined check of every group, and the locate pass over the members
    of the groups that failed it (the invalid neighbours; their message points are read again beside the crafted ones)."""
    crafted = [g2.compress(g2.mul(SK[v] * K2 % R, g2.G2)) for v in CRAFTED_SIGNERS]
    good = [g2.compress(g2.mul(SK[v] * H_NEIGHBOUR % R, g2.G2)) for v in NEIGHBOUR_SIGNERS]
    spoilt = [good[0], g2.compress(g2.mul((SK[NEIGHBOUR_SIGNERS[1]] * H_NEIGHBOUR + 1) % R, g2.G2))]
    h_nb = _p2(H_NEIGHBOUR)
    for part in _chunks(wc.cases("g2")):
        sigs, signer, off, msgs, want_g, want_m, names = [], [], [0], [], [], [], []

        def group(who, blobs, msg, verdict, members, name):
            sigs.extend(blobs)
            signer.extend(who)
            off.append(len(signer))
            msgs.append(msg)
            want_g.append(verdict)
            want_m.append(members)
            names.append(name)

        group(NEIGHBOUR_SIGNERS, good, h_nb, 1, [1, 1], "neighbour")
        for i, c in enumerate(part):
            v = VERIFY_VERDICT[c.expect]
            group(CRAFTED_SIGNERS, crafted, c.enc, v, [1, 1, 1] if v == 1 else [0, 0, 0], c.name)
            if i & 1:
                group(NEIGHBOUR_SIGNERS, spoilt, h_nb, 0, [1, 0], "neighbour")
            else:
                group(NEIGHBOUR_SIGNERS, good, h_nb, 1, [1, 1], "neighbour")
        n = len(signer)
        member, status, grp, _ = registry.verify_signatures(_rows(sigs, 96), np.array(signer, dtype=np.uint32),
                                                            np.array(off, dtype=np.uint32), _rows(msgs, 192),
                                                            scalars=_scalars(n), aggregates=False)
        _assert(grp.tolist(), want_g, names)
        assert status.tolist() == [0] * n
        assert member.tolist() == [m for ms in want_m for m in ms]
        assert registry._profile_verify_stats()["pairing_runs"] == 2


# ------------------------------------------------------------------ bad and skipped pairs at the Miller kernel's layout edges
EDGE_INDEX = (0, 5, 6, 11, 12)      # lane pair k scans pairs k, k + 6, k + 12: the first and last pair of each round of 13


@pytest.fixture(scope="module")
def thirteen():
    """Groups of 13 pairs as (G1 bytes, G2 bytes, verdict): the valid one, its twin, and per edge index i the pairs re-balanced
    so that the twelve pairs OTHER than i sum to 0 (and the twin with one scalar off by one)."""
    rng = np.random.default_rng(1381)
    a = [int.from_bytes(rng.bytes(32), "big") % R or 1 for _ in range(13)]
    b = [int.from_bytes(rng.bytes(32), "big") % R or 1 for _ in range(13)]
    b[12] = -sum(x * y for x, y in zip(a[:12], b[:12])) * _inv(a[12]) % R
    assert sum(x * y for x, y in zip(a, b)) % R == 0
    pts1, pts2 = [_p1(x) for x in a], [_p2(y) for y in b]
    out = {"valid": (pts1, pts2, 1)}
    twin = list(pts2)
    twin[6] = _p2(b[6] + 1)
    out["invalid"] = (pts1, twin, 0)
    for i in EDGE_INDEX:
        j = (i + 1) % 13
        bj = (b[j] + a[i] * b[i] * _inv(a[j])) % R
        assert (sum(x * y for k, (x, y) in enumerate(zip(a, b)) if k not in (i, j)) + a[j] * bj) % R == 0
        for name, d, verdict in (("without", 0, 1), ("without_twin", 1, 0)):
            q = list(pts2)
            q[j] = _p2(bj + d)
            out[name, i] = (pts1, q, verdict)
    return out


def _crafted_thirteen(thirteen, i):
    """[(name, group)] for edge index i: a bad point on either side, and an infinity on either side of the re-balanced group."""
    bad1, bad2 = wc.case("g1:x:plus_p"), wc.case("g2:x.c0:plus_kp_max")
    assert bad1.expect == bad2.expect == wm.BAD
    out = []
    p, q, _ = thirteen["valid"]
    out.append(("bad_g1", (p[:i] + [bad1.enc] + p[i + 1:], q, 2)))
    out.append(("bad_g2", (p, q[:i] + [bad2.enc] + q[i + 1:], 2)))
    for key in ("without", "without_twin"):
        p, q, v = thirteen[key, i]
        out.append((key + "_inf_g1", (p[:i] + [INF1] + p[i + 1:], q, v)))
        out.append((key + "_inf_g2", (p, q[:i] + [wc.case("g2:point:inf_60").enc] + q[i + 1:], v)))
    return out


@pytest.mark.parametrize("i", EDGE_INDEX)
def test_bad_and_skipped_pairs_in_every_round_and_row(engine, pair_groups, thirteen, i):
    """k_bls_miller: the scan for a bad pair (idx += 6 per lane pair, ORed across the 16-lane row) and the skipped pair's line
    of 1, with the pair in the first, second and third round (index 0 | 5, 6 | 11, 12), in each of the four rows of a wave
    beside valid and invalid neighbours of 2 and 13 pairs."""
    neighbours = [pair_groups["valid"], thirteen["invalid"], thirteen["valid"], pair_groups["invalid"]]
    for name, grp in _crafted_thirteen(thirteen, i):
        for row in range(4):
            groups = neighbours[:row] + [grp] + neighbours[row:]
            got = engine.pairing_check(*_pairing_args(groups)).tolist()
            assert got == [g[2] for g in groups], (name, i, row, got)


@pytest.mark.parametrize("n_groups", (4, 5))
def test_only_the_last_group_is_crafted(engine, pair_groups, thirteen, n_groups):
    """The last group in the last row of a full wave (4) and alone in a second wave whose rows 1 to 3 are past the end (5)."""
    before = [thirteen["valid"], pair_groups["invalid"], pair_groups["valid"], thirteen["invalid"]][:n_groups - 1]
    for i in (6, 12):
        for name, grp in _crafted_thirteen(thirteen, i):
            groups = before + [grp]
            got = engine.pairing_check(*_pairing_args(groups)).tolist()
            assert got == [g[2] for g in groups], (name, i, got)


# ------------------------------------------------------------------ the converters that check nothing
def test_the_unchecked_converters_mask_the_flags(engine):
    """k_g1_convert / k_g2_convert (pe_g1_sum, pe_g2_sum, and behind them pe_g1_key_validate, pe_g2_subgroup_check,
    pe_set_validators) validate nothing.  What from_bytes96 / from_bytes192 define is pinned: every spelling with bit 6 is the
    identity, and bits 7 and 5 of the leading byte change nothing in the sum's bytes."""
    for side, width, other, sums in (("g1", 96, _p1(FULL), lambda pts, off: engine.g1_sum(off, points96=pts)),
                                     ("g2", 192, _p2(FULL), lambda pts, off: engine.g2_sum(pts, off))):
        table = wc.cases(side)
        flagged = [c for c in table if c.element == 0 and c.edge in ("bit7", "bit5")]
        infinite = [c for c in table if c.expect == wm.INFINITY]
        assert len(flagged) == 2 and len(infinite) == 5
        canonical, identity = wc.canonical(side), (INF1 if side == "g1" else INF2)
        pts, off = [], [0]
        for c in flagged + infinite:                         # alone, and beside another point
            pts += [c.enc, c.enc, other]
            off += [len(pts) - 2, len(pts)]
        pts += [canonical, canonical, other, other]
        off += [len(pts) - 3, len(pts) - 1, len(pts)]
        got = [r.tobytes() for r in sums(_rows(pts, width), np.array(off, dtype=np.uint32))]
        alone, beside, other_alone = got[-3], got[-2], got[-1]
        assert alone == canonical and other_alone == other and beside not in (canonical, other)
        for k, c in enumerate(flagged + infinite):
            want = (alone, beside) if c in flagged else (identity, other)
            assert (got[2 * k], got[2 * k + 1]) == want, c.name
