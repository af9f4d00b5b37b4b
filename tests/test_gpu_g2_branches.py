"""The rare branches of the G2 kernels and of the two wire-format decoders, driven with crafted inputs (tests/g2_special.py;
tests/test_oracle_g2_special.py proves on the CPU that each input is what its name says) and compared bit for bit with
oracle/g1.py / oracle/g2.py.  fp381.h, fp_sqrt.h and g2.h are device only: these tests are the only check of the branches a
multiple of the generator cannot reach -- and that a crafted BLSSignature / BLSPubkey from the network reaches at will.

The numbered items in the docstrings are those of the list this file was written from:
 1 g2_decompress_one's `a1 == 0` root (g2_kernels.hip:109-114)
 2 the sign rule with a zero half of y: decoder (g2_kernels.hip:147-151), device compressor (g2_kernels.hip:599), host
   compressor (pe_g2_compress, engine_g1.cpp:451; on the CPU in tests/test_oracle_g2_special.py and here through its callers)
 3 canonical-form boundaries of both decoders (fp_is_canonical, fp_sqrt.h:24; g1_kernels.hip:89; g2_kernels.hip:74, :81)
 4 the group law at each add site of pe_g2_sum (g2_kernels.hip:333-338 lane run, :352-385 workgroup tree, :411-415
   k_g2_finish; g2x_add's infinities g2.h:160-161 and doubling g2.h:173)
 5 the pair predicates of g2.h (pair_and g2.h:20; f2_is_zero at g2.h:135-136 and g2.h:172-173)
 6 k_g2_aggregate_rows' edge cases (g2_kernels.hip:569-588)
 7 k_g2_subgroup_check on odd points (g2_kernels.hip:478-523)
"""
import numpy as np
import pytest

from oracle import g1, g2
from tests import g2_special as S

pytestmark = pytest.mark.gpu
R_ORDER = g1.R_ORDER
INF192 = g2.to_bytes192(None)


def _rows(points):
    return np.stack([np.frombuffer(g2.to_bytes192(p), dtype=np.uint8) for p in points])


def _wire(encs):
    return np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(len(encs), -1).copy()


def _crafted_with_negatives():
    """[(name, point)] for every crafted point and its negative: 16 points, four with y.c1 == 0, four with y.c0 == 0."""
    return [(n + s, q) for n, p in S.crafted_points() for s, q in (("", p), ("-", g2.neg(p)))]


# ---------------------------------------------------------------- the decoders
def test_g2_decompress_rhs_in_fp(engine_factory):
    """Items 1 and 2.  x^3 + 4(1+u) in Fp: `if (fp_is_zero(a1))` of g2_decompress_one (g2_kernels.hip, the fp_sqrt_candidate
    branch: y = (t, 0) or (0, t)), then the sign rule `fp_is_zero(y1) ? fp_is_larger_half(y0) : ...` and the flip
    `fp_neg(y0, y0)` with y0 == 0, which must put 0 and not p on the wire.  Both encodings of every such point, in the first, a
    middle and the last lane of a 64-lane workgroup and in a trailing partial workgroup, between generic neighbours that take
    the general branch (the branch diverges inside a wave); every encoding visits every position."""
    e = engine_factory()
    r = S.rhs_in_fp_points()
    special = [q for kind in ("real", "imag") for p in r[kind] for q in (p, g2.neg(p))]
    assert len(special) == 8
    n = 64 * 3 + 17
    generic = g2.synthetic_points(n, 0x1234567, 0x89ABCDE)
    positions = [0, 29, 63, 64, 100, 127, 192, n - 1]
    for rot in range(len(special)):
        pts = list(generic)
        for j, pos in enumerate(positions):
            pts[pos] = special[(j + rot) % len(special)]
        comp = _wire([g2.compress(p) for p in pts])
        out, status = e.g2_decompress(comp)
        assert not status.any(), (rot, np.nonzero(status)[0])
        for i, p in enumerate(pts):
            want = g2.to_bytes192(g2.decompress(comp[i].tobytes()))
            assert want == g2.to_bytes192(p)
            assert out[i].tobytes() == want, (rot, i)


def test_g2_decompress_montgomery_rows_of_crafted_points(engine_factory):
    """Items 1, 2 and 7.  g2_decompress_one's SECOND output (out_mont48; pe_g2_decompress uses only out_be192): one-member
    groups of pe_aggregate_signatures, whose aggregate must be the member's own encoding -- k_g2_decompress, k_g2_accumulate's
    first add, k_g2_finish and the host compressor pe_g2_compress with its `y.c1 == 0` rule (engine_g1.cpp).  With the subgroup
    check on, the crafted members (all outside G2, says the oracle) are reported 3 and their groups sum to infinity."""
    e = engine_factory()
    crafted = _crafted_with_negatives()
    generic = g2.synthetic_points(70, 0x5151, 0x77)
    pts = list(generic)
    for j, (_, p) in enumerate(crafted):                      # spread: lanes 0, 4, 8, ... 60 of the decoder's first workgroup
        pts[4 * j] = p
    pts[67] = crafted[0][1]                                   # ... and the trailing partial one
    pts[69] = None
    sig = _wire([g2.compress(p) for p in pts])
    n = len(pts)
    offsets = np.arange(n + 1, dtype=np.uint32)
    agg, status, bad = e.aggregate_signatures(sig, offsets)
    assert not status.any() and not bad.any()
    for i in range(n):
        assert bytes(agg[i]) == sig[i].tobytes(), i
    perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
    agg, status, bad = e.aggregate_signatures(sig, offsets, index=perm)
    assert not status.any() and not bad.any()
    for i in range(n):
        assert bytes(agg[i]) == sig[perm[i]].tobytes(), i
    outside = np.array([p is not None and g2.mul(R_ORDER, p) is not None for p in pts])
    assert outside.sum() >= 1 and not outside[[1, 2, 3, 66, 68, 69]].any()
    agg, status, bad = e.aggregate_signatures(sig, offsets, check_subgroup=True)
    assert np.array_equal(status, np.where(outside, 3, 0)) and np.array_equal(bad, outside.astype(np.uint32))
    for i in range(n):
        assert bytes(agg[i]) == (g2.compress(None) if outside[i] else sig[i].tobytes()), i


def test_g2_decompress_boundaries(engine_factory):
    """Item 3.  `fp_is_canonical` (fp_sqrt.h) on both halves of x in g2_decompress_one: x.c1 = p / x.c0 = p, p - 1, p + s with s
    an abscissa on the curve (a decoder that reduced instead of rejecting would answer 0), flag bits or-ed into the leading byte
    of x.c0 (that byte carries none: its limb is reloaded unmasked), malformed infinities with one stray byte in either half.
    Status as the oracle's, rejected rows all zero, accepted rows the oracle's bytes."""
    e = engine_factory()
    cases = S.g2_boundary_encodings()
    out, status = e.g2_decompress(_wire([enc for _, enc, _ in cases]))
    for i, (name, enc, st) in enumerate(cases):
        assert status[i] == st == S.oracle_status(g2.decompress, enc), name
        want = g2.to_bytes192(g2.decompress(enc)) if st == 0 else bytes(192)
        assert out[i].tobytes() == want, name
    # each on its own at lane 0 and between generic neighbours: no case may lean on the one beside it
    gen = g2.compress(g2.mul(5, g2.G2))
    for name, enc, st in cases:
        out, status = e.g2_decompress(_wire([enc, gen, enc]))
        assert status.tolist() == [st, 0, st], name
        want = g2.to_bytes192(g2.decompress(enc)) if st == 0 else bytes(192)
        assert out[0].tobytes() == want and out[2].tobytes() == want, name
        assert out[1].tobytes() == g2.to_bytes192(g2.mul(5, g2.G2))


def test_g1_decompress_boundaries(engine_factory):
    """Item 3.  `fp_is_canonical` in k_g1_decompress (g1_kernels.hip): x = p, p - 1, p + s (s on the curve), 2^381 - 1, x = 0
    (on the curve: y = 2), malformed infinities (0xC0...01, 0xE0..., x under 0xC0), missing compression flag; both signs.
    pe_g1_decompress: status as the oracle's, rejected rows zero, accepted rows the oracle's bytes.  pe_set_pubkeys_compressed
    (the Montgomery-row output): raises when any key is rejected and leaves no keys behind; loads the accepted ones so that
    one-member sums give the oracle's points back."""
    import pos_evolution_amd as pea
    import pos_evolution_amd.synth as synth
    e = engine_factory()
    cases = S.g1_boundary_encodings()
    n = len(cases)
    keys = _wire([enc for _, enc, _ in cases])
    out, status = e.g1_decompress(keys)
    for i, (name, enc, st) in enumerate(cases):
        assert status[i] == st == S.oracle_status(g1.decompress, enc), name
        want = g1.to_bytes96(g1.decompress(enc)) if st == 0 else bytes(96)
        assert out[i].tobytes() == want, name
    e.set_validators(synth.balances(n, 3), np.ones(n, dtype=np.uint8))
    with pytest.raises(pea.EngineError):
        e.set_pubkeys_compressed(keys)
    with pytest.raises(pea.EngineError):                       # the failed load leaves no pubkeys behind
        e.g1_sum([0, 1])
    # one rejected key among accepted ones, for every rejected encoding, over a registry that held keys before
    good = [enc for _, enc, st in cases if st == 0]
    assert len(good) >= 7
    e2 = engine_factory()
    e2.set_validators(synth.balances(len(good) + 1, 3), np.ones(len(good) + 1, dtype=np.uint8))
    for name, enc, st in cases:
        if st == 0:
            continue
        e2.set_pubkeys_compressed(_wire(good[:3] + [good[0]] + good[3:]))
        assert e2.g1_sum([0, 1])[0].tobytes() == g1.to_bytes96(g1.decompress(good[0])), name
        with pytest.raises(pea.EngineError):
            e2.set_pubkeys_compressed(_wire(good[:3] + [enc] + good[3:]))
        with pytest.raises(pea.EngineError):
            e2.g1_sum([0, 1])
    e3 = engine_factory()
    e3.set_validators(synth.balances(len(good), 3), np.ones(len(good), dtype=np.uint8))
    e3.set_pubkeys_compressed(_wire(good))
    got = e3.g1_sum(np.arange(len(good) + 1))
    for i, enc in enumerate(good):
        assert got[i].tobytes() == g1.to_bytes96(g1.decompress(enc)), i
    assert np.array_equal(e3.g1_compress(got), _wire(good))


# ---------------------------------------------------------------- pe_g2_sum: the group law at each of its three add sites
A_K, B_K = 7, 11                                  # A = 7 G2, B = 11 G2
TA, TNA, TB, TINF = 0, 1, 2, 3                    # rows of the point table [A, -A, B, infinity]
K = 4                                             # members per lane pair: G1_MIN_K while a call has <= 4 * 65536 members
WG = 128 * K                                      # members per workgroup of a WIDE group (n_tasks > 128, i.e. > 512 members)


def _law_groups():
    """[(name, member list over the table)].  The planner (plan_g1, engine_internal.h) gives every lane pair k = 4 consecutive
    members (the lane run, g2x_add_affine in k_g2_accumulate); a group of up to 512 members is a block of 2^l lanes summed by
    the workgroup tree (g2x_add in k_g2_accumulate's LDS levels) into one partial; a larger one is WIDE: whole workgroups of
    512 members, one partial each, added one after the other by k_g2_finish (g2x_add again)."""
    a, na, b, o = [TA], [TNA], [TB], [TINF]
    g = []
    # n copies of A: every add meets an equal point.  2, 3: the doubling inside g2x_add_affine (lane run).  64: 16 lanes of
    # 4A, the tree doubles at each of its 4 levels.  129: 32 lanes of 4A and one of A (tree: doublings, then 128A + A).
    # 1024: two workgroups of 512A, k_g2_finish adds 512A to infinity and then DOUBLES.  20000: 40 partials in k_g2_finish,
    # the first add a doubling, the last partial a short one (32A).
    for n in (2, 3, 64, 129, 1024, 20000):
        g.append((f"{n}xA", a * n))
    # m x A then m x -A, then B: the sum goes on from infinity.
    g.append(("cancel_in_lane_run_m1", a + na + b))                       # A, -A, B in ONE lane: g2x_add_affine P + (-P), then first add
    g.append(("cancel_in_lane_run_m2", a * 2 + na * 2 + b))               # 2A (doubling) - A - A in one lane; B in the next
    g.append(("cancel_at_tree_level_1", a * K + na * K + b))              # lanes 0 / 1 hold 4A / -4A: g2x_add P + (-P); B in lane 2
    g.append(("cancel_at_tree_level_5", a * 16 * K + na * 16 * K + b))    # 16 lanes against 16: the tree's level 5 of a 64-lane block
    g.append(("cancel_at_tree_top", a * 64 * K + na * 64 * K + b))        # wide (129 lanes): workgroup 0's top level adds 256A and -256A;
    #                                                                       k_g2_finish: infinity + infinity, then + B
    g.append(("cancel_in_finish", a * WG + na * WG + b))                  # workgroup partials 512A, -512A, B meet in k_g2_finish
    g.append(("cancel_in_finish_halves", a * 2 * WG + na * 2 * WG + b))   # 512A + 512A (doubling), - 512A, - 512A (to infinity), + B
    # rows of zeros (infinity) filling whole lanes / a whole workgroup: g2x_add with infinity on either side, and on both
    g.append(("inf_lane_first", o * K + a * K + b))                       # tree: infinity + 4A (p infinite: p = q)
    g.append(("inf_lane_middle", a * K + o * K + b * K))                  # tree: 4A + infinity (q infinite), then + (infinity + 4B)
    g.append(("inf_lane_last", a * K + b * K + o * K))                    # tree: infinity + padding infinity, then P + infinity
    g.append(("inf_two_lanes_first", o * 2 * K + a))                      # infinity + infinity at level 1, then infinity + A
    g.append(("inf_members_inside_a_run", o + a + o + b + o + a))         # q_inf inside the lane run, before and after the first add
    g.append(("inf_only", o * 5))
    g.append(("inf_workgroup_first", o * WG + a * WG + b))                # wide: partial 0 is infinity in k_g2_finish
    g.append(("inf_workgroup_middle", a * WG + o * WG + b * K))
    g.append(("inf_workgroup_last", a * (WG + K) + o * WG))
    g.append(("empty", []))
    return g


def _law_expected(members):
    cnt = np.bincount(np.asarray(members, dtype=np.int64), minlength=4)
    return g2.to_bytes192(g2.mul(((int(cnt[TA]) - int(cnt[TNA])) * A_K + int(cnt[TB]) * B_K) % R_ORDER, g2.G2))


def test_g2_sum_group_law_at_every_add_site(engine_factory):
    """Item 4 (and g2.h's g2x_add: doubling at `if (f2_is_zero(P))`, infinity on either side at its first two lines).  Equal,
    opposite and infinite operands at each place pe_g2_sum adds: k_g2_accumulate's lane run, its workgroup tree, and
    k_g2_finish across workgroup partials; _law_groups says which input reaches which.  All groups and an empty one in ONE call
    beside generic groups (out_base / slot_base bookkeeping), in two orders; expected values: one oracle multiplication each."""
    e = engine_factory()
    A, B = g2.mul(A_K, g2.G2), g2.mul(B_K, g2.G2)
    n_gen = 300
    table = [A, g2.neg(A), B, None] + g2.synthetic_points(n_gen, 3, 5)
    pts = _rows(table)
    rng = np.random.default_rng(4)
    groups = _law_groups()
    assert {len(m) for _, m in groups} >= {2, 3, 64, 129, 1024, 20000, 0}
    for j, size in enumerate((1, 5, 37, 130, 600)):                         # generic groups in between
        idx = (4 + rng.integers(0, n_gen, size=size)).tolist()
        groups.insert(3 + 4 * j, (f"generic{size}", idx))
    want = {}
    for name, m in groups:
        if name.startswith("generic"):
            want[name] = g2.to_bytes192(g2.mul(sum(3 + 5 * (i - 4) for i in m) % R_ORDER, g2.G2))
        else:
            want[name] = _law_expected(m)
    assert want["inf_only"] == INF192 and want["empty"] == INF192
    assert want["cancel_in_finish"] == g2.to_bytes192(B) and want["2xA"] == g2.to_bytes192(g2.double(A))
    for order in (groups, groups[::-1]):
        index = np.array([i for _, m in order for i in m], dtype=np.uint32)
        assert index.size <= K * 65536                                      # the planner's k stays 4: the sites are as stated
        offsets = np.concatenate([[0], np.cumsum([len(m) for _, m in order])]).astype(np.uint32)
        got = e.g2_sum(pts, offsets, index=index)
        for (name, _), row in zip(order, got):
            assert row.tobytes() == want[name], name
    # each special group alone in its call (slot_base = out_base = 0), contiguous members without an index list
    for name, m in groups:
        if name.startswith("generic") or len(m) > 3000:
            continue
        got = e.g2_sum(_rows([table[i] for i in m]) if m else np.zeros((0, 192), dtype=np.uint8), [0, len(m)])
        assert got[0].tobytes() == want[name], name


def test_g2_pair_predicates(engine_factory):
    """Item 5 (and item 2's points in the group law).  Each Fp2 value lives in two lanes and every `is zero` must be the AND of
    both (pair_and, g2.h).  Operands that differ in ONE half: curve points with equal x.c0 and different x.c1, and the reverse
    (x difference zero in one half), P and -P with y.c1 == 0 or y.c0 == 0 (Y2 - Y1 zero in one half), P and P for the same --
    as adjacent members (one lane run: g2x_add_affine's `f2_is_zero(P)` / `f2_is_zero(R)`) and as the only members of two
    different lanes (workgroup tree: g2x_add's).  Expected: oracle.g2.add, plain curve arithmetic.
    (What this cannot see: a predicate on `R` that lets the two lanes of a pair DISAGREE.  For these inputs the lane that wrongly
    doubles still computes a zero half of ZZ -- the true double's ZZ = (2y)^2 lies in Fp -- so the pair reads as infinity, the
    right answer.  A predicate taken from one half by BOTH lanes is caught here.)"""
    e = engine_factory()
    named = dict(_crafted_with_negatives())
    names = sorted(named)
    table = [named[k] for k in names] + [None]
    row = {k: i for i, k in enumerate(names)}
    o = len(names)
    pairs = [("same_c0_0", "same_c0_1"), ("same_c0_1", "same_c0_0"), ("same_c1_0", "same_c1_1"), ("same_c1_1", "same_c1_0"),
             ("same_c0_0", "same_c0_1-"), ("same_c1_0-", "same_c1_1")]
    for base in ("real0", "real1", "imag0", "imag1", "same_c0_0", "same_c1_1"):
        pairs += [(base, base + "-"), (base + "-", base), (base, base), (base + "-", base + "-")]
    pairs += [("real0", "imag0"), ("imag1", "real1-"), ("real0", "real1"), ("imag0-", "imag1")]
    groups, want = [], []
    for p, q in pairs:
        exp = g2.to_bytes192(g2.add(named[p], named[q]))
        assert g2.is_on_curve(g2.add(named[p], named[q]))
        groups.append([row[p], row[q]])                                     # one lane run
        groups.append([row[p], o, o, o, row[q]])                            # lanes 0 and 1 of a block of two: the tree
        groups.append([o, o, o, row[p], row[q], o, o, o, o])                # run ends / starts at the pair: tree again, + padding lane
        want += [exp, exp, exp]
    assert sum(w == INF192 for w in want) == 3 * 12
    index = np.array([i for m in groups for i in m], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in groups])]).astype(np.uint32)
    got = e.g2_sum(_rows(table), offsets, index=index)
    for j, (row_got, w) in enumerate(zip(got, want)):
        assert row_got.tobytes() == w, (pairs[j // 3], j % 3)
    # k_g2_finish's g2x_add: the two operands as the partials of a wide group's two workgroups
    for p, q in [("same_c0_0", "same_c0_1"), ("same_c1_0", "same_c1_1"), ("real0", "real0-"), ("imag0-", "imag0"),
                 ("real1", "real1"), ("imag1", "imag1")]:
        m = [row[p]] + [o] * (WG - 1) + [row[q]]
        got = e.g2_sum(_rows(table), [0, len(m)], index=np.array(m, dtype=np.uint32))
        assert got[0].tobytes() == g2.to_bytes192(g2.add(named[p], named[q])), (p, q)


def test_g2_subgroup_check_on_crafted_points(engine_factory):
    """Item 7.  k_g2_subgroup_check (psi(P) == [z]P) on curve points with unusual coordinates -- a zero half in y, small halves
    in x, abscissas at p - 1 -- their negatives and doubles, between members of G2: 3 exactly where the oracle's
    mul(R_ORDER, P) is not infinity."""
    e = engine_factory()
    odd = [q for _, p in _crafted_with_negatives() for q in (p, g2.double(p))]
    odd += [g2.decompress(enc) for _, enc, st in S.g2_boundary_encodings() if st == 0]
    good = g2.synthetic_points(len(odd) + 3, 77, 5)
    pts = [good[0]]
    for i, p in enumerate(odd):
        pts += [p, good[i + 1]]
    pts += [None, good[-1]]
    want = [0 if p is None or g2.mul(R_ORDER, p) is None else 3 for p in pts]
    assert want.count(3) >= 16 and want.count(0) >= len(good)
    assert e.g2_subgroup_check(_rows(pts)).tolist() == want


# ---------------------------------------------------------------- k_g2_aggregate_rows and the device compressor
def _signed_cases():
    """[(name, the group's first members as points)]: what the chosen committees' partial aggregates carry; members beyond
    the listed ones carry the compressed infinity."""
    S7, T = g2.mul(7, g2.G2), g2.mul(11, g2.G2)
    named = dict(_crafted_with_negatives())
    cases = [(f"single:{k}", [named[k]]) for k in sorted(named)]           # the group's sum IS the crafted point
    for label, s in (("generic", S7), ("real0", named["real0"]), ("imag0", named["imag0"]), ("same_c0_0", named["same_c0_0"])):
        cases += [(f"{label}:S,S", [s, s]), (f"{label}:S,-S", [s, g2.neg(s)]), (f"{label}:inf,S", [None, s]),
                  (f"{label}:S,-S,T", [s, g2.neg(s), T]), (f"{label}:inf,S,S", [None, s, s])]
    cases += [("shared_c0", list(S.shared_half_points()["c0"])), ("shared_c1", list(S.shared_half_points()["c1"])),
              ("inf_only", [None, None])]
    return cases


@pytest.mark.parametrize("rows_mode", ["host", "device"])
@pytest.mark.parametrize("compressed", [True, False])
def test_aggregate_signed_rare_branches(engine_factory, rows_mode, compressed):
    """Items 6, 1, 2 and 5.  k_g2_aggregate_rows (the signature leg of pe_aggregate_signed) adds a committee's partial
    aggregates one after the other with g2x_add_affine and compresses on the device.  Committees whose members carry S, S
    (doubling: 2S); S, -S (the 0xC0 output); the compressed infinity first; S, -S, T (on from infinity: T); for a generic S and
    for S with a zero half in y or a shared half in x (the pair predicates).  Committees whose only point is a crafted one:
    k_g2_decompress_batch's `a1 == 0` root and Montgomery rows (compressed) or k_g2_convert (uncompressed), and the device
    compressor's `c1_zero ? c0_larger : c1_larger` on sums with y.c1 == 0 / y.c0 == 0.  Synchronous and inside a pipeline; with
    the subgroup check on, every member outside G2 is reported 3 and left out."""
    from tests.test_gpu_pipeline import _world
    from tests.test_gpu_resident_rows import _dev_arena, _dev_rows

    w = _world(engine_factory, 6000, 64, seed=3, density=0.8, parts=3)
    e, atts, arena = w["e"], w["atts"], w["arena"]
    n = len(atts)
    ref = e.aggregate(packed=(atts, arena))
    gof = np.asarray(ref["group_of"][:n])
    n_groups = int(ref["n_groups"])
    members = [np.nonzero(gof == k)[0] for k in range(n_groups)]            # in input order, as member_row lists them
    sig_pts = list(g2.synthetic_points(n, 0xABCDEF12345, 0x1357))
    cases = _signed_cases()
    free = sorted(range(n_groups), key=lambda k: (len(members[k]), k))
    placed = {}
    for name, pts in sorted(cases, key=lambda c: -len(c[1])):               # the longest lists take the largest groups
        k = free.pop()
        assert len(members[k]) >= len(pts), f"{name}: no committee with {len(pts)} partial aggregates left"
        placed[name] = k
        for j, row in enumerate(members[k]):
            sig_pts[row] = pts[j] if j < len(pts) else None
    assert len(placed) == len(cases) and len(free) >= 4                     # generic committees remain beside them
    wire = _wire([g2.compress(p) if compressed else g2.to_bytes192(p) for p in sig_pts])
    packed = (_dev_rows(atts), _dev_arena(arena)) if rows_mode == "device" else (atts, arena)
    want = [g2.compress(g2.sum_points([sig_pts[i] for i in members[k]])) for k in range(n_groups)]
    named = dict(_crafted_with_negatives())
    for k in sorted(named):
        assert want[placed[f"single:{k}"]] == g2.compress(named[k])
    S7 = g2.mul(7, g2.G2)
    assert want[placed["generic:S,S"]] == g2.compress(g2.mul(14, g2.G2)) and want[placed["generic:inf,S"]] == g2.compress(S7)
    assert want[placed["generic:S,-S"]] == g2.compress(None) and want[placed["generic:S,-S,T"]] == g2.compress(g2.mul(11, g2.G2))
    assert want[placed["real0:S,-S"]] == g2.compress(None) and want[placed["real0:S,S"]] == g2.compress(g2.double(named["real0"]))

    def check(res, want_sig, want_st):
        assert res["n_groups"] == n_groups and np.array_equal(res["group_of"][:n], gof)
        assert np.array_equal(res["sig_status"], want_st)
        by_group = {k: name for name, k in placed.items()}
        for k in range(n_groups):
            assert res["sig96c"][k].tobytes() == want_sig[k], (k, by_group.get(k, "generic"))

    zero = np.zeros(n, dtype=np.int32)
    check(e.aggregate_signed(wire, packed=packed, compressed=compressed, check_subgroup=False), want, zero)
    with e.pipeline():
        res = e.aggregate_signed(wire, packed=packed, compressed=compressed, check_subgroup=False)
    check(res, want, zero)
    outside = np.array([p is not None and g2.mul(R_ORDER, p) is not None for p in sig_pts])
    assert outside.sum() >= 16
    want_in = [g2.compress(g2.sum_points([sig_pts[i] for i in members[k] if not outside[i]])) for k in range(n_groups)]
    with e.pipeline():
        res = e.aggregate_signed(wire, packed=packed, compressed=compressed, check_subgroup=True)
    check(res, want_in, np.where(outside, 3, 0).astype(np.int32))
