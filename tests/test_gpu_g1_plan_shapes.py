"""-m gpu: the G1 plan that k_att_plan forms on the device (rows resident: the path the benchmark times) at RAGGED committee
sizes -- the shapes at which its clamp to the lane-partial buffer, its cap of 256 tasks per group and the k re-derived from a
clamped block size decide something (tests/g1_plan_model.py names them; tests/test_g1_plan_model.py shows on the CPU that
each shape reaches its branch under both lane targets).  Which (k, L) the device took is INFERRED from that pinned formula,
never read back.

The reference is independent of both engine paths: every group's sum against the closed form of the synthetic registry
(keys A + v*B: |S|*A + (sum v)*B over exactly the members whose bit is set), spot-checked by adding the points themselves
with oracle/g1.py; every group's union bits and count against a numpy OR of the input bit rows.  The host-row path on a
twin engine comes second: cheap, and it pins the two planners to each other."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import g1
from tests import g1_plan_model as M
from tests import helpers as H
from tests.test_gpu_resident_rows import _dev_arena, _dev_rows

pytestmark = pytest.mark.gpu
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT
SPE = 32
ST_OK, ST_BITS_LENGTH, ST_EMPTY = 0, 10, 11
INF96 = bytes([0x40]) + bytes(95)
MODES = (("sync", False), ("pipelined", True), ("sync", True), ("pipelined", False))   # (how, bits in a DeviceArena)


@functools.lru_cache(maxsize=None)
def _tree():
    return synth.random_tree(8, 2, "chain")


EPOCH = int(_tree().slot.max()) // SPE + 1


@functools.lru_cache(maxsize=None)
def _registry(n_val):
    pts, ab = H.oracle_points(n_val)
    return pts, ab


def _natural_n_val(tag):
    return sum(M.SHAPES[tag]["sizes"])


def _bit_rows(tag, density, seed):
    """One bit row per attested committee: the big one at `density`, the rest too -- but one group with no bit set and one
    with exactly one (the last member of a committee of two or more)."""
    s = M.SHAPES[tag]
    sizes, big = s["sizes"], s["big"]
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [np.ones(z, dtype=bool) if density >= 1.0 else rng.random(z) < density for z in sizes]
    n = len(sizes)
    empty = next(i for i in range(1, n) if i != big)
    single = next(i for i in range(n - 2, 0, -1) if i not in (big, empty) and sizes[i] >= 2)
    rows[empty] = np.zeros(sizes[empty], dtype=bool)
    rows[single] = np.zeros(sizes[single], dtype=bool)
    rows[single][-1] = True
    if big is not None and density < 1.0:
        assert 0.4 < rows[big].mean() < 0.6 or sizes[big] < 64
    return rows, empty, single


def _case(tag, density, n_val=None, parts=1):
    """The inputs of one shape and everything the engine must answer, computed once and shared (never modified)."""
    return _case_built(tag, density, _natural_n_val(tag) if n_val is None else n_val, parts)


@functools.lru_cache(maxsize=None)
def _case_built(tag, density, n_val, parts):
    s = M.SHAPES[tag]
    sizes, big, refused = s["sizes"], s["big"], s["refused"]
    n = len(sizes)
    (pts, (a, b)) = _registry(n_val)
    comm = H.ragged_committees(sizes, n_val, seed=1000 + n)
    union, empty, single = _bit_rows(tag, density, seed=17 + n)
    for g in refused:                          # len(aggregation_bits) != len(committee): eight bits more than members
        union[g] = np.concatenate([union[g], np.ones(8, dtype=bool)])
    if parts == 1:
        in_rows, committees = union, list(range(n))
    else:                                      # every committee's bits split into `parts` disjoint partial aggregates;
        rng = np.random.Generator(np.random.PCG64(5))   # rows of a group lie n rows apart
        part_of = [rng.integers(0, parts, size=u.size) for u in union]
        in_rows = [u & (p == q) for q in range(parts) for u, p in zip(union, part_of)]
        committees = list(range(n)) * parts
    atts, arena = H.committee_attestations(comm, _tree(), EPOCH, committees, in_rows)
    # ---- expectations: numpy over the input rows, closed form over the members whose bit is set
    want_union = [np.zeros(u.size, dtype=bool) for u in union]
    for c, r in zip(committees, in_rows):
        want_union[c] |= r
    out_arena, out_off, _ = synth.pack_bit_rows(want_union)
    members = [comm.members[comm.offsets[g]:comm.offsets[g + 1]] for g in range(n)]
    voters = [members[g][want_union[g]] if g not in refused else members[g][:0] for g in range(n)]
    sums = np.frombuffer(b"".join(H.closed_form_sums(voters, a, b)), dtype=np.uint8).reshape(n, 96)
    # the same sums once more for three groups, by adding the registry's points themselves
    spot = {}
    for g in [x for x in (big, single, n - 1, 0) if x is not None and x not in refused][:3]:
        spot[g] = g1.to_bytes96(g1.sum_points(g1.from_bytes96(pts[v].tobytes()) for v in voters[g]))
    count = np.array([int(u.sum()) for u in want_union], dtype=np.uint32)
    status = np.where(count > 0, ST_OK, ST_EMPTY).astype(np.int32)
    for g in refused:
        status[g] = ST_BITS_LENGTH
    assert sums[empty].tobytes() == INF96 and count[single] == 1 and count[empty] == 0
    return SimpleNamespace(tag=tag, n=n, n_val=n_val, comm=comm, atts=atts, arena=arena, n_rows=len(atts),
                           group_of=np.asarray(committees, dtype=np.uint32), union=want_union, out_arena=out_arena,
                           out_off=out_off, count=count, count_ok=np.where(status == ST_OK, count, 0).astype(np.uint32),
                           status=status, sums=sums, spot=spot, big=big, empty=empty, single=single, refused=refused,
                           n_bits=np.array([u.size for u in want_union], dtype=np.uint32))


def _engine(engine_factory, n_val):
    e = engine_factory()
    tree = _tree()
    H.load_tree(e, tree)
    pts, _ = _registry(n_val)
    e.set_validators(synth.balances(n_val, 2), np.ones(n_val, dtype=np.uint8), pts)
    e.on_tick((EPOCH + 1) * SPE * 12)
    return e


def _resident(e, case, how, dev_arena, want_pk=True):
    rows = _dev_rows(case.atts)
    bits = _dev_arena(case.arena) if dev_arena else case.arena

    def calls():
        agg = e.aggregate(packed=(rows, bits), want_aggregate_pubkeys=want_pk)
        status, _, count = e.on_attestation_batch(packed=(RR, RES), cap=case.n_rows)
        return agg, status, count

    if how == "sync":
        return calls()
    with e.pipeline():
        out = calls()
    return out


def _check(case, out, want_pk=True):
    agg, status, count = out
    g = case.n
    assert agg["n_groups"] == g
    assert np.array_equal(agg["group_of"][:case.n_rows], case.group_of)
    # union bits and counts: the numpy OR, in the byte-packed layout of the output arena
    assert np.array_equal(agg["atts"]["n_bits"], case.n_bits)
    assert np.array_equal(agg["atts"]["bits_offset"], case.out_off)
    assert np.array_equal(agg["out_arena"], case.out_arena)
    assert np.array_equal(agg["count"], case.count)
    # statuses: fine wherever a bit is set, ST_EMPTY where none is (the sum is then the point at infinity)
    assert np.array_equal(status[:g], case.status) and (status[g:] == 0).all()
    assert np.array_equal(count[:g], case.count_ok) and (count[g:] == 0).all()
    if not want_pk:
        return
    pk = agg["aggpk96"]
    bad = np.flatnonzero((pk != case.sums).any(axis=1))
    assert bad.size == 0, (case.tag, "groups whose sum is not the closed form", bad[:8].tolist(), "big group", case.big)
    assert pk[case.empty].tobytes() == INF96
    for grp, want in case.spot.items():
        assert pk[grp].tobytes() == want, (case.tag, "group", grp, "against the points added one by one")


def _host_rows(e, case):
    return e.aggregate(packed=(case.atts, case.arena), want_aggregate_pubkeys=True)


def _check_against_host(case, out, host):
    agg = out[0]
    assert host["n_groups"] == case.n
    assert np.array_equal(agg["atts"], host["atts"]), "output rows (data, bits_offset, flags)"
    assert np.array_equal(agg["group_of"][:case.n_rows], host["group_of"])
    assert np.array_equal(agg["out_arena"], host["out_arena"])
    assert np.array_equal(agg["count"], host["count"])
    assert np.array_equal(agg["aggpk96"], host["aggpk96"])


PLAN_TAGS = ("tiny", "five", "edge1024", "over1024", "size1025", "cap8192", "deep")


@pytest.mark.parametrize("density", [1.0, 0.5])
@pytest.mark.parametrize("tag", PLAN_TAGS)
def test_ragged_shape_sums_are_the_closed_form(engine_factory, tag, density):
    """Every group of the shape, on a fresh engine: synchronously and inside a pipeline, bits from a host arena and from a
    DeviceArena."""
    case = _case(tag, density)
    e = _engine(engine_factory, case.n_val)
    e.set_committees(EPOCH, case.comm.offsets, case.comm.members)
    outs = []
    for how, dev_arena in MODES:
        out = _resident(e, case, how, dev_arena)
        _check(case, out)
        outs.append(out)
    twin = _engine(engine_factory, case.n_val)
    twin.set_committees(EPOCH, case.comm.offsets, case.comm.members)
    host = _host_rows(twin, case)
    assert np.array_equal(host["aggpk96"], case.sums), "the host planner against the closed form"
    for out in outs:
        _check_against_host(case, out, host)


@pytest.mark.parametrize("first,second,density", [("deep", "tiny", 0.5), ("tiny", "edge1024", 1.0)])
def test_a_second_call_with_another_shape_answers_as_a_fresh_engine(engine_factory, first, second, density):
    """The plan records, the committees' row counts and the partial buffer across shapes: one engine, one registry, the
    committee table replaced between the calls; each call's answers are those of the closed form (what a fresh engine
    gives, test_ragged_shape_sums_are_the_closed_form), the first shape's once more at the end."""
    n_val = max(_natural_n_val(first), _natural_n_val(second))
    e = _engine(engine_factory, n_val)
    steps = ((first, "sync", False), (second, "pipelined", True), (first, "pipelined", True), (second, "sync", False))
    for tag, how, dev_arena in steps:
        case = _case(tag, density, n_val)
        e.set_committees(EPOCH, case.comm.offsets, case.comm.members)
        _check(case, _resident(e, case, how, dev_arena))


@pytest.mark.parametrize("density", [1.0, 0.5])
def test_edge1024_in_two_partial_aggregates_per_committee(engine_factory, density):
    """2048 rows, still 1024 groups of which one has 1024 members: slot_cap is what it was, the lane-partial buffer is still
    filled to its last lane, and the answers are those of the single rows."""
    single, case = _case("edge1024", density), _case("edge1024", density, None, 2)
    assert case.n_rows == 2048 and case.n == 1024
    assert M.shape_plan("edge1024", M.TARGETS[0], rows_per_group=2) == (4, 8, 262144, 262144)
    assert np.array_equal(case.sums, single.sums) and np.array_equal(case.out_arena, single.out_arena)
    e = _engine(engine_factory, case.n_val)
    e.set_committees(EPOCH, case.comm.offsets, case.comm.members)
    for how, dev_arena in MODES[:2]:
        _check(case, _resident(e, case, how, dev_arena))
    _check(single, _resident(e, single, "sync", True))


@pytest.mark.parametrize("density", [1.0, 0.5])
def test_a_refused_group_does_not_shape_the_plan(engine_factory, density):
    """64 committees of 4 and one of 4096 whose row carries 8 bits too many (ST_BITS_LENGTH).  With aggregate pubkeys the
    call fails as the host path does; without, all 65 groups form and their union bits come out, the big one refused;
    and the 64 alone, on the same engine afterwards, sum to the closed form (nothing of the 4096 is left behind)."""
    case = _case("refused_big", density)
    big = case.big
    e = _engine(engine_factory, case.n_val)
    e.set_committees(EPOCH, case.comm.offsets, case.comm.members)
    twin = _engine(engine_factory, case.n_val)
    twin.set_committees(EPOCH, case.comm.offsets, case.comm.members)
    with pytest.raises(pea.EngineError) as host_err:
        _host_rows(twin, case)
    assert host_err.value.status == -1           # PE_ERR_INVALID_ARG: len(aggregation_bits) != len(committee)
    for how, dev_arena in MODES:
        with pytest.raises(pea.EngineError) as err:
            _resident(e, case, how, dev_arena)
        assert err.value.status == host_err.value.status
        out = _resident(e, case, how, dev_arena, want_pk=False)
        _check(case, out, want_pk=False)
        assert out[1][big] == ST_BITS_LENGTH and case.n_bits[big] == 4096 + 8
    # the fine groups alone: the same rows without the refused one
    keep = np.arange(case.n) != big
    atts = np.ascontiguousarray(case.atts[keep])
    for how, dev_arena in MODES[:2]:
        rest = SimpleNamespace(atts=atts, arena=case.arena, n_rows=case.n - 1)
        agg, status, count = _resident(e, rest, how, dev_arena)
        assert agg["n_groups"] == case.n - 1
        assert np.array_equal(agg["aggpk96"], case.sums[keep])
        assert np.array_equal(agg["count"], case.count[keep])
        assert np.array_equal(status[:case.n - 1], case.status[keep])
        for g_out, g_in in enumerate(np.flatnonzero(keep)):
            assert np.array_equal(agg["bits"][g_out], case.union[g_in])


# ---------------------------------------------------------------- packed_same: how the union bits are copied out
@pytest.mark.parametrize("how,dev_arena", MODES[:2])
@pytest.mark.parametrize("n_bits", [(33, 64, 7), (32, 64, 7), (32, 64, 33)])
def test_union_bits_come_out_byte_packed_wherever_the_first_ragged_group_sits(engine_factory, n_bits, how, dev_arena):
    """The device keeps unions word-aligned and the output arena is byte-packed; the two layouts agree as long as every
    union but the last is a whole number of words (AttPlan::packed_same, from mis_key: the FIRST group that is not).  That
    group first, nowhere but last, and last; two disjoint partial rows per group, whose last byte carries stray bits above
    n_bits that belong to nobody."""
    n_val = sum(n_bits)
    pts, (a, b) = _registry(n_val)
    comm = H.ragged_committees(n_bits, n_val, seed=3)
    rng = np.random.Generator(np.random.PCG64(sum(n_bits)))
    union = [rng.random(z) < 0.7 for z in n_bits]
    for u in union:
        u[-1] = True                              # the top bit itself is a member's
    half = [rng.random(z) < 0.5 for z in n_bits]
    in_rows = [u & h for u, h in zip(union, half)] + [u & ~h for u, h in zip(union, half)]
    atts, arena = H.committee_attestations(comm, _tree(), EPOCH, [0, 1, 2] * 2, in_rows)
    arena = arena.copy()
    for r in atts:                                # stray high bits in the last byte of every member row
        nb = int(r["n_bits"])
        if nb % 8:
            arena[int(r["bits_offset"]) + nb // 8] |= (0xFF << (nb % 8)) & 0xFF
    want_arena, want_off, _ = synth.pack_bit_rows(union)
    assert [int(o) for o in want_off] == [0, (n_bits[0] + 7) // 8, (n_bits[0] + 7) // 8 + (n_bits[1] + 7) // 8]
    case = SimpleNamespace(atts=atts, arena=arena, n_rows=6)
    e = _engine(engine_factory, n_val)
    e.set_committees(EPOCH, comm.offsets, comm.members)
    agg, status, count = _resident(e, case, how, dev_arena)
    assert agg["n_groups"] == 3 and list(agg["group_of"][:6]) == [0, 1, 2, 0, 1, 2]
    assert list(agg["atts"]["bits_offset"]) == list(want_off) and list(agg["atts"]["n_bits"]) == list(n_bits)
    assert np.array_equal(agg["out_arena"], want_arena), "byte-packed: (n_bits + 7) // 8 bytes per group, no stray bits"
    for g in range(3):
        assert np.array_equal(agg["bits"][g], union[g])
    assert list(agg["count"]) == [int(u.sum()) for u in union]
    assert list(status[:3]) == [ST_OK] * 3 and list(count[:3]) == [int(u.sum()) for u in union]
    voters = [comm.members[comm.offsets[g]:comm.offsets[g + 1]][union[g]] for g in range(3)]
    assert [x.tobytes() for x in agg["aggpk96"]] == H.closed_form_sums(voters, a, b)
    twin = _engine(engine_factory, n_val)
    twin.set_committees(EPOCH, comm.offsets, comm.members)
    host = twin.aggregate(packed=(atts, arena), want_aggregate_pubkeys=True)
    assert np.array_equal(host["out_arena"], want_arena) and np.array_equal(host["count"], agg["count"])
    assert np.array_equal(host["atts"], agg["atts"])
