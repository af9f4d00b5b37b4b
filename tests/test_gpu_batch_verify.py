"""GPU: pe_batch_verify / pe_batch_fast_aggregate_verify.  Every case is held to tests/batch_verify_model.py (verdicts and the
stats of pe_profile_batch_stats) and to the per-group path (Engine.pairing_check / fast_aggregate_verify) on the same inputs.

Points are made BY CONSTRUCTION, as in tests/test_gpu_bls_verify.py: pk = a G1, H = b G2, sig = a b G2 is valid,
sig = (a b + 1) G2 is not; the model then decides every product in the exponent of e(G1, G2) (its `dlogs` route, which
tests/test_batch_verify_model.py holds to its pairing route), so no pairing is computed in Python here -- except for the two
three-group batches whose pe_profile_batch_gt bytes are compared with the model's.

Layout edges: a chunk is c groups and one signature pair = c + 1 pairs of one Miller row, whose six lane pairs take the pairs
six at a time (c = 5 | 6, c = 11 end and begin a round); four rows make a wave (4 c | 4 c + 1 groups); the product tree gains a
level at c F | c F + 1 groups.  c and F are read from the stats."""
import numpy as np
import pytest

from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from tests import batch_verify_model as bm

pytestmark = pytest.mark.gpu
NEG_G1 = g1.to_bytes96(g1.neg(g1.G))
STAT_NAMES = ("live", "chunks", "product_launches", "top_exps", "fallback_exps", "rechecked", "c", "F")
SCALAR_EDGES = (1, 2, 1 << 63, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0xFFFFFFFF00000000, 0x8000000000000001)


def _group(a, b, s):
    return (g1.mul(a, g1.G), g2.mul(b, g2.G2), g2.mul(s, g2.G2))


@pytest.fixture(scope="module")
def pool():
    """90 valid groups with their discrete logs (a, b, a b): the first eight with full-width scalars, the rest 64-bit ones (the
    points are made in Python; the kernels see full-width coordinates either way)."""
    rng = np.random.default_rng(2381)
    groups, dlogs = [], []
    for i in range(90):
        width = 32 if i < 8 else 8
        a = int.from_bytes(rng.bytes(width), "big") % R_ORDER or 1
        b = int.from_bytes(rng.bytes(width), "big") % R_ORDER or 1
        dlogs.append((a, b, a * b % R_ORDER))
        groups.append(_group(*dlogs[-1]))
    return groups, dlogs


@pytest.fixture(scope="module")
def engine(engine_factory):
    return engine_factory(device=0)


def _scalars(n, seed=1):
    rng = np.random.default_rng(seed)
    return [int(v) | 1 for v in rng.integers(1, 1 << 63, size=n, dtype=np.uint64)]


def _spoil(groups, dlogs, where):
    groups, dlogs = list(groups), list(dlogs)
    for i in where:
        a, b, s = dlogs[i]
        dlogs[i] = (a, b, (s + 1) % R_ORDER)
        groups[i] = (groups[i][0], groups[i][1], g2.add(groups[i][2], g2.G2))
    return groups, dlogs


def _wire(groups):
    pk = np.frombuffer(b"".join(g1.to_bytes96(g[0]) for g in groups), dtype=np.uint8).reshape(-1, 96)
    msg = np.frombuffer(b"".join(g2.to_bytes192(g[1]) for g in groups), dtype=np.uint8).reshape(-1, 192)
    sig = np.frombuffer(b"".join(g2.to_bytes192(g[2]) for g in groups), dtype=np.uint8).reshape(-1, 192)
    return pk, msg, sig


def _per_group(engine, groups):
    """The per-group path on the same inputs: the pairs (pk, H), (-g1, sig) through pairing_check, then
    pe_fast_aggregate_verify's rule for the identity signature."""
    pk, msg, sig = _wire(groups)
    n = len(groups)
    a = np.zeros((2 * n, 96), np.uint8)
    b = np.zeros((2 * n, 192), np.uint8)
    a[0::2], a[1::2] = pk, np.frombuffer(NEG_G1, dtype=np.uint8)
    b[0::2], b[1::2] = msg, sig
    v = engine.pairing_check(a, b, np.arange(0, 2 * n + 1, 2, dtype=np.uint32)).tolist()
    return [0 if (x == 1 and g[2] is None) else x for x, g in zip(v, groups)]


def _check(engine, groups, dlogs, r, skip_per_group=()):
    """One batch call against the model (verdicts, stats) and against the per-group path; -> (verdicts, stats)."""
    pk, msg, sig = _wire(groups)
    got = engine.batch_verify(pk, msg, sig, np.array(r, dtype=np.uint64)).tolist()
    stats = engine._profile_batch_stats()
    want, want_stats, _ = bm.batch_verify(groups, r, c=stats["c"], fan=stats["F"], dlogs=dlogs)
    print("verdicts", got, "stats", stats)
    assert got == want
    assert tuple(stats[k] for k in STAT_NAMES) == want_stats
    ref = _per_group(engine, groups)
    assert [v for i, v in enumerate(got) if i not in skip_per_group] == [v for i, v in enumerate(ref) if i not in skip_per_group]
    return got, stats


def _honest(stats):
    return stats["top_exps"] == 1 and stats["fallback_exps"] == 0 and stats["rechecked"] == 0


@pytest.mark.parametrize("c", (1, 5, 6, 11))
def test_layout_edges(engine_factory, pool, c):
    e = engine_factory(device=0)
    e._profile_batch_set_chunk(c)
    groups, dlogs = pool
    e.batch_verify(*_wire(groups[:1]), np.array([3], dtype=np.uint64))
    stats = e._profile_batch_stats()
    assert stats["c"] == c
    fan = stats["F"]
    for n in sorted({1, c, c + 1, 4 * c, 4 * c + 1, c * fan, c * fan + 1}):
        got, stats = _check(e, groups[:n], dlogs[:n], _scalars(n, seed=n))
        assert got == [1] * n and _honest(stats)
        assert stats["live"] == n and stats["chunks"] == -(-n // c)
        assert stats["product_launches"] == bm.product_launches(stats["chunks"], fan)


def test_67_groups_at_the_default_chunk(engine, pool):
    groups, dlogs = pool
    got, stats = _check(engine, groups[:67], dlogs[:67], _scalars(67))
    assert got == [1] * 67 and _honest(stats) and stats["c"] == bm.CHUNK and stats["chunks"] == -(-67 // bm.CHUNK)


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_one_invalid_group(engine, pool, where):
    n = 23
    c = engine._profile_batch_stats()["c"] or bm.CHUNK
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    groups, dlogs = _spoil(pool[0][:n], pool[1][:n], [i])
    got, stats = _check(engine, groups, dlogs, _scalars(n, seed=5))
    assert got == [0 if j == i else 1 for j in range(n)]
    first = i // c * c
    assert stats["top_exps"] == 1 and stats["fallback_exps"] == stats["chunks"] == -(-n // c) > 1
    assert stats["rechecked"] == min(n, first + c) - first        # that chunk's live groups, nothing else


def test_two_invalid_groups_in_different_chunks_and_all_invalid(engine, pool):
    n = 17
    c = engine._profile_batch_stats()["c"] or bm.CHUNK
    bad = [1, n - 1]
    assert bad[0] // c != bad[1] // c
    groups, dlogs = _spoil(pool[0][:n], pool[1][:n], bad)
    got, stats = _check(engine, groups, dlogs, _scalars(n, seed=6))
    assert got == [0 if j in bad else 1 for j in range(n)]
    assert stats["rechecked"] == c + (n - bad[1] // c * c)
    groups, dlogs = _spoil(pool[0][:n], pool[1][:n], range(n))
    got, stats = _check(engine, groups, dlogs, _scalars(n, seed=7))
    assert got == [0] * n and stats["rechecked"] == n and stats["fallback_exps"] == stats["chunks"]


def test_scalar_edges_mixed_within_a_wave(engine, pool):
    """Neighbouring lanes (k_bls_scale_g1) and lane pairs (k_bls_scale_g2) disagree on every addition: the scalars cycle through
    1, 2, 2^63, 2^64 - 1 and alternating bit patterns."""
    n = 72
    r = [SCALAR_EDGES[i % len(SCALAR_EDGES)] for i in range(n)]
    got, stats = _check(engine, pool[0][:n], pool[1][:n], r)
    assert got == [1] * n and _honest(stats)
    groups, dlogs = _spoil(pool[0][:n], pool[1][:n], [2, 40])
    got, stats = _check(engine, groups, dlogs, r)
    assert got == [0 if j in (2, 40) else 1 for j in range(n)]


def test_gt_bytes_against_the_model(engine, pool):
    """pe_profile_batch_gt for one valid and one invalid batch (three groups, edge scalars): the model's pairing route."""
    r = [1, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA]
    for bad in ((), (1,)):
        groups, dlogs = _spoil(pool[0][:3], pool[1][:3], bad)
        _check(engine, groups, dlogs, r)
        gt = engine._profile_batch_gt()
        want_v, _, want_gt = bm.batch_verify(groups, r, c=engine._profile_batch_stats()["c"])
        assert gt == want_gt
        assert (gt == (1).to_bytes(48, "big") + bytes(528)) == (not bad)
        assert want_v == [0 if j in bad else 1 for j in range(3)]


@pytest.mark.parametrize("c", (5, 1))       # the two groups in one chunk, and in two
def test_the_forgery_passes_with_known_scalars_and_is_caught_with_drawn_ones(engine_factory, pool, c):
    e = engine_factory(device=0)
    e._profile_batch_set_chunk(c)
    groups, dlogs = pool[0][:2], pool[1][:2]
    r1, r2, d = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x1234567
    D = g2.mul(d, g2.G2)
    forged = [(groups[0][0], groups[0][1], g2.add(groups[0][2], g2.mul(r2, D))),
              (groups[1][0], groups[1][1], g2.add(groups[1][2], g2.neg(g2.mul(r1, D))))]
    fd = [(dlogs[0][0], dlogs[0][1], (dlogs[0][2] + r2 * d) % R_ORDER), (dlogs[1][0], dlogs[1][1], (dlogs[1][2] - r1 * d) % R_ORDER)]
    pk, msg, sig = _wire(forged)
    # the scalars the forger knew: the top-level product decides, and it is 1 (the per-group path says 0, 0)
    got = e.batch_verify(pk, msg, sig, np.array([r1, r2], dtype=np.uint64)).tolist()
    stats = e._profile_batch_stats()
    want, want_stats, _ = bm.batch_verify(forged, [r1, r2], c=c, fan=stats["F"], dlogs=fd)
    assert got == want == [1, 1] and tuple(stats[k] for k in STAT_NAMES) == want_stats and _honest(stats)
    assert stats["chunks"] == (1 if c == 5 else 2)
    assert _per_group(e, forged) == [0, 0]
    # any other scalars, and the engine's own: caught
    got, stats = _check(e, forged, fd, [r1, r2 + 1])
    assert got == [0, 0]
    assert e.batch_verify(pk, msg, sig).tolist() == [0, 0]
    assert e._profile_batch_stats()["rechecked"] == 2
    # drawn scalars on honest input
    assert e.batch_verify(*_wire(groups)).tolist() == [1, 1] and _honest(e._profile_batch_stats())


def _outside_g2():
    """A point of the twist outside the r-torsion, as tests/test_oracle_g2_psi.py builds them."""
    import random
    rng = random.Random(8)
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = g2.f2_sqrt(g2.f2_add(g2.f2_mul(g2.f2_sqr(x), x), (4, 4)))
        if y is not None and g2.mul(R_ORDER, (x, y)) is not None:
            return (x, y)


@pytest.mark.parametrize("invalid_neighbour", (False, True))
def test_settled_groups_among_valid_ones(engine, pool, invalid_neighbour):
    n = 13
    groups, dlogs = _spoil(pool[0][:n], pool[1][:n], [12] if invalid_neighbour else [])
    pk, msg, sig = groups[1]
    groups[1] = ((pk[0], (pk[1] + 1) % P), msg, sig)                                          # key off the curve
    groups[3] = (groups[3][0], (msg[0], ((msg[1][0] + 1) % P, msg[1][1])), groups[3][2])      # message point off the curve
    groups[4] = (groups[4][0], groups[4][1], (sig[0], ((sig[1][0] + 1) % P, sig[1][1])))      # signature off the curve
    groups[6] = (groups[6][0], groups[6][1], None)                                            # identity signature
    groups[7] = (None, groups[7][1], groups[7][2])                                            # identity key
    groups[9] = (groups[9][0], groups[9][1], _outside_g2())                                   # on the curve, outside G2
    groups[11] = (None, groups[11][1], (sig[0], ((sig[1][0] + 1) % P, sig[1][1])))            # identity key AND a bad point
    want = [1] * 12 + [0 if invalid_neighbour else 1]
    for i, v in ((1, 2), (3, 2), (4, 2), (6, 0), (7, 0), (9, 0), (11, 2)):
        want[i], dlogs[i] = v, None
    # (the per-group path has no subgroup check: group 9 is outside what the two calls agree on)
    got, stats = _check(engine, groups, dlogs, _scalars(n, seed=8), skip_per_group=(9,))
    assert got == want and stats["live"] == 6
    # the neighbours keep their 1, at the price of the honest case when nothing else is wrong
    assert _honest(stats) == (not invalid_neighbour)


@pytest.fixture(scope="module")
def registry(engine_factory):
    e = engine_factory(device=0)
    n = 24
    sk = [(0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R_ORDER for i in range(n)]
    keys = np.frombuffer(b"".join(g1.to_bytes96(g1.mul(k, g1.G)) for k in sk), dtype=np.uint8).reshape(n, 96)
    e.set_validators(np.full(n, 32 * 10 ** 9, dtype=np.uint64), np.ones(n, dtype=np.uint8), keys)
    return e, sk


def test_the_indexed_call(registry):
    from pos_evolution_amd import forkchoice
    e, sk = registry
    n = len(sk)
    m = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R_ORDER
    msg = g2.to_bytes192(g2.mul(m, g2.G2))

    def sig(signers):
        return g2.to_bytes192(g2.mul(sum(sk[i] for i in signers) % R_ORDER * m % R_ORDER, g2.G2))

    everyone, odd = list(range(n)), [i for i in range(n) if i & 1]
    cases = [([5], sig([5]), 1), ([2, 9], sig([2, 9]), 1), (everyone, sig(everyone), 1), (odd, sig(odd), 1),
             ([], sig([]), 0),                                   # an empty index group
             (odd, g2.to_bytes192(None), 0),                     # an identity signature
             (everyone, sig(everyone[:-1]), 0), (odd + [0], sig(odd), 0), ([7, 8], sig([7, 8]), 1)]
    index = np.array([i for c in cases for i in c[0]], dtype=np.uint32)
    off = np.cumsum([0] + [len(c[0]) for c in cases]).astype(np.uint32)
    msgs = np.frombuffer(msg * len(cases), dtype=np.uint8).reshape(-1, 192)
    sigs = np.frombuffer(b"".join(c[1] for c in cases), dtype=np.uint8).reshape(-1, 192)
    want = [c[2] for c in cases]
    assert e.fast_aggregate_verify(index, off, msgs, sigs).tolist() == want
    assert e.batch_fast_aggregate_verify(index, off, msgs, sigs, _scalars(len(cases))).tolist() == want
    stats = e._profile_batch_stats()
    assert stats["live"] == 7 and stats["top_exps"] == 1 and stats["rechecked"] >= 2
    assert e.batch_fast_aggregate_verify(index, off, msgs, sigs).tolist() == want          # drawn scalars
    # the valid ones alone: the honest case
    keep = [i for i, c in enumerate(cases) if c[2] == 1]
    index = np.array([i for k in keep for i in cases[k][0]], dtype=np.uint32)
    off = np.cumsum([0] + [len(cases[k][0]) for k in keep]).astype(np.uint32)
    assert e.batch_fast_aggregate_verify(index, off, msgs[keep], sigs[keep]).tolist() == [1] * len(keep)
    assert _honest(e._profile_batch_stats())

    class _Store:
        engine = e
    got = forkchoice.batch_fast_aggregate_verify(_Store, [c[0] for c in cases], [msg] * len(cases), [c[1] for c in cases])
    assert got == [v == 1 for v in want]


def test_handle_states(engine_factory, pool):
    import pos_evolution_amd as pea
    import pos_evolution_amd.synth as synth
    from pos_evolution_amd import _abi

    groups, dlogs = pool[0][:6], pool[1][:6]
    pk, msg, sig = _wire(groups)
    e = engine_factory(device=0)
    # a zero scalar
    with pytest.raises(pea.EngineError) as err:
        e.batch_verify(pk, msg, sig, np.array([1, 2, 0, 4, 5, 6], dtype=np.uint64))
    assert err.value.status == -1           # PE_ERR_INVALID_ARG of include/posevo.h
    # no pubkeys loaded: the indexed call
    with pytest.raises(pea.EngineError) as err:
        e.batch_fast_aggregate_verify(np.array([0], np.uint32), np.array([0, 1], np.uint32), msg[:1], sig[:1])
    assert err.value.status == _abi.PE_ERR_STATE
    # no group at all
    empty = np.zeros((0, 192), np.uint8)
    assert e.batch_verify(np.zeros((0, 96), np.uint8), empty, empty).tolist() == []
    assert e.batch_fast_aggregate_verify(np.zeros(0, np.uint32), np.zeros(1, np.uint32), empty, empty).tolist() == []
    assert e._profile_batch_stats()["live"] == 0
    # the knob's range
    with pytest.raises(pea.EngineError):
        e._profile_batch_set_chunk(0)
    # a call inside an open pipeline completes it: the aggregate enqueued before it is done when the call returns
    n_val, n_blocks, n_comm, spe = 2048, 96, 64, 32
    tree = synth.random_tree(n_blocks, 1, "branchy")
    e.store_init(0, 0, tree.roots[0].tobytes())
    for i in range(1, n_blocks):
        e.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]))
    e.set_validators(synth.balances(n_val, 1, mixed=True), synth.validator_flags(n_val, 1, inactive_frac=0.01),
                     synth.registry_points(e, n_val))
    epoch = int(tree.slot.max()) // spe + 1
    comm = synth.random_committees(n_val, n_comm, 1)
    e.set_committees(epoch, comm.offsets, comm.members)
    e.on_tick((epoch + 1) * spe * 12)
    atts, arena, _ = synth.epoch_attestations(comm, tree, epoch, spe, seed=1, density=0.9, parts=3,
                                              source=(0, tree.roots[0].tobytes()))
    with e.pipeline():
        agg = e.aggregate(packed=(atts, arena), want_aggregate_pubkeys=True)
        assert e.batch_verify(pk, msg, sig, _scalars(6)).tolist() == [1] * 6
    assert agg["n_groups"] == n_comm
    # two calls in a row on one handle, the second after a fallback
    bad_groups, _ = _spoil(groups, dlogs, [4])
    assert e.batch_verify(*_wire(bad_groups)).tolist() == [1, 1, 1, 1, 0, 1]
    assert e.batch_verify(pk, msg, sig).tolist() == [1] * 6 and _honest(e._profile_batch_stats())
    # under pe_dist_init_custom: PE_ERR_STATE
    d = engine_factory(device=0)
    d.dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    with pytest.raises(pea.EngineError) as err:
        d.batch_verify(pk, msg, sig)
    assert err.value.status == _abi.PE_ERR_STATE
    d.set_validators(np.full(4, 32 * 10 ** 9, dtype=np.uint64), np.ones(4, dtype=np.uint8), synth.registry_points(d, 4))
    with pytest.raises(pea.EngineError) as err:
        d.batch_fast_aggregate_verify(np.array([0], np.uint32), np.array([0, 1], np.uint32), msg[:1], sig[:1])
    assert err.value.status == _abi.PE_ERR_STATE
