"""GPU: pe_pairing_check / pe_fast_aggregate_verify.  The verdicts are tested BY CONSTRUCTION -- for pairs (a_i G1, b_i G2) the
product of pairings is 1 iff sum a_i b_i == 0 (mod r) -- so no pairing is computed in Python here; the only Python pairing
values are the committed fixtures of tests/golden/pairing_vectors.json (GT parity).

Layout edges (fp12.h / bls_kernels.hip): a group is a 16-lane row whose six lane pairs work the point steps of pairs k, k + 6,
...: group sizes 6 | 7 and 12 | 13 are where a second and a third round begin.  Four groups share a wave = a workgroup:
n_groups 3 | 4 | 5 are one below, at and above it."""
import json
import os

import numpy as np
import pytest

from oracle import g1, g2
from oracle.g1 import R_ORDER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SIZES = (1, 2, 3, 5, 6, 7, 12, 13)       # 6 | 7, 12 | 13: the rounds of the lane layout
N_GROUPS = (1, 3, 4, 5, 67)                    # 3 | 4 | 5: groups per wave = per workgroup is 4
FULL = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R_ORDER


def _enc(pairs):
    a = np.frombuffer(b"".join(g1.to_bytes96(p) for p, _ in pairs), dtype=np.uint8).reshape(-1, 96)
    b = np.frombuffer(b"".join(g2.to_bytes192(q) for _, q in pairs), dtype=np.uint8).reshape(-1, 192)
    return a.copy(), b.copy()


def _points(a, b):
    return [(g1.mul(x, g1.G) if x else None, g2.mul(y, g2.G2) if y else None) for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def pool():
    """[(pairs, verdict)]: for every size a valid group and its twin with one scalar changed by 1, alternating."""
    rng = np.random.default_rng(381)
    out = []
    for n in GROUP_SIZES:
        if n == 1:   # valid only through an infinity
            out.append(([(None, g2.mul(FULL, g2.G2))], 1))
            out.append(([(g1.G, g2.mul(R_ORDER - 1, g2.G2))], 0))
            continue
        a = [int.from_bytes(rng.bytes(32), "big") % R_ORDER or 1 for _ in range(n)]
        b = [int.from_bytes(rng.bytes(32), "big") % R_ORDER or 1 for _ in range(n)]
        a[0], b[0] = 1, R_ORDER - 1                         # the scalars 1 and r - 1; the others are full-width
        if n > 2:
            a[1], b[1] = R_ORDER - 1, FULL
        s = sum(x * y for x, y in zip(a[:-1], b[:-1])) % R_ORDER
        b[-1] = -s * pow(a[-1], -1, R_ORDER) % R_ORDER
        assert sum(x * y for x, y in zip(a, b)) % R_ORDER == 0
        out.append((_points(a, b), 1))
        b2 = list(b)
        b2[n // 2] = (b2[n // 2] + 1) % R_ORDER
        out.append((_points(a, b2), 0))
    return out


@pytest.fixture(scope="module")
def engine(engine_factory):
    return engine_factory(device=0)


def _call(groups):
    pairs = [p for g, _ in groups for p in g]
    off = np.cumsum([0] + [len(g) for g, _ in groups]).astype(np.uint32)
    a, b = _enc(pairs) if pairs else (np.zeros((0, 96), np.uint8), np.zeros((0, 192), np.uint8))
    return a, b, off, np.array([v for _, v in groups], dtype=np.int32)


@pytest.mark.parametrize("n_groups", N_GROUPS)
def test_verdicts_by_construction(engine, pool, n_groups):
    # valid and invalid groups interleaved; each call starts at another group of the pool, so every size meets every row
    groups = [pool[(i + 3 * n_groups) % len(pool)] for i in range(n_groups)]
    if n_groups == 67:
        groups = [pool[i % len(pool)] for i in range(n_groups)]      # the whole pool, four times over
    a, b, off, want = _call(groups)
    got = engine.pairing_check(a, b, off)
    assert got.tolist() == want.tolist()


def test_every_pool_group_alone_in_its_wave(engine, pool):
    for grp in pool:
        a, b, off, want = _call([grp])
        assert engine.pairing_check(a, b, off).tolist() == want.tolist(), len(grp[0])


def test_fast_aggregate_verify(engine_factory):
    e = engine_factory(device=0)
    n = 64
    sk = [(0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R_ORDER for i in range(n)]
    keys = np.frombuffer(b"".join(g1.to_bytes96(g1.mul(k, g1.G)) for k in sk), dtype=np.uint8).reshape(n, 96)
    e.set_validators(np.full(n, 32 * 10 ** 9, dtype=np.uint64), np.ones(n, dtype=np.uint8), keys)
    m = FULL
    msg = g2.to_bytes192(g2.mul(m, g2.G2))

    def sig(signers):
        return g2.to_bytes192(g2.mul(sum(sk[i] for i in signers) % R_ORDER * m % R_ORDER, g2.G2))

    everyone = list(range(n))
    odd = [i for i in range(n) if i & 1]
    cases = [
        (everyone, sig(everyone), 1),                       # a full committee
        (everyone, sig(everyone[:-1]), 0),                  # one signer missing from the signature
        (odd + [0], sig(odd), 0),                           # one extra index
        ([17], sig([17]), 1),                               # a committee of one
        ([], sig([]), 0),                                   # FastAggregateVerify refuses n = 0 (the identity signature)
        (odd, g2.to_bytes192(None), 0),                     # an identity signature
        (odd, sig(odd), 1),
    ]
    index = np.array([i for c in cases for i in c[0]], dtype=np.uint32)
    off = np.cumsum([0] + [len(c[0]) for c in cases]).astype(np.uint32)
    msgs = np.frombuffer(msg * len(cases), dtype=np.uint8).reshape(-1, 192)
    sigs = np.frombuffer(b"".join(c[1] for c in cases), dtype=np.uint8).reshape(-1, 192)
    got = e.fast_aggregate_verify(index, off, msgs, sigs)
    assert got.tolist() == [c[2] for c in cases]
    # the forkchoice-level call: the boolean a caller may pass on as signature_valid
    from pos_evolution_amd import forkchoice

    class _Store:
        engine = e
    assert forkchoice.fast_aggregate_verify(_Store, odd, msg, sig(odd)) is True
    assert forkchoice.fast_aggregate_verify(_Store, odd, msg, sig(everyone)) is False


def test_gt_parity_with_the_committed_vectors(engine):
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_vectors.json")))["groups"]
    a = np.frombuffer(bytes.fromhex("".join(h for g in vec for h in g["g1"])), dtype=np.uint8).reshape(-1, 96)
    b = np.frombuffer(bytes.fromhex("".join(h for g in vec for h in g["g2"])), dtype=np.uint8).reshape(-1, 192)
    off = np.cumsum([0] + [len(g["g1"]) for g in vec]).astype(np.uint32)
    got = engine._profile_pairing_gt(a, b, off)
    for i, g in enumerate(vec):
        assert got[i].tobytes().hex() == g["gt"], g["name"]


def test_bad_points_and_infinity(engine, pool):
    valid2, invalid2 = pool[2], pool[3]
    (p0, q0), (p1, q1) = valid2[0]
    off_g1 = (p0[0], (p0[1] + 1) % g1.P)
    off_g2 = (q1[0], ((q1[1][0] + 1) % g1.P, q1[1][1]))
    groups = [valid2, ([(off_g1, q0), (p1, q1)], 2), invalid2, ([(p0, q0), (p1, off_g2)], 2), ([], 1),
              ([(None, None), (None, q0), (p0, None)], 1), valid2]
    a, b, off, want = _call(groups)
    assert engine.pairing_check(a, b, off).tolist() == want.tolist()
    assert engine.pairing_check(np.zeros((0, 96), np.uint8), np.zeros((0, 192), np.uint8), np.zeros(3, np.uint32)).tolist() == [1, 1]


def test_handle_states(engine_factory, pool):
    import pos_evolution_amd as pea
    import pos_evolution_amd.synth as synth
    from pos_evolution_amd import _abi

    a, b, off, want = _call(pool[:6])
    # a call inside an open pipeline completes it: the aggregate enqueued before it is done when the call returns
    n_val, n_blocks, n_comm, spe = 2048, 96, 64, 32
    e = engine_factory(device=0)
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
        got = e.pairing_check(a, b, off)
        assert got.tolist() == want.tolist()
    assert agg["n_groups"] == n_comm
    # two calls in a row on one handle
    assert e.pairing_check(a, b, off).tolist() == want.tolist()
    assert e.pairing_check(a, b, off).tolist() == want.tolist()
    # under pe_dist_init_custom: PE_ERR_STATE
    d = engine_factory(device=0)
    d.dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    with pytest.raises(pea.EngineError) as err:
        d.pairing_check(a, b, off)
    assert err.value.status == _abi.PE_ERR_STATE
    d.set_validators(np.full(4, 32 * 10 ** 9, dtype=np.uint64), np.ones(4, dtype=np.uint8), synth.registry_points(d, 4))
    with pytest.raises(pea.EngineError) as err:
        d.fast_aggregate_verify(np.array([0], np.uint32), np.array([0, 1], np.uint32), b[:1], b[:1])
    assert err.value.status == _abi.PE_ERR_STATE
