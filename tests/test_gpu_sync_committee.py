"""-m gpu: sync committees on the GPU -- pe_sync_committee_compute / _set / _get / _rotate and pe_process_sync_aggregate --
against the model of tests/sync_committee_model.py (tests/test_sync_committee_model.py ties that to the proposer model and
to cases worked by hand).  Shapes: the `position // 256` and `i % total` edges of the walk (1, 2, 3, 255, 256, 257, 1000
active validators), committee sizes around a wave (1, 32, 63, 64, 65, 512), a last acceptance on the last lane of a candidate
batch and on the first lane of the next.  Registry keys are sk_v = A + v B (synth.registry_points), so every aggregate key and
signature has a closed form."""
import functools
import hashlib

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import g1, g2
from pos_evolution_amd import _abi
from pos_evolution_amd.engine import SYNC_APPLY, SYNC_CURRENT, SYNC_NEXT, SYNC_VERIFY
from tests import hash_to_curve_model as hm
from tests import sync_committee_model as M

pytestmark = pytest.mark.gpu
ETH = 10**9
MAX_EFF = 32 * ETH
FAR = 2**64 - 1
BATCH = 16384                       # kernels.h: SYNC_SAMPLE_BATCH
A, B = 0x1234567, 0x89ABCDE         # sk_v = A + v B: synth.registry_points' progression
R = g1.R_ORDER
INFINITY_KEY = b"\xc0" + bytes(47)
UNDECODABLE = bytes([0x9F]) + b"\xff" * 95   # compressed, x.c1 >= p


def _seed(tag, k=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), k)).digest()


def _balances(kind, n, rng):
    if kind == "mixed":
        return rng.choice(np.array([0, 0, 1, 7, 16, 31, 32], dtype=np.uint64), size=n) * np.uint64(ETH)
    return np.full(n, (32 if kind == "full" else 1) * ETH, dtype=np.uint64)


_POINTS = {}


def _engine(engine_factory, bal, points=None):
    """A handle whose registry holds the progression's pubkeys (or `points`) and `bal` as effective balances."""
    n = len(bal)
    e = engine_factory()
    if points is None:
        if n not in _POINTS:
            _POINTS[n] = synth.registry_points(e, n, A, B)
        points = _POINTS[n]
    e.set_validators(np.asarray(bal, dtype=np.uint64), np.ones(n, dtype=np.uint8), points)
    return e


def _key_of(members):
    """eth_aggregate_pubkeys over the progression, with multiplicity."""
    idx = [int(v) for v in members]
    return g1.compress(g1.mul((len(idx) * A + sum(idx) * B) % R, g1.G))


def _snapshot(e):
    bal = e.state_get_balances()
    return (e.sync_committee_get(SYNC_CURRENT), e.sync_committee_get(SYNC_NEXT), bal[0].tobytes() if bal[3] else None)


def _same(a, b):
    def flat(s):
        return [None if c is None else (c[0].tobytes(), c[1]) for c in s[:2]] + [s[2]]
    return flat(a) == flat(b)


def _status(fn):
    with pytest.raises(pea.EngineError) as err:
        fn()
    return err.value.status


def _active(e, form, n_val, n_active, rng):
    """-> (the engine's argument, the index list the model walks)."""
    if form == "int":
        return n_active, list(range(n_active))
    chosen = np.sort(rng.choice(n_val, size=n_active, replace=False)).astype(np.uint32)
    if form == "host":
        return chosen, [int(v) for v in chosen]
    act = np.full(n_val, FAR, dtype=np.uint64)
    act[chosen] = 0
    e.registry_set_epochs(act, np.full(n_val, FAR, dtype=np.uint64))
    assert e.active_set(3)[0] == n_active
    return pea.ACTIVE_RESIDENT, [int(v) for v in chosen]


def _check_compute(e, seed, active, indices, bal, rounds, size, refusal=True, max_eff=MAX_EFF):
    """The engine's committee against the model's, its key, member 0 against compute_proposers, and max_tries at and one
    below the model's tries.  -> (members, tries)"""
    want, want_tries = M.next_sync_committee_indices(indices, bal, seed, rounds, max_eff, size)
    got, key, tries = e.sync_committee_compute(seed, active, rounds, max_eff, size)
    assert got.tolist() == want and tries == want_tries
    assert key == _key_of(want)
    nxt = e.sync_committee_get(SYNC_NEXT)
    assert nxt[0].tolist() == want and nxt[1] == key
    prop, prop_tries = e.compute_proposers([seed], active, rounds, max_eff, 1 << 20)
    first = M.next_sync_committee_indices(indices, bal, seed, rounds, max_eff, 1)[1] - 1   # the i of member 0
    assert (int(prop[0]), int(prop_tries[0])) == (want[0], first)
    if refusal:
        before = _snapshot(e)
        again, key2, tries2 = e.sync_committee_compute(seed, active, rounds, max_eff, size, max_tries=want_tries)
        assert (again.tolist(), key2, tries2) == (want, key, want_tries)
        if want_tries > 1:
            idx = np.full(_abi.PE_SYNC_COMMITTEE_MAX, 0xABABABAB, dtype=np.uint32)
            out_key = np.full(48, 0xAB, dtype=np.uint8)
            out_tries = np.zeros(1, dtype=np.uint32)
            sd = np.frombuffer(seed, dtype=np.uint8).copy()
            if isinstance(active, np.ndarray):
                act_ptr, n_act = active.ctypes.data, active.size
            else:
                act_ptr, n_act = (_abi.PE_ACTIVE_RESIDENT, len(indices)) if active is pea.ACTIVE_RESIDENT else (None, active)
            rc = e._lib.pe_sync_committee_compute(e._h, sd.ctypes.data, act_ptr, n_act, rounds, max_eff, size, want_tries - 1,
                                                  idx.ctypes.data, out_key.ctypes.data, out_tries.ctypes.data)
            assert rc == _abi.PE_ERR_CAPACITY and int(out_tries[0]) == want_tries - 1
            assert (idx == 0xABABABAB).all() and (out_key == 0xAB).all()
            assert _same(before, _snapshot(e))
    return want, want_tries


# ---------------------------------------------------------------- sampling
# every n_active sees every value of {size, rounds, active-set form, balances}; the product is covered across the sizes.
# 90 rounds go with full balances: there the model walks `size` candidates, not tens of thousands.
CONFIGS = [(1, 10, "host", "mixed"), (32, 90, "int", "full"), (63, 10, "resident", "one"), (64, 90, "host", "full"),
           (65, 10, "int", "mixed"), (512, 10, "resident", "one")]


@pytest.mark.parametrize("n_active", [1, 2, 3, 255, 256, 257, 1000])
def test_sampling_vs_model(engine_factory, n_active):
    n_val = n_active + 37
    rng = np.random.default_rng(n_active)
    seen_duplicates = False
    for c, (size, rounds, form, kind) in enumerate(CONFIGS):
        bal = _balances(kind, n_val, rng)
        e = _engine(engine_factory, bal)
        active, indices = _active(e, form, n_val, n_active, rng)
        if kind == "mixed":   # at least one candidate of the active set can be accepted
            bal[indices[0]] = 32 * ETH
            e.state_set_validators(bal, np.ones(n_val, dtype=np.uint8))
        members, _ = _check_compute(e, _seed(f"s{n_active}", c), active, indices, bal, rounds, size, refusal=c in (0, 2, 5))
        seen_duplicates |= len(set(members)) < len(members)
    assert seen_duplicates or n_active >= 512


def test_sampling_cases_cover_duplicates_and_the_batch_edges(engine_factory):
    """From the model's own tries: a committee with duplicates, one that needs a second candidate batch, one whose last
    acceptance is the last lane of the first batch and one on the first lane of the second (seeds found with the model at
    10 rounds: 512 members at 1 ETH against 32 take 16 384 +- 700 candidates)."""
    n = 1000
    bal = _balances("one", n, None)
    e = _engine(engine_factory, bal)
    tries_seen = {}
    for tag in (22, 838, 0):
        _, tries_seen[tag] = _check_compute(e, _seed("sync-edge", tag), n, list(range(n)), bal, 10, 512)
    assert tries_seen[22] == BATCH            # i = 16383: the last lane of the first batch
    assert tries_seen[838] == BATCH + 1       # i = 16384: the first lane of the second
    assert any(t > BATCH for t in tries_seen.values()), tries_seen
    three = _balances("full", 3, None)
    members, tries = _check_compute(_engine(engine_factory, three), _seed("dup"), 3, [0, 1, 2], three, 10, 32)
    assert tries == 32 and len(set(members)) == 3   # total < size: every validator several times


# ---------------------------------------------------------------- the aggregate key, the two resident committees
def test_aggregate_key_multiplicity_and_identity(engine_factory):
    bal = _balances("full", 9, None)
    e = _engine(engine_factory, bal)
    # one active validator: 512 times the same key -- a doubling at every level of the sum
    got, key, tries = e.sync_committee_compute(_seed("solo"), np.array([5], dtype=np.uint32), 90, MAX_EFF, 512)
    assert got.tolist() == [5] * 512 and tries == 512
    assert key == g1.compress(g1.mul(512 * (A + 5 * B) % R, g1.G)) == _key_of([5] * 512)
    e.sync_committee_set(SYNC_CURRENT, [2, 7, 2, 2])
    assert e.sync_committee_get(SYNC_CURRENT)[1] == _key_of([2, 7, 2, 2])
    # a key and its negation: the sum is the identity, compressed infinity
    p = g1.mul(0xC0FFEE, g1.G)
    pts = np.frombuffer(g1.to_bytes96(p) + g1.to_bytes96(g1.neg(p)), dtype=np.uint8).reshape(2, 96).copy()
    e2 = _engine(engine_factory, _balances("full", 2, None), pts)
    e2.sync_committee_set(SYNC_NEXT, [0, 1])
    assert e2.sync_committee_get(SYNC_NEXT)[1] == INFINITY_KEY
    e2.sync_committee_set(SYNC_NEXT, [0, 1, 0])
    assert e2.sync_committee_get(SYNC_NEXT)[1] == g1.compress(p)


def test_set_get_rotate_and_lifetime(engine_factory):
    n = 40
    bal = _balances("full", n, None)
    e = _engine(engine_factory, bal)
    assert e.sync_committee_get(SYNC_CURRENT) is None and e.sync_committee_get(SYNC_NEXT) is None
    assert _status(e.sync_committee_rotate) == _abi.PE_ERR_STATE
    cur, nxt = [3, 3, 39, 0], list(range(1, 34))
    e.sync_committee_set(SYNC_CURRENT, cur)
    e.sync_committee_set(SYNC_NEXT, nxt)
    before = _snapshot(e)
    assert _status(lambda: e.sync_committee_set(SYNC_NEXT, [1, n])) == _abi.PE_ERR_INVALID_ARG     # index < n
    assert _status(lambda: e.sync_committee_set(SYNC_NEXT, [])) == _abi.PE_ERR_INVALID_ARG
    assert _status(lambda: e.sync_committee_set(SYNC_NEXT, [0] * 513)) == _abi.PE_ERR_INVALID_ARG
    assert _status(lambda: e.sync_committee_set(2, [0])) == _abi.PE_ERR_INVALID_ARG
    # ... and the sampling's own argument refusals: size 0 and 513, an empty active set, a round count beyond a uint8, an
    # active index outside the registry
    for size, active, rounds in ((0, n, 10), (513, n, 10), (4, 0, 10), (4, n, 256), (4, np.array([1, n], dtype=np.uint32), 10),
                                 (4, n + 1, 10)):
        assert _status(lambda: e.sync_committee_compute(_seed("r"), active, rounds, MAX_EFF, size)) == _abi.PE_ERR_INVALID_ARG
    assert _status(lambda: e.sync_committee_compute(_seed("r"), pea.ACTIVE_RESIDENT, 10, MAX_EFF, 4)) == _abi.PE_ERR_STATE
    assert _same(before, _snapshot(e))
    got = e.sync_committee_get(SYNC_CURRENT)
    assert got[0].tolist() == cur and got[1] == _key_of(cur)
    # checkpoint / resume: what _get returns, handed to _set on another handle, gives the same pair
    e2 = _engine(engine_factory, bal)
    for which in (SYNC_CURRENT, SYNC_NEXT):
        e2.sync_committee_set(which, e.sync_committee_get(which)[0])
    assert _same(_snapshot(e), _snapshot(e2))
    e.sync_committee_rotate()
    got = e.sync_committee_get(SYNC_CURRENT)
    assert got[0].tolist() == nxt and got[1] == _key_of(nxt) and e.sync_committee_get(SYNC_NEXT) is None
    assert _status(e.sync_committee_rotate) == _abi.PE_ERR_STATE
    # lifetime: a new store, other pubkeys and another registry size drop both; a changed balance does not
    e.sync_committee_set(SYNC_NEXT, cur)
    e.set_balances(bal, np.ones(n, dtype=np.uint8))
    assert e.sync_committee_get(SYNC_CURRENT) is not None and e.sync_committee_get(SYNC_NEXT) is not None
    e.store_init(0, 0, bytes(32))
    assert e.sync_committee_get(SYNC_CURRENT) is None and e.sync_committee_get(SYNC_NEXT) is None
    e.sync_committee_set(SYNC_CURRENT, cur)
    e.set_validators(bal, np.ones(n, dtype=np.uint8), _POINTS[n])
    assert e.sync_committee_get(SYNC_CURRENT) is None
    e.sync_committee_set(SYNC_CURRENT, cur)
    e.set_pubkeys_compressed(np.frombuffer(b"".join(g1.compress(g1.from_bytes96(bytes(r))) for r in _POINTS[n]), dtype=np.uint8))
    assert e.sync_committee_get(SYNC_CURRENT) is None
    e.sync_committee_set(SYNC_CURRENT, cur)
    e.set_validators(bal[:30], np.ones(30, dtype=np.uint8))
    assert e.sync_committee_get(SYNC_CURRENT) is None
    # without pubkeys there is no aggregate key to make
    e3 = engine_factory()
    e3.set_validators(bal, np.ones(n, dtype=np.uint8))
    assert _status(lambda: e3.sync_committee_set(SYNC_CURRENT, cur)) == _abi.PE_ERR_STATE
    assert _status(lambda: e3.sync_committee_compute(_seed("x"), n, 10, MAX_EFF, 4)) == _abi.PE_ERR_STATE


def test_committees_survive_deposits(engine_factory):
    """pe_process_deposits appends a validator: every resident array moves, both committees stay -- indices, keys -- and the
    next aggregate verifies over the moved pubkeys and pays onto the grown balances, the new validator as its proposer."""
    from tests.test_gpu_deposits import MSG_SCALAR, Rig, dep, registry
    n = 40
    rig = Rig(engine_factory, registry(n, 3), points=lambda eng: synth.registry_points(eng, n, A, B))
    e = rig.e
    cur, nxt = [3, 3, 39, 0, 17], list(range(1, 34))
    e.sync_committee_set(SYNC_CURRENT, cur)
    e.sync_committee_set(SYNC_NEXT, nxt)
    before = _snapshot(e)
    sk = 0x1F2E3D4C5B6A7988
    new_key = dep(g1.compress(g1.mul(sk, g1.G)), g2.compress(g2.mul(sk * MSG_SCALAR % R, g2.G2)))
    res = rig.run([new_key], [True], [g2.to_bytes192(g2.mul(MSG_SCALAR, g2.G2))])
    assert res["n_appended"] == 1 and e.num_validators == n + 1
    after = _snapshot(e)
    assert _same(before[:2] + (None,), after[:2] + (None,))
    assert after[0][1] == _key_of(cur) and after[1][1] == _key_of(nxt)
    total = 32 * ETH * 1000
    pr, qr = M.reward_scalars(total, len(cur))
    aggs = [_agg(cur, [0, 2, 3], proposer=n), _agg(cur, [1, 4], proposer=n)]
    want = [int(b) for b in e.state_get_balances()[0]]
    assert len(want) == n + 1
    st = M.process_sync_aggregates(want, cur, [(a["bits"], a["proposer_index"]) for a in aggs], pr, qr)
    got = e.process_sync_aggregate(aggs, total, SYNC_VERIFY | SYNC_APPLY)
    assert got["verdict"].tolist() == [1, 1] and got["applied"] == 1 and {k: got[k] for k in st} == st
    assert e.state_get_balances()[0].tolist() == want and want[n] == 32 * ETH + 5 * qr
    e.sync_committee_rotate()                                   # and the next committee is still the one that was set
    assert e.sync_committee_get(SYNC_CURRENT)[0].tolist() == nxt


# ---------------------------------------------------------------- verdicts
@functools.lru_cache(maxsize=None)
def _point(message: bytes):
    return hm.hash_to_g2(message, hm.ETH2_DST)


@functools.lru_cache(maxsize=None)
def _signature(message: bytes, sk: int) -> bytes:
    """sk * H(message), compressed"""
    return g2.compress(hm.curve_mul(sk % R, _point(message)))


def _bits(positions):
    b = bytearray(64)
    for p in positions:
        b[p // 8] |= 1 << (p % 8)
    return bytes(b)


ROOT, DOMAIN = hashlib.sha256(b"block").digest(), bytes([7, 0, 0, 0]) + hashlib.sha256(b"fork").digest()[:28]


def _agg(members, positions, proposer=0, root=ROOT, domain=DOMAIN, signature=None, signed_root=None, signed_domain=None):
    """An aggregate whose participants (the members at `positions`) signed (signed_root, signed_domain), default its own."""
    if signature is None:
        sk = sum(A + int(members[p]) * B for p in positions)
        message = M.signing_root(signed_root or root, signed_domain or domain)
        signature = _signature(message, sk) if positions else M.INFINITY_SIGNATURE
    return {"bits": _bits(positions), "signature": signature, "block_root": root, "domain": domain, "proposer_index": proposer}


def _committee(size, n_val):
    """`size` members out of n_val validators with a duplicate pair at positions 0 and 2 (size >= 3)."""
    rng = np.random.default_rng(size)
    members = [int(v) for v in rng.integers(0, n_val, size=size)]
    if size >= 3:
        members[2] = members[0]
    return members


@pytest.mark.parametrize("size", [1, 65, 512])
def test_verdicts(engine_factory, size):
    n_val = 600
    e = _engine(engine_factory, _balances("full", n_val, None))
    members = _committee(size, n_val)
    e.sync_committee_set(SYNC_CURRENT, members)
    everyone = list(range(size))
    other_root, other_domain = hashlib.sha256(b"other").digest(), bytes([8]) + DOMAIN[1:]
    cases = [("everyone", _agg(members, everyone), 1, 0),
             ("one participant", _agg(members, [size - 1]), 1, 0),
             ("nobody, the infinity signature", _agg(members, []), 1, 0),
             ("nobody, another signature", _agg(members, [], signature=_signature(M.signing_root(ROOT, DOMAIN), A)), 0, 0),
             ("a participant, the infinity signature", _agg(members, [0], signature=M.INFINITY_SIGNATURE), 0, 0),
             ("wrong root", _agg(members, everyone, signed_root=other_root), 0, 0),
             ("wrong domain", _agg(members, everyone, signed_domain=other_domain), 0, 0),
             ("an undecodable signature", _agg(members, everyone, signature=UNDECODABLE), 0, 1)]
    if size >= 3:
        cases.append(("a duplicate member participating twice", _agg(members, [0, 2]), 1, 0))
        cases.append(("a duplicate member, key counted once", _agg(members, [0, 2], signature=_signature(
            M.signing_root(ROOT, DOMAIN), A + members[0] * B)), 0, 0))
        flipped = dict(_agg(members, everyone))
        flipped["bits"] = _bits(everyone[:-1])
        cases.append(("one flipped bit", flipped, 0, 0))
    for name, agg, want, want_status in cases:          # n = 1
        res = e.process_sync_aggregate([agg], 32 * ETH * n_val, SYNC_VERIFY)
        assert (int(res["verdict"][0]), int(res["sig_status"][0])) == (want, want_status), name
        assert res["applied"] == 0 and res["n_participants"] == len(M.participants(members, agg["bits"]))
    for start in range(0, len(cases) - 2, 3):           # n = 3, mixed outcomes in one call
        trio = cases[start:start + 3]
        res = e.process_sync_aggregate([c[1] for c in trio], 32 * ETH * n_val, SYNC_VERIFY)
        assert res["verdict"].tolist() == [c[2] for c in trio] and res["sig_status"].tolist() == [c[3] for c in trio]


def test_identity_aggregate_key_is_refused(engine_factory):
    p = g1.mul(0xC0FFEE, g1.G)
    pts = np.frombuffer(g1.to_bytes96(p) + g1.to_bytes96(g1.neg(p)), dtype=np.uint8).reshape(2, 96).copy()
    e = _engine(engine_factory, _balances("full", 2, None), pts)
    e.sync_committee_set(SYNC_CURRENT, [0, 1])
    message = M.signing_root(ROOT, DOMAIN)
    both = {"bits": _bits([0, 1]), "signature": _signature(message, 5), "block_root": ROOT, "domain": DOMAIN, "proposer_index": 0}
    alone = dict(both, bits=_bits([0]), signature=_signature(message, 0xC0FFEE))
    res = e.process_sync_aggregate([both, alone, dict(both, signature=M.INFINITY_SIGNATURE)], 64 * ETH, SYNC_VERIFY)
    assert res["verdict"].tolist() == [0, 1, 0]


# ---------------------------------------------------------------- rewards
def _run_rewards(e, members, bal, aggs, total, flags=SYNC_APPLY, size_for_scalars=None):
    """One call against the model: the whole balance array and the stats.  -> the model's balances"""
    pr, qr = M.reward_scalars(total, size_for_scalars or len(members))
    want = [int(b) for b in bal]
    st = M.process_sync_aggregates(want, members, [(a["bits"], a["proposer_index"]) for a in aggs], pr, qr)
    e.state_set_balances(np.asarray(bal, dtype=np.uint64))
    res = e.process_sync_aggregate(aggs, total, flags)
    got = e.state_get_balances()[0]
    assert got.tolist() == want
    assert (res["participant_reward"], res["proposer_reward"], res["applied"]) == (pr, qr, 1)
    assert {k: res[k] for k in st} == st
    return want


def _plain(members, positions, proposer):
    return {"bits": _bits(positions), "signature": M.INFINITY_SIGNATURE, "block_root": ROOT, "domain": DOMAIN, "proposer_index": proposer}


def test_rewards_hand_cases(engine_factory):
    n_val = 12
    total = 32 * ETH * 1_000_000
    e = _engine(engine_factory, _balances("full", n_val, None))
    pr, _ = M.reward_scalars(total, 2)
    e.sync_committee_set(SYNC_CURRENT, [5, 5])
    for start in (0, pr - 1):          # a member twice, bits (1, 0) and (0, 1), from an empty and a nearly empty balance
        for positions in ([0], [1]):
            bal = [10**6] * n_val
            bal[5] = start
            _run_rewards(e, [5, 5], bal, [_plain([5, 5], positions, 9)], total)
    for members in ([3, 1, 2], [1, 2, 3]):   # the proposer is an absent member at an earlier / a later position
        e.sync_committee_set(SYNC_CURRENT, members)
        positions = [p for p, v in enumerate(members) if v != 3]
        want = _run_rewards(e, members, [0] * n_val, [_plain(members, positions, 3)], total)
        assert want[3] == (2 * M.reward_scalars(total, 3)[1] if members[0] == 3 else 0)
        _run_rewards(e, members, [0] * n_val, [_plain(members, positions, 3)] * 3, total)      # n = 3, the same proposer
    _run_rewards(e, [1, 2, 3], [7] * n_val, [_plain([1, 2, 3], [0, 2], 11), _plain([1, 2, 3], [], 11), _plain([1, 2, 3], [1], 10)],
                 total)                # proposers outside the committee, one of them twice


@pytest.mark.parametrize("size,n", [(1, 1), (65, 3), (512, 1), (512, 3)])
def test_rewards_vs_model(engine_factory, size, n):
    n_val = 700
    rng = np.random.default_rng(100 * size + n)
    total = int(rng.integers(20_000, 900_000)) * 32 * ETH
    e = _engine(engine_factory, _balances("full", n_val, None))
    members = _committee(size, n_val)
    e.sync_committee_set(SYNC_CURRENT, members)
    pr, _ = M.reward_scalars(total, size)
    bal = rng.choice(np.array([0, 1, pr - 1, pr, pr + 1, 3 * pr, 32 * ETH], dtype=np.uint64), size=n_val)
    aggs = []
    for b in range(n):
        positions = [p for p in range(size) if rng.random() < 0.6]
        proposer = int(members[int(rng.integers(0, size))]) if b % 2 else int(rng.integers(0, n_val))
        aggs.append(_plain(members, positions, proposer))
    want = _run_rewards(e, members, bal, aggs, total)
    outside = np.setdiff1d(np.arange(n_val), np.array(members + [a["proposer_index"] for a in aggs]))
    assert [want[v] for v in outside] == [int(bal[v]) for v in outside]       # nobody outside the committee is touched
    # process_effective_balance_updates then reads what the call left, where it lies
    n_changed, eff = e.effective_balance_updates(pea.BALANCES_RESIDENT, MAX_EFF)
    from tests import epoch_model
    new, changed = epoch_model.effective_balance_updates(np.array(want, dtype=np.uint64), np.full(n_val, 32 * ETH, dtype=np.uint64),
                                                         ETH, 4, 1, 5, MAX_EFF)
    assert n_changed == changed and eff.tolist() == new.tolist()


def test_verify_and_apply_together(engine_factory):
    n_val, size = 80, 5
    total = 32 * ETH * 50_000
    e = _engine(engine_factory, _balances("full", n_val, None))
    members = _committee(size, n_val)
    e.sync_committee_set(SYNC_CURRENT, members)
    good = [_agg(members, [0, 1, 2, 4], proposer=members[3]), _agg(members, [], proposer=1), _agg(members, [3], proposer=2)]
    bal = [5 * ETH] * n_val
    want = _run_rewards(e, members, bal, good, total, SYNC_VERIFY | SYNC_APPLY)
    assert want != bal
    # one invalid aggregate among them: verdicts say which, and no balance moves
    bad = [good[0], dict(good[2], bits=_bits([4])), good[1]]
    e.state_set_balances(np.asarray(bal, dtype=np.uint64))
    before = _snapshot(e)
    res = e.process_sync_aggregate(bad, total, SYNC_VERIFY | SYNC_APPLY)
    assert res["verdict"].tolist() == [1, 0, 1] and res["applied"] == 0
    assert (res["credited"], res["debited"], res["n_saturated"]) == (0, 0, 0)
    assert _same(before, _snapshot(e))


# ---------------------------------------------------------------- every refusal changes nothing
def test_errors_change_nothing(engine_factory):
    n_val = 50
    total = 32 * ETH * n_val
    bal = _balances("full", n_val, None)
    e = _engine(engine_factory, bal)
    members = [4, 9, 4, 30, 2]
    ok = _plain(members, [0, 1], 7)
    assert _status(lambda: e.process_sync_aggregate([ok], total, SYNC_APPLY)) == _abi.PE_ERR_STATE          # no current committee
    e.sync_committee_set(SYNC_CURRENT, members)
    assert _status(lambda: e.process_sync_aggregate([ok], total, SYNC_APPLY)) == _abi.PE_ERR_STATE          # no resident balances
    e.state_set_balances(bal)
    e.sync_committee_set(SYNC_NEXT, [1, 2])
    before = _snapshot(e)
    refused = [([ok], total, 0), ([ok], total, 4), ([ok], total, SYNC_APPLY | 8),                            # flags
               ([_plain(members, [0, 5], 7)], total, SYNC_APPLY), ([_plain(members, [511], 7)], total, SYNC_VERIFY),   # a bit >= size
               ([ok, _plain(members, [0], n_val)], total, SYNC_APPLY),                                       # proposer >= n
               ([ok] * 65, total, SYNC_APPLY),                                                               # n > 64
               ([ok], ETH - 1, SYNC_APPLY), ([ok], 0, SYNC_APPLY)]                                           # total < increment
    for aggs, tot, flags in refused:
        assert _status(lambda: e.process_sync_aggregate(aggs, tot, flags)) == _abi.PE_ERR_INVALID_ARG, (len(aggs), tot, flags)
        assert _same(before, _snapshot(e))
    # the scalar chain in 128 bits: increment * base_reward_factor beyond 64 bits; per_increment * increments beyond 64 bits
    assert _status(lambda: e.process_sync_aggregate([ok], total, SYNC_APPLY, base_reward_factor=2**62)) == _abi.PE_ERR_INVALID_ARG
    assert _status(lambda: e.process_sync_aggregate([ok], 2**63, SYNC_APPLY, base_reward_factor=2**34)) == _abi.PE_ERR_INVALID_ARG
    assert _same(before, _snapshot(e))
    res = e.process_sync_aggregate([], total, SYNC_APPLY)                                                    # n = 0: nothing to do
    assert res["applied"] == 0 and _same(before, _snapshot(e))
    # a handle that exchanges with other ranks refuses every call that reads or writes the committees, and loses nothing
    e.dist_init_custom(0, 1, lambda *args: 0, lambda *args: 0)
    for call in (lambda: e.process_sync_aggregate([ok], total, SYNC_APPLY), lambda: e.process_sync_aggregate([ok], total, SYNC_VERIFY),
                 lambda: e.sync_committee_compute(_seed("d"), n_val, 10, MAX_EFF, 4), lambda: e.sync_committee_set(SYNC_NEXT, [3])):
        assert _status(call) == _abi.PE_ERR_STATE
    e.dist_destroy()
    assert _same(before, _snapshot(e))
    got, key, _ = e.sync_committee_compute(_seed("d"), n_val, 10, MAX_EFF, 4)                                # ... and works again
    assert got.tolist() == M.next_sync_committee_indices(range(n_val), bal, _seed("d"), 10, MAX_EFF, 4)[0] and key == _key_of(got)
    e.sync_committee_set(SYNC_NEXT, [1, 2])
    assert _same(before, _snapshot(e))
    # VERIFY without pubkeys
    e2 = engine_factory()
    e2.set_validators(bal, np.ones(n_val, dtype=np.uint8))
    assert _status(lambda: e2.process_sync_aggregate([ok], total, SYNC_VERIFY)) == _abi.PE_ERR_STATE
    e.process_sync_aggregate([ok], total, SYNC_APPLY)                                                        # and the handle still works
    assert e.state_get_balances()[0].tolist() != bal.tolist()
