"""CPU: tests/withdrawals_model.py -- the specification's sequential loops (get_expected_withdrawals, process_withdrawals,
process_bls_to_execution_change) held to the closed form the kernels compute, on the explicit case matrix of
tests/test_gpu_withdrawals.py's shapes and on seeded random states; the SSZ roots pinned to tests/ssz_model.py; the recorded
vectors of tests/golden/withdrawals_vectors.json."""
import hashlib
import json

import numpy as np
import pytest

from tests import ssz_model as SSZ
from tests import withdrawals_model as W

EPOCH = 10
MIN = W.Params(max_withdrawals_per_payload=4, max_validators_per_sweep=16)


def both(a, epoch, next_index, start, p, payload=None, apply=False):
    s = W.process_withdrawals_sequential(a, epoch, next_index, start, p, payload, apply)
    c = W.process_withdrawals_closed(a, epoch, next_index, start, p, payload, apply)
    assert s[1] == c[1] and s[2] == c[2]
    assert all(np.array_equal(s[0][k], c[0][k]) for k in W.FIELDS)
    return s


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 255, 256, 257, 600])
def test_sizes_starts_and_sweeps(n):
    for sweep in (n, max(1, n // 2), n + 13, 16384):
        p = W.Params(max_validators_per_sweep=sweep)
        for start in sorted({0, n - 1, (n - 40) % n}):
            a = W.set_hits(W.blank_registry(n, p), range(0, n, 3), p)
            b, expected, res = both(a, EPOCH, 77, start, p, None, False)
            assert [w[0] for w in expected] == list(range(77, 77 + len(expected)))
            b, _, res2 = both(a, EPOCH, 77, start, p, expected, True)
            assert res2["applied"] == 1 and res2["status"] == 0
            if len(expected) < p.max_withdrawals_per_payload:
                assert res["next_withdrawal_validator_index"] == (start + sweep) % n
            else:
                assert res["next_withdrawal_validator_index"] == (expected[-1][1] + 1) % n
            assert int(b["bal"].astype(object).sum()) == int(a["bal"].astype(object).sum()) - res["total_gwei"]


@pytest.mark.parametrize("k,sweep,n", [(16, 600, 600), (4, 16, 40)])
def test_hit_counts_around_k(k, sweep, n):
    p = W.Params(max_withdrawals_per_payload=k, max_validators_per_sweep=sweep)
    for hits in (0, 1, k - 1, k, k + 1):
        positions = [sweep - 1 - 2 * i for i in range(hits)][::-1]  # the last hit at the last swept position
        a = W.set_hits(W.blank_registry(n, p), positions, p)
        b, expected, res = both(a, EPOCH, 0, 0, p, None, False)
        assert res["n_withdrawals"] == min(hits, k)
        b, expected, res = both(a, EPOCH, 0, 0, p, expected, True)
        if hits == k + 1:
            assert b["bal"][positions[-1]] == a["bal"][positions[-1]]  # behind the k-th hit: not debited


@pytest.mark.parametrize("edge", [63, 255])
def test_kth_hit_across_an_edge(edge):
    n, p = 600, W.Params(max_validators_per_sweep=600)
    k = p.max_withdrawals_per_payload
    hits = list(range(edge - k + 1, edge + 2))  # the k-th at `edge`, the (k+1)-th behind it
    a = W.set_hits(W.blank_registry(n, p), hits, p)
    b, expected, res = both(a, EPOCH, 5, 0, p, None, False)
    assert expected[-1][1] == edge and res["next_withdrawal_validator_index"] == edge + 1
    # ... and across the wrap: validator n - 1 | 0
    start = n - k
    a = W.set_hits(W.blank_registry(n, p), list(range(start, n)) + [0], p)
    _, expected, res = both(a, EPOCH, 5, start, p, None, False)
    assert expected[-1][1] == n - 1 and res["next_withdrawal_validator_index"] == 0


def test_every_inequality():
    p = W.Params()
    m = p.max_effective_balance
    cred1, cred0, cred2 = W.eth1_credentials(0), bytes(32), W.eth1_credentials(0, 2)
    for wdr, want in ((EPOCH - 1, True), (EPOCH, True), (EPOCH + 1, False), (W.FAR, False)):
        assert W.is_fully_withdrawable_validator(cred1, wdr, 1, EPOCH, p) is want
    assert not W.is_fully_withdrawable_validator(cred1, EPOCH, 0, EPOCH, p)
    assert not W.is_fully_withdrawable_validator(cred0, EPOCH, 1, EPOCH, p) and not W.is_fully_withdrawable_validator(cred2, EPOCH, 1, EPOCH, p)
    assert not W.is_partially_withdrawable_validator(cred1, m, m, p) and W.is_partially_withdrawable_validator(cred1, m, m + 1, p)
    assert not W.is_partially_withdrawable_validator(cred1, m - W.ETH, m + 5 * W.ETH, p)
    assert not W.is_partially_withdrawable_validator(cred0, m, m + 1, p) and not W.is_partially_withdrawable_validator(cred2, m, m + 1, p)
    # both: a full withdrawal of the whole balance
    a = W.set_hits(W.blank_registry(3, p), [0], p, kind="partial")
    a["wdr"][0] = EPOCH
    _, expected, res = both(a, EPOCH, 0, 0, p)
    assert expected == [(0, 0, W.address_of(0), int(a["bal"][0]))] and res["n_full"] == 1 and res["n_partial"] == 0


def test_payload_asserts():
    n, p = 40, MIN
    a = W.set_hits(W.blank_registry(n, p), [1, 2, 5, 9], p)
    _, expected, _ = both(a, EPOCH, 9, 0, p)
    assert len(expected) == 4
    cases = [(expected, W.WD_OK, 0), (expected[:3], W.WD_COUNT, 3), (expected[:2] + [expected[1]], W.WD_COUNT, 3)]
    for i, (field, status) in enumerate(((0, W.WD_INDEX), (1, W.WD_VALIDATOR), (2, W.WD_ADDRESS), (3, W.WD_AMOUNT))):
        bad = [list(w) for w in expected]
        bad[i][field] = bytes(20) if field == 2 else bad[i][field] + 1
        cases.append(([tuple(w) for w in bad], status, i))
    for payload, status, first in cases:
        b, _, res = both(a, EPOCH, 9, 0, p, payload, True)
        assert (res["status"], res["first_mismatch"]) == (status, first)
        assert res["applied"] == (status == 0)
        if status:
            assert all(np.array_equal(b[k], a[k]) for k in W.FIELDS)
    short = W.set_hits(W.blank_registry(n, p), [1, 2], p)
    _, _, res = both(short, EPOCH, 9, 0, p, W.get_expected_withdrawals(short, EPOCH, 9, 0, p)[0] + [expected[3]], True)
    assert (res["status"], res["first_mismatch"]) == (W.WD_COUNT, 2)


def test_the_refusals():
    a = W.blank_registry(4)
    for n, start, index, p, n_payload in ((0, 0, 0, W.Params(), None), (4, 4, 0, W.Params(), None),
                                          (4, 0, 0, W.Params(max_effective_balance=0), None),
                                          (4, 0, 0, W.Params(max_withdrawals_per_payload=0), None),
                                          (4, 0, 0, W.Params(max_validators_per_sweep=0), None), (4, 0, 0, W.Params(eth1_prefix=0), None),
                                          (4, 0, 0, W.Params(eth1_prefix=256), None),
                                          (4, 0, 0, W.Params(max_withdrawals_per_payload=65), None), (4, 0, 0, W.Params(), 17),
                                          (4, 0, 2**64 - 16, W.Params(), None)):
        with pytest.raises(ValueError):
            W.check_params(n, start, index, p, n_payload)
    W.check_params(4, 3, 2**64 - 65, W.Params(max_withdrawals_per_payload=64), 64)
    with pytest.raises(ValueError):
        W.process_withdrawals_sequential(a, EPOCH, 0, 0, W.Params(), None, True)


def test_random_states_and_what_their_seeds_yield():
    """the seeds are fixed so that the model alone yields 0, fewer than k and exactly k withdrawals"""
    seen = set()
    for n, seed, density, start in W.RANDOM_CASES:
        for p in (W.Params(), MIN, W.Params(max_validators_per_sweep=n + 5, max_withdrawals_per_payload=64)):
            a = W.random_registry(n, seed, EPOCH, p, density)
            _, expected, res = both(a, EPOCH, seed, start, p)
            both(a, EPOCH, seed, start, p, expected, True)
            k = p.max_withdrawals_per_payload
            seen.add("0" if not expected else "k" if len(expected) == k else "<k")
            if expected:
                assert res["n_full"] and res["n_partial"] or len(expected) < 3 or density == 1.0
    assert seen == {"0", "<k", "k"}


def changes_matrix(n):
    """(credentials, changes) pairs: every status, one validator twice, an invalid change in the middle, the hash's byte 0 and 1"""
    a = W.blank_registry(n)
    cred = a["cred"]
    cred[n - 1] = np.frombuffer(W.eth1_credentials(n - 1), dtype=np.uint8)
    v = 0
    yield cred, [W.change_for(v)]
    yield cred, [W.change_for(n)]                                   # BAD_INDEX
    yield cred, [W.change_for(n - 1)]                               # NOT_BLS
    yield cred, [W.change_for(v, pubkey=W.pubkey_of(99))]           # PUBKEY_MISMATCH
    yield cred, [W.change_for(v, valid=False)]                      # BAD_SIGNATURE
    yield cred, [W.change_for(v), W.change_for(v, address=bytes(20))]  # the first wins, the second fails the prefix check
    yield cred, [W.change_for(v, valid=False), W.change_for(v)]     # the first is not potent: the second is valid by itself
    if n > 2:
        yield cred, [W.change_for(0), W.change_for(1, valid=False), W.change_for(2)]
        yield cred, [W.change_for(2), W.change_for(1), W.change_for(0)]
    # the hash's edge: credentials whose byte 0 is not the hash's (it is the prefix), then byte 1 off
    h = hashlib.sha256(W.pubkey_of(v)).digest()
    edge = cred.copy()
    edge[v] = np.frombuffer(bytes([0]) + h[1:], dtype=np.uint8)
    yield edge, [W.change_for(v)]
    edge = cred.copy()
    edge[v] = np.frombuffer(bytes([0, h[1] ^ 1]) + h[2:], dtype=np.uint8)
    yield edge, [W.change_for(v)]


@pytest.mark.parametrize("n", [2, 5, 300])
def test_changes_sequential_against_closed(n):
    seen = set()
    for cred, changes in changes_matrix(n):
        s = W.process_bls_changes_sequential(cred, changes)
        c = W.process_bls_changes_closed(cred, changes)
        assert s[1] == c[1] and s[2] == c[2] and np.array_equal(s[0], c[0])
        seen |= set(s[1])
        if s[2]["n_invalid"]:
            assert np.array_equal(s[0], cred)
    assert seen == {W.CRED_OK, W.CRED_BAD_INDEX, W.CRED_NOT_BLS, W.CRED_PUBKEY_MISMATCH, W.CRED_BAD_SIGNATURE}
    rng = np.random.default_rng(n)
    for _ in range(40):
        cred = W.blank_registry(n)["cred"]
        changes = [W.change_for(int(rng.integers(0, n + 1)), valid=bool(rng.integers(0, 5)),
                                pubkey=None if rng.integers(0, 6) else W.pubkey_of(1000)) for _ in range(int(rng.integers(1, 9)))]
        s, c = W.process_bls_changes_sequential(cred, changes), W.process_bls_changes_closed(cred, changes)
        assert s[1] == c[1] and s[2] == c[2] and np.array_equal(s[0], c[0])


def test_a_change_makes_the_validator_withdrawable():
    p = MIN
    a = W.blank_registry(8, p)
    a["bal"][5] += 123
    assert both(a, EPOCH, 0, 0, p)[1] == []
    a["cred"], status, _ = W.process_bls_changes_sequential(a["cred"], [W.change_for(5)])
    assert status == [0] and both(a, EPOCH, 0, 0, p)[1] == [(0, 5, W.address_of(5), 123)]


def test_ssz_roots_are_ssz_models():
    w = (2**40 + 7, 2**33 + 1, bytes(range(1, 21)), 2**63 + 9)
    leaves = [SSZ.u64_chunk(w[0]), SSZ.u64_chunk(w[1]), w[2] + bytes(12), SSZ.u64_chunk(w[3])]
    assert W.withdrawal_root(w) == SSZ.merkleize_literal(leaves, 2)
    for limit, depth in ((1, 0), (3, 2), (4, 2), (16, 4), (64, 6)):
        for count in sorted({0, 1, limit - 1, limit}):
            if count < 0:
                continue
            ws = [(i, 2 * i, bytes([i]) * 20, 3 * i) for i in range(count)]
            want = SSZ.mix_in_length(SSZ.merkleize_literal([W.withdrawal_root(x) for x in ws], depth), count)
            assert W.withdrawals_list_root(ws, limit) == want
    c = W.change_for(2**35 + 1)
    root = SSZ.merkleize_literal([SSZ.u64_chunk(c[0]), SSZ.H(c[1] + bytes(16)), c[2] + bytes(12), bytes(32)], 2)
    assert W.bls_change_root(c) == root
    assert W.bls_change_signing_root(c, b"\x07" * 32) == SSZ.H(root + b"\x07" * 32)


def test_recorded_vectors():
    assert json.load(open(W.GOLDEN_PATH)) == json.loads(json.dumps(W.golden_cases()))
