"""-m gpu: pe_process_withdrawals, pe_process_bls_to_execution_changes and pe_bls_change_signing_roots (withdrawal_kernels.hip)
against the sequential loops of tests/withdrawals_model.py, bit for bit: the expected withdrawals, every word of the result, the
balances, withdrawable epochs and credentials read back, and the balances' and validators' SSZ roots against tests/ssz_model.py.
There is no tolerance anywhere in this file.  256 = the positions of one workgroup (WD_WG), 64 = a wave; the registries hold 1 to
600 validators, at most 3 workgroups: k_withdrawals_scan sees one wave of counts here.  Sweeps of 64, 65 and 259 workgroups (the
scan's cross-wave term, its tile loop and the ragged last tile) are tests/test_gpu_scan_tiles.py, with this file's helpers."""
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd as pea
from pos_evolution_amd import engine as E
from pos_evolution_amd import forkchoice as FC
from tests import ssz_model as SSZ
from tests import withdrawals_model as W
from tests.test_withdrawals_model import EPOCH, MIN, changes_matrix

pytestmark = pytest.mark.gpu
FAR = W.FAR
ROOTS = E.ROOT_BALANCES | E.ROOT_VALIDATORS


def keys(n):
    return np.frombuffer(b"".join(W.pubkey_of(v) for v in range(n)), dtype=np.uint8).reshape(n, 48)


def load(e, a, static=True, balances=True, epochs=True, view=True):
    n = len(a["bal"])
    flags = np.ones(n, dtype=np.uint8)
    e.set_validators(a["eff"], flags)
    if view:
        e.state_set_validators(a["eff"], (flags | 8).astype(np.uint8))
    if epochs:
        e.registry_set_epochs(np.zeros(n, dtype=np.uint64), np.full(n, FAR, dtype=np.uint64))
    if balances:
        e.state_set_balances(a["bal"], None, a["wdr"])
    if static:
        e.registry_set_static(keys(n), a["cred"], np.zeros(n, dtype=np.uint64))


def assert_state(e, want, roots=True):
    """the resident arrays the two calls read or write, and what pe_state_roots makes of them"""
    n = len(want["bal"])
    bal, _, wdr, _ = e.state_get_balances()
    _, cred, _, _ = e.registry_static()
    eff, _, _ = e.state_validators()
    for k, x in (("bal", bal), ("wdr", wdr), ("cred", cred), ("eff", eff)):
        assert np.array_equal(x, want[k]), (k, np.argwhere(x != want[k])[:3].tolist())
    if roots:
        got = e.state_roots(ROOTS)
        assert got["balances"] == SSZ.u64_list_root([int(x) for x in want["bal"]])
        leaves = [SSZ.validator_root(W.pubkey_of(v), bytes(want["cred"][v]), int(want["eff"][v]), 0, 0, 0, FAR, int(want["wdr"][v]))
                  for v in range(n)]
        assert got["validators"] == SSZ.validators_root(leaves)


def tuples(rows):
    return [(int(w["index"]), int(w["validator_index"]), w["address"].tobytes(), int(w["amount"])) for w in rows]


def check(e, a, epoch, next_index, start, p, payload=None, apply=False, roots=False):
    """One call held to the loop; -> (the registry after it, the expected withdrawals, the result)."""
    want, expected, res = W.process_withdrawals_sequential(a, epoch, next_index, start, p, payload, apply)
    rows, got = e.process_withdrawals(epoch, next_index, start, payload, apply, p.abi())
    assert tuples(rows) == expected
    assert got == res, (got, res)
    assert_state(e, want, roots)
    return want, expected, res


def status_of(call, *args, **kw):
    try:
        call(*args, **kw)
    except pea.EngineError as err:
        return err.status
    return 0


# ---------------------------------------------------------------- registry and sweep sizes, starts, the wrap
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 255, 256, 257, 600])
def test_sizes_starts_and_sweeps(engine_factory, n):
    e = engine_factory()
    a = W.set_hits(W.blank_registry(n), range(0, n, 3))
    load(e, a)
    index = 2**40
    for sweep in (n, max(1, n // 2), n + 13):
        p = W.Params(max_validators_per_sweep=sweep)
        for start in sorted({0, n - 1, (n - 40) % n}):  # (n - 40) mod n: the wrap falls inside a wave
            _, expected, res = check(e, a, EPOCH, index, start, p)                     # computes only: nothing moves
            if len(expected) < p.max_withdrawals_per_payload:
                assert res["next_withdrawal_validator_index"] == (start + sweep) % n  # the parameter, not the bound
            a, _, res = check(e, a, EPOCH, index, start, p, expected, True, roots=start == 0)
            assert res["applied"] == 1
            index = res["next_withdrawal_index"]
            a = W.set_hits(a, [w[1] for w in expected if w[1] % 3 == 0])  # fully withdrawn ones get a balance again
            e.state_set_balances(a["bal"], None, a["wdr"])
    e.close()


# ---------------------------------------------------------------- hit counts around k; the k-th hit at the last position
@pytest.mark.parametrize("k,sweep,n", [(16, 600, 600), (4, 16, 40)])
def test_hit_counts_around_k(engine_factory, k, sweep, n):
    p = W.Params(max_withdrawals_per_payload=k, max_validators_per_sweep=sweep)
    e = engine_factory()
    for hits in (0, 1, k - 1, k, k + 1):
        positions = [sweep - 1 - 2 * i for i in range(hits)][::-1]
        a = W.set_hits(W.blank_registry(n, p), positions, p)
        load(e, a)
        _, expected, res = check(e, a, EPOCH, 3, 0, p)
        assert res["n_withdrawals"] == min(hits, k) == len(expected)
        b, _, res = check(e, a, EPOCH, 3, 0, p, expected, True, roots=True)
        if hits == k + 1:  # the k-th hit at sweep - 3, the (k+1)-th at the last swept position: not debited
            assert b["bal"][sweep - 1] == a["bal"][sweep - 1] and res["next_withdrawal_validator_index"] == sweep - 2
        if hits == k:
            assert expected[-1][1] == sweep - 1 and res["next_withdrawal_validator_index"] == sweep % n
    e.close()


@pytest.mark.parametrize("edge", [63, 255, "wrap"])
def test_the_kth_and_the_next_hit_on_either_side_of_an_edge(engine_factory, edge):
    """a wave boundary (positions 63 | 64), a workgroup boundary (255 | 256) and the wrap (validator n - 1 | 0)"""
    n, p = 600, W.Params(max_validators_per_sweep=600)
    k = p.max_withdrawals_per_payload
    if edge == "wrap":
        start, last = n - k, n - 1
        hits = list(range(start, n)) + [0]
    else:
        start, last = 0, edge
        hits = list(range(edge - k + 1, edge + 2))
    a = W.set_hits(W.blank_registry(n, p), hits, p)
    e = engine_factory()
    load(e, a)
    _, expected, res = check(e, a, EPOCH, 5, start, p)
    b, _, res = check(e, a, EPOCH, 5, start, p, expected, True, roots=True)
    behind = (last + 1) % n
    assert expected[-1][1] == last and res["next_withdrawal_validator_index"] == behind
    assert b["bal"][behind] == a["bal"][behind] and b["bal"][last] != a["bal"][last]
    e.close()


def test_hits_in_one_workgroup_and_one_hit_per_workgroup(engine_factory):
    n, p = 600, W.Params(max_validators_per_sweep=600)
    e = engine_factory()
    for hits in (list(range(256, 256 + 16)), list(range(300, 300 + 17)), [10, 300, 550], [255, 256, 511, 512, 599]):
        for start in (0, 100):
            a = W.set_hits(W.blank_registry(n, p), hits, p)
            load(e, a)
            _, expected, _ = check(e, a, EPOCH, 0, start, p)
            check(e, a, EPOCH, 0, start, p, expected, True)
    e.close()


# ---------------------------------------------------------------- every inequality's edge
def test_every_inequality(engine_factory):
    p = W.Params(max_withdrawals_per_payload=64)
    m, inc = p.max_effective_balance, W.ETH
    rows = []  # (prefix, withdrawable epoch, effective balance, balance)
    for wdr in (EPOCH - 1, EPOCH, EPOCH + 1, FAR):
        rows.append((1, wdr, m, 5))
    rows += [(1, EPOCH, m, 0), (1, EPOCH, m, 1)]                        # full: balance 0 and 1
    rows += [(1, FAR, m, m), (1, FAR, m, m + 1)]                        # partial: balance = max, max + 1
    rows += [(1, FAR, m - inc, m + 5 * inc), (1, FAR, m, m + 5 * inc)]  # effective = max - increment with excess, = max
    rows += [(0, EPOCH, m, m + 7), (2, EPOCH, m, m + 7), (1, EPOCH, m, m + 7)]  # the prefixes; the last: both -> a full one
    n = len(rows)
    a = W.blank_registry(n, p)
    for v, (prefix, wdr, eff, bal) in enumerate(rows):
        a["cred"][v] = np.frombuffer(W.eth1_credentials(v, prefix), dtype=np.uint8)
        a["wdr"][v], a["eff"][v], a["bal"][v] = wdr, eff, bal
    e = engine_factory()
    load(e, a)
    _, expected, res = check(e, a, EPOCH, 0, 0, p)
    assert [w[1] for w in expected] == [0, 1, 5, 7, 9, 12] and expected[-1][3] == m + 7
    assert res["n_full"] == 4 and res["n_partial"] == 2
    check(e, a, EPOCH, 0, 0, p, expected, True, roots=True)
    e.close()


# ---------------------------------------------------------------- the payload's asserts
def test_payload_asserts(engine_factory):
    n, p = 40, MIN
    a = W.set_hits(W.blank_registry(n, p), [1, 2, 5, 9], p)
    e = engine_factory()
    load(e, a)
    _, expected, _ = check(e, a, EPOCH, 9, 0, p)
    assert len(expected) == 4
    cases = [(expected[:3], W.WD_COUNT, 3), ([], W.WD_COUNT, 0)]
    for i, (field, status) in enumerate(((0, W.WD_INDEX), (1, W.WD_VALIDATOR), (2, W.WD_ADDRESS), (3, W.WD_AMOUNT))):
        bad = [list(w) for w in expected]
        bad[i][field] = bad[i][2][:19] + bytes([bad[i][2][19] ^ 1]) if field == 2 else bad[i][field] + 2**32
        cases.append(([tuple(w) for w in bad], status, i))
    for payload, status, first in cases:
        for apply in (True, False):
            b, _, res = check(e, a, EPOCH, 9, 0, p, payload, apply, roots=True)  # every array unchanged
            assert (res["status"], res["first_mismatch"], res["applied"]) == (status, first, 0)
    # longer: a state with two hits against a payload of three
    short = W.set_hits(W.blank_registry(n, p), [1, 2], p)
    load(e, short)
    two = W.get_expected_withdrawals(short, EPOCH, 9, 0, p)[0]
    _, _, res = check(e, short, EPOCH, 9, 0, p, two + [expected[3]], True)
    assert (res["status"], res["first_mismatch"]) == (W.WD_COUNT, 2)
    # equal, without PE_WD_APPLY: the same outputs, unchanged arrays; then with it
    load(e, a)
    _, _, dry = check(e, a, EPOCH, 9, 0, p, expected, False, roots=True)
    _, _, wet = check(e, a, EPOCH, 9, 0, p, expected, True, roots=True)
    assert dry["status"] == 0 and {**dry, "applied": 1} == wet
    e.close()


# ---------------------------------------------------------------- random states
def test_random_states(engine_factory):
    e = engine_factory()
    for n, seed, density, start in W.RANDOM_CASES:
        for p in (W.Params(), MIN, W.Params(max_validators_per_sweep=n + 5, max_withdrawals_per_payload=64)):
            a = W.random_registry(n, seed, EPOCH, p, density)
            load(e, a)
            _, expected, _ = check(e, a, EPOCH, seed, start, p)
            check(e, a, EPOCH, seed, start, p, expected, True, roots=n <= 65)
    e.close()


def test_the_view_that_still_mirrors_the_registry(engine_factory):
    """no pe_state_set_validators: the effective balances are the pe_set_validators data, and the call does not materialise a view"""
    p = MIN
    a = W.set_hits(W.blank_registry(20, p), [3, 4, 8], p)
    a["eff"][4] -= W.ETH  # no longer at the maximum: not partially withdrawable
    e = engine_factory()
    load(e, a, view=False)
    want, expected, res = W.process_withdrawals_sequential(a, EPOCH, 0, 0, p)
    rows, got = e.process_withdrawals(EPOCH, 0, 0, None, False, p.abi())
    assert tuples(rows) == expected and got == res and [w[1] for w in expected] == [3, 8]
    assert not e.state_validators()[2]
    e.close()


# ---------------------------------------------------------------- address changes
def run_changes(e, cred, changes):
    want, status, stats = W.process_bls_changes_sequential(cred, changes)
    got_status, got = e.process_bls_to_execution_changes(changes)
    assert [int(s) for s in got_status] == status and got == stats
    return want, status


@pytest.mark.parametrize("n", [2, 5, 300])
def test_changes(engine_factory, n):
    e = engine_factory()
    seen = set()
    for cred, changes in changes_matrix(n):
        a = W.blank_registry(n)
        a["cred"] = cred.copy()
        load(e, a)
        a["cred"], status = run_changes(e, cred, changes)
        seen |= set(status)
        assert_state(e, a, roots=n <= 5)
    assert seen == {W.CRED_OK, W.CRED_BAD_INDEX, W.CRED_NOT_BLS, W.CRED_PUBKEY_MISMATCH, W.CRED_BAD_SIGNATURE}
    status, stats = e.process_bls_to_execution_changes([])
    assert status.size == 0 and stats == dict(n_applied=0, n_invalid=0)
    e.close()


def test_many_changes_and_one_validator_many_times(engine_factory):
    """more than a workgroup of changes; validator 650 is named by every fourth: the first of them wins"""
    n = 700
    a = W.blank_registry(n)
    changes = [W.change_for(650 if i % 4 == 0 else i, address=bytes([i % 251]) * 20) for i in range(600)]
    e = engine_factory()
    load(e, a)
    _, status = run_changes(e, a["cred"], changes)
    assert status[0] == 0 and set(status[4::4]) == {W.CRED_NOT_BLS} and status.count(0) == 600 - 149
    assert_state(e, a, roots=False)  # an invalid block: nothing moved
    valid = [c for c, s in zip(changes, status) if s == 0]
    a["cred"], status = run_changes(e, a["cred"], valid)
    assert set(status) == {0} and bytes(a["cred"][650][12:]) == bytes(20)
    assert_state(e, a, roots=False)
    e.close()


def test_a_change_then_a_withdrawal(engine_factory):
    p = MIN
    a = W.blank_registry(8, p)
    a["bal"][5] += 123
    e = engine_factory()
    load(e, a)
    assert check(e, a, EPOCH, 0, 0, p)[1] == []
    a["cred"], status = run_changes(e, a["cred"], [W.change_for(5)])
    assert status == [0]
    _, expected, _ = check(e, a, EPOCH, 0, 0, p)
    assert expected == [(0, 5, W.address_of(5), 123)]
    check(e, a, EPOCH, 0, 0, p, expected, True, roots=True)
    e.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_signing_roots(engine_factory, n):
    e = engine_factory()
    changes = [W.change_for(v * 2**33 + v) for v in range(n)]
    domain = bytes(range(100, 132))
    got = e.bls_change_signing_roots(changes, domain)
    assert [r.tobytes() for r in got] == [W.bls_change_signing_root(c, domain) for c in changes]
    assert e.bls_change_signing_roots([], domain).shape == (0, 32)
    e.close()


# ---------------------------------------------------------------- refusals: nothing changes
def test_refusals(engine_factory):
    INVALID, STATE = pea._abi.PE_ERR_INVALID_ARG, pea._abi.PE_ERR_STATE
    a = W.set_hits(W.blank_registry(8), [1, 2, 3])
    e = engine_factory()
    load(e, a)
    pw = e.process_withdrawals
    for start, index, p, payload, apply in ((8, 0, {}, None, False), (0, 0, dict(max_effective_balance=0), None, False),
                                            (0, 0, dict(max_withdrawals_per_payload=0), None, False),
                                            (0, 0, dict(max_validators_per_sweep=0), None, False), (0, 0, dict(eth1_prefix=0), None, False),
                                            (0, 0, dict(eth1_prefix=256), None, False),
                                            (0, 0, dict(max_withdrawals_per_payload=65), None, False),
                                            (0, 0, dict(max_withdrawals_per_payload=2), [(0, 0, bytes(20), 0)] * 3, True),
                                            (0, 2**64 - 16, {}, None, False), (0, 0, {}, None, True)):
        assert status_of(pw, EPOCH, index, start, payload, apply, p) == INVALID, (start, index, p)
        assert_state(e, a)
    assert status_of(pw, EPOCH, 2**64 - 17, 0, None, False, {}) == 0
    e.close()
    for missing in ("static", "balances", "epochs"):
        e = engine_factory()
        load(e, a, **{missing: False})
        assert status_of(e.process_withdrawals, EPOCH, 0, 0) == STATE, missing
        if missing == "static":
            assert status_of(e.process_bls_to_execution_changes, [W.change_for(0)]) == STATE
            assert np.array_equal(e.state_get_balances()[0], a["bal"])
        e.close()
    e = engine_factory()  # an empty registry
    e.set_validators(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    e.registry_set_epochs(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    e.state_set_balances(np.zeros(0, dtype=np.uint64))
    e.registry_set_static(np.zeros((0, 48), dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8), np.zeros(0, dtype=np.uint64))
    assert status_of(e.process_withdrawals, EPOCH, 0, 0) == INVALID
    status, _ = e.process_bls_to_execution_changes([W.change_for(0)])
    assert [int(s) for s in status] == [W.CRED_BAD_INDEX]
    e.close()


# ---------------------------------------------------------------- the forkchoice mirrors; two blocks
def make_state(a, slot):
    vals = [SimpleNamespace(pubkey=W.pubkey_of(v), withdrawal_credentials=bytes(a["cred"][v]), effective_balance=int(a["eff"][v]),
                            slashed=False, activation_eligibility_epoch=0, activation_epoch=0, exit_epoch=FAR,
                            withdrawable_epoch=int(a["wdr"][v])) for v in range(len(a["bal"]))]
    n = len(vals)
    cp = SimpleNamespace(epoch=0, root=bytes(32))
    return SimpleNamespace(slot=slot, validators=vals, balances=[int(x) for x in a["bal"]], current_epoch_participation=[0] * n,
                           previous_epoch_participation=[0] * n, inactivity_scores=[0] * n, current_justified_checkpoint=cp,
                           previous_justified_checkpoint=cp, next_withdrawal_index=11, next_withdrawal_validator_index=17)


def test_forkchoice_mirrors_over_two_blocks(engine_factory):
    p = MIN
    n = 20
    a = W.set_hits(W.blank_registry(n, p), [1, 3, 5, 17, 18, 19], p)
    e = engine_factory()
    e.set_validators(a["eff"], np.ones(n, dtype=np.uint8))
    state = make_state(a, EPOCH * int(e.cfg.slots_per_epoch))
    FC.bind_state(e, state, bytes(32), 1)
    index, start = 11, 17
    for block in range(2):
        want, expected, res = W.process_withdrawals_sequential(a, EPOCH, index, start, p, None, False)
        assert tuples(FC.get_expected_withdrawals(state, **p.abi())) == expected and len(expected) == (4, 2)[block]
        payload = SimpleNamespace(withdrawals=[SimpleNamespace(index=w[0], validator_index=w[1], address=w[2], amount=w[3])
                                               for w in expected])
        bad = SimpleNamespace(withdrawals=payload.withdrawals[:-1])
        with pytest.raises(AssertionError):
            FC.process_withdrawals(state, bad, **p.abi())
        assert state.balances == [int(x) for x in a["bal"]] and state.next_withdrawal_index == index
        FC.process_withdrawals(state, payload, **p.abi())
        a, _, res = W.process_withdrawals_sequential(a, EPOCH, index, start, p, expected, True)
        index, start = res["next_withdrawal_index"], res["next_withdrawal_validator_index"]
        assert state.balances == [int(x) for x in a["bal"]]
        assert (state.next_withdrawal_index, state.next_withdrawal_validator_index) == (index, start)
    assert (index, start) == (17, (2 + 16) % n)
    # an address change, then the validator's withdrawal in the next block
    state.balances[8] += 55
    a["bal"][8] += 55
    m = SimpleNamespace(validator_index=8, from_bls_pubkey=W.pubkey_of(8), to_execution_address=W.address_of(8))
    with pytest.raises(AssertionError):
        FC.process_bls_to_execution_change(state, SimpleNamespace(message=m), signature_valid=False)
    assert state.validators[8].withdrawal_credentials == bytes(a["cred"][8])
    FC.process_bls_to_execution_change(state, SimpleNamespace(message=m))
    a["cred"], status, _ = W.process_bls_changes_sequential(a["cred"], [W.change_for(8)])
    assert status == [0] and state.validators[8].withdrawal_credentials == bytes(a["cred"][8])
    with pytest.raises(AssertionError):
        FC.process_bls_to_execution_change(state, SimpleNamespace(message=m))
    assert tuples(FC.get_expected_withdrawals(state, **p.abi())) == W.get_expected_withdrawals(a, EPOCH, index, start, p)[0]
    e.close()
