"""CPU: the own-words model of the sync committee (tests/sync_committee_model.py) against what it can be held to without
a GPU -- tests/epoch_model.proposer for the first member (itself pinned to the reference's compute_proposer_index), a
brute-force formulation of the sampling, and rewards worked by hand -- and forkchoice.compute_sync_committee_period /
is_assigned_to_sync_committee against the reference's own text (pe:564-587) where that is on the machine.
tests/test_gpu_sync_committee.py holds the engine to the same model."""
import __future__
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import ref_extract
from pos_evolution_amd import forkchoice as fc
from tests import epoch_model
from tests import sync_committee_model as M

ETH = 10**9
MAX_EFF = 32 * ETH
needs_reference = pytest.mark.skipif(not ref_extract.reference_available(), reason="the reference's Markdown is not on this machine")


def _seed(tag, k=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), k)).digest()


def _mixed(n, rng):
    bal = rng.choice(np.array([0, 1, 7, 16, 31, 32], dtype=np.int64), size=n) * ETH
    bal[0] = 32 * ETH
    return [int(b) for b in bal]


# ---------------------------------------------------------------- sampling
def test_walk_is_compute_shuffled_index():
    for count, rounds in ((1, 10), (2, 10), (255, 3), (256, 10), (257, 10), (1000, 5)):
        seed = _seed("walk", count)
        walk = M.Walk(seed, count, rounds)
        got = [walk(i) for i in range(count)]
        assert got == [epoch_model.shuffled_index(i, count, seed, rounds) for i in range(count)]
        assert sorted(got) == list(range(count))


@pytest.mark.parametrize("n_active", [1, 2, 3, 255, 257])
def test_member_0_is_the_proposer(n_active):
    rng = np.random.default_rng(n_active)
    for k, kind in enumerate(("full", "one", "mixed")):
        eff = _mixed(n_active + 5, rng) if kind == "mixed" else [(32 if kind == "full" else 1) * ETH] * (n_active + 5)
        indices = sorted(int(v) for v in rng.choice(n_active + 5, size=n_active, replace=False))
        eff[indices[0]] = 32 * ETH
        seed = _seed("first", 16 * n_active + k)
        members, tries = M.next_sync_committee_indices(indices, eff, seed, 10, MAX_EFF, 1)
        assert (members[0], tries - 1) == epoch_model.proposer(indices, eff, seed, 10, MAX_EFF, 0)
        longer, _ = M.next_sync_committee_indices(indices, eff, seed, 10, MAX_EFF, 7)
        assert longer[0] == members[0]


def test_members_are_the_first_accepting_candidates():
    """The same list from another formulation: every accepting i listed first, then the first `size` of them."""
    rng = np.random.default_rng(5)
    for case, (n_active, size) in enumerate(((3, 32), (100, 32), (257, 65), (1000, 64))):
        eff = _mixed(n_active, rng)
        seed = _seed("brute", case)
        members, tries = M.next_sync_committee_indices(range(n_active), eff, seed, 10, MAX_EFF, size)
        horizon = tries + 40
        accepting = []
        for i in range(horizon):
            candidate = epoch_model.shuffled_index(i % n_active, n_active, seed, 10)
            byte = hashlib.sha256(seed + (i // 32).to_bytes(8, "little")).digest()[i % 32]
            if eff[candidate] * 255 >= MAX_EFF * byte:
                accepting.append((i, candidate))
        assert [c for _, c in accepting[:size]] == members
        assert accepting[size - 1][0] + 1 == tries
        assert len(accepting) > size   # the horizon reached beyond the last member


def test_fewer_active_than_size_gives_duplicates_and_max_tries_bounds():
    eff = [32 * ETH] * 3
    members, tries = M.next_sync_committee_indices(range(3), eff, _seed("dup"), 10, MAX_EFF, 32)
    assert len(members) == 32 and tries == 32 and set(members) == {0, 1, 2}
    assert M.next_sync_committee_indices(range(3), eff, _seed("dup"), 10, MAX_EFF, 32, max_tries=32)[0] == members
    assert M.next_sync_committee_indices(range(3), eff, _seed("dup"), 10, MAX_EFF, 32, max_tries=31) == (None, 31)


# ---------------------------------------------------------------- the scalars
def test_scalar_chain_by_hand():
    """total active balance 1 000 000 x 32 ETH = 3.2e16 Gwei: isqrt = 178 885 438 (178885438^2 = 31 999 999 929 451 844 <=
    3.2e16 < 178885439^2), per_increment = 64e9 // 178885438 = 357, total_base = 357 x 32e6 = 11 424 000 000,
    x 2 // 64 = 357 000 000, // 32 = 11 156 250, // 512 = 21 789 (21 789 x 512 = 11 155 968), proposer = 21 789 x 8 // 56 = 3 112."""
    assert 178885438**2 <= 32 * 10**15 < 178885439**2
    assert M.reward_scalars(32 * 10**15, 512) == (21789, 3112)
    # the minimal preset's committee and slots: // 8 // 32
    assert M.reward_scalars(32 * 10**15, 32, slots_per_epoch=8) == (357000000 // 8 // 32, (357000000 // 8 // 32) * 8 // 56)
    # division order matters: one combined division would give another value
    assert M.reward_scalars(10**9 * 1000, 512)[0] == (10**9 * 64 // 1000000) * 1000 * 2 // 64 // 32 // 512


def test_signing_root_and_bits():
    root, domain = bytes(range(32)), bytes(range(32, 64))
    assert M.signing_root(root, domain) == hashlib.sha256(bytes(range(64))).digest()
    bits = bytearray(64)
    bits[0], bits[1], bits[63] = 0b00000101, 0b10000000, 0b10000000
    assert [p for p in range(512) if M.bit(bits, p)] == [0, 2, 15, 511]
    assert M.participants([7, 8, 7], bytes([0b101]) + bytes(63)) == [7, 7]
    with pytest.raises(AssertionError):
        M.participants([7, 8], bytes([0b100]) + bytes(63))


# ---------------------------------------------------------------- rewards by hand
def _bits(*positions):
    b = bytearray(64)
    for p in positions:
        b[p // 8] |= 1 << (p % 8)
    return bytes(b)


PR, QR = 1000, 142   # participant_reward, proposer_reward = 1000 * 8 // 56


@pytest.mark.parametrize("start", [0, PR - 1])
def test_member_twice_reward_then_penalty_and_penalty_then_reward(start):
    """Validator 5 sits at positions 0 and 1; validator 9 proposes and is no member."""
    bal = [10**6] * 10
    bal[5] = start
    st = M.process_sync_aggregates(bal, [5, 5], [(_bits(0), 9)], PR, QR)     # bits (1, 0): + then -
    assert bal[5] == start and bal[9] == 10**6 + QR
    assert st == {"n_participants": 1, "credited": PR + QR, "debited": PR, "n_saturated": 0}
    bal = [10**6] * 10
    bal[5] = start
    st = M.process_sync_aggregates(bal, [5, 5], [(_bits(1), 9)], PR, QR)     # bits (0, 1): - (cut at 0) then +
    assert bal[5] == PR and bal[9] == 10**6 + QR
    assert st == {"n_participants": 1, "credited": PR + QR, "debited": start, "n_saturated": 1}


def test_proposer_who_is_an_absent_member_earlier_and_later():
    """Validator 3 proposes and is an absent member; two others participate.  At an EARLIER position the penalty meets the
    empty balance before any proposer reward arrives; at a LATER position it takes back what the rewards brought."""
    bal = [0] * 8
    st = M.process_sync_aggregates(bal, [3, 1, 2], [(_bits(1, 2), 3)], PR, QR)
    assert bal[3] == 2 * QR and (bal[1], bal[2]) == (PR, PR)
    assert st == {"n_participants": 2, "credited": 2 * (PR + QR), "debited": 0, "n_saturated": 1}
    bal = [0] * 8
    st = M.process_sync_aggregates(bal, [1, 2, 3], [(_bits(0, 1), 3)], PR, QR)
    assert bal[3] == 0 and (bal[1], bal[2]) == (PR, PR)
    assert st == {"n_participants": 2, "credited": 2 * (PR + QR), "debited": 2 * QR, "n_saturated": 1}
    # a second aggregate starts from what the first left
    bal = [0] * 8
    M.process_sync_aggregates(bal, [3, 1, 2], [(_bits(1, 2), 3), (_bits(1, 2), 3)], PR, QR)
    assert bal[3] == 2 * QR + 2 * QR - min(2 * QR, PR) and bal[1] == 2 * PR


# ---------------------------------------------------------------- forkchoice.py against the reference's text
def test_period_and_assignment():
    assert [fc.compute_sync_committee_period(e) for e in (0, 255, 256, 511, 512)] == [0, 0, 1, 1, 2]
    assert fc.compute_sync_committee_period(17, preset={"EPOCHS_PER_SYNC_COMMITTEE_PERIOD": 8}) == 2
    cur, nxt = [4, 9, 4], [7]
    assert fc.is_assigned_to_sync_committee(300, 511, 4, cur, nxt) and not fc.is_assigned_to_sync_committee(300, 511, 7, cur, nxt)
    assert fc.is_assigned_to_sync_committee(300, 512, 7, cur, nxt) and not fc.is_assigned_to_sync_committee(300, 767, 9, cur, nxt)
    for epoch in (255, 768):
        with pytest.raises(AssertionError):
            fc.is_assigned_to_sync_committee(300, epoch, 4, cur, nxt)


@needs_reference
def test_period_and_assignment_equal_the_reference_text():
    by_name = ref_extract.index_fences(ref_extract.fences())
    rng = np.random.default_rng(564)
    for period_len in (256, 8):
        state_box, preset = {}, {"EPOCHS_PER_SYNC_COMMITTEE_PERIOD": period_len}
        ns = {"EPOCHS_PER_SYNC_COMMITTEE_PERIOD": period_len, "get_current_epoch": lambda state: state_box["epoch"]}
        for name in ("compute_sync_committee_period", "is_assigned_to_sync_committee"):
            fence = by_name[name]
            exec(compile(fence.code, f"<pe:{fence.first}-{fence.last}>", "exec", flags=__future__.annotations.compiler_flag,
                         dont_inherit=True), ns)
        n_val = 40
        pubkeys = [hashlib.sha256(b"pk-%d" % v).digest() + bytes(16) for v in range(n_val)]   # distinct, as process_deposit keeps them
        for case in range(200):
            cur = [int(v) for v in rng.integers(0, n_val, size=6)]
            nxt = [int(v) for v in rng.integers(0, n_val, size=6)]
            state = SimpleNamespace(validators=[SimpleNamespace(pubkey=pk) for pk in pubkeys],
                                    current_sync_committee=SimpleNamespace(pubkeys=[pubkeys[v] for v in cur]),
                                    next_sync_committee=SimpleNamespace(pubkeys=[pubkeys[v] for v in nxt]))
            state_box["epoch"] = int(rng.integers(0, 5 * period_len))
            epoch = int(rng.integers(max(0, state_box["epoch"] - period_len), state_box["epoch"] + 2 * period_len + 1))
            v = int(rng.integers(0, n_val)) if case % 2 else int(rng.choice(cur + nxt))
            assert fc.compute_sync_committee_period(epoch, preset=preset) == ns["compute_sync_committee_period"](epoch)
            try:
                want = ns["is_assigned_to_sync_committee"](state, epoch, v)
            except AssertionError:
                with pytest.raises(AssertionError):
                    fc.is_assigned_to_sync_committee(state_box["epoch"], epoch, v, cur, nxt, preset=preset)
                continue
            assert fc.is_assigned_to_sync_committee(state_box["epoch"], epoch, v, cur, nxt, preset=preset) == want
