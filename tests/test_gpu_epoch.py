"""-m gpu: the epoch boundary on the GPU -- pe_compute_proposers (compute_proposer_index, pe:604-618) and
pe_effective_balance_updates (process_effective_balance_updates, pe:122-133) -- against the model of tests/epoch_model.py
and the recorded answers of the reference's own text (tests/golden/epoch_vectors.json); tests/test_epoch_model.py ties
those two to the reference.  Shapes: the `position // 256` and `i % total` edges of the sampling kernel (1, 2, 3, 255, 256,
257, 1000 active validators), more seeds than one, both round counts; the wave, workgroup and four-element padding edges
of the streaming pass (1, 63, 64, 65, 255, 257, 4099 validators)."""
import hashlib
import importlib.util
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd.synth as synth
from tests import epoch_model as M
from tests import helpers as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ETH = 10**9
MAX_EFF = 32 * ETH
NONE32 = 0xFFFFFFFF


def _generator():
    spec_ = importlib.util.spec_from_file_location("generate_epoch", os.path.join(HERE, "golden", "generate_epoch.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


GEN = _generator()
PROPOSER_ROWS, HYSTERESIS_ROWS = GEN.load()


def _seeds(tag: str, n: int):
    return [hashlib.sha256(b"%s-%d" % (tag.encode(), k)).digest() for k in range(n)]


def _balances(kind: str, n: int, rng):
    if kind == "mixed":
        bal = rng.choice(np.array([0, 0, 1, 7, 16, 31, 32], dtype=np.uint64), size=n) * np.uint64(ETH)
        bal[rng.integers(0, n)] = 32 * ETH
        return bal
    return np.full(n, (32 if kind == "full" else 1) * ETH, dtype=np.uint64)


def _check_against_model(e, seeds, active, bal, rounds, max_eff=MAX_EFF, max_tries=0):
    prop, tries = e.compute_proposers(seeds, active, rounds, max_eff, max_tries)
    indices = list(range(active)) if isinstance(active, int) else [int(x) for x in active]
    for k, seed in enumerate(seeds):
        want, want_tries = M.proposer(indices, bal, seed, rounds, max_eff, max_tries)
        assert int(prop[k]) == (NONE32 if want is None else want), (k, int(prop[k]), want)
        assert int(tries[k]) == want_tries, (k, int(tries[k]), want_tries)
    return prop, tries


# ---------------------------------------------------------------- proposers
# every n_active sees every value of {seeds, rounds, active-set form, balances}; the product is covered across the sizes
CONFIGS = [(1, 10, False, "full"), (32, 90, True, "one"), (33, 10, True, "mixed"), (33, 90, False, "full"),
           (32, 10, False, "one"), (1, 90, True, "mixed")]


@pytest.mark.parametrize("n_active", [1, 2, 3, 255, 256, 257, 1000])
def test_proposers_vs_model(engine_factory, n_active):
    n_val = n_active + 37
    e = engine_factory()
    rng = np.random.default_rng(n_active)
    for c, (n_seeds, rounds, subset, kind) in enumerate(CONFIGS):
        bal = _balances(kind, n_val, rng)
        active = np.sort(rng.choice(n_val, size=n_active, replace=False)).astype(np.uint32) if subset else n_active
        if kind == "mixed":   # at least one candidate of the active set can be accepted
            bal[int(active[0]) if subset else 0] = 32 * ETH
        e.set_validators(bal, np.ones(n_val, dtype=np.uint8))
        _check_against_model(e, _seeds(f"p{n_active}-{c}", n_seeds), active, bal, rounds)


def test_proposers_golden_vectors(engine_factory):
    """The answers the reference's own function gave, the late-acceptance classes and the exhausted registry among them."""
    engines, late, outcomes = {}, set(), set()
    for r in PROPOSER_ROWS:
        n_val = r["n_val"]
        if n_val not in engines:
            engines[n_val] = engine_factory()
        e = engines[n_val]
        e.set_validators(np.array(GEN.expand_eff(r), dtype=np.uint64), np.ones(n_val, dtype=np.uint8))
        active = r["n_active"] if r["indices"] is None else np.array(r["indices"], dtype=np.uint32)
        prop, tries = e.compute_proposers([bytes.fromhex(r["seed"])], active, r["rounds"], r["max_eff"], r["max_tries"])
        assert int(prop[0]) == (NONE32 if r["proposer"] is None else r["proposer"]), r["tag"]
        assert int(tries[0]) == r["tries"], r["tag"]
        if r["tag"] == "late":
            late.add(128 if r["tries"] >= 128 else r["tries"])
        if r["tag"] == "zero":   # a bounded loop reaching its bound: 0xFFFFFFFF / tries == 128 exactly where there is no proposer
            assert (int(prop[0]) == NONE32) == (r["proposer"] is None) == (int(tries[0]) == 128)
            outcomes.add(r["proposer"] is None)
    assert late == {0, 31, 32, 63, 64, 128}
    assert outcomes == {True, False}


def test_proposers_exhausted_and_max_tries_inside_a_batch(engine_factory):
    """max_tries is rounded up to whole batches inside the kernel, the reported tries never exceeds it, and a candidate
    beyond it is not accepted."""
    n = 5
    e = engine_factory()
    bal = np.zeros(n, dtype=np.uint64)
    e.set_validators(bal, np.ones(n, dtype=np.uint8))
    seeds = _seeds("zero", 33)
    for max_tries in (1, 63, 64, 65, 128, 300):
        prop, tries = _check_against_model(e, seeds, n, bal, 10, MAX_EFF, max_tries)
        assert (tries <= max_tries).all() and ((prop == NONE32) == (tries == max_tries)).all()
    _check_against_model(e, seeds[:4], n, bal, 10)   # max_tries = 0 means 4096
    # the seed the golden file accepts at i = 21: one try short of it there is no proposer, with it there is
    r = next(r for r in PROPOSER_ROWS if r["tag"] == "zero" and r["proposer"] is not None)
    seed = [bytes.fromhex(r["seed"])]
    prop, tries = e.compute_proposers(seed, n, r["rounds"], MAX_EFF, r["tries"])
    assert (int(prop[0]), int(tries[0])) == (NONE32, r["tries"])
    prop, tries = e.compute_proposers(seed, n, r["rounds"], MAX_EFF, r["tries"] + 1)
    assert (int(prop[0]), int(tries[0])) == (r["proposer"], r["tries"])


def test_proposers_follow_the_working_state_view(engine_factory):
    """Before state_set_validators the sampling reads set_validators' balances, after it the view's."""
    n = 300
    rng = np.random.default_rng(7)
    e = engine_factory()
    reg = _balances("mixed", n, rng)
    e.set_validators(reg, np.ones(n, dtype=np.uint8))
    seeds = _seeds("view", 8)
    before, _ = _check_against_model(e, seeds, n, reg, 10)
    view = np.roll(reg, 11)
    view[:5] = 0
    e.state_set_validators(view, np.ones(n, dtype=np.uint8))
    after, _ = _check_against_model(e, seeds, n, view, 10)
    assert not np.array_equal(before, after)
    e.set_balances(np.full(n, 32 * ETH, dtype=np.uint64), np.ones(n, dtype=np.uint8))   # the registry moves, the view stays
    _check_against_model(e, seeds, n, view, 10)


def test_proposers_validate_the_active_set(engine_factory):
    import pos_evolution_amd as pea
    n = 64
    e = engine_factory()
    bal = np.full(n, 32 * ETH, dtype=np.uint64)
    e.set_validators(bal, np.ones(n, dtype=np.uint8))
    seed = _seeds("bad", 1)
    for bad in ([1, 1, 2], [3, 2, 2], [0, n], n + 1):    # duplicated (sorted or not), out of range, more than the registry
        with pytest.raises(pea.EngineError):
            e.compute_proposers(seed, bad if isinstance(bad, int) else np.array(bad, dtype=np.uint32), 10)
        with pytest.raises(pea.EngineError):             # ... exactly what compute_committees refuses
            e.compute_committees(5, seed[0], bad if isinstance(bad, int) else np.array(bad, dtype=np.uint32), 32, 10)
    with pytest.raises(pea.EngineError):
        e.compute_proposers(seed, 0, 10)                                      # assert len(indices) > 0 (pe:608)
    with pytest.raises(pea.EngineError):
        e.compute_proposers(seed, np.zeros(0, dtype=np.uint32), 10)
    with pytest.raises(pea.EngineError):
        e.compute_proposers(seed, n, 256)                                     # the round is a uint8
    # distinct but unsorted is a valid index list for both calls: candidate = indices[shuffled(i)]
    perm = np.random.default_rng(1).permutation(n).astype(np.uint32)
    _check_against_model(e, seed, perm, bal, 10)
    prop, tries = e.compute_proposers([], n, 10)
    assert prop.size == 0 and tries.size == 0


def test_proposers_million_validators(engine_factory):
    n = 1 << 20
    e = engine_factory()
    bal = synth.balances(n, 3)
    e.set_validators(bal, synth.validator_flags(n, 3))
    seeds = _seeds("million", 32)
    e.compute_proposers(seeds[:1], n, 90)    # first use: the code object is loaded
    t0 = time.perf_counter()
    prop, tries = e.compute_proposers(seeds, n, 90)
    dt = time.perf_counter() - t0
    print(f"\n1M validators, 32 seeds, 90 rounds, 32 ETH flat (one batch): pe_compute_proposers {dt * 1e3:.3f} ms")
    bal_list = bal.tolist()
    index_list = range(n)
    for k, seed in enumerate(seeds):
        assert (int(prop[k]), int(tries[k])) == M.proposer(index_list, bal_list, seed, 90, MAX_EFF)
    # the config-5 mix against a cap of 65535 ETH: nearly every candidate is refused, several batches per seed
    mixed = synth.balances(n, 3, mixed=True)
    e.state_set_validators(mixed, np.ones(n, dtype=np.uint8))
    t0 = time.perf_counter()
    prop, tries = e.compute_proposers(seeds[:16], n, 90, 65535 * ETH)
    dt = time.perf_counter() - t0
    print(f"1M validators, 16 seeds, 90 rounds, mixed balances against 65535 ETH (up to {int(tries.max()) // 64 + 1} batches): "
          f"pe_compute_proposers {dt * 1e3:.3f} ms")
    mixed_list = mixed.tolist()
    for k, seed in enumerate(seeds[:16]):
        assert (int(prop[k]), int(tries[k])) == M.proposer(index_list, mixed_list, seed, 90, 65535 * ETH)
    assert int(tries.max()) >= 64


# ---------------------------------------------------------------- effective balances
def _threshold_vectors(n, rng):
    """eff / balance pairs of the golden threshold row, repeated or cut to n, then shuffled."""
    row = next(r for r in HYSTERESIS_ROWS if r["tag"] == "thresholds")
    pick = rng.permutation(np.resize(np.arange(len(row["eff"])), n))
    return np.array(row["eff"], dtype=np.uint64)[pick], np.array(row["balances"], dtype=np.uint64)[pick]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099])
def test_effective_balance_updates_vs_model(engine_factory, n):
    import pos_evolution_amd as pea
    rng = np.random.default_rng(n)
    e = engine_factory()
    flags = rng.choice(np.array([0, 1, 1, 1, 3], dtype=np.uint8), size=n)
    reg = rng.integers(0, 33, size=n).astype(np.uint64) * np.uint64(ETH)
    e.set_validators(reg, flags)
    tree = synth.random_tree(24, 5, "branchy")
    H.load_tree(e, tree)
    if n >= 255:   # latest messages, so that the weights are not all zero
        H.install_votes(e, tree, synth.random_committees(n, 32, 5), synth.zipf_votes(n, 24, 5))
    weights = e.get_weights()
    assert n < 255 or weights.any()

    # 1. the view still mirrors the registry: it is materialised from it, flags included
    _, view_flags, is_set = e.state_validators()
    assert not is_set
    bal = np.clip(reg.astype(np.int64) + rng.integers(-3 * ETH, 3 * ETH, size=n), 0, None).astype(np.uint64)
    want, want_changed = M.effective_balance_updates(bal, reg, ETH, 4, 1, 5, MAX_EFF)
    n_changed, new = e.effective_balance_updates(bal)
    assert n_changed == want_changed and np.array_equal(new, want)
    s_bal, s_flags, is_set = e.state_validators()
    assert is_set and np.array_equal(s_bal, want) and np.array_equal(s_flags, view_flags)
    active = (s_flags & 1) != 0
    assert e.ffg_balances()[0] == max(ETH, int(want[active].sum(dtype=np.uint64)))
    assert np.array_equal(e.get_weights(), weights)          # the justified-state balances are untouched
    # 2. the same balances again: inside the band, nothing moves
    assert e.effective_balance_updates(bal, want_result=False) == (0, None)
    assert np.array_equal(e.state_validators()[0], want)

    # 3. the threshold vectors over a view of their own
    eff, bal = _threshold_vectors(n, rng)
    e.state_set_validators(eff, s_flags)
    want, want_changed = M.effective_balance_updates(bal, eff, ETH, 4, 1, 5, MAX_EFF)
    n_changed, new = e.effective_balance_updates(bal)
    assert n_changed == want_changed and np.array_equal(new, want)
    s_bal, _, is_set = e.state_validators()
    assert is_set and np.array_equal(s_bal, want)
    assert e.ffg_balances()[0] == max(ETH, int(want[active].sum(dtype=np.uint64)))
    assert np.array_equal(e.get_weights(), weights)
    assert e.effective_balance_updates(bal)[0] == 0

    # 4. other constants
    want2, changed2 = M.effective_balance_updates(bal, want, ETH, 8, 3, 7, 20 * ETH)
    n_changed, new = e.effective_balance_updates(bal, 20 * ETH, 8, 3, 7)
    assert n_changed == changed2 and np.array_equal(new, want2)

    # 5. refused calls leave the view as it was
    for args in ((bal[:-1] if n > 1 else np.zeros(2, dtype=np.uint64),), (bal, 65536 * ETH), (bal, MAX_EFF, 0)):
        with pytest.raises(pea.EngineError):
            e.effective_balance_updates(*args)
    s_bal, s_flags2, is_set = e.state_validators()
    assert is_set and np.array_equal(s_bal, want2) and np.array_equal(s_flags2, s_flags)


def test_effective_balance_updates_golden_vectors(engine_factory):
    for r in HYSTERESIS_ROWS:
        n = len(r["eff"])
        e = engine_factory(effective_balance_increment=r["increment"])
        e.set_validators(np.array(r["eff"], dtype=np.uint64), np.ones(n, dtype=np.uint8))
        n_changed, new = e.effective_balance_updates(np.array(r["balances"], dtype=np.uint64), r["max_eff"], r["quotient"],
                                                     r["down"], r["up"])
        assert new.tolist() == r["new"] and n_changed == r["n_changed"], r["tag"]


def test_effective_balance_updates_feed_the_flag_passes_and_the_sampling(engine_factory):
    """The u16 increments and d_sbalance are one view: after an update the proposer sampling reads the new balances."""
    n = 257
    rng = np.random.default_rng(3)
    e = engine_factory()
    reg = np.full(n, 32 * ETH, dtype=np.uint64)
    e.set_validators(reg, np.ones(n, dtype=np.uint8))
    bal = rng.choice(np.array([0, 1, 16, 40], dtype=np.uint64), size=n) * np.uint64(ETH)
    bal[0] = 40 * ETH
    _, new = e.effective_balance_updates(bal)
    assert np.array_equal(new, np.minimum(bal, np.uint64(MAX_EFF)))
    _check_against_model(e, _seeds("after", 4), n, new, 10)


def test_million_validator_balance_update(engine_factory):
    n = 1 << 20
    rng = np.random.default_rng(20)
    e = engine_factory()
    reg = synth.balances(n, 3)
    e.set_validators(reg, synth.validator_flags(n, 3))
    bal = (reg.astype(np.int64) + rng.integers(-2 * ETH, 2 * ETH, size=n)).astype(np.uint64)
    e.effective_balance_updates(reg, want_result=False)    # first use: staging block sized, nothing moves
    t0 = time.perf_counter()
    n_changed, _ = e.effective_balance_updates(bal, want_result=False)
    dt = time.perf_counter() - t0
    print(f"\n1M validators: pe_effective_balance_updates (8 MB of balances staged, no read-back) {dt * 1e3:.3f} ms")
    want, want_changed = M.effective_balance_updates(bal, reg, ETH, 4, 1, 5, MAX_EFF)
    assert n_changed == want_changed and np.array_equal(e.state_validators()[0], want)


# ---------------------------------------------------------------- the pyspec-level mirror
def test_forkchoice_mirror(engine_factory):
    from pos_evolution_amd import forkchoice as fc
    n = 200
    rng = np.random.default_rng(11)
    eff = (rng.choice([0, 1, 16, 31, 32], size=n) * ETH).tolist()
    eff[0] = 32 * ETH
    balances = [max(0, b + int(d)) for b, d in zip(eff, rng.integers(-2 * ETH, 2 * ETH, size=n))]
    validators = [SimpleNamespace(effective_balance=b, slashed=False, activation_epoch=0, exit_epoch=2**64 - 1) for b in eff]
    cp = SimpleNamespace(epoch=0, root=bytes(32))
    state = SimpleNamespace(slot=64, validators=validators, balances=balances,
                            current_epoch_participation=[0] * n, previous_epoch_participation=[0] * n,
                            current_justified_checkpoint=cp, previous_justified_checkpoint=cp)
    e = engine_factory()
    e.set_validators(np.array(eff, dtype=np.uint64), np.ones(n, dtype=np.uint8))
    with pytest.raises(AssertionError):
        fc.compute_proposer_index(state, list(range(n)), bytes(32))            # not bound
    fc.bind_state(e, state, bytes(32), 1000)
    indices = sorted(int(x) for x in rng.choice(n, size=150, replace=False))
    for seed in _seeds("mirror", 4):
        assert fc.compute_proposer_index(state, indices, seed) == M.proposer(indices, eff, seed, 90, MAX_EFF)[0]
    with pytest.raises(AssertionError):
        fc.compute_proposer_index(state, [], bytes(32))                        # pe:608
    nobody = [i for i in range(n) if eff[i] == 0]
    exhausted = next(s for s in _seeds("nobody", 64) if M.proposer(nobody, eff, s, 90, MAX_EFF, 64)[0] is None)
    with pytest.raises(AssertionError):
        fc.compute_proposer_index(state, nobody, exhausted, max_tries=64)      # 0xFFFFFFFF: the reference would not return
    want, _ = M.effective_balance_updates(balances, eff, ETH, 4, 1, 5, MAX_EFF)
    fc.process_effective_balance_updates(state)
    assert [v.effective_balance for v in state.validators] == want.tolist()
    assert np.array_equal(e.state_validators()[0], want)
    seed = _seeds("mirror", 1)[0]
    assert fc.compute_proposer_index(state, indices, seed) == M.proposer(indices, want.tolist(), seed, 90, MAX_EFF)[0]
