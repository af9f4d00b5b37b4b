"""-m gpu: rewards and penalties over resident balances -- pe_state_set_balances / _get, pe_rewards_and_penalties
(k_reward_sums, the host step, k_reward_apply) and pe_effective_balance_updates(PE_BALANCES_RESIDENT) -- against
tests/rewards_model.py, bit for bit: balances, scores and all nine words of pe_rewards_stats.  Shapes: the wave and
workgroup edges of both kernels (1, 63, 64, 65, 255, 256, 257 validators), two workgroups of the first pass (4097), a
second grid-stride trip with a ragged tail behind 256 full workgroups (65537), and one million validators, where the
first pass runs at its cap of 256 workgroups and the second takes two trips."""
import ctypes as C
import json
import time
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from pos_evolution_amd._abi import pe_state_ctx
from tests import epoch_model as EM
from tests import rewards_model as M

pytestmark = pytest.mark.gpu
ETH = 10**9
MAX_EFF = 32 * ETH
WHICH = [M.DO_INACTIVITY, M.DO_DELTAS, M.DO_BOTH]


def stats_words(st: dict):
    return [st["total_active_balance"], *st["unslashed_balance"], st["n_eligible"], st["in_leak"], st["rewards"],
            st["penalties"], st["n_saturated"]]


def load(e, a):
    """A registry of rewards_model.random_registry's arrays into an engine: view, previous participation, resident arrays."""
    n = a["eff"].size
    e.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))
    e.state_set_validators(a["eff"], a["sflags"])
    e.participation_set(1, a["participation"])
    e.state_set_balances(a["balances"], a["scores"], a["withdrawable"])
    assert e.num_validators == n


def params_dict(p: M.Params):
    d = dict(vars(p))
    d.pop("increment")
    return d


def check_call(e, a, current, finalized, which, p=None):
    """One call against the numpy model -> (the model's Stats, the arrays after it)."""
    p = p or M.Params()
    want_bal, want_sc, want = M.run_numpy(**a, current_epoch=current, finalized_epoch=finalized, p=p, which=which)
    got = e.rewards_and_penalties(current, finalized, params_dict(p), which)
    bal, sc, wd, is_set = e.state_get_balances()
    assert is_set and np.array_equal(wd, a["withdrawable"])
    assert np.array_equal(sc, want_sc), np.flatnonzero(sc != want_sc)[:8]
    assert np.array_equal(bal, want_bal), np.flatnonzero(bal != want_bal)[:8]
    assert stats_words(got) == want.abi()
    return want, dict(a, balances=bal, scores=sc)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 65537])
def test_rewards_vs_model_at_the_kernels_shape_edges(engine_factory, n):
    e = engine_factory()
    current = 12
    a = M.random_registry(n, 100 + n, current)
    load(e, a)
    seen = M.Stats()
    for finalized in (10, 2):                    # out of a leak, in one
        for which in WHICH:
            e.state_set_balances(a["balances"], a["scores"], a["withdrawable"])
            st, _ = check_call(e, a, current, finalized, which)
            assert st.in_leak == (finalized == 2)
            for k in ("n_saturated", "n_slashed_eligible", "n_flag_rewards", "n_flag_penalties", "n_inactivity_penalties"):
                setattr(seen, k, getattr(seen, k) + getattr(st, k))
    if n >= 256:   # the inputs exercised every class: a test whose registry holds none of them proves nothing
        assert seen.n_saturated and seen.n_slashed_eligible and seen.n_flag_rewards and seen.n_flag_penalties
        assert seen.n_inactivity_penalties
        edge = M.get_previous_epoch(current) + 1
        assert len(set(a["sflags"].tolist())) == 8 and len(set((a["participation"] & 7).tolist())) == 8
        assert (a["participation"] & 0xF8).any() and {edge - 1, edge, edge + 1} <= set(a["withdrawable"].tolist())
    # the view and participation are read, never written
    s_bal, s_flags, _ = e.state_validators()
    assert np.array_equal(s_bal, a["eff"]) and np.array_equal(s_flags, a["sflags"])
    assert np.array_equal(e.participation_get(1), a["participation"])


def test_consecutive_epochs_compound(engine_factory):
    """Three calls in a row on one handle: each reads what the last one wrote."""
    e = engine_factory()
    a = M.random_registry(300, 7, 5)
    load(e, a)
    for current, finalized in ((5, 4), (6, 4), (11, 4)):
        _, a = check_call(e, a, current, finalized, M.DO_BOTH)


def test_genesis_epoch_launches_nothing(engine_factory):
    e = engine_factory()
    a = M.random_registry(100, 3, 0)
    load(e, a)
    st = e.rewards_and_penalties(0, 0)
    assert stats_words(st) == [0] * 9
    bal, sc, _, _ = e.state_get_balances()
    assert np.array_equal(bal, a["balances"]) and np.array_equal(sc, a["scores"])
    check_call(e, a, 1, 0, M.DO_BOTH)            # epoch 1: the previous epoch clamps to 0


def test_defaults_of_set_balances_and_params(engine_factory):
    e = engine_factory()
    n = 70
    a = M.random_registry(n, 4, 9)
    load(e, a)
    e.state_set_balances(a["balances"])          # scores: zeros, withdrawable: FAR_FUTURE_EPOCH
    bal, sc, wd, is_set = e.state_get_balances()
    assert is_set and np.array_equal(bal, a["balances"]) and not sc.any() and (wd == np.uint64(M.FAR_FUTURE_EPOCH)).all()
    p = e.rewards_params()
    assert (p.base_reward_factor, p.inactivity_score_bias, p.inactivity_score_recovery_rate, p.inactivity_penalty_quotient,
            p.min_epochs_to_inactivity_penalty) == (64, 4, 16, 2**24, 4)
    a = dict(a, scores=sc, withdrawable=wd)
    check_call(e, a, 9, 7, M.DO_BOTH)
    e.state_set_balances(a["balances"])
    check_call(e, a, 9, 1, M.DO_BOTH, M.Params(inactivity_penalty_quotient=3 * 2**24, base_reward_factor=32))


# ---------------------------------------------------------------- the recorded vectors
def _golden():
    return json.load(open(M.GOLDEN_PATH))


def test_golden_vectors_through_the_c_abi(engine_factory):
    engines = {}
    for c in _golden():
        reg = M.Registry(**c["registry"])
        n = len(reg.balances)
        if n not in engines:
            engines[n] = engine_factory()
        e = engines[n]
        a = dict(eff=np.array(reg.effective_balance, dtype=np.uint64), sflags=np.array(reg.sflags(), dtype=np.uint8),
                 participation=np.array(reg.participation, dtype=np.uint8),
                 withdrawable=np.array(reg.withdrawable_epoch, dtype=np.uint64),
                 balances=np.array(reg.balances, dtype=np.uint64), scores=np.array(reg.scores, dtype=np.uint64))
        load(e, a)
        p = dict(c["params"])
        assert p.pop("increment") == ETH
        st = e.rewards_and_penalties(c["current_epoch"], c["finalized_epoch"], p, c["which"])
        bal, sc, _, _ = e.state_get_balances()
        assert bal.tolist() == c["balances"] and sc.tolist() == c["scores"], c["name"]
        assert stats_words(st) == c["stats"], c["name"]


def _state_of(c):
    reg = c["registry"]
    far = 2**64 - 1
    validators = [SimpleNamespace(effective_balance=reg["effective_balance"][v], slashed=bool(reg["slashed"][v]),
                                  activation_epoch=0 if reg["active_prev"][v] else (c["current_epoch"] if reg["active_cur"][v] else far),
                                  exit_epoch=far if reg["active_cur"][v] else (c["current_epoch"] if reg["active_prev"][v] else far),
                                  withdrawable_epoch=reg["withdrawable_epoch"][v]) for v in range(len(reg["balances"]))]
    cp = SimpleNamespace(epoch=0, root=bytes(32))
    return SimpleNamespace(slot=32 * c["current_epoch"], validators=validators, balances=list(reg["balances"]),
                           inactivity_scores=list(reg["scores"]), current_epoch_participation=[0] * len(validators),
                           previous_epoch_participation=list(reg["participation"]), current_justified_checkpoint=cp,
                           previous_justified_checkpoint=cp, finalized_checkpoint=SimpleNamespace(epoch=c["finalized_epoch"], root=bytes(32)))


def test_golden_vectors_through_the_forkchoice_mirror(engine_factory):
    """process_inactivity_updates(state), then process_rewards_and_penalties(state): pyspec names on a duck-typed state
    whose validators carry activation / exit epochs that give the recorded activity."""
    from pos_evolution_amd import forkchoice as fc
    cases = [c for c in _golden() if c["which"] == M.DO_BOTH and c["name"].startswith("issue") and c["current_epoch"] >= 1]
    assert len(cases) >= 5
    e = engine_factory()
    for c in cases:
        state = _state_of(c)
        e.set_validators(np.array(c["registry"]["effective_balance"], dtype=np.uint64),
                         np.ones(len(state.validators), dtype=np.uint8))
        with pytest.raises(AssertionError):
            fc.process_rewards_and_penalties(state)            # not bound
        fc.bind_state(e, state, bytes(32), 1000)
        p = dict(c["params"])
        p.pop("increment")
        fc.process_inactivity_updates(state, **p)
        assert state.inactivity_scores == c["scores"] and state.balances == c["registry"]["balances"], c["name"]
        fc.process_rewards_and_penalties(state, **p)
        assert state.balances == c["balances"] and state.inactivity_scores == c["scores"], c["name"]
        assert state._last_rewards_stats["n_eligible"] == c["stats"][4]


# ---------------------------------------------------------------- failing calls change nothing
def test_failing_calls_change_nothing(engine_factory):
    n = 300
    a = M.random_registry(n, 8, 12)
    a["eff"] = a["eff"] * np.uint64(100)         # up to 3200 increments: room for base_reward * 26 * U to leave 64 bits
    a["scores"] = np.minimum(a["scores"], np.uint64(2**20 + 3))
    fresh = engine_factory()
    fresh.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))
    for call in (lambda: fresh.rewards_and_penalties(12, 10),                       # no resident balances
                 lambda: fresh.effective_balance_updates(pea.BALANCES_RESIDENT)):
        with pytest.raises(pea.EngineError) as err:
            call()
        assert err.value.status == pea._abi.PE_ERR_STATE
    assert fresh.state_get_balances()[3] is False

    e = engine_factory()
    load(e, a)

    def unchanged():
        bal, sc, wd, is_set = e.state_get_balances()
        assert is_set and np.array_equal(bal, a["balances"]) and np.array_equal(sc, a["scores"])
        assert np.array_equal(wd, a["withdrawable"])
        assert np.array_equal(e.state_validators()[0], a["eff"])

    def refused(status, call):
        with pytest.raises(pea.EngineError) as err:
            call()
        assert err.value.status == status, err.value
        unchanged()

    invalid = -1                                                                     # PE_ERR_INVALID_ARG
    refused(invalid, lambda: e.state_set_balances(a["balances"][:-1]))              # a wrong n
    refused(invalid, lambda: e.state_set_balances(np.zeros(n + 1, dtype=np.uint64)))
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, which=0))
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, which=4))
    refused(invalid, lambda: e.rewards_and_penalties(12, 12))                        # finalized after the previous epoch
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, dict(inactivity_score_bias=0)))
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, dict(inactivity_penalty_quotient=2**63)))
    # the two overflow refusals, decided between the kernels: base_reward * 26 * U, and effective_balance * score
    big_factor = M.Params(base_reward_factor=2**34)
    with pytest.raises(OverflowError):
        M.run_numpy(**a, current_epoch=12, finalized_epoch=10, p=big_factor)
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, params_dict(big_factor)))
    eligible = np.flatnonzero((a["sflags"] & M.VAL_ACTIVE_PREV) != 0)
    worst = eligible[np.argmax(a["eff"][eligible])]
    big = dict(a, scores=a["scores"].copy())
    big["scores"][worst] = 2**64 // int(a["eff"][worst]) + 1
    with pytest.raises(OverflowError):
        M.run_numpy(**big, current_epoch=12, finalized_epoch=10)
    e.state_set_balances(big["balances"], big["scores"], big["withdrawable"])
    saved, a = a, big
    refused(invalid, lambda: e.rewards_and_penalties(12, 10))
    refused(invalid, lambda: e.rewards_and_penalties(12, 10, which=M.DO_DELTAS))
    check_call(e, a, 12, 10, M.DO_INACTIVITY)                                       # no product without the deltas
    a = saved
    e.state_set_balances(a["balances"], a["scores"], a["withdrawable"])
    # a handle that exchanges with other ranks
    e.dist_init_custom(0, 1, lambda *args: 0, lambda *args: 0)
    refused(pea._abi.PE_ERR_STATE, lambda: e.rewards_and_penalties(12, 10))
    e.dist_destroy()
    check_call(e, a, 12, 10, M.DO_BOTH)                                             # ... and after all of them the call stands


def test_the_arrays_are_dropped_where_the_view_is(engine_factory):
    e = engine_factory()
    a = M.random_registry(64, 2, 5)
    load(e, a)
    e.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))                  # the same size: kept
    assert e.state_get_balances()[3]
    e.set_validators(a["eff"][:-1], (a["sflags"][:-1] & 3).astype(np.uint8))        # another size: dropped
    assert not e.state_get_balances()[3]
    with pytest.raises(pea.EngineError):
        e.rewards_and_penalties(5, 4)
    e.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))
    load(e, a)
    e.store_init(0, 0, bytes(32))                                                   # a new store: dropped
    assert not e.state_get_balances()[3]


# ---------------------------------------------------------------- PE_BALANCES_RESIDENT
def _threshold_registry(n, seed, current):
    """random_registry with effective balances and balances on both sides of each hysteresis edge (the golden threshold
    row of tests/golden/epoch_vectors.json, as tests/test_gpu_epoch.py builds its vectors)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_epoch.py")
    spec_ = importlib.util.spec_from_file_location("generate_epoch", path)
    gen = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(gen)
    row = next(r for r in gen.load()[1] if r["tag"] == "thresholds")
    rng = np.random.default_rng(seed)
    pick = rng.permutation(np.resize(np.arange(len(row["eff"])), n))
    a = M.random_registry(n, seed, current)
    a["eff"] = np.array(row["eff"], dtype=np.uint64)[pick]
    a["balances"] = np.array(row["balances"], dtype=np.uint64)[pick]
    a["sflags"] = (a["sflags"] | M.VAL_ACTIVE).astype(np.uint8)
    return a


@pytest.mark.parametrize("n", [65, 257, 4099])
def test_balance_update_from_the_resident_vector_equals_the_host_route(engine_factory, n):
    """pe_rewards_and_penalties, then pe_effective_balance_updates(PE_BALANCES_RESIDENT) on one engine; on its twin the
    balances are downloaded and handed back from host memory.  Equal: n_changed, the effective balances, the FFG sums and
    what pe_compute_proposers samples from them.  (The u16 increments the next flag pass reads are compared by the
    end-to-end test below, through process_attestation's numerators.)"""
    current = 12
    a = _threshold_registry(n, n, current)
    # with no reward and a score of 0 the balances stay ON the threshold vectors for a third of the validators
    keep = np.arange(n) % 3 == 0
    a["scores"][keep] = 0
    a["participation"][keep] = 7
    res, twin = engine_factory(), engine_factory()
    for e in (res, twin):
        load(e, a)
        e.rewards_and_penalties(current, 2)      # a leak: no rewards; full participants with score 0 lose nothing
    bal, _, _, _ = twin.state_get_balances()
    still = keep & ((a["sflags"] & M.VAL_SLASHED) == 0) & ((a["sflags"] & M.VAL_ACTIVE_PREV) != 0)
    assert still.any() and np.array_equal(bal[still], a["balances"][still]) and not np.array_equal(bal, a["balances"])
    want, want_changed = EM.effective_balance_updates(bal, a["eff"], ETH, 4, 1, 5, MAX_EFF)
    assert 0 < want_changed < n
    got_res = res.effective_balance_updates(pea.BALANCES_RESIDENT)
    got_twin = twin.effective_balance_updates(bal)
    assert got_res[0] == got_twin[0] == want_changed
    assert np.array_equal(got_res[1], want) and np.array_equal(got_twin[1], want)
    assert np.array_equal(res.state_validators()[0], want) and np.array_equal(res.state_get_balances()[0], bal)
    assert res.effective_balance_updates(pea.BALANCES_RESIDENT, want_result=False) == (0, None)   # inside the band now
    seeds = [bytes([k]) * 32 for k in range(4)]
    for x, y in zip(res.compute_proposers(seeds, n, 10), twin.compute_proposers(seeds, n, 10)):
        assert np.array_equal(x, y)
    assert res.ffg_balances() == twin.ffg_balances()
    n_changed = C.c_uint64(0)
    with pytest.raises(pea.EngineError):                                             # n must be the registry's
        res._check(res._lib.pe_effective_balance_updates(res._h, n - 1, pea._abi.PE_BALANCES_RESIDENT, MAX_EFF, 4, 1, 5,
                                                         C.addressof(n_changed), None))
    assert np.array_equal(res.state_validators()[0], want)
    # other constants through the same argument
    want2, changed2 = EM.effective_balance_updates(bal, want, ETH, 8, 3, 7, 20 * ETH)
    assert res.effective_balance_updates(pea.BALANCES_RESIDENT, 20 * ETH, 8, 3, 7)[0] == changed2
    assert np.array_equal(res.state_validators()[0], want2)


# ---------------------------------------------------------------- two epochs end to end
class _Chain:
    """A small store with committees for two epochs, as the smoke run builds one."""

    def __init__(self, n_val, seed):
        self.n_val, self.spe, self.n_comm = n_val, 32, 64
        self.tree = synth.random_tree(96, seed, "branchy")
        self.epoch0 = int(self.tree.slot.max()) // self.spe + 1
        self.comm = [synth.random_committees(n_val, self.n_comm, seed + k) for k in range(2)]
        self.eff = synth.balances(n_val, seed, mixed=True)
        self.flags = synth.validator_flags(n_val, seed, inactive_frac=0.02)

    def start(self, e, balances, scores):
        e.store_init(0, 0, self.tree.roots[0].tobytes())
        for i in range(1, 96):
            e.add_block(self.tree.roots[i].tobytes(), self.tree.roots[int(self.tree.parent[i])].tobytes(), int(self.tree.slot[i]))
        e.set_validators(self.eff, self.flags, synth.registry_points(e, self.n_val))
        for k in range(2):
            e.set_committees(self.epoch0 + k, self.comm[k].offsets, self.comm[k].members)
        e.state_set_balances(balances, scores)

    def step(self, e, k):
        """The aggregate and flag passes of epoch0 + k's attestations, included in the epoch after it."""
        epoch = self.epoch0 + k
        e.on_tick((epoch + 1) * self.spe * 12)
        root0 = self.tree.roots[0].tobytes()
        atts, arena, _ = synth.epoch_attestations(self.comm[k], self.tree, epoch, self.spe, seed=1 + k, density=0.8, parts=2,
                                                  source=(0, root0))
        agg = e.aggregate(packed=(atts, arena))
        status, _, _ = e.on_attestation_batch(packed=(agg["atts"], agg["out_arena"]))
        ctx = pe_state_ctx()
        ctx.slot = (epoch + 1) * self.spe
        ctx.chain_tip_root[:] = self.tree.roots[95].tobytes()
        ctx.current_justified_root[:] = root0
        ctx.previous_justified_root[:] = root0
        ctx.base_reward_per_increment = 1000
        st, num = e.process_attestation_batch(ctx, packed=(agg["atts"], agg["out_arena"]))
        assert (status == 0).all() and (st == 0).all() and int(num.sum()) > 0
        return epoch + 1, num                    # get_current_epoch of the state that includes them | the proposer numerators


def test_two_epochs_end_to_end_with_checkpoint_resume(engine_factory):
    """Flag passes -> FFG sums -> rewards -> balance update -> rotation, twice on one handle with no per-validator
    download between the calls; a twin that reads everything back after every call feeds the model.  Then the resumed
    handle: pe_state_get_balances, pe_store_init, pe_state_set_balances reproduces the second epoch."""
    n = 3000
    rng = np.random.default_rng(5)
    chain = _Chain(n, 3)
    balances = (chain.eff.astype(np.int64) + rng.integers(-2 * ETH, 2 * ETH, size=n)).clip(0).astype(np.uint64)
    balances[rng.integers(0, n, 40)] = rng.integers(0, 9000, 40).astype(np.uint64)
    scores = rng.choice(np.array([0, 1, 15, 16, 17, 900], dtype=np.uint64), size=n)
    main, twin, resumed = engine_factory(), engine_factory(), engine_factory()
    for e in (main, twin):
        chain.start(e, balances, scores)
    far = np.full(n, M.FAR_FUTURE_EPOCH, dtype=np.uint64)
    p = M.Params(min_epochs_to_inactivity_penalty=0)
    saved = None
    for k in range(2):
        current, num_main = chain.step(main, k)
        _, num_twin = chain.step(twin, k)
        assert np.array_equal(num_main, num_twin)    # the flag pass read the same u16 increments on both
        finalized = current - 1 - k              # with min_epochs_to_inactivity_penalty = 0: no leak, then a leak
        # the model's inputs, from the twin
        eff, sflags, _ = twin.state_validators()
        part = twin.participation_get(1)
        assert (part & 7).any() and len(set((part & 7).tolist())) > 2
        bal0, sc0, wd0, _ = twin.state_get_balances()
        assert np.array_equal(wd0, far)
        if k == 1:
            saved = dict(eff=eff, sflags=sflags, part=part, bal=bal0, sc=sc0)
        want_bal, want_sc, want = M.run_numpy(eff, sflags, part, wd0, bal0, sc0, current, finalized, p)
        assert want.in_leak == k
        want_eff, want_changed = EM.effective_balance_updates(want_bal, eff, ETH, 4, 1, 5, MAX_EFF)
        for e in (main, twin):
            ffg = e.ffg_balances()
            st = e.rewards_and_penalties(current, finalized, params_dict(p))
            assert st["total_active_balance"] == ffg[0] and stats_words(st) == want.abi()
            assert st["unslashed_balance"][1] == ffg[1]                  # previous_target_balance, the same set
            # the main handle reads the vector where it lies; the twin downloads it and hands it back from host memory
            vector = pea.BALANCES_RESIDENT if e is main else e.state_get_balances()[0]
            assert e.effective_balance_updates(vector, want_result=False)[0] == want_changed
            e.participation_rotate()
        assert want_changed > 0
        assert want.rewards > 0 or k == 1
        assert want.penalties > 0
    for e in (main, twin):
        bal, sc, _, _ = e.state_get_balances()
        assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc)
        assert np.array_equal(e.state_validators()[0], want_eff)
        assert not e.participation_get(0).any()
    # checkpoint / resume: the state before the second boundary, handed to a handle whose store is initialised afterwards
    chain.start(resumed, balances, scores)
    resumed.state_set_balances(saved["bal"], saved["sc"], far)
    assert resumed.state_get_balances()[3]
    resumed.store_init(0, 0, chain.tree.roots[0].tobytes())              # drops the view, participation and the arrays
    assert not resumed.state_get_balances()[3]
    with pytest.raises(pea.EngineError):
        resumed.rewards_and_penalties(current, finalized, params_dict(p))
    resumed.state_set_validators(saved["eff"], saved["sflags"])
    resumed.participation_set(1, saved["part"])
    resumed.state_set_balances(saved["bal"], saved["sc"], far)
    st = resumed.rewards_and_penalties(current, finalized, params_dict(p))
    assert stats_words(st) == want.abi()
    assert resumed.effective_balance_updates(pea.BALANCES_RESIDENT, want_result=False)[0] == want_changed
    bal, sc, _, _ = resumed.state_get_balances()
    assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc)
    assert np.array_equal(resumed.state_validators()[0], want_eff)


# ---------------------------------------------------------------- a million validators
def test_million_validators_vs_numpy_model(engine_factory):
    n = 1 << 20
    e = engine_factory()
    a = M.random_registry(n, 21, 12)
    load(e, a)
    e.rewards_and_penalties(0, 0)                # first use of the library path; launches nothing
    want_bal, want_sc, want = M.run_numpy(**a, current_epoch=12, finalized_epoch=10)
    t0 = time.perf_counter()
    st = e.rewards_and_penalties(12, 10)
    dt = time.perf_counter() - t0
    print(f"\n1M validators: pe_rewards_and_penalties (two kernels and the host step between them; first launch, code "
          f"object load included) {dt * 1e3:.3f} ms wall -- not a kernel duration")
    bal, sc, _, _ = e.state_get_balances()
    assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc) and stats_words(st) == want.abi()
    assert want.n_saturated and want.n_slashed_eligible and want.n_flag_rewards and want.n_inactivity_penalties
    a2 = dict(a, balances=bal, scores=sc)
    want_bal, want_sc, want = M.run_numpy(**a2, current_epoch=13, finalized_epoch=3)
    t0 = time.perf_counter()
    st = e.rewards_and_penalties(13, 3)
    dt = time.perf_counter() - t0
    print(f"1M validators: pe_rewards_and_penalties, second call (a leak) {dt * 1e3:.3f} ms wall")
    bal, sc, _, _ = e.state_get_balances()
    assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc) and stats_words(st) == want.abi()
