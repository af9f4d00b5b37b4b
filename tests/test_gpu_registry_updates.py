"""-m gpu: pe_registry_updates and pe_process_slashings (registry_kernels.hip) against tests/registry_updates_model.py, bit
for bit: the five arrays after the call and every word of both stats structs.  There is no tolerance anywhere in this file.

256 = the validators of one workgroup (REGISTRY_WG), 1024 = the workgroup counts one pass of the scan takes
(ACTIVE_SCAN_TILE): 256 * 1024 + 257 validators are the first registry whose counts need a second scan tile, with a ragged
tail in both."""
import importlib.util
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd as pea
from pos_evolution_amd import engine as E
from tests import registry_model as RM
from tests import registry_updates_model as M
from tests import ssz_model as SSZ

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, pea._abi.PE_ERR_STATE
CUR, FIN = 20, 18
SHAPES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 65537, 256 * 1024 + 257]
ARRAYS = ("elig", "act", "ext", "wdr", "bal")


def test_the_tiles_are_the_kernels():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pos_evolution_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"REGISTRY_WG\s*=\s*(\d+)", text).group(1)) == 256
    assert int(re.search(r"ACTIVE_SCAN_TILE\s*=\s*(\d+)", text).group(1)) == 1024


def load(e, a, cur, static=True, epochs=True, balances=True, keys=None):
    n = a["eff"].size
    flags = M.view_flags(a, cur)
    e.set_validators(a["eff"], (flags & 3).astype(np.uint8))
    e.state_set_validators(a["eff"], flags)
    if epochs:
        e.registry_set_epochs(a["act"], a["ext"])
    if balances:
        e.state_set_balances(a["bal"], None, a["wdr"])
    if static:
        pk = np.zeros((n, 48), dtype=np.uint8) if keys is None else keys[0]
        wc = np.zeros((n, 32), dtype=np.uint8) if keys is None else keys[1]
        e.registry_set_static(pk, wc, a["elig"])
    return flags


def read(e):
    act, ext, _ = e.registry_get_epochs()
    bal, _, wdr, _ = e.state_get_balances()
    return dict(elig=e.registry_static()[2], act=act, ext=ext, wdr=wdr, bal=bal)


def assert_arrays(e, want):
    got = read(e)
    for k in ARRAYS:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (k, int(bad[0]), int(got[k][bad[0]]), int(want[k][bad[0]]))


def check_updates(e, a, cur, fin, p):
    """One call held to the model; -> (the registry after it, the stats)."""
    want, st = M.registry_updates_numpy(a, cur, fin, p)
    got = e.registry_updates(cur, fin, p.abi())
    assert got == st, (got, st)
    assert_arrays(e, want)
    return want, st


def status_of(call, *args, **kw):
    try:
        call(*args, **kw)
    except pea.EngineError as err:
        return err.status
    return 0


# ---------------------------------------------------------------- shape edges
@pytest.mark.parametrize("n", SHAPES)
def test_registry_updates_at_the_shape_edges(engine_factory, n):
    p = M.Params(min_per_epoch_churn_limit=3, max_per_epoch_activation_churn_limit=5 if n % 2 else 0)
    a, counters = M.random_registry(n, 7000 + n, CUR, FIN, p)
    if n >= 256:
        assert M.every_class_occurred(counters), counters
    e = engine_factory()
    load(e, a, CUR)
    want, st = check_updates(e, a, CUR, FIN, p)
    if n >= 256:
        assert st["n_ejected"] > 3 and st["last_exit_epoch"] > st["first_exit_epoch"]
        assert st["queue_len"] > st["n_activated"] > 0 and st["n_marked_eligible"] > 0
    # a second call over what the first left: the exits just set are the queue's end now, the marks are not marks again
    check_updates(e, want, CUR, FIN, p)
    e.close()


@pytest.mark.parametrize("n", SHAPES)
def test_slashings_at_the_shape_edges(engine_factory, n):
    a, counters = M.random_registry(n, 8000 + n, CUR, FIN, vector=64)
    e = engine_factory()
    flags = load(e, a, CUR, static=False, epochs=False)
    total = RM.total_balance(a["eff"], (flags & 1) != 0)
    before = read_balances_only(e)
    for sum_slashings in (0, total // 3 - 1, total):          # adj = 0; 3 * sum < total; 3 * sum > total: both sides of the min
        want, st = M.slashings_numpy(a, flags, CUR, sum_slashings, 3, 64)
        got = e.process_slashings(CUR, sum_slashings, 3, 64)
        assert got == st, (got, st)
        bal, _, wdr, _ = e.state_get_balances()
        assert np.array_equal(bal, want) and np.array_equal(wdr, a["wdr"])
        assert st["adjusted_total_slashing_balance"] == min(3 * sum_slashings, total)
        hit = (a["slashed"] != 0) & (a["wdr"] == np.uint64(CUR + 32))
        assert np.array_equal(bal[~hit], a["bal"][~hit])      # the neighbours of the target and the unslashed at it: untouched
        if n >= 256 and sum_slashings == total:
            assert counters["slashed_before"] and counters["slashed_after"] and counters["unslashed_at"]
            assert st["n_penalised"] == counters["slashed_at"] > 0 and 0 < st["n_saturated"] < st["n_penalised"]
        e.state_set_balances(before[0], None, before[1])
    e.close()


def read_balances_only(e):
    bal, _, wdr, _ = e.state_get_balances()
    return bal.copy(), wdr.copy()


# ---------------------------------------------------------------- the exit queue
@pytest.mark.parametrize("L", [1, 2, 5])
def test_exit_queue_edges(engine_factory, L):
    e = engine_factory()
    for c0 in sorted({0, L - 1, L, L + 1}):
        for e0_beyond in (False, True):       # E0 = the look-ahead epoch (no exit set anywhere when c0 == 0) | an exit beyond it
            fill = 0 if c0 >= L else c0
            for n_eject, interleave in [(k, i) for k in sorted({0, 1, L - fill, L - fill + 1, 3 * L + 2}) for i in (False, True)]:
                a, p = M.exit_queue_case(300, CUR, L, c0, e0_beyond, n_eject, interleave)
                load(e, a, CUR)
                want, st = check_updates(e, a, CUR, FIN, p)
                assert st["n_ejected"] == n_eject
                if c0 == 0 and not e0_beyond and not interleave:
                    assert (a["ext"] == np.uint64(M.FAR)).all() and (n_eject == 0 or st["first_exit_epoch"] == CUR + 5)
                if n_eject > 3 * L:
                    assert st["last_exit_epoch"] >= st["first_exit_epoch"] + 2     # spills over several epochs


def test_ejections_across_wave_and_workgroup_seams(engine_factory):
    """Ranks 1 | 2 on lanes 63 | 64 and 5 | 6 on lanes 255 | 256, with two exits per epoch: the epoch steps on both seams."""
    p = M.Params(min_per_epoch_churn_limit=2)
    a = M.blank_registry(600, p)
    lanes = np.array([62, 63, 64, 65, 254, 255, 256, 257, 599])
    a["eff"][lanes] = p.ejection_balance
    a["eff"][[100, 300]] = p.ejection_balance          # ... and two whose exit is already set, between them: k stays
    a["ext"][[100, 300]] = CUR + 1
    e = engine_factory()
    load(e, a, CUR)
    want, st = check_updates(e, a, CUR, FIN, p)
    base = CUR + 5
    assert [int(x) for x in want["ext"][lanes]] == [base, base, base + 1, base + 1, base + 2, base + 2, base + 3, base + 3, base + 4]
    assert st["n_ejected"] == 9 and int(want["ext"][100]) == CUR + 1


# ---------------------------------------------------------------- the activation queue
def queue_case(n, queued, eligs, p):
    a = M.blank_registry(n, p)
    a["act"][queued] = M.FAR
    a["elig"][queued] = eligs
    return a


def test_activation_queue_lengths(engine_factory):
    p = M.Params(min_per_epoch_churn_limit=12, max_per_epoch_activation_churn_limit=8)
    A = 8
    e = engine_factory()
    rng = np.random.default_rng(5)
    for queue_len in (0, A - 1, A, A + 1, 50 * A):
        queued = np.sort(rng.choice(1500, size=queue_len, replace=False))
        a = queue_case(1500, queued, rng.integers(FIN - 3, FIN + 1, size=queue_len, dtype=np.uint64), p)
        load(e, a, CUR)
        want, st = check_updates(e, a, CUR, FIN, p)
        assert st["queue_len"] == queue_len and st["n_activated"] == min(A, queue_len)


@pytest.mark.parametrize("cap,cut_after", [(4, 63), (8, 255), (10, 257)])
def test_a_tie_on_the_threshold_straddles_the_seams(engine_factory, cap, cut_after):
    """Twelve queued validators with ONE eligibility epoch on lanes 60 .. 65, 254 .. 257, 300 and 520 -- two waves, two
    workgroups -- and the cut between 63 | 64, 255 | 256 or behind 257; then the same with a later index that was eligible
    earlier and goes first, and with eligibility FIN + 1 that is not queued at all."""
    p = M.Params(min_per_epoch_churn_limit=12, max_per_epoch_activation_churn_limit=cap)
    queued = np.array([60, 61, 62, 63, 64, 65, 254, 255, 256, 257, 300, 520])
    e = engine_factory()
    a = queue_case(600, queued, FIN, p)
    load(e, a, CUR)
    want, st = check_updates(e, a, CUR, FIN, p)
    taken = queued[want["act"][queued] != np.uint64(M.FAR)]
    assert taken.size == cap and taken[-1] == cut_after and (taken == queued[:cap]).all()
    a["elig"][520] = FIN - 1                              # later index, earlier epoch
    a["elig"][60] = FIN + 1                               # one epoch too late: out
    load(e, a, CUR)
    want, st = check_updates(e, a, CUR, FIN, p)
    assert st["queue_len"] == 11 and int(want["act"][520]) == CUR + 5 and int(want["act"][60]) == M.FAR
    assert int((want["act"][queued] != np.uint64(M.FAR)).sum()) == cap


def test_activation_cap_against_the_churn_limit(engine_factory):
    e = engine_factory()
    queued = np.arange(3, 600, 13)
    for cap, want_n in ((0, 12), (8, 8)):
        p = M.Params(min_per_epoch_churn_limit=12, max_per_epoch_activation_churn_limit=cap)
        a = queue_case(600, queued, FIN - (queued % 3).astype(np.uint64), p)
        load(e, a, CUR)
        want, st = check_updates(e, a, CUR, FIN, p)
        assert st["churn_limit"] == 12 and st["activation_churn_limit"] == want_n == st["n_activated"]


def test_selection_over_high_bytes(engine_factory):
    """finalized_epoch >= 2^16: three byte passes, and queued epochs that differ in byte 2 or byte 1 alone."""
    fin, cur = 0x030005, 0x030009
    p = M.Params(min_per_epoch_churn_limit=5)
    queued = np.arange(1, 1200, 9)
    eligs = np.array([0x010005, 0x020005, 0x030005, 0x000005, 0x020105, 0x020004], dtype=np.uint64)[np.arange(queued.size) % 6]
    e = engine_factory()
    a = queue_case(1200, queued, eligs, p)
    load(e, a, cur)
    want, st = check_updates(e, a, cur, fin, p)
    took = queued[want["act"][queued] != np.uint64(M.FAR)]
    assert st["n_activated"] == 5 and (a["elig"][took] == np.uint64(5)).all()      # the five smallest: byte 2 decides
    p = M.Params(min_per_epoch_churn_limit=50)                                     # ... the cut inside 0x0200xx: byte 1, then 0
    load(e, a, cur)
    want, st = check_updates(e, a, cur, fin, p)
    assert st["n_activated"] == 50 and {int(x) for x in a["elig"][queued[want["act"][queued] != np.uint64(M.FAR)]]} >= {5, 0x010005, 0x020004}


# ---------------------------------------------------------------- failing calls change nothing
def test_failing_calls_change_nothing(engine_factory):
    p = M.Params(min_per_epoch_churn_limit=3)
    a, _ = M.random_registry(1025, 77, CUR, FIN, p)
    seed = bytes(range(32))
    for missing in ("epochs", "balances", "static"):
        e = engine_factory()
        load(e, a, CUR, **{missing: False})
        assert status_of(e.registry_updates, CUR, FIN, p.abi()) == STATE, missing
        if missing == "balances":
            assert status_of(e.process_slashings, CUR, 10**12, 3, 64) == STATE
        # what IS resident reads back unchanged, and the missing part is still reported as not held
        act, ext, have_epochs = e.registry_get_epochs()
        bal, _, wdr, have_balances = e.state_get_balances()
        _, _, elig, have_static = e.registry_static()
        assert (have_epochs, have_balances, have_static) == tuple(missing != m for m in ("epochs", "balances", "static"))
        if have_epochs:
            assert np.array_equal(act, a["act"]) and np.array_equal(ext, a["ext"])
        if have_balances:
            assert np.array_equal(bal, a["bal"]) and np.array_equal(wdr, a["wdr"])
        if have_static:
            assert np.array_equal(elig, a["elig"])
        eff, fl, _ = e.state_validators()
        assert np.array_equal(eff, a["eff"]) and np.array_equal(fl, M.view_flags(a, CUR))
        e.close()
    e = engine_factory()
    load(e, a, CUR)
    n_active, _, _ = e.active_set(CUR)
    refusals = [(CUR, dict(churn_limit_quotient=0)), (M.FAR - 5, {}), (M.FAR - 1, {}),
                (CUR, dict(min_validator_withdrawability_delay=M.FAR - CUR - 6)), (CUR, dict(min_per_epoch_churn_limit=0))]
    for cur, over in refusals:
        assert status_of(e.registry_updates, cur, FIN, {**p.abi(), **over}) == INVALID, (cur, over)
        assert_arrays(e, a)
        e.compute_proposers([seed], pea.ACTIVE_RESIDENT, 10)              # the resident list is still valid
    flags = M.view_flags(a, CUR)
    for args in ((CUR, 2**63, 3, 64), (M.FAR - 3, 1, 3, 64), (CUR, 2**63, 2, 64)):
        with pytest.raises(ValueError):
            M.slashings_numpy(a, flags, *args)
        assert status_of(e.process_slashings, *args) == INVALID, args
        assert_arrays(e, a)
    # the penalty's product: eight validators of 60000 increments make total, and with it adj, exceed 2^64 / 60000
    rich = M.blank_registry(1025, p)
    rich["eff"][:8] = 60000 * M.ETH
    rich["slashed"][0], rich["wdr"][0] = 1, CUR + 32
    flags = load(e, rich, CUR)
    with pytest.raises(ValueError):
        M.slashings_numpy(rich, flags, CUR, 2**62, 3, 64)
    assert status_of(e.process_slashings, CUR, 2**62, 3, 64) == INVALID
    assert_arrays(e, rich)
    want_bal, sst = M.slashings_numpy(rich, flags, CUR, 10**13, 3, 64)       # ... and below the bound the call stands
    assert e.process_slashings(CUR, 10**13, 3, 64) == sst and sst["penalties"] > 0
    assert np.array_equal(e.state_get_balances()[0], want_bal)
    # a call that writes only marks keeps the resident list; one that writes an epoch drops it
    quiet = M.blank_registry(1025, p)
    quiet["elig"][[5, 700]] = M.FAR
    load(e, quiet, CUR)
    e.active_set(CUR)
    want, st = check_updates(e, quiet, CUR, FIN, p)
    assert st["n_marked_eligible"] == 2 and st["n_ejected"] == 0 and st["n_activated"] == 0
    e.compute_proposers([seed], pea.ACTIVE_RESIDENT, 10)
    want["eff"][9] = p.ejection_balance
    load(e, want, CUR)
    e.active_set(CUR)
    check_updates(e, want, CUR, FIN, p)
    assert status_of(e.compute_proposers, [seed], pea.ACTIVE_RESIDENT, 10) == STATE
    e.close()


# ---------------------------------------------------------------- the boundary as a chain
def test_the_boundary_as_a_chain(engine_factory):
    """Three epochs on one handle.  Between the boundaries the epoch's flag passes are stood in for by fresh participation
    bytes in both lists, and the scores start above the recovery rate, so that every one of the five lists changes in every
    epoch and all five roots must move.  The rewards and the hysteresis rule are test_gpu_rewards.py's and
    test_gpu_epoch.py's: their results are read back and carried into the model's arrays."""
    n, vector = 4097, 64
    p = M.Params(min_per_epoch_churn_limit=3, max_per_epoch_activation_churn_limit=2)
    a, _ = M.random_registry(n, 4097, CUR, FIN, p, vector=vector)
    rng = np.random.default_rng(3)
    pk = rng.integers(0, 256, size=(n, 48), dtype=np.uint8)
    wc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    e = engine_factory()
    flags = load(e, a, CUR, keys=(pk, wc))
    e.state_set_balances(a["bal"], rng.integers(100, 1000, size=n, dtype=np.uint64), a["wdr"])
    previous_roots = None
    for step in range(3):
        cur, fin = CUR + step, FIN + step
        part_prev, part_cur = (rng.integers(0, 8, size=n, dtype=np.uint8) for _ in range(2))
        e.participation_set(1, part_prev)
        e.participation_set(0, part_cur)
        e.rewards_and_penalties(cur, fin)
        bal, scores, _, _ = e.state_get_balances()
        a["bal"] = bal.copy()
        a, st = M.registry_updates_numpy(a, cur, fin, p)
        assert e.registry_updates(cur, fin, p.abi()) == st
        a["bal"], sst = M.slashings_numpy(a, flags, cur, 10**13, 3, vector)
        assert e.process_slashings(cur, 10**13, 3, vector) == sst
        assert_arrays(e, a)
        _, eff = e.effective_balance_updates(E.BALANCES_RESIDENT)
        a["eff"] = eff.copy()
        e.state_refresh_activity(cur + 1)
        flags = M.view_flags(a, cur + 1)
        assert np.array_equal(e.state_validators()[1], flags)
        n_active, _, idx = e.active_set(cur + 1, want_indices=True)
        assert np.array_equal(idx, RM.active_indices(a["act"], a["ext"], cur + 1)) and n_active == idx.size
        roots = e.state_roots(E.ROOT_ALL)
        leaves = [SSZ.validator_root(pk[v].tobytes(), wc[v].tobytes(), int(a["eff"][v]), int(a["slashed"][v]), int(a["elig"][v]),
                                     int(a["act"][v]), int(a["ext"][v]), int(a["wdr"][v])) for v in range(n)]
        want = {"validators": SSZ.validators_root(leaves), "balances": SSZ.u64_list_root([int(x) for x in a["bal"]]),
                "inactivity_scores": SSZ.u64_list_root([int(x) for x in scores]),
                "previous_epoch_participation": SSZ.u8_list_root([int(x) for x in part_prev]),
                "current_epoch_participation": SSZ.u8_list_root([int(x) for x in part_cur])}
        assert roots == want
        assert st["n_ejected"] or st["n_activated"] or st["n_marked_eligible"]            # the registry did change
        if previous_roots is not None:
            for name in want:
                assert roots[name] != previous_roots[name], name
        previous_roots = roots
    e.close()


# ---------------------------------------------------------------- the pyspec names over a bound state
def state_of(a, cur, fin, slots_per_epoch, slashings, rng):
    n = a["eff"].size
    validators = [SimpleNamespace(pubkey=rng.bytes(48), withdrawal_credentials=rng.bytes(32), effective_balance=int(a["eff"][v]),
                                  slashed=bool(a["slashed"][v]), activation_eligibility_epoch=int(a["elig"][v]),
                                  activation_epoch=int(a["act"][v]), exit_epoch=int(a["ext"][v]),
                                  withdrawable_epoch=int(a["wdr"][v])) for v in range(n)]
    cp = SimpleNamespace(epoch=0, root=bytes(32))
    return SimpleNamespace(slot=slots_per_epoch * cur + 3, validators=validators, balances=[int(x) for x in a["bal"]],
                           inactivity_scores=list(range(n)), slashings=list(slashings), current_epoch_participation=[0] * n,
                           previous_epoch_participation=[0] * n, current_justified_checkpoint=cp, previous_justified_checkpoint=cp,
                           finalized_checkpoint=SimpleNamespace(epoch=fin, root=bytes(32)))


def epochs_of(state):
    return {k: [int(getattr(v, name)) for v in state.validators]
            for k, name in (("elig", "activation_eligibility_epoch"), ("act", "activation_epoch"), ("ext", "exit_epoch"),
                            ("wdr", "withdrawable_epoch"))}


def test_the_forkchoice_mirror(engine_factory):
    """process_registry_updates(state), then process_slashings(state), under the pyspec's names on duck-typed states built
    from the committed vectors and from a random registry: the validators' four epochs, state.balances and both recorded
    stats against the SEQUENTIAL model; nothing else of the state moves; an unbound state is refused."""
    from pos_evolution_amd import forkchoice as fc
    spec = importlib.util.spec_from_file_location("generate_registry_updates", os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "golden", "generate_registry_updates.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    work = [(gen.from_json(c["registry"]), c["current_epoch"], c["finalized_epoch"], M.Params(**c["params"]), c["vector"])
            for c in json.load(open(M.GOLDEN_PATH))]
    p = M.Params(min_per_epoch_churn_limit=3, max_per_epoch_activation_churn_limit=2)
    work.append((M.random_registry(300, 31, CUR, FIN, p, vector=64)[0], CUR, FIN, p, 64))
    rng = np.random.default_rng(17)
    e = engine_factory()
    spe = int(e.cfg.slots_per_epoch)
    for a, cur, fin, p, vector in work:
        n = a["eff"].size
        slashings = [7 * M.ETH, 0, 10**13, 5]                      # the caller's vector: its SUM is what the engine is given
        state = state_of(a, cur, fin, spe, slashings, rng)
        e.set_validators(a["eff"], np.ones(n, dtype=np.uint8))
        with pytest.raises(AssertionError):
            fc.process_registry_updates(state)                     # not bound
        with pytest.raises(AssertionError):
            fc.process_slashings(state)
        assert epochs_of(state) == {k: [int(x) for x in a[k]] for k in ("elig", "act", "ext", "wdr")}
        fc.bind_state(e, state, bytes(32), 1000)
        want, st = M.registry_updates_sequential(a, cur, fin, p)
        fc.process_registry_updates(state, **p.abi())
        assert state._last_registry_stats == st
        assert epochs_of(state) == {k: [int(x) for x in want[k]] for k in ("elig", "act", "ext", "wdr")}
        assert state.balances == [int(x) for x in a["bal"]]        # not this function's
        bal, sst = M.slashings_sequential(want, M.view_flags(a, cur), cur, sum(slashings), 3, vector)
        fc.process_slashings(state, proportional_slashing_multiplier=3, epochs_per_slashings_vector=vector)
        assert state._last_slashings_stats == sst
        assert state.balances == [int(x) for x in bal]
        assert epochs_of(state) == {k: [int(x) for x in want[k]] for k in ("elig", "act", "ext", "wdr")}
        assert state.slashings == slashings and state.inactivity_scores == list(range(n))
        assert [v.effective_balance for v in state.validators] == [int(x) for x in a["eff"]]
        # what the engine holds after the two calls is the state's registry: its validators root is the model's
        leaves = [SSZ.validator_root(v.pubkey, v.withdrawal_credentials, v.effective_balance, v.slashed,
                                     v.activation_eligibility_epoch, v.activation_epoch, v.exit_epoch, v.withdrawable_epoch)
                  for v in state.validators]
        assert e.state_roots(E.ROOT_VALIDATORS)["validators"] == SSZ.validators_root(leaves)
        fc.unbind_state(state)
    e.close()


# ---------------------------------------------------------------- one million validators: the grid caps
def test_one_million_validators(engine_factory):
    n = 1 << 20
    p = M.Params(max_per_epoch_activation_churn_limit=8)
    a, counters = M.random_registry(n, 2**20, CUR, FIN, p, vector=64)
    assert M.every_class_occurred(counters)
    e = engine_factory()
    flags = load(e, a, CUR)
    want, st = check_updates(e, a, CUR, FIN, p)
    assert st["n_ejected"] > 1000 and st["queue_len"] > 1000 and st["n_activated"] == 8
    bal, sst = M.slashings_numpy(want, flags, CUR, 10**15, 3, 64)
    assert e.process_slashings(CUR, 10**15, 3, 64) == sst and sst["n_penalised"] > 1000
    assert np.array_equal(e.state_get_balances()[0], bal)
    e.close()
