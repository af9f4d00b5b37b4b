"""CPU: the model of the active validator set (tests/registry_model.py) and the scalar functions of
pos_evolution_amd/forkchoice.py that count it are pinned to the reference's own text -- get_committee_count_per_slot
(pe:461-468), compute_weak_subjectivity_period (pe:1257-1287), get_latest_weak_subjectivity_checkpoint_epoch (pe:1225-1241),
whose fences are taken from the reference's Markdown at test time and executed as they stand over the model
(tests/golden/generate_registry.py; nothing of that text is committed) -- and to tests/golden/registry_vectors.json, the
recorded answers of those fences, which travels everywhere.  The GPU tests (tests/test_gpu_registry.py) hold the engine to
the same model."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import ref_extract
from pos_evolution_amd import forkchoice as fc
from tests import registry_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ETH = 10**9


def _generator():
    spec_ = importlib.util.spec_from_file_location("generate_registry", os.path.join(HERE, "golden", "generate_registry.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


GEN = _generator()
ROWS = GEN.load()
needs_reference = pytest.mark.skipif(not ref_extract.reference_available(), reason="the reference's Markdown is not on this machine")


# ---------------------------------------------------------------- the golden file: coverage
def test_golden_covers_the_committee_count_clamps_and_the_worked_example():
    by_n = {r["n_active"]: r["count_per_slot"] for r in ROWS}
    assert by_n[0] == by_n[1] == by_n[4095] == by_n[4096] == by_n[8191] == 1      # max(1, ...): 0 and 1 both give 1
    assert by_n[8192] == 2
    assert by_n[262143] == 63 and by_n[262144] == 64                               # pe:472: 262 144 active -> 64 per slot
    assert by_n[262145] == by_n[1048576] == by_n[4194304] == 64                    # min(MAX_COMMITTEES_PER_SLOT, ...)


def test_golden_covers_both_branches_of_the_period():
    period = [r for r in ROWS if r["tag"] == "period"]
    sides = {32 * 230 < r["eff_eth"] * 320 for r in period}                        # pe:1274 with D = 10, T = 32
    assert sides == {True, False}
    assert {r["eff_eth"] for r in period} >= {23, 24}                              # the two averages next to the boundary
    assert any(r["n_active"] >= 262144 and r["churn_limit"] > 4 for r in period)   # a churn limit above its floor
    assert all(r["ws_period"] >= 256 for r in period)


def test_golden_covers_both_branches_of_the_checkpoint_epoch():
    cp = [r for r in ROWS if r["tag"] == "checkpoint"]
    assert {r["n_active"] >= 4 * 65536 for r in cp} == {True, False}               # pe:1235
    assert {262143, 262144} <= {r["n_active"] for r in cp}
    assert len({r["safety_decay"] for r in cp}) > 1 and len({r["finalized_epoch"] for r in cp}) > 2
    assert any(r["ws_checkpoint_epoch"] not in (0, r["finalized_epoch"]) for r in cp)


# ---------------------------------------------------------------- the model against the golden file
@pytest.mark.parametrize("k", range(len(ROWS)))
def test_model_equals_golden(k):
    r = ROWS[k]
    activation, exit_, eff = GEN.registry(r)
    epoch = r["slot"] // 32
    mask = M.active_mask(activation, exit_, epoch)
    idx = M.active_indices(activation, exit_, epoch)
    assert idx.size == r["n_active"] and np.array_equal(idx, np.arange(r["n_active"], dtype=np.uint32))
    assert M.total_balance(eff, mask, ETH) == r["total_active_balance"]
    assert M.churn_limit(idx.size) == r["churn_limit"]
    # the validators outside the list: exited in this very epoch, or activated in the next
    assert not M.active_mask(activation, exit_, epoch)[r["n_active"]:].any()
    assert M.active_mask(activation, exit_, epoch - 1)[r["n_active"]::2].all()
    assert M.active_mask(activation, exit_, epoch + 1)[r["n_active"] + 1::2].all()


def test_model_compares_unsigned_and_clamps_the_previous_epoch():
    top = 2**64 - 1
    activation = np.array([0, 5, top, 2**63, 2**63 - 1, 7, 0], dtype=np.uint64)
    exit_ = np.array([top, 6, top, top, 2**63, 3, 0], dtype=np.uint64)
    assert M.active_mask(activation, exit_, 5).tolist() == [True, True, False, False, False, False, False]
    assert M.active_mask(activation, exit_, 2**63).tolist() == [True, False, False, True, False, False, False]
    assert M.active_mask(activation, exit_, 2**63 - 1).tolist() == [True, False, False, False, True, False, False]
    flags = np.array([0x02, 0x0B, 0x09, 0, 0, 0x06, 0x01], dtype=np.uint8)
    assert M.activity_flags(activation, exit_, 5, flags).tolist() == [0x0B, 0x03, 0, 0, 0, 0x06, 0]
    assert M.activity_flags(activation, exit_, 6, flags).tolist() == [0x0B, 0x0A, 0, 0, 0, 0x06, 0]
    assert M.activity_flags(activation, exit_, 0, flags).tolist() == [0x0B, 0x02, 0, 0, 0, 0x06, 0]   # epoch 0 precedes itself
    assert M.total_balance([5, 7], [False, False], 3) == 3 and M.total_balance([5, 7], [True, True], 3) == 12


# ---------------------------------------------------------------- forkchoice.py's scalar functions, fed plain numbers
@pytest.mark.parametrize("k", range(len(ROWS)))
def test_forkchoice_scalars_equal_golden(k):
    r = ROWS[k]
    n = r["n_active"]
    assert fc.get_committee_count_per_slot(None, r["slot"] // 32, n_active=n) == r["count_per_slot"]
    assert fc.get_validator_churn_limit(None, n_active=n) == r["churn_limit"]
    got = fc.get_latest_weak_subjectivity_checkpoint_epoch(None, r["safety_decay"], n_active=n,
                                                           finalized_epoch=r["finalized_epoch"])
    assert got == r["ws_checkpoint_epoch"] and type(got) is type(r["ws_checkpoint_epoch"])
    if n:
        period = fc.compute_weak_subjectivity_period(None, n_active=n, total_active_balance=r["total_active_balance"])
        assert period == r["ws_period"] and type(period) is int
        ws_epoch = r["slot"] // 32
        assert fc.is_within_weak_subjectivity_period(ws_epoch + period, ws_epoch, period)
        assert not fc.is_within_weak_subjectivity_period(ws_epoch + period + 1, ws_epoch, period)
    else:
        with pytest.raises(ZeroDivisionError):     # pe:1268 divides by the count
            fc.compute_weak_subjectivity_period(None, n_active=0, total_active_balance=ETH)


def test_forkchoice_scalars_take_another_preset():
    minimal = dict(SLOTS_PER_EPOCH=8, MAX_COMMITTEES_PER_SLOT=4, TARGET_COMMITTEE_SIZE=4)
    assert [fc.get_committee_count_per_slot(None, 0, n_active=n, preset=minimal) for n in (0, 31, 63, 64, 128, 1000)] == [1, 1, 1, 2, 4, 4]
    assert fc.get_validator_churn_limit(None, n_active=100, preset=dict(MIN_PER_EPOCH_CHURN_LIMIT=2, CHURN_LIMIT_QUOTIENT=32)) == 3
    assert fc.is_active_validator(type("V", (), dict(activation_epoch=3, exit_epoch=5)), 3)
    assert not fc.is_active_validator(type("V", (), dict(activation_epoch=3, exit_epoch=5)), 5)


# ---------------------------------------------------------------- the reference's text
@needs_reference
def test_golden_file_is_what_the_reference_text_gives():
    """Byte for byte: the committed vectors are the output of the reference's three fences."""
    assert GEN.render() == open(GEN.OUT).read()


@needs_reference
def test_forkchoice_scalars_equal_the_reference_text():
    """Random registries, scattered active sets and balances: the fences over the model against forkchoice.py over the
    model's count and sum."""
    ns = GEN.reference_namespace()
    rng = np.random.default_rng(1257)
    for case in range(40):
        n_val = int(rng.integers(1, 5000)) if case % 4 else int(rng.integers(262000, 300000))
        epoch = int(rng.integers(0, 2000))
        activation = rng.integers(0, epoch + 2, size=n_val).astype(np.uint64)
        exit_ = rng.integers(0, epoch + 3, size=n_val).astype(np.uint64)
        exit_[rng.random(n_val) < 0.9] = np.uint64(M.FAR_FUTURE_EPOCH)
        eff = rng.integers(0, 33, size=n_val).astype(np.uint64) * np.uint64(ETH)
        state = M.make_state(32 * epoch + int(rng.integers(0, 32)), activation, exit_, eff, finalized_epoch=int(rng.integers(0, epoch + 1)))
        mask = M.active_mask(activation, exit_, epoch)
        n, total = int(mask.sum()), M.total_balance(eff, mask, ETH)
        assert fc.get_committee_count_per_slot(None, epoch, n_active=n) == ns["get_committee_count_per_slot"](state, epoch)
        decay = float(rng.choice([0.1, 0.25, 0.5]))
        want = ns["get_latest_weak_subjectivity_checkpoint_epoch"](state, decay)
        assert fc.get_latest_weak_subjectivity_checkpoint_epoch(None, decay, n_active=n,
                                                                finalized_epoch=state.finalized_checkpoint.epoch) == want
        if n and total // n // ETH < 32:    # pe:1284 divides by T - t
            got = fc.compute_weak_subjectivity_period(None, n_active=n, total_active_balance=total)
            assert got == ns["compute_weak_subjectivity_period"](state), case
