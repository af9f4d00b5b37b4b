"""-m gpu: sync committee and proposer sampling held to the models at their bounds, on the cases of
tests/sync_bounds_cases.py (tests/test_sync_bounds_cases.py shows from the models alone what those cases reach and which wrong
kernels they tell apart).
  A  sample_accepts where the 128-bit products decide, through pe_compute_proposers and pe_sync_committee_compute
  B  k_sync_rewards at 4, 36, 37, 63 and 64 aggregates: the whole balance array and every stat
  C  k_sync_members and the verdict composition at 64 aggregates, by position; a stray bit at the committee's size and at 511
  D  k_sync_sample / k_sync_append across three candidate batches, and a registry that never yields the committee"""
import numpy as np
import pytest

import pos_evolution_amd.synth as synth
from pos_evolution_amd import _abi
from pos_evolution_amd.engine import SYNC_APPLY, SYNC_CURRENT, SYNC_NEXT, SYNC_VERIFY
from tests import epoch_model
from tests import sync_bounds_cases as C
from tests import sync_committee_model as M
from tests import test_gpu_sync_committee as T

pytestmark = pytest.mark.gpu
ETH = C.ETH
NONE32 = 0xFFFFFFFF


def _engine(engine_factory, bal, **cfg):
    """T._engine with a configuration: the progression's pubkeys, `bal` as effective balances."""
    n = len(bal)
    e = engine_factory(**cfg)
    if n not in T._POINTS:
        T._POINTS[n] = synth.registry_points(e, n, C.A_SK, C.B_SK)
    e.set_validators(np.array(bal, dtype=np.uint64), np.ones(n, dtype=np.uint8), T._POINTS[n])
    return e


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("case", C.acceptance_cases(), ids=lambda c: c["name"])
def test_acceptance_over_the_whole_u64_range(engine_factory, case):
    bal, indices, rounds, max_eff = case["bal"], case["indices"], case["rounds"], case["max_eff"]
    e = _engine(engine_factory, bal, effective_balance_increment=C.WIDE_INCREMENT)
    active = case["active"] if isinstance(case["active"], int) else np.array(case["active"], dtype=np.uint32)
    prop, tries = e.compute_proposers(case["proposer_seeds"], active, rounds, max_eff)
    for k, sd in enumerate(case["proposer_seeds"]):
        want, want_tries = epoch_model.proposer(indices, bal, sd, rounds, max_eff)
        assert (int(prop[k]), int(tries[k])) == (NONE32 if want is None else want, want_tries), (case["name"], k)
    for size, sd in case["syncs"]:
        T._check_compute(e, sd, active, indices, bal, rounds, size, refusal=True, max_eff=max_eff)


# ---------------------------------------------------------------- B
@pytest.fixture(scope="module")
def rewards_engine(engine_factory):
    return T._engine(engine_factory, T._balances("full", C.N_VAL_REWARDS, None))


@pytest.mark.parametrize("case", C.rewards_cases(), ids=lambda c: c["name"])
def test_rewards_at_the_batch_bounds(rewards_engine, case):
    e = rewards_engine
    e.sync_committee_set(SYNC_CURRENT, case["members"])
    aggs = [{"bits": bits, "signature": M.INFINITY_SIGNATURE, "block_root": C.ROOT, "domain": C.DOMAIN, "proposer_index": proposer}
            for bits, proposer in case["aggs"]]
    want = T._run_rewards(e, case["members"], case["bal"], aggs, case["total"], SYNC_APPLY)
    touched = set(case["members"]) | {p for _, p in case["aggs"]}
    assert all(want[v] == case["bal"][v] for v in range(C.N_VAL_REWARDS) if v not in touched)


# ---------------------------------------------------------------- C
@pytest.fixture(scope="module")
def verdict_engine(engine_factory):
    return T._engine(engine_factory, T._balances("full", C.N_VAL_VERDICTS, None))


def _signed(row):
    if row["signature"] == "infinity":
        signature = M.INFINITY_SIGNATURE
    elif row["signature"] == "undecodable":
        signature = C.UNDECODABLE
    else:
        signature = T._signature(M.signing_root(row["signed_root"], row["domain"]), row["sk"])
    return {"bits": row["bits"], "signature": signature, "block_root": row["root"], "domain": row["domain"],
            "proposer_index": row["proposer"]}


def _check_verdicts(e, members, rows, total, flags):
    """One call against the model by position; nothing may move.  -> the result"""
    want = [C.model_verdict(members, r) for r in rows]
    before = T._snapshot(e)
    res = e.process_sync_aggregate([_signed(r) for r in rows], total, flags)
    assert res["verdict"].tolist() == [w[0] for w in want], [r["kind"] for r in rows]
    assert res["sig_status"].tolist() == [w[1] for w in want]
    assert res["n_participants"] == sum(w[2] for w in want)
    assert 0 < sum(w[0] for w in want) < len(rows)
    assert res["applied"] == 0 and (res["credited"], res["debited"], res["n_saturated"]) == (0, 0, 0)
    assert T._same(before, T._snapshot(e))
    return res


def test_verdicts_by_position_in_a_full_batch(verdict_engine):
    e = verdict_engine
    total = 32 * ETH * 50_000
    members, rows = C.verdict_batch()
    e.sync_committee_set(SYNC_CURRENT, members)
    bal = [5 * ETH] * C.N_VAL_VERDICTS
    e.state_set_balances(np.asarray(bal, dtype=np.uint64))
    _check_verdicts(e, members, rows, total, SYNC_VERIFY)
    _check_verdicts(e, members, rows, total, SYNC_VERIFY | SYNC_APPLY)
    # every invalid one replaced by a valid one: all 64 verify and the call pays exactly the model's rewards
    _, fixed = C.verdict_batch(valid_only=True)
    want = T._run_rewards(e, members, bal, [_signed(r) for r in fixed], total, SYNC_VERIFY | SYNC_APPLY)
    assert want != bal


def test_verdicts_over_all_eight_waves(verdict_engine):
    e = verdict_engine
    members, rows = C.wide_verdict_batch()
    e.sync_committee_set(SYNC_CURRENT, members)
    e.state_set_balances(np.full(C.N_VAL_VERDICTS, 5 * ETH, dtype=np.uint64))
    _check_verdicts(e, members, rows, 32 * ETH * 50_000, SYNC_VERIFY)


@pytest.mark.parametrize("size", [1, 63, 64, 65, 511])
def test_a_set_bit_at_the_size_or_at_the_end_is_refused(verdict_engine, size):
    e = verdict_engine
    total = 32 * ETH * 50_000
    bal = np.full(C.N_VAL_VERDICTS, 5 * ETH, dtype=np.uint64)
    e.sync_committee_set(SYNC_CURRENT, list(range(size)))
    e.sync_committee_set(SYNC_NEXT, [1, 2])
    e.state_set_balances(bal)
    before = T._snapshot(e)
    mine = [(b, position) for s, b, position in C.out_of_range_cases() if s == size]
    assert len(mine) == (2 if size == 511 else 4)
    for b, position in mine:
        _, rows = C.out_of_range_batch(size, b, position)
        aggs = [_signed(r) for r in rows]
        for flags in (SYNC_APPLY, SYNC_VERIFY, SYNC_VERIFY | SYNC_APPLY):
            assert T._status(lambda: e.process_sync_aggregate(aggs, total, flags)) == _abi.PE_ERR_INVALID_ARG, (size, b, position, flags)
            assert T._same(before, T._snapshot(e))
    # the same batch without the stray bit is taken: the bit alone was refused
    _, rows = C.out_of_range_batch(size, 0, size)
    rows[0] = dict(rows[0], bits=C.bits_of(rows[0]["positions"][:-1]))
    res = e.process_sync_aggregate([_signed(r) for r in rows], total, SYNC_APPLY)
    assert res["applied"] == 1 and not T._same(before, T._snapshot(e))


# ---------------------------------------------------------------- D
@pytest.fixture(scope="module")
def thin_engine(engine_factory):
    c = C.three_batch_cases()[0]
    return T._engine(engine_factory, np.array(c["bal"], dtype=np.uint64))


@pytest.mark.parametrize("case", C.three_batch_cases(), ids=lambda c: c["seed"].hex()[:8])
def test_sampling_across_three_batches(thin_engine, case):
    n = case["n_val"]
    _, tries = T._check_compute(thin_engine, case["seed"], n, list(range(n)), case["bal"], case["rounds"], case["size"])
    assert tries > 2 * C.BATCH and tries % C.BATCH > 1    # a third launch; max_tries = tries - 1 lies inside it


def test_sampling_exhausted_after_two_batches_and_one_candidate(engine_factory):
    c = C.exhaustion_case()
    n = c["n_val"]
    e = T._engine(engine_factory, np.array(c["bal"], dtype=np.uint64))
    e.sync_committee_set(SYNC_NEXT, [1, 2])
    before = T._snapshot(e)
    idx = np.full(_abi.PE_SYNC_COMMITTEE_MAX, 0xABABABAB, dtype=np.uint32)
    out_key = np.full(48, 0xAB, dtype=np.uint8)
    out_tries = np.zeros(1, dtype=np.uint32)
    sd = np.frombuffer(c["seed"], dtype=np.uint8).copy()
    rc = e._lib.pe_sync_committee_compute(e._h, sd.ctypes.data, None, n, c["rounds"], C.MAX_EFF, c["size"], c["max_tries"],
                                          idx.ctypes.data, out_key.ctypes.data, out_tries.ctypes.data)
    assert rc == _abi.PE_ERR_CAPACITY and int(out_tries[0]) == c["max_tries"]
    assert (idx == 0xABABABAB).all() and (out_key == 0xAB).all()
    assert T._same(before, T._snapshot(e))
    # ... and the handle still samples: the few a zero balance yields, where the model finds them
    want, want_tries = M.next_sync_committee_indices(range(n), c["bal"], c["seed"], c["rounds"], C.MAX_EFF, 64)
    got, key, tries = e.sync_committee_compute(c["seed"], n, c["rounds"], C.MAX_EFF, 64)
    assert (got.tolist(), tries, key) == (want, want_tries, T._key_of(want)) and want_tries < c["max_tries"]
