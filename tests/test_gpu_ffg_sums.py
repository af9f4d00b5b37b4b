"""-m gpu: k_ffg_balances (the three Gwei sums of process_justification_and_finalization, pe:791-802) against numpy uint64
sums under the kernel's documented predicates, from one workgroup to the full grid of 256 with and without a ragged tail;
and k_state_view_from_registry, the working-state view a fresh store_init rebuilds from the registry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INC = 10**9
ACTIVE_CUR, SLASHED, ACTIVE_PREV, TIMELY_TARGET = 0x01, 0x02, 0x08, 0x02
# validators: 1 / 1 / 1 / 1 / 2 / 17 / 256 / 256 workgroups (16 validators per lane, at most 256 workgroups)
SIZES = [1, 63, 65, 4096, 4097, 65537, 1 << 20, (1 << 20) + 1]


def _want(bal, sflags, part_cur, part_prev):
    """total_active_balance, previous_target_balance, current_target_balance, each floored at one increment
    (get_total_balance)."""
    cur, prev, unsl = (sflags & ACTIVE_CUR) != 0, (sflags & ACTIVE_PREV) != 0, (sflags & SLASHED) == 0
    sums = (bal[cur].sum(dtype=np.uint64),
            bal[unsl & prev & ((part_prev & TIMELY_TARGET) != 0)].sum(dtype=np.uint64),
            bal[unsl & cur & ((part_cur & TIMELY_TARGET) != 0)].sum(dtype=np.uint64))
    return tuple(max(INC, int(s)) for s in sums)


@pytest.mark.parametrize("n", SIZES)
def test_ffg_balances_vs_numpy(engine_factory, n):
    rng = np.random.default_rng(n)
    e = engine_factory()
    reg_bal = rng.integers(16, 2049, size=n).astype(np.uint64) * np.uint64(INC)
    reg_flags = rng.choice(np.array([0, 1, 1, 1, 2, 3], dtype=np.uint8), size=n)
    e.set_validators(reg_bal, reg_flags)
    e.store_init(0, 0, b"\x01" * 32)
    bal = rng.integers(16, 2049, size=n).astype(np.uint64) * np.uint64(INC)
    # every combination of {active now, slashed, active in the previous epoch}
    sflags = rng.choice(np.array([0, 1, 2, 3, 8, 9, 10, 11], dtype=np.uint8), size=n)
    part = [rng.integers(0, 8, size=n).astype(np.uint8) for _ in range(2)]     # 0: current epoch, 1: previous
    e.state_set_validators(bal, sflags)
    e.participation_set(0, part[0])
    e.participation_set(1, part[1])
    want = _want(bal, sflags, part[0], part[1])
    if n >= 63:
        assert len(set(want)) == 3 and min(want) > INC                          # three different sums, none at the floor
    assert e.ffg_balances() == want
    # nobody active in either epoch: every sum sits at the floor
    e.state_set_validators(bal, sflags & np.uint8(SLASHED))
    assert e.ffg_balances() == (INC, INC, INC)
    # everybody slashed: only the total is left
    e.state_set_validators(bal, sflags | np.uint8(SLASHED))
    assert e.ffg_balances() == (max(INC, int(bal[(sflags & ACTIVE_CUR) != 0].sum(dtype=np.uint64))), INC, INC)
    # a fresh store: k_state_view_from_registry makes the working state mirror the registry again
    e.store_init(0, 0, b"\x01" * 32)
    s_bal, s_flags, is_set = e.state_validators()
    assert not is_set
    assert np.array_equal(s_bal, reg_bal)
    assert np.array_equal(s_flags, (reg_flags & 3) | np.where(reg_flags & 1, 8, 0).astype(np.uint8))
    assert e.ffg_balances()[0] == max(INC, int(reg_bal[(reg_flags & 1) != 0].sum(dtype=np.uint64)))
    assert e.ffg_balances() == _want(reg_bal, s_flags, np.zeros(n, np.uint8), np.zeros(n, np.uint8))
