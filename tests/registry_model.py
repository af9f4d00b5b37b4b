"""An own-words model of the active validator set the engine keeps on the GPU (pe_registry_set_epochs, pe_active_set,
pe_state_refresh_activity): who is active, the ordered list, its total balance, the activity flags, the churn limit.
The reference names these (get_active_validator_indices at pe:467, pe:1234, pe:1267; get_total_active_balance at pe:1268;
get_validator_churn_limit at pe:1270) without giving their text; the functions that CALL them are the reference's own
(tests/golden/generate_registry.py runs them over this model).  The GPU tests compare the engine with it."""
from types import SimpleNamespace

import numpy as np

FAR_FUTURE_EPOCH = 2**64 - 1
ACTIVE, SLASHED, ACTIVE_PREV = 0x01, 0x02, 0x08
ETH = 10**9


def active_mask(activation_epoch, exit_epoch, epoch: int) -> np.ndarray:
    """A validator is active from its activation epoch up to, not including, its exit epoch; unsigned 64-bit values."""
    a = np.asarray(activation_epoch, dtype=np.uint64)
    x = np.asarray(exit_epoch, dtype=np.uint64)
    e = np.uint64(epoch)
    return (a <= e) & (e < x)


def active_indices(activation_epoch, exit_epoch, epoch: int) -> np.ndarray:
    """The active validators in increasing order of index."""
    return np.flatnonzero(active_mask(activation_epoch, exit_epoch, epoch)).astype(np.uint32)


def total_balance(effective_balance, mask, increment: int = ETH) -> int:
    """The effective balances of the chosen validators, never less than one increment; slashed ones count."""
    chosen = np.asarray(effective_balance, dtype=np.uint64)[np.asarray(mask, dtype=bool)]
    # exact over the integers: the two 32-bit halves summed apart (each sum stays far below 2^64)
    total = (int((chosen >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((chosen & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
    assert total < 2**64, "the engine's 64-bit sum would wrap"
    return max(increment, total)


def activity_flags(activation_epoch, exit_epoch, current_epoch: int, flags) -> np.ndarray:
    """The view's flags after a refresh: active now, active one epoch earlier (epoch 0 is its own predecessor), the rest kept."""
    before = max(current_epoch, 1) - 1
    kept = np.asarray(flags, dtype=np.uint8) & np.uint8(0xFF & ~(ACTIVE | ACTIVE_PREV))
    now = active_mask(activation_epoch, exit_epoch, current_epoch).astype(np.uint8) * np.uint8(ACTIVE)
    then = active_mask(activation_epoch, exit_epoch, before).astype(np.uint8) * np.uint8(ACTIVE_PREV)
    return kept | now | then


def churn_limit(n_active: int, min_per_epoch: int = 4, quotient: int = 65536) -> int:
    return max(min_per_epoch, n_active // quotient)


# ---- the same, under the names the reference's functions call, over a state that holds the registry as arrays:
# state.slot, .activation_epoch, .exit_epoch, .effective_balance, .finalized_checkpoint.epoch
def make_state(slot: int, activation_epoch, exit_epoch, effective_balance, finalized_epoch: int = 0):
    return SimpleNamespace(slot=slot, activation_epoch=np.asarray(activation_epoch, dtype=np.uint64),
                           exit_epoch=np.asarray(exit_epoch, dtype=np.uint64),
                           effective_balance=np.asarray(effective_balance, dtype=np.uint64),
                           finalized_checkpoint=SimpleNamespace(epoch=finalized_epoch))


def callees(slots_per_epoch: int = 32, increment: int = ETH, min_churn: int = 4, churn_quotient: int = 65536) -> dict:
    def get_current_epoch(state):
        return state.slot // slots_per_epoch

    def get_active_validator_indices(state, epoch):
        return active_indices(state.activation_epoch, state.exit_epoch, epoch)

    def get_total_active_balance(state):
        return total_balance(state.effective_balance,
                             active_mask(state.activation_epoch, state.exit_epoch, get_current_epoch(state)), increment)

    def get_validator_churn_limit(state):
        return churn_limit(len(get_active_validator_indices(state, get_current_epoch(state))), min_churn, churn_quotient)

    return dict(get_current_epoch=get_current_epoch, get_active_validator_indices=get_active_validator_indices,
                get_total_active_balance=get_total_active_balance, get_validator_churn_limit=get_validator_churn_limit)
