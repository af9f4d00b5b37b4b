"""An own-words model of the two epoch-boundary functions the engine runs on the GPU (pe_compute_proposers,
pe_effective_balance_updates).  tests/test_epoch_model.py holds it to the reference's own text (compute_proposer_index
pe:604-618, process_effective_balance_updates pe:122-133) where that text is on the machine, and to
tests/golden/epoch_vectors.json everywhere; the GPU tests compare the engine with it."""
import hashlib

import numpy as np

from oracle import spec

NONE32 = 0xFFFFFFFF
DEFAULT_MAX_TRIES = 4096


def shuffled_index(index: int, count: int, seed: bytes, rounds: int) -> int:
    """spec.compute_shuffled_index reads SHUFFLE_ROUND_COUNT from its module: bind it for the call."""
    saved = spec.SHUFFLE_ROUND_COUNT
    spec.SHUFFLE_ROUND_COUNT = rounds
    try:
        return int(spec.compute_shuffled_index(index, count, seed))
    finally:
        spec.SHUFFLE_ROUND_COUNT = saved


def proposer(indices, effective_balance, seed: bytes, rounds: int, max_eff: int, max_tries: int = 0):
    """-> (validator | None, tries).  Candidate i is indices[shuffled(i mod total)]; it is taken when its effective balance,
    scaled to a byte against max_eff, reaches byte (i mod 32) of sha256(seed | i div 32 as 8 little-endian bytes).
    tries = the i of the accepted candidate, or max_tries (0 = 4096) with validator None when none of them was."""
    total = len(indices)
    assert total > 0
    if max_tries == 0:
        max_tries = DEFAULT_MAX_TRIES
    digest, digest_of = b"", -1
    for i in range(max_tries):
        if i // 32 != digest_of:
            digest_of = i // 32
            digest = hashlib.sha256(bytes(seed) + digest_of.to_bytes(8, "little")).digest()
        candidate = int(indices[shuffled_index(i % total, total, seed, rounds)])
        if int(effective_balance[candidate]) * 255 >= max_eff * digest[i % 32]:
            return candidate, i
    return None, max_tries


def effective_balance_updates(balances, eff, increment: int, quotient: int, down: int, up: int, max_eff: int):
    """-> (new effective balances uint64[n], n_changed).  A validator moves only when its balance has left the band
    [eff - down_threshold, eff + up_threshold]; it then lands on its balance rounded down to whole increments, capped."""
    balances = np.asarray(balances, dtype=np.uint64)
    eff = np.asarray(eff, dtype=np.uint64)
    step = increment // quotient
    lo, hi = np.uint64(step * down), np.uint64(step * up)
    inc = np.uint64(increment)
    above, below = balances > eff, eff > balances
    # differences of the larger minus the smaller: no uint64 wrap-around
    fell = below & ((eff - np.minimum(balances, eff)) > lo)
    rose = above & ((balances - np.minimum(balances, eff)) > hi)
    landed = np.minimum(balances - balances % inc, np.uint64(max_eff))
    new = np.where(fell | rose, landed, eff).astype(np.uint64)
    return new, int(np.count_nonzero(new != eff))
