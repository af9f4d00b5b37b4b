"""An own-words model of Altair's sync committee as the engine runs it on the GPU (pe_sync_committee_compute,
pe_process_sync_aggregate): the sampling of get_next_sync_committee_indices, the signing root, and process_sync_aggregate's
scalars and balance changes.  Plain integers, sequential.  The reference holds none of these three functions;
tests/test_sync_committee_model.py ties the sampling to tests/epoch_model.proposer (itself held to the reference's
compute_proposer_index, pe:604-618) and to a brute-force formulation, and the rewards to cases worked by hand."""
import hashlib
from math import isqrt

DEFAULT_MAX_TRIES = 1 << 20
SYNC_REWARD_WEIGHT, PROPOSER_WEIGHT, WEIGHT_DENOMINATOR = 2, 8, 64
INFINITY_SIGNATURE = b"\xc0" + bytes(95)


class Walk:
    """compute_shuffled_index for one (seed, count, rounds), with every hash it asks for computed once."""

    def __init__(self, seed: bytes, count: int, rounds: int):
        assert count > 0 and 0 <= rounds <= 255
        self.seed, self.count, self.rounds = bytes(seed), count, rounds
        self.pivots = [int.from_bytes(hashlib.sha256(self.seed + bytes([r])).digest()[:8], "little") % count for r in range(rounds)]
        self.sources = {}

    def __call__(self, index: int) -> int:
        for r in range(self.rounds):
            flip = (self.pivots[r] + self.count - index) % self.count
            position = max(index, flip)
            key = (r, position // 256)
            source = self.sources.get(key)
            if source is None:
                source = self.sources[key] = hashlib.sha256(self.seed + bytes([r]) + (position // 256).to_bytes(4, "little")).digest()
            if (source[(position % 256) // 8] >> (position % 8)) & 1:
                index = flip
        return index


def accepts(effective_balance: int, max_eff: int, seed: bytes, i: int) -> bool:
    random_byte = hashlib.sha256(bytes(seed) + (i // 32).to_bytes(8, "little")).digest()[i % 32]
    return effective_balance * 255 >= max_eff * random_byte


def next_sync_committee_indices(indices, effective_balance, seed: bytes, rounds: int, max_eff: int, size: int, max_tries: int = 0):
    """-> (members | None, tries).  i = 0, 1, ...: the candidate indices[shuffled(i mod total)] is appended when its effective
    balance, scaled to a byte against max_eff, reaches byte (i mod 32) of sha256(seed | i div 32 as 8 little-endian bytes) --
    until `size` are appended; a validator may be appended again.  tries = the i of the last appended candidate + 1; None and
    max_tries (0 = 2^20) when the first max_tries candidates did not yield `size`."""
    total = len(indices)
    assert total > 0 and size > 0
    if max_tries == 0:
        max_tries = DEFAULT_MAX_TRIES
    walk = Walk(seed, total, rounds)
    members = []
    for i in range(max_tries):
        candidate = int(indices[walk(i % total)])
        if accepts(int(effective_balance[candidate]), max_eff, seed, i):
            members.append(candidate)
            if len(members) == size:
                return members, i + 1
    return None, max_tries


def signing_root(block_root: bytes, domain: bytes) -> bytes:
    """hash_tree_root(SigningData(object_root, domain)): two 32-byte leaves, one hash."""
    assert len(block_root) == 32 and len(domain) == 32
    return hashlib.sha256(bytes(block_root) + bytes(domain)).digest()


def bit(bits: bytes, p: int) -> int:
    return (bits[p // 8] >> (p % 8)) & 1


def participants(members, bits: bytes):
    """The validators whose bit is set, in committee order, one entry per position."""
    assert not any(bit(bits, p) for p in range(len(members), 8 * len(bits))), "a set bit beyond the committee"
    return [int(members[p]) for p in range(len(members)) if bit(bits, p)]


def reward_scalars(total_active_balance: int, size: int, increment: int = 10**9, base_reward_factor: int = 64,
                   slots_per_epoch: int = 32):
    """-> (participant_reward, proposer_reward), every division where the reference has it."""
    per_increment = increment * base_reward_factor // isqrt(total_active_balance)
    total_base = per_increment * (total_active_balance // increment)
    participant_reward = total_base * SYNC_REWARD_WEIGHT // WEIGHT_DENOMINATOR // slots_per_epoch // size
    proposer_reward = participant_reward * PROPOSER_WEIGHT // (WEIGHT_DENOMINATOR - PROPOSER_WEIGHT)
    return participant_reward, proposer_reward


def process_sync_aggregates(balances, members, aggregates, participant_reward: int, proposer_reward: int):
    """aggregates: (bits, proposer_index) per block, in order.  Changes `balances` (a list of ints) in place, position by
    position; additions wrap at 2^64 as the engine's do.  -> {"n_participants", "credited", "debited", "n_saturated"}."""
    stats = {"n_participants": 0, "credited": 0, "debited": 0, "n_saturated": 0}
    for bits, proposer in aggregates:
        for p, v in enumerate(members):
            if bit(bits, p):
                balances[v] = (balances[v] + participant_reward) % 2**64
                balances[proposer] = (balances[proposer] + proposer_reward) % 2**64
                stats["n_participants"] += 1
                stats["credited"] += participant_reward + proposer_reward
            else:
                cut = min(balances[v], participant_reward)
                stats["n_saturated"] += balances[v] < participant_reward
                balances[v] -= cut
                stats["debited"] += cut
    return stats
