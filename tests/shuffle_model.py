"""The swap-or-not shuffle of compute_shuffled_index (pe:513-534) for a whole list at once, and compute_committee's slicing
(pe:495-504) over it: plain numpy + hashlib, written from the reference's text and oracle/spec.py.  tests/test_shuffle_model.py
holds it to spec.compute_shuffled_index / spec.compute_committee index by index; tests/test_gpu_shuffle_edges.py holds the
engine to it on whole lists.  Nothing here knows how the GPU lays a round out.

round_pivots, blocks_read and find_seed only choose inputs (a seed whose rounds meet a wanted pivot); no expected value
comes from them."""
import hashlib

import numpy as np

SEED_SEARCH_LIMIT = 4000


def _hash(data: bytes) -> bytes:
    return hashlib.sha256(data).digest()


def _pivot(n: int, seed: bytes, current_round: int) -> int:
    """pe:522: bytes_to_uint64(hash(seed + uint_to_bytes(uint8(current_round)))[0:8]) % index_count, little-endian."""
    return int.from_bytes(_hash(seed + bytes([current_round]))[0:8], "little") % n


def shuffle_list(n: int, seed: bytes, rounds: int) -> np.ndarray:
    """-> int64[n], element i = compute_shuffled_index(i, n, seed) with SHUFFLE_ROUND_COUNT = rounds.

    Per round, for every index at once (pe:521-532):
        pivot    = bytes_to_uint64(hash(seed + uint8(round))[0:8]) % n
        flip     = (pivot + n - index) % n
        position = max(index, flip)
        source   = hash(seed + uint8(round) + uint32(position // 256))          one digest per 256 positions
        bit      = (source[(position % 256) // 8] >> (position % 8)) % 2
        index    = flip if bit else index
    The ceil(n / 256) digests of a round lie one after the other in one byte array, so that byte (position % 256) // 8 of
    digest position // 256 is byte position // 8 of the array."""
    assert n >= 1 and 0 <= rounds <= 255 and len(seed) == 32
    index = np.arange(n, dtype=np.int64)
    n_digests = (n + 255) // 256
    for current_round in range(rounds):
        round_byte = bytes([current_round])
        pivot = _pivot(n, seed, current_round)
        source = np.frombuffer(b"".join(_hash(seed + round_byte + block.to_bytes(4, "little")) for block in range(n_digests)),
                               dtype=np.uint8)
        flip = (pivot + n - index) % n
        position = np.maximum(index, flip)
        bit = (source[position >> 3] >> (position & 7).astype(np.uint8)) & 1
        index = np.where(bit == 1, flip, index)
    return index


def committees(indices, seed: bytes, count: int, rounds: int):
    """compute_committee for index = 0 .. count - 1 in one table -> (offsets uint32[count + 1], members uint32[n]):
    committee c is members[offsets[c]:offsets[c + 1]], start = n * c // count and end = n * (c + 1) // count (pe:502-503),
    members[i] = indices[compute_shuffled_index(i, n, seed)] (pe:504)."""
    indices = np.asarray(indices, dtype=np.uint32)
    n = indices.size
    offsets = np.array([n * c // count for c in range(count + 1)], dtype=np.uint32)
    return offsets, indices[shuffle_list(n, seed, rounds)]


def round_pivots(n: int, seed: bytes, rounds: int) -> list:
    return [_pivot(n, seed, r) for r in range(rounds)]


def blocks_read(pivot, n: int):
    """How many 256-position blocks of a round's `source` the positions of that round can lie in (pivot: an int or an
    integer array of pivots).

    With p = pivot, 0 <= p < n, position = max(index, flip) and flip = (p + n - index) % n:
      index <= p:  flip = p - index, so {index, flip} = {k, p - k} and position = max(k, p - k) >= p / 2; every value of
                   [ceil(p / 2), p] is taken (position = j comes from index = j).
      index >  p:  flip = p + n - index, also in (p, n - 1], so position = max(k, p + n - k) >= (p + n) / 2; every value of
                   [ceil((p + n) / 2), n - 1] is taken.  For p = n - 1 no index is above p and the range is empty.
    Each range is a span of its own: the result is the sum of the two spans' block counts (a block that both touch counts
    twice, an empty range counts 0)."""
    p = np.asarray(pivot, dtype=np.int64)
    lo_a, hi_a = (p + 1) // 2, p
    lo_b, hi_b = (p + n + 1) // 2, n - 1
    in_a = (hi_a >> 8) - (lo_a >> 8) + 1
    in_b = np.where(lo_b <= hi_b, (hi_b >> 8) - (lo_b >> 8) + 1, 0)
    total = in_a + in_b
    return int(total) if total.ndim == 0 else total


# The pivots the GPU tests ask find_seed for, as predicates over (pivot, n): the ends of the list (one range is a single
# position, the other is empty or a single position), both sides of a 256-position block boundary, and the middle.
PIVOT_EDGES = {
    "0": lambda p, n: p == 0,
    "1": lambda p, n: p == 1,
    "n-1": lambda p, n: p == n - 1,
    "n-2": lambda p, n: p == n - 2,
    "last of a block": lambda p, n: p % 256 == 255,
    "first of a block": lambda p, n: p % 256 == 0 and p > 0,
    "n//2": lambda p, n: p == n // 2,
    "n//2-1": lambda p, n: p == n // 2 - 1,
}
# (n, edge): every edge at both sizes of the LDS form, the two ends of the list at a size the gather takes
PIVOT_EDGE_CASES = [(n, edge) for n in (4096, 4099) for edge in PIVOT_EDGES] + [(300, "0"), (300, "n-1")]


def find_seed(n: int, rounds: int, want, limit: int = SEED_SEARCH_LIMIT) -> bytes:
    """The first of sha256(b"shuffle-edge-0"), sha256(b"shuffle-edge-1"), ... for which want(pivot) holds for the pivot of
    some round.  Deterministic; raises when `limit` seeds have none."""
    for k in range(limit):
        seed = _hash(b"shuffle-edge-%d" % k)
        if any(want(p) for p in round_pivots(n, seed, rounds)):
            return seed
    raise LookupError(f"no seed among {limit} gives n = {n}, {rounds} rounds the wanted pivot")
