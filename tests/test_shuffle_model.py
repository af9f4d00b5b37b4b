"""CPU: the whole-list shuffle model (tests/shuffle_model.py) is pinned to compute_shuffled_index (pe:513-534) and
compute_committee (pe:495-504) as oracle/spec.py runs them, index by index, and to tests/golden/shuffle_vectors.json.  The GPU
tests (tests/test_gpu_shuffle_edges.py) hold pe_compute_committees to the same model on whole lists.

Also pinned here, as arithmetic: how many 256-position blocks of a round's hashes one round can read.  launch_shuffle
(shuffle_kernels.hip) reserves ceil(n / 256) // 2 + 4 blocks of LDS for them and takes the LDS form while that is at most
96 KiB = 3072 blocks, i.e. up to ceil(n / 256) = 6137, n = 1 571 072."""
import json
import os

import numpy as np
import pytest

from oracle import spec
from tests import shuffle_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_BLOCKS = 96 * 1024 // 32                    # 32-byte digests in 96 KiB
LAST_LDS_N = 1571072                            # ceil(n / 256) = 6137: 6137 // 2 + 4 = 3072 blocks
TIGHTEST_N = 1570817                            # the smallest n with ceil(n / 256) = 6137


def _reserved(n: int) -> int:
    return (n + 255) // 256 // 2 + 4


@pytest.mark.parametrize("rounds", [0, 1, 9, 10, 90])
def test_shuffle_list_is_compute_shuffled_index_at_every_index(rounds):
    spec.use_preset("mainnet", SHUFFLE_ROUND_COUNT=rounds)
    try:
        for n in (1, 2, 3, 255, 256, 257, 1000):
            seed = spec.sha256(b"model-%d-%d" % (n, rounds))
            got = M.shuffle_list(n, seed, rounds)
            want = [spec.compute_shuffled_index(i, n, seed) for i in range(n)]
            assert got.tolist() == want, (n, rounds)
    finally:
        spec.use_preset("mainnet")


def test_shuffle_list_reproduces_the_golden_vectors():
    rows = json.load(open(os.path.join(HERE, "golden", "shuffle_vectors.json")))
    assert rows
    for row in rows:
        got = M.shuffle_list(row["index_count"], bytes.fromhex(row["seed"]), row["rounds"])
        assert got.tolist() == row["shuffled"], (row["index_count"], row["rounds"])


@pytest.mark.parametrize("rounds", [10, 90])
def test_committees_is_compute_committee(rounds):
    n, n_val, count = 333, 500, 32
    indices = np.sort(np.random.default_rng(333).choice(n_val, size=n, replace=False)).astype(np.uint32)
    seed = spec.sha256(b"model-committees")
    spec.use_preset("mainnet", SHUFFLE_ROUND_COUNT=rounds)
    try:
        off, mem = M.committees(indices, seed, count, rounds)
        assert off.dtype == np.uint32 and mem.dtype == np.uint32 and off.size == count + 1
        assert off[0] == 0 and off[-1] == n
        for c in range(count):
            assert mem[off[c]:off[c + 1]].tolist() == spec.compute_committee([int(x) for x in indices], seed, c, count), c
    finally:
        spec.use_preset("mainnet")


def test_blocks_read_counts_the_blocks_the_positions_of_a_round_lie_in():
    """blocks_read against the definition: every position a round takes, by brute force."""
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 1000, 1025):
        index = np.arange(n)
        for pivot in range(n):
            flip = (pivot + n - index) % n
            position = np.maximum(index, flip)
            low, high = position[index <= pivot], position[index > pivot]
            assert low.min() == (pivot + 1) // 2 and low.max() == pivot
            assert np.unique(low).size == pivot - (pivot + 1) // 2 + 1                      # the whole range, no holes
            want = np.unique(low >> 8).size
            if high.size:
                assert high.min() == (pivot + n + 1) // 2 and high.max() == n - 1
                assert np.unique(high).size == n - (pivot + n + 1) // 2
                want += np.unique(high >> 8).size
            assert M.blocks_read(pivot, n) == want, (n, pivot)
            assert M.blocks_read(np.array([pivot]), n)[0] == want


def test_a_round_fits_the_lds_the_launcher_reserves():
    """blocks_read(p, n) <= ceil(n / 256) // 2 + 4 for every pivot of every n in 4096 .. 12000 and at the top of the LDS form;
    one block more where range B is empty (pivot = n - 1): the kernel loads the block of position n - 1 there all the same.
    At n = 1 570 817 the fullest round fills 3071 of the 3072 blocks."""
    for n in list(range(4096, 12001)) + [1570816, TIGHTEST_N, LAST_LDS_N]:
        pivots = np.arange(n)
        count = M.blocks_read(pivots, n)
        count[n - 1] += 1
        assert count.max() <= _reserved(n), (n, int(count.max()))
    assert _reserved(TIGHTEST_N) == _reserved(LAST_LDS_N) == LDS_BLOCKS
    assert _reserved(LAST_LDS_N + 1) == LDS_BLOCKS + 1                                     # the first size the gather takes
    assert M.blocks_read(np.arange(TIGHTEST_N), TIGHTEST_N).max() == 3071
    assert M.blocks_read(np.arange(LAST_LDS_N), LAST_LDS_N).max() <= 3071


def test_round_pivots_are_the_pivots_of_the_spec():
    seed = spec.sha256(b"pivots")
    for n in (1, 300, 4099):
        want = [spec.bytes_to_uint64(spec.sha256(seed + spec.uint_to_bytes(r, 1))[0:8]) % n for r in range(90)]
        assert M.round_pivots(n, seed, 90) == want


@pytest.mark.parametrize("n,edge", M.PIVOT_EDGE_CASES)
def test_find_seed_finds_every_pivot_the_gpu_tests_ask_for(n, edge):
    want = M.PIVOT_EDGES[edge]
    seed = M.find_seed(n, 90, lambda p: want(p, n))
    assert any(want(p, n) for p in M.round_pivots(n, seed, 90))
    assert seed == M.find_seed(n, 90, lambda p: want(p, n))                                # deterministic


def test_find_seed_finds_the_fullest_round_and_fails_loudly():
    seed = M.find_seed(TIGHTEST_N, 10, lambda p: M.blocks_read(p, TIGHTEST_N) == 3071)
    assert any(M.blocks_read(p, TIGHTEST_N) == 3071 for p in M.round_pivots(TIGHTEST_N, seed, 10))
    with pytest.raises(LookupError):
        M.find_seed(4096, 90, lambda p: p == 4096, limit=20)                               # no pivot reaches n
