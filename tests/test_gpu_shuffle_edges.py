"""-m gpu: pe_compute_committees (and its asynchronous and resident-list forms) against the whole-list model of
tests/shuffle_model.py, which tests/test_shuffle_model.py pins to compute_shuffled_index / compute_committee (pe:495-534).
Every comparison is equality of the whole `offsets` and `members` arrays: a swap-or-not shuffle that reads one wrong bit in
one round is still a permutation and moves only the few indices that met that bit.

The shapes are launch_shuffle's own arithmetic (shuffle_kernels.hip):
  n < 4096 or rounds == 0        k_shuffle_indices (the gather)
  4096 <= n <= 1 571 072         k_shuffle_indices_lds<4>: 4096 indices per workgroup, each round's two block ranges in LDS,
                                 ceil(n / 256) // 2 + 4 blocks reserved, at most 96 KiB = 3072 blocks
  n >= 1 571 073                 the gather again
so: both sides of 4096, of its multiples (a last workgroup of mostly padding lanes) and of 1 571 072; n = 1 570 817, where one
round fills 3071 of the 3072 blocks; round counts 0, 1, odd, even and 255 (the loop does two rounds per pass); pivots at the
ends of the list, on both sides of a block boundary and in the middle; active sets other than 0 .. n - 1; committee counts that
do not divide n; the two other callers of launch_shuffle; and a small shuffle after a large one on the same handle."""
import functools
import hashlib
import itertools

import numpy as np
import pytest

import pos_evolution_amd as pea
from tests import shuffle_model as M

pytestmark = pytest.mark.gpu
ETH = 10**9
FAR = 2**64 - 1
LAST_LDS_N = 1571072
TIGHTEST_N = 1570817
_epoch = itertools.count(1)          # every shuffle registers its table under an epoch of its own


def _seed(tag: str) -> bytes:
    return hashlib.sha256(tag.encode()).digest()


@functools.lru_cache(maxsize=None)
def _shuffled(n: int, seed: bytes, rounds: int) -> np.ndarray:
    out = M.shuffle_list(n, seed, rounds)
    out.setflags(write=False)
    return out


def _want(indices, seed, count, rounds):
    """M.committees, with the list itself computed once per (n, seed, rounds)."""
    indices = np.arange(indices, dtype=np.uint32) if isinstance(indices, int) else np.asarray(indices, dtype=np.uint32)
    n = indices.size
    return np.array([n * c // count for c in range(count + 1)], dtype=np.uint32), indices[_shuffled(n, seed, rounds)]


def _assert_table(got, indices, seed, count, rounds):
    off, mem = got
    want_off, want_mem = _want(indices, seed, count, rounds)
    assert off.dtype == np.uint32 and mem.dtype == np.uint32
    assert np.array_equal(off, want_off)
    assert off[-1] == want_mem.size
    if not np.array_equal(mem, want_mem):
        bad = np.flatnonzero(mem != want_mem)
        pytest.fail(f"{bad.size} of {mem.size} members differ, first at position {bad[0]}: got {mem[bad[0]]}, "
                    f"want {want_mem[bad[0]]}; pivots {M.round_pivots(mem.size, seed, rounds)[:8]} ...")


def _new_engine(engine_factory, n_val):
    e = engine_factory()
    e.set_validators(np.full(n_val, 32 * ETH, dtype=np.uint64), np.ones(n_val, dtype=np.uint8))
    return e


@pytest.fixture(scope="module")
def engine_of(engine_factory):
    """One engine per registry size, shared by the cases of this module."""
    made = {}

    def get(n_val):
        if n_val not in made:
            made[n_val] = _new_engine(engine_factory, n_val)
        return made[n_val]

    return get


def test_model_agrees_with_itself():
    """_want is M.committees."""
    seed = _seed("self")
    idx = np.sort(np.random.default_rng(0).choice(900, size=700, replace=False)).astype(np.uint32)
    for a, b in zip(_want(idx, seed, 32, 10), M.committees(idx, seed, 32, 10)):
        assert np.array_equal(a, b)
    for a, b in zip(_want(700, seed, 32, 10), M.committees(np.arange(700), seed, 32, 10)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8191, 8192, 8193, 12289])
def test_kernel_switch_and_grid_edges(engine_of, n):
    """4095: the last size of the gather; 4096, 8192: whole workgroups; 4097, 8193, 12289: one index in the last workgroup."""
    seed = _seed(f"grid-{n}")
    _assert_table(engine_of(n).compute_committees(next(_epoch), seed, n, 32, 90), n, seed, 32, 90)


@pytest.mark.parametrize("n,rounds", [(4097, r) for r in (0, 1, 2, 3, 89, 90, 255)] + [(300, 0), (300, 1)])
def test_round_loop_tails(engine_of, n, rounds):
    seed = _seed(f"tails-{n}-{rounds}")
    off, mem = got = engine_of(n).compute_committees(next(_epoch), seed, n, 32, rounds)
    _assert_table(got, n, seed, 32, rounds)
    if rounds == 0:
        assert np.array_equal(mem, np.arange(n, dtype=np.uint32))          # the sliced identity
        assert off.tolist() == [n * c // 32 for c in range(33)]


@pytest.mark.parametrize("n,edge", M.PIVOT_EDGE_CASES)
def test_pivot_edges(engine_of, n, edge):
    want = M.PIVOT_EDGES[edge]
    seed = M.find_seed(n, 90, lambda p: want(p, n))
    assert any(want(p, n) for p in M.round_pivots(n, seed, 90))
    _assert_table(engine_of(n).compute_committees(next(_epoch), seed, n, 32, 90), n, seed, 32, 90)


@pytest.mark.parametrize("kind", ["sorted subset", "permutation"])
def test_active_set_that_is_not_the_identity(engine_of, kind):
    n_val = 9000
    rng = np.random.default_rng(9000)
    if kind == "sorted subset":
        active = np.sort(rng.choice(n_val, size=5000, replace=False)).astype(np.uint32)
    else:
        active = rng.permutation(n_val).astype(np.uint32)
    seed = _seed(f"active-{kind}")
    got = engine_of(n_val).compute_committees(next(_epoch), seed, active, 64, 90)
    _assert_table(got, active, seed, 64, 90)
    assert np.array_equal(got[1], active[M.shuffle_list(active.size, seed, 90)])


@pytest.mark.parametrize("count", [32, 64, 2048])
def test_committee_counts_that_do_not_divide_n(engine_of, count):
    n = 4097
    seed = _seed("counts")
    off, _ = got = engine_of(n).compute_committees(next(_epoch), seed, n, count, 90)
    _assert_table(got, n, seed, count, 90)
    assert off.tolist() == [n * c // count for c in range(count + 1)] and off[-1] == n
    assert len(set(np.diff(off.astype(np.int64)).tolist())) == 2           # two committee sizes: count does not divide n


def test_asynchronous_shuffle_against_the_model(engine_of):
    n, count = 8193, 64
    seed = _seed("async-model")
    e = engine_of(n)
    epoch = next(_epoch)
    e.compute_committees_async(epoch, seed, n, count, 90)
    _assert_table(e.committees(epoch), n, seed, count, 90)


def test_shuffle_over_the_resident_active_list_against_the_model(engine_of):
    n_val, n_active, at = 6000, 4500, 10
    rng = np.random.default_rng(6000)
    mask = np.zeros(n_val, dtype=bool)
    mask[rng.choice(n_val, size=n_active, replace=False)] = True
    # active at epoch `at`: activated at or before it, leaving after it or never; the others left at or before it or are to come
    activation = rng.integers(0, at + 1, size=n_val).astype(np.uint64)
    exit_ = rng.integers(at + 1, at + 50, size=n_val).astype(np.uint64)
    exit_[mask & (rng.random(n_val) < 0.5)] = np.uint64(FAR)
    gone = ~mask & (rng.random(n_val) < 0.5)
    exit_[gone] = rng.integers(0, at + 1, size=int(gone.sum())).astype(np.uint64)
    activation[gone] = 0
    activation[~mask & ~gone] = np.uint64(at + 1)
    want_active = np.flatnonzero((activation <= np.uint64(at)) & (np.uint64(at) < exit_)).astype(np.uint32)
    assert np.array_equal(want_active, np.flatnonzero(mask))
    e = engine_of(n_val)
    e.registry_set_epochs(activation, exit_)
    assert e.active_set(at)[0] == n_active
    seed = _seed("resident-model")
    got = e.compute_committees(next(_epoch), seed, pea.ACTIVE_RESIDENT, 64, 90)
    _assert_table(got, want_active, seed, 64, 90)


def _top_seed(n):
    if n == TIGHTEST_N:     # a round that fills 3071 of the 3072 blocks reserved
        seed = M.find_seed(n, 10, lambda p: M.blocks_read(p, n) == 3071)
        assert any(M.blocks_read(p, n) == 3071 for p in M.round_pivots(n, seed, 10))
        return seed
    return _seed(f"top-{n}")


@pytest.mark.parametrize("n", [TIGHTEST_N, LAST_LDS_N, LAST_LDS_N + 1])
def test_top_of_the_lds_form(engine_of, n):
    """1 570 817: the tightest fit; 1 571 072: the last size of the LDS form; 1 571 073: the first size above it (the gather).
    10 rounds: what is at stake is LDS capacity, which the round count does not change."""
    seed = _top_seed(n)
    _assert_table(engine_of(n).compute_committees(next(_epoch), seed, n, 2048, 10), n, seed, 2048, 10)


def test_small_shuffle_after_a_large_one_on_one_handle(engine_factory):
    """The scratch of the round tables is sized by the first call; the second call's tables lie at other strides in it."""
    e = _new_engine(engine_factory, LAST_LDS_N)
    seed = _top_seed(LAST_LDS_N)
    _assert_table(e.compute_committees(next(_epoch), seed, LAST_LDS_N, 2048, 10), LAST_LDS_N, seed, 2048, 10)
    seed = _seed("after-the-large-one")
    _assert_table(e.compute_committees(next(_epoch), seed, 4096, 32, 90), 4096, seed, 32, 90)
