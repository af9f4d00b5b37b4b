"""CPU: the per-validator rule of rewards and penalties (pos_evolution_amd/csrc/reward_row.h), its division by a
call-wide divisor and the host step that forms the scalars, compiled for the HOST from the very header the engine and
the gfx950 kernels include (tests/native/reward_row_host.cpp) and held to tests/rewards_model.py and to Python integers.
The same source builds as a stand-alone program that runs under AddressSanitizer and UBSan.  The kernels' resource log
must show no scratch."""
import copy
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rewards_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "reward_row_host.cpp")
U64 = 2**64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("reward_row") / "libreward_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.rrh_div.argtypes = [C.c_uint64, C.c_uint64]
    lib.rrh_div.restype = C.c_uint64
    lib.rrh_isqrt.argtypes = [C.c_uint64]
    lib.rrh_isqrt.restype = C.c_uint64
    lib.rrh_run.argtypes = [C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint64, C.c_int, C.c_uint32, C.c_void_p]
    lib.rrh_run.restype = C.c_int
    return lib


def host_run(lib, arrays, current_epoch, finalized_epoch, p, which=M.DO_BOTH):
    """-> (refusal code, balances, scores, stats) of the header's rule over numpy copies of `arrays`."""
    a = {k: np.ascontiguousarray(v).copy() for k, v in arrays.items()}
    params = np.array([p.increment, p.base_reward_factor, p.inactivity_score_bias, p.inactivity_score_recovery_rate,
                       p.inactivity_penalty_quotient], dtype=np.uint64)
    stats = np.zeros(9, dtype=np.uint64)
    rc = lib.rrh_run(a["eff"].size, a["eff"].ctypes.data, a["sflags"].ctypes.data, a["participation"].ctypes.data,
                     a["withdrawable"].ctypes.data, a["balances"].ctypes.data, a["scores"].ctypes.data, params.ctypes.data,
                     M.get_previous_epoch(current_epoch), int(M.is_in_inactivity_leak(current_epoch, finalized_epoch, p)),
                     which, stats.ctypes.data)
    return rc, a["balances"], a["scores"], [int(x) for x in stats]


def arrays_of(reg: M.Registry):
    return dict(eff=np.array(reg.effective_balance, dtype=np.uint64), sflags=np.array(reg.sflags(), dtype=np.uint8),
                participation=np.array(reg.participation, dtype=np.uint8),
                withdrawable=np.array(reg.withdrawable_epoch, dtype=np.uint64),
                balances=np.array(reg.balances, dtype=np.uint64), scores=np.array(reg.scores, dtype=np.uint64))


def divisors():
    """1, 64, A * 64 for A = 1 and 2^27, the increment, bias * quotient of both forks, and every power of two with its
    neighbours."""
    out = {1, 64, 1 * 64, 2**27 * 64, 10**9, 4 * 2**24, 4 * 3 * 2**24, 3, U64 - 1, U64 - 2, 2**63 + 1}
    for k in range(64):
        out |= {2**k - 1, 2**k, 2**k + 1}
    return sorted(d for d in out if 1 <= d < U64)


def test_division_is_exact_at_adversarial_numerators(lib):
    """Products just below 2^64, numerators at both sides of a multiple of the divisor, and the ends of the range."""
    checked = 0
    for d in divisors():
        top = (U64 - 1) // d
        numerators = {0, 1, d - 1, d, d + 1, U64 - 1, U64 - 2, U64 - d, 2**63, 2**63 - 1, 2**32 * (2**32 - 1)}
        for q in (1, 2, top // 2, top - 1, top):
            numerators |= {q * d - 1, q * d, q * d + 1}
        for n in numerators:
            if 0 <= n < U64:
                assert lib.rrh_div(n, d) == n // d, (n, d)
                checked += 1
    assert checked > 2000


def test_division_on_random_pairs(lib):
    rng = np.random.default_rng(11)
    for bits_n in (64, 63, 40):
        for bits_d in (1, 7, 31, 33, 62, 64):
            for _ in range(50):
                n = int(rng.integers(0, 2**63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2)) >> (64 - bits_n)
                d = max(1, int(rng.integers(0, 2**63, dtype=np.uint64)) * 2 + 1 >> (64 - bits_d))
                assert lib.rrh_div(n, d) == n // d, (n, d)


def test_isqrt(lib):
    from math import isqrt
    for n in [0, 1, 2, 3, 4, 8, 9, 2**20 * 32 * 10**9, 207 * 10**9, U64 - 1, 2**64 - 2**33, (2**32 - 1)**2, (2**32 - 1)**2 - 1]:
        assert lib.rrh_isqrt(n) == isqrt(n), n
    assert lib.rrh_isqrt(2**20 * 32 * 10**9) == 183178688


def test_the_fixture_through_the_header(lib):
    cases = json.load(open(M.GOLDEN_PATH))
    assert len(cases) >= 10
    for c in cases:
        p = M.Params(**c["params"])
        reg = M.Registry(**c["registry"])
        rc, bal, sc, stats = host_run(lib, arrays_of(reg), c["current_epoch"], c["finalized_epoch"], p, c["which"])
        if c["current_epoch"] == 0:
            continue  # the engine launches nothing at GENESIS_EPOCH: the rule is not asked
        assert rc == 0, c["name"]
        assert [int(x) for x in bal] == c["balances"], c["name"]
        assert [int(x) for x in sc] == c["scores"], c["name"]
        assert stats == c["stats"], c["name"]


@pytest.mark.parametrize("which", [M.DO_INACTIVITY, M.DO_DELTAS, M.DO_BOTH])
@pytest.mark.parametrize("finalized", [9, 2])
def test_random_registries_through_the_header(lib, which, finalized):
    for seed, n in ((5, 300), (6, 1000)):
        a = M.random_registry(n, seed, 12)
        want_bal, want_sc, st = M.run_numpy(**a, current_epoch=12, finalized_epoch=finalized, which=which)
        rc, bal, sc, stats = host_run(lib, a, 12, finalized, M.Params(), which)
        assert rc == 0
        assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc)
        assert stats == st.abi()


@pytest.mark.parametrize("score", [0, 1, 15, 16, 17])
def test_scores_around_the_recovery_rate_and_balances_around_each_penalty(lib, score):
    """One validator that misses every flag, with its balance one below, at and one above: the first flag penalty, the
    first two, all three penalties -- every place one of the sequential subtractions starts or stops being cut."""
    p = M.Params()
    eff = 32 * 10**9
    others = 100  # full participants: they fix total_active and keep the validator under test a small part of it
    base = M.Registry(effective_balance=[eff] * (others + 1), slashed=[0] * (others + 1), active_prev=[1] * (others + 1),
                      active_cur=[1] * (others + 1), participation=[7] * others + [0xF8],
                      withdrawable_epoch=[M.FAR_FUTURE_EPOCH] * (others + 1), balances=[eff] * (others + 1),
                      scores=[0] * others + [score])
    for finalized in (9, 2):
        probe = copy.deepcopy(base)
        pairs = []
        M.run(probe, 12, finalized, p, pairs_out=pairs)
        pens = [pairs[k][1][others] for k in (0, 1, 3)]
        assert pens[0] > 0 and pens[1] > 0 and pairs[2][1][others] == 0
        for upto in (pens[0], pens[0] + pens[1], sum(pens)):
            for delta in (-1, 0, 1):
                reg = copy.deepcopy(base)
                reg.balances[others] = max(0, upto + delta)
                want = copy.deepcopy(reg)
                st = M.run(want, 12, finalized, p)
                rc, bal, sc, stats = host_run(lib, arrays_of(reg), 12, finalized, p)
                assert rc == 0 and [int(x) for x in bal] == want.balances and [int(x) for x in sc] == want.scores
                assert stats == st.abi()
                assert st.n_saturated == (1 if reg.balances[others] < sum(pens) else 0)


def test_the_overflow_refusals_are_the_models(lib):
    p = M.Params()
    reg = M.issue_registry()
    big_score = copy.deepcopy(reg)
    big_score.scores[3] = 2**64 // (31 * 10**9)          # eff * (score + bias) leaves 64 bits, eff * score does not
    with pytest.raises(OverflowError):
        M.run(copy.deepcopy(big_score), 10, 8, p)
    assert host_run(lib, arrays_of(big_score), 10, 8, p)[0] == 5
    assert host_run(lib, arrays_of(big_score), 10, 8, p, M.DO_INACTIVITY)[0] == 0   # no product without the deltas
    wrap_score = copy.deepcopy(reg)
    wrap_score.scores[3] = 2**64 - 2
    assert host_run(lib, arrays_of(wrap_score), 10, 8, p, M.DO_INACTIVITY)[0] == 4
    rich = copy.deepcopy(reg)                             # 32000 increments each: base_reward * 26 fits, times U does not
    rich.effective_balance = [x * 1000 for x in reg.effective_balance]
    big_factor = M.Params(base_reward_factor=2**34)
    with pytest.raises(OverflowError):
        M.run(copy.deepcopy(rich), 10, 8, big_factor)
    assert host_run(lib, arrays_of(rich), 10, 8, big_factor)[0] == 3
    M.run(copy.deepcopy(rich), 10, 3, big_factor)         # in a leak no reward is formed: the call stands
    assert host_run(lib, arrays_of(rich), 10, 3, big_factor)[0] == 0
    assert host_run(lib, arrays_of(reg), 10, 8, M.Params(base_reward_factor=2**60))[0] == 1


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "reward_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRRH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "divisions exact" in out.stdout, out.stdout + out.stderr


def test_reward_kernels_use_no_scratch():
    """k_reward_sums / k_reward_apply: no spill, no dynamic stack, no dynamic LDS (the Makefile keeps the compiler's report)."""
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "reward_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("reward_kernels.resource.log is written by the build")
    text = open(log).read()
    for kernel in ("k_reward_sums", "k_reward_apply"):
        m = re.search(r"Function Name: \S*" + kernel + r"\S*(.*?)(?=Function Name:|\Z)", text, flags=re.S)
        assert m, kernel
        block = m.group(1)
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block), kernel
        assert "Dynamic Stack: False" in block, kernel
        assert int(re.search(r"VGPRs: (\d+)", block).group(1)) <= 64, kernel   # eight waves per SIMD
