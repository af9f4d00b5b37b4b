"""CPU: the predicates, the exit queue's closed form, the (largest exit epoch, holders) pair and the slashing penalty of
pos_evolution_amd/csrc/registry_row.h, compiled for the HOST from the very header the engine and the gfx950 kernels include
(tests/native/registry_row_host.cpp) and held to tests/registry_updates_model.py.  The same source builds as a stand-alone
program that runs under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import registry_updates_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "registry_row_host.cpp")
CUR, FIN = 20, 18


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("registry_row") / "libregistry_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.rgh_registry_updates.argtypes = [C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_void_p]
    lib.rgh_registry_updates.restype = C.c_int
    lib.rgh_slashings.argtypes = [C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] * 5 + [C.c_void_p]
    lib.rgh_slashings.restype = C.c_int
    return lib


def host_updates(lib, a, cur, fin, p):
    b = M.copy_registry(a)
    params = np.array(list(p.abi().values()), dtype=np.uint64)
    stats = np.zeros(10, dtype=np.uint64)
    rc = lib.rgh_registry_updates(b["eff"].size, b["elig"].ctypes.data, b["act"].ctypes.data, b["ext"].ctypes.data,
                                  b["wdr"].ctypes.data, b["eff"].ctypes.data, params.ctypes.data, cur, fin, stats.ctypes.data)
    return rc, b, dict(zip(M.REGISTRY_STATS, (int(x) for x in stats)))


def host_slashings(lib, a, flags, cur, sum_slashings, multiplier, vector):
    bal = a["bal"].copy()
    stats = np.zeros(5, dtype=np.uint64)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    rc = lib.rgh_slashings(bal.size, a["eff"].ctypes.data, fl.ctypes.data, a["wdr"].ctypes.data, bal.ctypes.data, M.ETH, cur,
                           sum_slashings, multiplier, vector, stats.ctypes.data)
    return rc, bal, dict(zip(M.SLASHINGS_STATS, (int(x) for x in stats)))


@pytest.mark.parametrize("limit,cap", [(1, 0), (2, 1), (3, 0), (4, 8), (9, 8)])
def test_random_registries_through_the_header(lib, limit, cap):
    p = M.Params(min_per_epoch_churn_limit=limit, max_per_epoch_activation_churn_limit=cap)
    for seed, n in ((1, 1), (2, 63), (3, 300), (4, 1025)):
        a, _ = M.random_registry(n, seed, CUR, FIN, p)
        want, st = M.registry_updates_sequential(a, CUR, FIN, p)
        rc, got, stats = host_updates(lib, a, CUR, FIN, p)
        assert rc == 0 and stats == st
        for k in M.FIELDS:
            assert np.array_equal(got[k], want[k]), k


def test_the_refusals_are_the_models(lib):
    a, _ = M.random_registry(300, 9, CUR, FIN)
    for code, cur, p in ((1, CUR, M.Params(churn_limit_quotient=0)), (2, M.FAR - 5, M.Params()),
                         (3, CUR, M.Params(min_per_epoch_churn_limit=0)),
                         (4, CUR, M.Params(min_validator_withdrawability_delay=M.FAR - CUR - 6))):
        with pytest.raises(ValueError):
            M.registry_updates_numpy(a, cur, FIN, p)
        rc, got, _ = host_updates(lib, a, cur, FIN, p)
        assert rc == code and all(np.array_equal(got[k], a[k]) for k in M.FIELDS)


@pytest.mark.parametrize("sum_slashings", [0, 10**9, 10**13, 2**62])
def test_slashings_through_the_header(lib, sum_slashings):
    for seed, n in ((1, 1), (2, 300), (3, 1025)):
        a, _ = M.random_registry(n, seed, CUR, FIN, vector=64)
        flags = M.view_flags(a, CUR)
        want, st = M.slashings_sequential(a, flags, CUR, sum_slashings, 3, 64)
        rc, bal, stats = host_slashings(lib, a, flags, CUR, sum_slashings, 3, 64)
        assert rc == 0 and stats == st and np.array_equal(bal, want)
    assert host_slashings(lib, a, flags, CUR, 2**63, 3, 64)[0] == 1
    assert host_slashings(lib, a, flags, M.FAR - 3, 1, 3, 64)[0] == 2


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "registry_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRGH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "closed form exact" in out.stdout, out.stdout + out.stderr
