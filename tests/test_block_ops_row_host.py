"""CPU: pos_evolution_amd/csrc/block_ops_row.h -- what an operation's own fields decide, the slots, the candidates' potency and
events, the statuses, the host step and the balance rule -- compiled for the HOST from the very header the engine and the
gfx950 kernels include (tests/native/block_ops_row_host.cpp walks the kernels' steps over host arrays) and held to
tests/block_ops_model.py.  The same source builds as a stand-alone program that runs under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pos_evolution_amd import _abi
from pos_evolution_amd.engine import pack_block_ops
from tests import block_ops_cases as K
from tests import block_ops_model as B
from tests import registry_updates_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "block_ops_row_host.cpp")
PARAM_NAMES = [name for name, _ in _abi.pe_block_ops_params._fields_]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("block_ops_row") / "libblock_ops_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.boh_block_operations.argtypes = ([C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p])
    lib.boh_block_operations.restype = C.c_int
    assert lib.boh_sizeof_op() == C.sizeof(_abi.pe_block_op)
    return lib


def host_call(lib, a, cur, proposer, ops, p):
    """-> (return code, registry after the call, statuses, stats)"""
    b = M.copy_registry(a)
    flags = M.view_flags(a, cur)
    arr, flat = pack_block_ops(ops)
    flat = np.ascontiguousarray(np.concatenate([flat, np.zeros(1, dtype=np.uint32)]))
    params = np.array([getattr(p, k) for k in PARAM_NAMES], dtype=np.uint64)
    status, stats = np.zeros(max(len(ops), 1), dtype=np.int32), np.zeros(11, dtype=np.uint64)
    rc = lib.boh_block_operations(b["eff"].size, b["act"].ctypes.data, b["ext"].ctypes.data, b["wdr"].ctypes.data, b["eff"].ctypes.data,
                                  flags.ctypes.data, b["bal"].ctypes.data, cur, proposer, C.addressof(arr), len(ops),
                                  flat.ctypes.data, flat.size - 1, params.ctypes.data, status.ctypes.data, stats.ctypes.data)
    b["slashed"] = ((flags >> 1) & 1).astype(np.uint8)
    return rc, b, [int(s) for s in status[:len(ops)]], dict(zip(B.STATS, (int(x) for x in stats)))


@pytest.mark.parametrize("knobs", K.GRID, ids=lambda k: "-".join(str(v) for v in k.values()))
def test_random_blocks_through_the_header(lib, knobs):
    a, proposer, ops, p = K.random_block(**knobs)
    want, status, st = B.block_operations_sequential(a, K.CUR, proposer, ops, p)
    rc, got, got_status, stats = host_call(lib, a, K.CUR, proposer, ops, p)
    assert rc == 0 and got_status == status and stats == st
    for k in M.FIELDS:
        assert np.array_equal(got[k], want[k]), k


def test_long_lists_and_their_edges(lib):
    """lists beyond a workgroup, the intersection in the last element only, a list bad in its last pair, an index equal to n"""
    n, p = 2049, K.params()
    a = K.registry(n, 5, 3, False, p)
    d1, d2 = B.double_vote(K.CUR - 1)
    whole = list(range(n))
    ops = [B.attester_slashing(d1, d2, whole, whole), B.voluntary_exit(7, K.CUR)]
    for block in (ops, [B.attester_slashing(d1, d2, list(range(0, 600, 2)) + [n - 1], list(range(1, 600, 2)) + [n - 1])],
                  [B.attester_slashing(d1, d2, whole[:-2] + [n - 1, n - 2], whole)], [B.attester_slashing(d1, d2, whole, whole + [n])],
                  [B.attester_slashing(d1, d2, whole, list(range(1, 600, 2)))]):
        want, status, st = B.block_operations_sequential(a, K.CUR, 11, block, p)
        rc, got, got_status, stats = host_call(lib, a, K.CUR, 11, block, p)
        assert rc == 0 and got_status == status and stats == st
        assert all(np.array_equal(got[k], want[k]) for k in M.FIELDS)


def test_the_refusals_are_the_models(lib):
    p = K.params()
    a = M.blank_registry(8, p)
    d1, d2 = B.double_vote(K.CUR - 1)
    ops = [B.attester_slashing(d1, d2, [1, 2], [1, 2])]
    big = M.copy_registry(a)
    big["eff"][:] = 2**63
    for code, b, cur, proposer, q in ((-7, a, K.CUR, 8, p), (1, a, K.CUR, 0, K.params(min_slashing_penalty_quotient=0)),
                                      (1, a, K.CUR, 0, K.params(whistleblower_reward_quotient=0)), (2, a, M.FAR - 8192, 0, p),
                                      (3, a, M.FAR - 9000, 0, K.params(max_seed_lookahead=9000)),
                                      (4, a, K.CUR, 0, K.params(0)),
                                      (5, a, K.CUR, 0, K.params(min_validator_withdrawability_delay=M.FAR - K.CUR - 5)),
                                      (6, big, K.CUR, 0, p)):
        with pytest.raises(ValueError):
            B.block_operations_sequential(b, cur, proposer, ops, q)
        rc, got, _, _ = host_call(lib, b, cur, proposer, ops, q)
        assert rc == code and all(np.array_equal(got[k], b[k]) for k in M.FIELDS)
    # a range past n_indices, an unknown kind
    arr, flat = pack_block_ops(ops)
    arr[0].indices_2_length = 3
    st, stats = np.zeros(1, dtype=np.int32), np.zeros(11, dtype=np.uint64)
    b, params = M.copy_registry(a), np.array([getattr(p, k) for k in PARAM_NAMES], dtype=np.uint64)
    flags = M.view_flags(a, K.CUR)
    args = lambda: (8, b["act"].ctypes.data, b["ext"].ctypes.data, b["wdr"].ctypes.data, b["eff"].ctypes.data, flags.ctypes.data,  # noqa: E731
                    b["bal"].ctypes.data, K.CUR, 0, C.addressof(arr), 1, flat.ctypes.data, flat.size, params.ctypes.data,
                    st.ctypes.data, stats.ctypes.data)
    assert lib.boh_block_operations(*args()) == -2
    arr[0].kind = 9
    assert lib.boh_block_operations(*args()) == -1


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "block_ops_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DBOH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "closed form exact" in out.stdout, out.stdout + out.stderr
