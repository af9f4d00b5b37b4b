"""CPU: pos_evolution_amd/csrc/withdrawals_row.h -- the predicates, the amount, the record, the next-index rule, the payload's
asserts, the list root, the change's checks, status rule and new credentials, the signing root -- compiled for the HOST from
the very header the engine and the gfx950 kernels include (tests/native/withdrawals_row_host.cpp walks the kernels' steps over
host arrays) and held to tests/withdrawals_model.py.  The same source builds as a stand-alone program that runs under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pos_evolution_amd.engine import pack_bls_changes, pack_withdrawals
from tests import withdrawals_model as W
from tests.test_withdrawals_model import EPOCH, MIN, changes_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "withdrawals_row_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("withdrawals_row") / "libwithdrawals_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.wrh_process_withdrawals.argtypes = ([C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] * 3 + [C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    lib.wrh_process_withdrawals.restype = C.c_int
    lib.wrh_bls_changes.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.wrh_bls_changes.restype = C.c_uint32
    lib.wrh_signing_roots.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert lib.wrh_record_words() * 4 == pack_withdrawals([]).dtype.itemsize
    assert lib.wrh_change_words() * 4 == pack_bls_changes([]).dtype.itemsize
    return lib


def host_call(lib, a, epoch, next_index, start, p, payload=None, apply=False):
    """-> (return code, registry after the call, expected withdrawals, result)"""
    b = W.copy_registry(a)
    cred = np.ascontiguousarray(b["cred"]).reshape(-1)
    cred = np.concatenate([cred, np.zeros(32, dtype=np.uint8)])
    arrs = [np.concatenate([b[k], np.zeros(1, dtype=np.uint64)]) for k in ("wdr", "eff", "bal")]
    params = np.array([p.max_effective_balance, p.max_withdrawals_per_payload, p.max_validators_per_sweep, p.eth1_prefix], dtype=np.uint64)
    rows = pack_withdrawals(payload or [])
    pay = np.frombuffer(rows.tobytes() + bytes(4), dtype=np.uint32).copy()
    out_list, res, root = np.zeros(64, dtype=rows.dtype), np.zeros(9, dtype=np.uint64), np.zeros(32, dtype=np.uint8)
    rc = lib.wrh_process_withdrawals(len(a["bal"]), cred.ctypes.data, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, epoch,
                                     next_index, start, params.ctypes.data, pay.ctypes.data, rows.size, payload is not None, apply,
                                     out_list.ctypes.data, res.ctypes.data, root.ctypes.data)
    b["bal"] = arrs[2][:-1]
    d = dict(zip(W.RESULT, (int(x) for x in res)))
    d["withdrawals_root"] = root.tobytes()
    got = [(int(w["index"]), int(w["validator_index"]), w["address"].tobytes(), int(w["amount"])) for w in out_list[:d["n_withdrawals"]]]
    return rc, b, got, d


def held(lib, a, epoch, next_index, start, p, payload=None, apply=False):
    want = W.process_withdrawals_sequential(a, epoch, next_index, start, p, payload, apply)
    rc, b, got, res = host_call(lib, a, epoch, next_index, start, p, payload, apply)
    assert rc == 0 and got == want[1] and res == want[2]
    assert all(np.array_equal(b[k], want[0][k]) for k in W.FIELDS)
    return want


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 255, 256, 257, 600])
def test_sweeps_through_the_header(lib, n):
    for p in (W.Params(max_validators_per_sweep=n), W.Params(max_validators_per_sweep=n + 13), MIN):
        for start in sorted({0, n - 1, (n - 40) % n}):
            a = W.set_hits(W.blank_registry(n, p), range(0, n, 3), p)
            _, expected, _ = held(lib, a, EPOCH, 2**40, start, p)
            held(lib, a, EPOCH, 2**40, start, p, expected, True)
            held(lib, a, EPOCH, 2**40, start, p, expected[:-1], True)


def test_random_states_through_the_header(lib):
    for n, seed, density, start in W.RANDOM_CASES:
        for p in (W.Params(), MIN, W.Params(max_validators_per_sweep=n + 5, max_withdrawals_per_payload=64)):
            a = W.random_registry(n, seed, EPOCH, p, density)
            _, expected, _ = held(lib, a, EPOCH, seed, start, p)
            held(lib, a, EPOCH, seed, start, p, expected, True)


def test_payload_asserts_through_the_header(lib):
    p = MIN
    a = W.set_hits(W.blank_registry(40, p), [1, 2, 5, 9], p)
    expected = W.get_expected_withdrawals(a, EPOCH, 9, 0, p)[0]
    for i, field in enumerate(range(4)):
        bad = [list(w) for w in expected]
        bad[i][field] = bytes(20) if field == 2 else bad[i][field] + 2**32
        _, _, res = held(lib, a, EPOCH, 9, 0, p, [tuple(w) for w in bad], True)
        assert res["status"] == W.WD_INDEX + field and res["first_mismatch"] == i and not res["applied"]
    held(lib, a, EPOCH, 9, 0, p, expected + [expected[0]][:0], False)
    held(lib, a, EPOCH, 9, 0, p, expected[:3], True)
    held(lib, a, EPOCH, 9, 0, p, [], True)


def test_the_refusals_are_the_models(lib):
    a = W.blank_registry(4)
    for start, index, p, payload, apply in ((4, 0, W.Params(), None, False), (0, 0, W.Params(max_effective_balance=0), None, False),
                                            (0, 0, W.Params(max_withdrawals_per_payload=0), None, False),
                                            (0, 0, W.Params(max_validators_per_sweep=0), None, False),
                                            (0, 0, W.Params(eth1_prefix=0), None, False), (0, 0, W.Params(eth1_prefix=256), None, False),
                                            (0, 0, W.Params(max_withdrawals_per_payload=65), None, False),
                                            (0, 0, MIN, [(0, 0, bytes(20), 0)] * 5, False), (0, 2**64 - 16, W.Params(), None, False),
                                            (0, 0, W.Params(), None, True)):
        with pytest.raises(ValueError):
            W.process_withdrawals_sequential(a, EPOCH, index, start, p, payload, apply)
        rc, b, _, _ = host_call(lib, a, EPOCH, index, start, p, payload, apply)
        assert rc != 0 and all(np.array_equal(b[k], a[k]) for k in W.FIELDS)


@pytest.mark.parametrize("n", [2, 5, 300])
def test_changes_through_the_header(lib, n):
    for cred, changes in changes_matrix(n):
        want, status, stats = W.process_bls_changes_sequential(cred, changes)
        got = np.concatenate([np.ascontiguousarray(cred).reshape(-1), np.zeros(32, dtype=np.uint8)])
        rows = pack_bls_changes(changes)
        st = np.zeros(len(changes), dtype=np.int32)
        n_invalid = lib.wrh_bls_changes(n, got.ctypes.data, rows.ctypes.data, rows.size, st.ctypes.data)
        assert [int(s) for s in st] == status and n_invalid == stats["n_invalid"]
        assert np.array_equal(got[:-32].reshape(n, 32), want)


def test_signing_roots_through_the_header(lib):
    changes = [W.change_for(v) for v in (0, 1, 2**40 + 3, 2**64 - 1)]
    rows, domain = pack_bls_changes(changes), np.arange(32, dtype=np.uint8)
    out = np.zeros((len(changes), 32), dtype=np.uint8)
    lib.wrh_signing_roots(rows.ctypes.data, rows.size, domain.ctypes.data, out.ctypes.data)
    assert [r.tobytes() for r in out] == [W.bls_change_signing_root(c, domain.tobytes()) for c in changes]


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "withdrawals_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DWRH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "closed form exact" in out.stdout, out.stdout + out.stderr
