"""CPU: tests/deposits_model.py (process_deposit restated with hashlib) against hand-written cases and the sequential rule, the
committed vectors tests/golden/deposit_vectors.json, and pos_evolution_amd/csrc/deposit_row.h compiled for the HOST from the
very header the engine and the gfx950 kernels include (tests/native/deposit_row_host.cpp).  The same native source builds as
a stand-alone program that runs under AddressSanitizer and UBSan.

oracle/_ref holds the reference functions oracle/ref_extract.py lists (fork choice, attestations, shuffling); process_deposit
is not among them, so the model is held to the reference's text (pos-evolution.md lines 139-175) by reading, not by execution."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import deposits_model as M
from tests import ssz_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deposit_row_host.cpp")
ETH = 10**9


def dep(key: int, amount=32 * ETH, sig=0):
    return M.DepositData(bytes([key]) * 48, bytes([key ^ 0x55]) * 32, amount, bytes([sig]) * 96)


def small_registry(keys):
    reg = S.random_registry(len(keys), 3, S.ENGINE_MAX_EFFECTIVE_BALANCE)
    reg.pubkeys = [bytes([k]) * 48 for k in keys]
    return reg


def random_case(seed, n_reg, n):
    rng = np.random.default_rng(seed)
    reg = small_registry([int(x) for x in rng.integers(0, 40, size=n_reg)])        # duplicated pubkeys included
    deposits = [dep(int(rng.integers(0, 80)), int(rng.integers(0, 2**40)), int(rng.integers(0, 256))) for _ in range(n)]
    return reg, deposits, [bool(x) for x in rng.integers(0, 2, size=n)]


def test_hand_written_cases():
    reg = small_registry([1, 7, 7, 7])
    bal = list(reg.balances)
    deposits = [dep(7, 5), dep(9, 33 * ETH + 5), dep(9, 31 * ETH + 999), dep(9, 1), dep(11), dep(9, 2), dep(12, 7 * ETH)]
    status, index = M.process_deposits(reg, deposits, [False, False, True, False, False, True, True])
    assert status == [M.TOPUP, M.IGNORED_BAD_SIGNATURE, M.APPENDED, M.TOPUP, M.IGNORED_BAD_SIGNATURE, M.TOPUP, M.APPENDED]
    assert index == [1, M.NONE, 4, 4, M.NONE, 4, 5]                                 # .index(): the lowest of the duplicates
    assert reg.balances == [bal[0], bal[1] + 5, bal[2], bal[3], 31 * ETH + 999 + 1 + 2, 7 * ETH]
    assert reg.effective_balance[4:] == [31 * ETH, 7 * ETH] and reg.slashed[4:] == [0, 0]
    for field in ("activation_eligibility_epoch", "activation_epoch", "exit_epoch", "withdrawable_epoch"):
        assert getattr(reg, field)[4:] == [M.FAR_FUTURE_EPOCH] * 2
    assert reg.inactivity_scores[4:] == [0, 0] and reg.current_epoch_participation[4:] == [0, 0]
    assert M.process_deposits(small_registry([1]), [dep(2, 40 * ETH)], [True])[0] == [M.APPENDED]


def test_effective_balance_is_capped_and_floored():
    reg = small_registry([1])
    M.process_deposits(reg, [dep(2, 40 * ETH + 1), dep(3, ETH - 1), dep(4, 0)], [True] * 3)
    assert reg.effective_balance[1:] == [32 * ETH, 0, 0] and reg.balances[1:] == [40 * ETH + 1, ETH - 1, 0]


def test_proofs_and_the_assert():
    deposits = [dep(20 + i, ETH * (i + 1), i) for i in range(5)]
    leaves = [M.deposit_data_root(d) for d in deposits]
    assert leaves[0] == S.merkleize([S.pubkey_leaf(deposits[0].pubkey), deposits[0].withdrawal_credentials, S.u64_chunk(ETH),
                                     S.merkleize_literal(S.chunks_of(deposits[0].signature) + [S.ZERO_CHUNK], 2)], 2)
    for first in (0, 1, 6):
        root, proofs = M.deposit_tree_proofs(leaves, first)
        # the root is the deposit contract's: merkleize over the leaves, mixed with the count
        assert root == S.mix_in_length(S.merkleize([S.ZERO_CHUNK] * first + leaves, 32), first + 5)
        reg = small_registry([1])
        status, _ = M.process_deposits(reg, deposits, [True] * 5, proofs, first, root)
        assert status == [M.APPENDED] * 5 and len(reg) == 6
        for level in (0, 31, 32):
            bad = [list(p) for p in proofs]
            bad[3][level] = bytes(31) + b"\x01"
            reg = small_registry([1])
            status, index = M.process_deposits(reg, deposits, [True] * 5, bad, first, root)
            assert status == [0, 0, 0, M.BAD_PROOF, 0] and index == [M.NONE] * 5 and len(reg) == 1
    big = 2**32 - 1 + 5
    branch = [bytes([i + 1]) * 32 for i in range(33)]
    assert M.is_valid_merkle_branch(leaves[0], branch, 33, big, M.branch_root(leaves[0], branch, big))
    assert M.branch_root(leaves[0], branch, big) != M.branch_root(leaves[0], branch, big - 2**32)   # bit 32 of the index counts


@pytest.mark.parametrize("seed", range(6))
def test_golden_vectors(seed):
    g = json.load(open(M.GOLDEN_PATH))["cases"][seed]
    reg, deposits, sig_ok = random_case(g["seed"], g["n_reg"], g["n"])
    status, index = M.process_deposits(reg, deposits, sig_ok)
    assert status == g["status"] and index == g["index"] and len(reg) == g["n_after"]
    assert S.state_roots(reg)["validators"].hex() == g["validators_root"] and S.state_roots(reg)["balances"].hex() == g["balances_root"]
    assert M.signing_root(deposits[0], bytes(range(32))).hex() == g["signing_root_0"]
    assert M.deposit_data_root(deposits[0]).hex() == g["data_root_0"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("deposit_row") / "libdeposit_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", SRC,
                           "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.dph_roots.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p]
    lib.dph_process.argtypes = [C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p] + [C.c_void_p] * 6
    return lib


def test_header_hashing_against_the_model(lib):
    rng = np.random.default_rng(1)
    for i in range(20):
        d = M.DepositData(rng.bytes(48), rng.bytes(32), int(rng.integers(0, 2**63)) * 2 + 1, rng.bytes(96))
        domain, index = rng.bytes(32), int(rng.integers(0, 2**34))
        branch = [rng.bytes(32) for _ in range(33)]
        root = M.branch_root(M.deposit_data_root(d), branch, index)
        leaf, data, signing, ok = C.create_string_buffer(32), C.create_string_buffer(32), C.create_string_buffer(32), C.c_int(-1)
        lib.dph_roots(d.wire(), domain, b"".join(branch), index, root, leaf, data, signing, C.addressof(ok))
        assert leaf.raw == S.pubkey_leaf(d.pubkey) and data.raw == M.deposit_data_root(d) and signing.raw == M.signing_root(d, domain)
        assert ok.value == 1
        for level in (0, 31, 32):
            bad = list(branch)
            bad[level] = bytes(32)
            lib.dph_roots(d.wire(), domain, b"".join(bad), index, root, leaf, data, signing, C.addressof(ok))
            assert ok.value == 0
        lib.dph_roots(d.wire(), domain, b"".join(branch), index ^ (1 << 32), root, leaf, data, signing, C.addressof(ok))
        assert ok.value == 0


@pytest.mark.parametrize("seed,n_reg,n", [(1, 1, 1), (2, 63, 16), (3, 64, 65), (4, 65, 300), (5, 300, 300)])
def test_header_rules_against_the_model(lib, seed, n_reg, n):
    reg, deposits, sig_ok = random_case(seed, n_reg, n)
    for bad_proofs in ((), (n // 2,)):
        work = S.Registry(**{k: list(v) for k, v in reg.__dict__.items()})
        reg_leaves = b"".join(S.pubkey_leaf(p) for p in work.pubkeys)
        proof_ok = bytes(0 if i in bad_proofs else 1 for i in range(n))
        status, index = (C.c_int32 * n)(), (C.c_uint32 * n)()
        val = (C.c_uint64 * (7 * n))()
        slots, probes = C.c_uint32(0), C.c_uint32(0)
        params = (C.c_uint64 * 3)(ETH, 32 * ETH, M.FAR_FUTURE_EPOCH)
        rc = lib.dph_process(n_reg, reg_leaves, n, b"".join(d.wire() for d in deposits), bytes(int(x) for x in sig_ok), proof_ok,
                             C.addressof(params), C.addressof(status), C.addressof(index), C.addressof(val), C.addressof(slots),
                             C.addressof(probes))
        want_status, want_index = M.process_deposits(work, deposits, sig_ok)
        if bad_proofs:
            want_status = [M.BAD_PROOF if i in bad_proofs else s for i, s in enumerate(want_status)]
            want_index = [M.NONE] * n
        assert rc == (1 if bad_proofs else 0) and list(status) == want_status and list(index) == want_index
        assert slots.value == M.index_slots(n_reg + n)
        for i in range(n):
            if want_status[i] == M.APPENDED and not bad_proofs:
                v = want_index[i]
                assert list(val[7 * i:7 * i + 7]) == [work.effective_balance[v], M.FAR_FUTURE_EPOCH, M.FAR_FUTURE_EPOCH,
                                                      M.FAR_FUTURE_EPOCH, M.FAR_FUTURE_EPOCH, 0, work.effective_balance[v] // ETH]


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "deposit_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDPH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "deposit rules exact" in out.stdout, out.stdout + out.stderr


def test_the_new_kernels_do_not_spill():
    """Every kernel of deposit_kernels.hip: no scratch, no dynamic stack (the Makefile keeps the compiler's report)."""
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "deposit_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("deposit_kernels.resource.log is written by the build")
    text = open(log).read()
    names = re.findall(r"Function Name: (\S+)", text)
    for k in ("k_deposit_index_build", "k_deposit_leaves", "k_deposit_probe", "k_deposit_resolve", "k_deposit_apply"):
        assert any(k in n for n in names), k
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)] == [0] * len(names)
    assert "Dynamic Stack: True" not in text
