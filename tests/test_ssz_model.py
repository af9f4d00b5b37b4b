"""CPU: the SSZ model the engine's state roots are held to (tests/ssz_model.py) against known answers and against itself,
the SHA-256 of pos_evolution_amd/csrc/sha256.h compiled for the HOST from the very header the gfx950 kernels include
(tests/native/sha256_host.cpp) against hashlib, the recorded vectors (tests/golden/ssz_vectors.json), and the resource
report of ssz_kernels.hip.  The same native source builds as a stand-alone program that runs under AddressSanitizer and
UBSan.  The GPU side is tests/test_gpu_ssz.py."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ssz_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sha256_host.cpp")


def _generator():
    spec_ = importlib.util.spec_from_file_location("generate_ssz", os.path.join(HERE, "golden", "generate_ssz.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("sha256_host") / "libsha256_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.shh_sha256_64.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.shh_sha256_64.restype = None
    lib.shh_sha256_one_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.shh_sha256_one_block.restype = C.c_int
    return lib


def host_sha256_64(lib, msgs: np.ndarray) -> np.ndarray:
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(-1, 64)
    out = np.zeros((msgs.shape[0], 32), dtype=np.uint8)
    lib.shh_sha256_64(msgs.ctypes.data, msgs.shape[0], out.ctypes.data)
    return out


def host_one_block(lib, msg: bytes) -> bytes:
    buf = np.frombuffer(bytes(msg) + b"\0", dtype=np.uint8).copy()
    out = np.zeros(32, dtype=np.uint8)
    assert lib.shh_sha256_one_block(buf.ctypes.data, len(msg), out.ctypes.data) == 0
    return out.tobytes()


# ------------------------------------------------------------------ the model
def test_zero_hashes_known_answers():
    assert M.Z[0] == bytes(32) and len(M.Z) == 65
    for k, (head, tail) in {1: ("f5a5fd42", "2759fb4b"), 2: ("db56114e", "748b5d71"), 3: ("c78009fd", "105ab33c")}.items():
        assert M.Z[k].hex().startswith(head) and M.Z[k].hex().endswith(tail), k
    for k in range(64):
        assert M.Z[k + 1] == hashlib.sha256(M.Z[k] * 2).digest()


def test_the_two_merkleize_forms_agree():
    rng = np.random.default_rng(65)
    chunks = [rng.bytes(32) for _ in range(130)]
    checked = 0
    for depth in range(10):
        for n in range(min(130, 2**depth) + 1):
            assert M.merkleize(chunks[:n], depth) == M.merkleize_literal(chunks[:n], depth), (n, depth)
            checked += 1
    assert checked == sum(min(130, 2**d) + 1 for d in range(10))
    with pytest.raises(AssertionError):
        M.merkleize(chunks[:5], 2)


def test_all_zero_chunks_give_the_zero_hash():
    for depth in range(8):
        for n in (0, 1, 2**depth):
            assert M.merkleize([bytes(32)] * n, depth) == M.Z[depth]


def test_empty_list_roots():
    for limit_log2 in (5, 6, 40, 64):
        want8 = hashlib.sha256(M.Z[limit_log2 - 5] + bytes(32)).digest()
        want64 = hashlib.sha256(M.Z[limit_log2 - 2] + bytes(32)).digest()
        assert M.u8_list_root([], limit_log2) == want8
        assert M.u64_list_root([], limit_log2) == want64
        assert M.validators_root([], limit_log2) == hashlib.sha256(M.Z[limit_log2] + bytes(32)).digest()


def test_packing():
    assert M.pack_u64([1, 2**64 - 1]) == [bytes([1]) + bytes(7) + b"\xff" * 8 + bytes(16)]
    assert M.pack_u64([0x0102030405060708] * 5)[1] == bytes([8, 7, 6, 5, 4, 3, 2, 1]) + bytes(24)
    assert M.pack_u8(range(33)) == [bytes(range(32)), bytes([32]) + bytes(31)]
    assert M.pack_u8([]) == [] and M.pack_u64([]) == []
    assert M.mix_in_length(bytes(32), 2**40 + 3) == hashlib.sha256(bytes(32) + (2**40 + 3).to_bytes(8, "little") + bytes(24)).digest()


def test_one_validator_root_by_hand():
    """The 15 hashes of hash_tree_root(Validator) written out: the pubkey's leaf, the seven nodes of the depth-3 tree, and
    for the list of this one validator the tree above it and the length."""
    sha = lambda b: hashlib.sha256(b).digest()  # noqa: E731
    pk, wc = bytes(range(48)), bytes(range(100, 132))
    eff, slashed, elig, act, ext, wdr = 32 * 10**9, 1, 5, 2**64 - 1, 0x0102030405060708, 77
    le = lambda v: v.to_bytes(8, "little") + bytes(24)  # noqa: E731
    leaf_pk = sha(pk[:32] + pk[32:] + bytes(16))
    h01 = sha(leaf_pk + wc)
    h23 = sha(le(eff) + bytes([1]) + bytes(31))
    h45 = sha(le(elig) + le(act))
    h67 = sha(le(ext) + le(wdr))
    root = sha(sha(h01 + h23) + sha(h45 + h67))
    assert M.validator_root(pk, wc, eff, slashed, elig, act, ext, wdr) == root
    assert M.validator_root(pk, wc, eff, 0, elig, act, ext, wdr) != root
    # List[Validator, 2^3] of that one: three levels against Z[0], Z[1], Z[2], then the length
    top = sha(sha(sha(root + M.Z[0]) + M.Z[1]) + M.Z[2])
    assert M.validators_root([root], 3) == sha(top + (1).to_bytes(32, "little"))


# ------------------------------------------------------------------ sha256.h on the host
def test_sha256_64_against_hashlib(lib):
    rng = np.random.default_rng(64)
    msgs = rng.integers(0, 256, size=(10_000, 64), dtype=np.uint8)
    msgs[0], msgs[1] = 0x00, 0xFF
    got = host_sha256_64(lib, msgs)
    for i in range(msgs.shape[0]):
        assert got[i].tobytes() == hashlib.sha256(msgs[i].tobytes()).digest(), i


def test_sha256_one_block_against_hashlib(lib):
    rng = np.random.default_rng(55)
    for length in range(56):
        for msg in (bytes(length), b"\xff" * length, rng.bytes(length)):
            assert host_one_block(lib, msg) == hashlib.sha256(msg).digest(), (length, msg.hex())
    for _ in range(10_000 - 3 * 56):
        msg = rng.bytes(int(rng.integers(0, 56)))
        assert host_one_block(lib, msg) == hashlib.sha256(msg).digest(), msg.hex()
    out = np.zeros(32, dtype=np.uint8)
    assert lib.shh_sha256_one_block(np.zeros(64, dtype=np.uint8).ctypes.data, 56, out.ctypes.data) == 1 and not out.any()


def test_zero_hashes_through_the_header(lib):
    z = bytes(32)
    for k in range(64):
        z = host_sha256_64(lib, np.frombuffer(z + z, dtype=np.uint8))[0].tobytes()
        assert z == M.Z[k + 1], k + 1


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same source with its own main, under AddressSanitizer and UBSan: a host program, nothing loaded into python."""
    exe = tmp_path / "sha256_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSHH_MAIN", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "zero hashes and padding table exact" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ the recorded vectors
def test_the_fixture_regenerates_byte_for_byte():
    assert GEN.render() == open(M.GOLDEN_PATH).read()


def test_the_fixture_holds_the_model():
    cases = json.load(open(M.GOLDEN_PATH))
    assert len(cases) >= 12
    for c in cases:
        reg = GEN.from_json(c["registry"])
        assert [x.hex() for x in reg.validator_leaves()] == c["validator_leaves"], c["name"]
        assert {k: v.hex() for k, v in M.state_roots(reg, c["limit_log2"]).items()} == c["roots"], c["name"]
        # ... and the literal form where it is small enough to write out
        if c["limit_log2"] <= 6:
            leaves = [bytes.fromhex(x) for x in c["validator_leaves"]]
            assert M.mix_in_length(M.merkleize_literal(leaves, c["limit_log2"]), len(leaves)).hex() == c["roots"]["validators"]
            assert M.mix_in_length(M.merkleize_literal(M.pack_u64(reg.balances), c["limit_log2"] - 2),
                                   len(reg)).hex() == c["roots"]["balances"]
            assert M.mix_in_length(M.merkleize_literal(M.pack_u8(reg.current_epoch_participation), c["limit_log2"] - 5),
                                   len(reg)).hex() == c["roots"]["current_epoch_participation"]


# ------------------------------------------------------------------ the boundary and the build
def test_the_c_abi_declares_the_state_root_entry_points():
    from pos_evolution_amd import _abi
    lib_ = _abi.load()
    for name in ("pe_registry_set_static", "pe_registry_get_static", "pe_state_roots", "pe_ssz_merkleize"):
        assert name in _abi.SIGNATURES and hasattr(lib_, name), name
    assert lib_.pe_abi_version() >= 13
    assert C.sizeof(_abi.pe_state_root_set) == 160
    assert [f[0] for f in _abi.pe_state_root_set._fields_] == list(M.state_roots(M.Registry()).keys())


def test_shuffle_kernels_share_the_header():
    """One source: the shuffle's kernels include sha256.h and keep no copy of the round constants or the function."""
    text = open(os.path.join(ROOT, "pos_evolution_amd", "csrc", "shuffle_kernels.hip")).read()
    assert '#include "sha256.h"' in text
    assert "0x428a2f98" not in text and not re.search(r"void\s+sha256_one_block", text)


def test_ssz_kernels_use_no_scratch():
    """k_ssz_merkle (both forms), k_ssz_validator_roots, k_ssz_pubkey_roots: the unrolled schedule stays in registers (the
    Makefile keeps the compiler's report)."""
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "ssz_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("ssz_kernels.resource.log is written by the build")
    text = open(log).read()
    blocks = re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S)
    for kernel, want in (("k_ssz_merkle", 2), ("k_ssz_validator_roots", 1), ("k_ssz_pubkey_roots", 1)):
        mine = [b for name, b in blocks if kernel in name]
        assert len(mine) == want, kernel
        for block in mine:
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block), kernel
            assert "Dynamic Stack: False" in block, kernel
            assert int(re.search(r"VGPRs: (\d+)", block).group(1)) <= 128, kernel   # 512 lanes per workgroup must fit
