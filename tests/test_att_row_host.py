"""CPU: the two row rules every attestation route shares (pos_evolution_amd/csrc/att_row.h: the bits lie inside the arena;
which committee (slot, index) names), compiled for the HOST from the very header the engine's host paths and the gfx950
bodies include (tests/native/att_row_host.cpp) and held against Python integers: tests/att_rules_model.py's flat_committee
for the position, the plain inequality for the arena.  Every expected value is computed here, in unbounded integers."""
import ctypes as C
import os
import subprocess

import pytest

from tests import att_rules_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPE, CPS = 32, 2
N_COMMITTEES = SPE * CPS
CC = M.CommitteeCtx(cps=CPS, size=32, loaded_epochs=frozenset())
K = M.Consts(spe=SPE, min_delay=1)
SLOTS_IN_EPOCH = (0, 3, 31)
INDICES = (0, 1, 2, 57, 58, 2**32 - 2, 2**32 - 1, 2**32, 2**64 - 6, 2**64 - 1)
N_BITS = (0, 1, 8, 9, 0x7FFFFFFF, 0x80000000)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("att_row") / "libatt_row.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "native", "att_row_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.arh_bits_in_arena.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    lib.arh_bits_in_arena.restype = C.c_int
    lib.arh_committee_pos.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.arh_committee_pos.restype = None
    return lib


@pytest.mark.parametrize("index", INDICES)
@pytest.mark.parametrize("in_epoch", SLOTS_IN_EPOCH)
def test_committee_position_equals_the_model(lib, in_epoch, index):
    """Slots of three epochs (the epoch does not enter the position), among them 2^64 - 32 + in_epoch: the last epoch a
    64-bit slot has."""
    for slot in (in_epoch, 5 * SPE + in_epoch, 2**64 - SPE + in_epoch):
        flat = M.flat_committee(dict(slot=slot, index=index), CC, K)
        out = (C.c_uint32 * 3)()
        lib.arh_committee_pos(N_COMMITTEES, SPE, slot, index, out)
        assert out[1] == (1 if flat < N_COMMITTEES else 0), (slot, index)
        assert out[2] == (1 if index >= CPS else 0), (slot, index)
        if flat < N_COMMITTEES:
            assert out[0] == flat, (slot, index)


def test_the_wrapping_index_of_the_plain_sum_names_no_committee(lib):
    """slot % 32 = 3, two committees per slot, index = 2^64 - 6: a 64-bit sum wraps to position 0, which exists."""
    slot, index = 3, 2**64 - 6
    assert ((slot % SPE) * CPS + index) % 2**64 == 0 and M.flat_committee(dict(slot=slot, index=index), CC, K) == 2**64
    out = (C.c_uint32 * 3)()
    lib.arh_committee_pos(N_COMMITTEES, SPE, slot, index, out)
    assert (out[1], out[2]) == (0, 1)


def _arena_cases():
    """(bits_offset, n_bits, arena_len): the bits end one byte before the arena's end, at it and one byte past it -- with the
    offset chosen from the arena's length, and with the largest offset a row can carry."""
    for n_bits in N_BITS:
        n_bytes = (n_bits + 7) // 8
        arena_len = 0x30000000  # more than the bytes of 2^31 bits: every offset below is a 32-bit offset
        for end in (arena_len - 1, arena_len, arena_len + 1):
            yield end - n_bytes, n_bits, arena_len
        for arena_len in (0xFFFFFFFF + n_bytes - 1, 0xFFFFFFFF + n_bytes, 0xFFFFFFFF + n_bytes + 1):
            yield 0xFFFFFFFF, n_bits, arena_len


def test_bits_in_arena_equals_the_plain_inequality(lib):
    cases = list(_arena_cases())
    assert len(cases) == 6 * len(N_BITS) and all(0 <= offset <= 0xFFFFFFFF for offset, _, _ in cases)
    verdicts = set()
    for offset, n_bits, arena_len in cases:
        want = n_bits <= 0x7FFFFFFF and offset + (n_bits + 7) // 8 <= arena_len
        assert lib.arh_bits_in_arena(offset, n_bits, arena_len) == (1 if want else 0), (offset, n_bits, arena_len)
        verdicts.add((n_bits, want))
    # every length up to 2^31 - 1 bits is accepted at the edge and refused past it; 2^31 bits are refused wherever they lie
    assert verdicts == {(nb, w) for nb in N_BITS[:-1] for w in (True, False)} | {(0x80000000, False)}
