"""CPU: which pe_att_status an attestation row gets (pos_evolution_amd/csrc/att_rules.h), compiled for the HOST from the very
header the engine's host routes and the gfx950 validators include (tests/native/att_rules_host.cpp, over a store of plain
arrays) and held to tests/att_rules_model.py -- which tests/test_att_rules_model.py pins row by row to oracle/spec.py -- on
every row of the boundary matrix (tests/att_rules_cases.py): the fork-choice side and the state side of every scenario,
under the committee tables of both kinds of route (every loaded epoch / the store's current and previous epoch) and both
readings of the bits' length the matrix exercises (host bits: at least the committee's; resident bits: exactly)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from tests import att_rules_cases as Cs
from tests import att_rules_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE32 = 0xFFFFFFFF
U64x10, U64x6, U64x4, U32x3 = C.c_uint64 * 10, C.c_uint64 * 6, C.c_uint64 * 4, C.c_uint32 * 3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("att_rules") / "libatt_rules.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "native", "att_rules_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    store = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.arl_fork_choice.argtypes = store + [U64x10, U64x4, U32x3, C.c_int, C.POINTER(C.c_uint32)]
    lib.arl_fork_choice.restype = C.c_int32
    lib.arl_state.argtypes = store + [C.c_uint32, U64x10, C.c_int, U64x6, U32x3, C.POINTER(C.c_int32)]
    lib.arl_state.restype = None
    lib.arl_indexed_status.argtypes = [C.c_int, C.c_int, C.c_uint32]
    lib.arl_indexed_status.restype = C.c_int32
    lib.arl_flag_mask.argtypes = [C.c_uint64] * 4 + [C.c_int, C.c_int]
    lib.arl_flag_mask.restype = C.c_uint32
    lib.arl_status_values.argtypes = [C.POINTER(C.c_int32)]
    lib.arl_status_values.restype = None
    return lib


class _Store:
    """The world's chain as the three arrays of the native store adapter; a root is its block's index + 1, a root the store
    does not know gets an id of its own."""

    def __init__(self, w):
        self.index = {w.R[name]: i for i, (name, _, _) in enumerate(w.chain)}
        n = len(w.chain)
        self.parent = (C.c_uint32 * n)(*[self.index[w.R[p]] if p else NONE32 for _, p, _ in w.chain])
        self.slot = (C.c_uint64 * n)(*[s for _, _, s in w.chain])
        self.root = (C.c_uint64 * n)(*range(1, n + 1))
        self.args = (n, self.parent, self.slot, self.root)
        self.unknown = {}

    def rid(self, root):
        if root in self.index:
            return self.index[root] + 1
        return self.unknown.setdefault(root, 2**40 + len(self.unknown))


def _row(store, r):
    return U64x10(r["slot"], r["index"], r["target"][0], store.rid(r["target"][1]), store.rid(r["beacon_block_root"]), r["n_bits"],
                  int(r["from_block"]), int(r["sig_valid"]), int(r["overlap"]), r["popcount"])


def _table(r, cc):
    return U32x3(int(r["target"][0] in cc.loaded_epochs), Cs.SPE * Cs.CPS, Cs.SIZE)


@pytest.fixture(scope="module")
def world():
    return Cs.world()


def test_status_constants_are_the_header_s(lib):
    out = (C.c_int32 * 15)()
    lib.arl_status_values(out)
    assert list(out) == sorted(v for name, v in M.ST.items() if v < 32) == list(range(15))


def test_fork_choice_matrix_equals_the_model(lib, world):
    w, store, compared = world, _Store(world), 0
    for sc in w.scenarios:
        cur_slot = sc["time"] // 12
        cur_epoch = cur_slot // Cs.SPE
        clock = U64x4(cur_slot, cur_epoch, max(cur_epoch - 1, 0), Cs.SPE)
        for resident in (False, True):
            cc = Cs.committee_ctx(sc["time"], resident)
            for i, r in enumerate(sc["rows"]):
                want = M.fork_choice_status(r, w.blocks, cur_slot, cc)
                blk = C.c_uint32()
                got = lib.arl_fork_choice(*store.args, _row(store, r), clock, _table(r, cc), int(resident), C.byref(blk))
                assert got == want, (sc["name"], resident, i, r["tag"])
                if want == M.OK:
                    assert blk.value == store.index[r["beacon_block_root"]], (sc["name"], i, r["tag"])
                compared += 1
    assert compared == 2 * sum(len(sc["rows"]) for sc in w.scenarios)


def test_state_matrix_equals_the_model(lib, world):
    w, store, compared = world, _Store(world), 0
    for sc in w.scenarios:
        s = sc["state"]
        cur_epoch = s.slot // Cs.SPE
        clock = U64x6(s.slot, cur_epoch, max(cur_epoch - 1, 0), Cs.SPE, M.MAINNET.min_delay, M.isqrt(Cs.SPE))
        for resident in (False, True):
            cc = Cs.committee_ctx(sc["time"], resident)
            for i, r in enumerate(sc["rows"]):
                want_st, want_mask, want_which = M.state_status(r, w.blocks, s, cc)
                justified = s.current_justified if r["target"][0] == cur_epoch else s.previous_justified
                out = (C.c_int32 * 4)()
                lib.arl_state(*store.args, store.index[s.tip], _row(store, r), int(tuple(r["source"]) == tuple(justified)), clock,
                              _table(r, cc), out)
                ladder, got_st, got_mask, got_which = out
                where = (sc["name"], resident, i, r["tag"])
                assert got_st == want_st and got_which == want_which, where
                assert (got_mask if got_st == M.OK else 0) == want_mask, where  # the model reports the mask of an accepted row
                assert ladder == M.OK or got_mask == 0, where
                compared += 1
    assert compared == 2 * sum(len(sc["rows"]) for sc in w.scenarios)


def test_indexed_status_asks_signature_then_overlap_then_emptiness(lib):
    """A.7 in the order the shared rule states: all eight combinations."""
    for sig_valid, overlap, empty in itertools.product((False, True), repeat=3):
        want = M.BAD_SIGNATURE if not sig_valid else M.BAD_SIGNATURE if overlap else M.EMPTY if empty else M.OK
        assert lib.arl_indexed_status(int(sig_valid), int(overlap), 0 if empty else 5) == want, (sig_valid, overlap, empty)


@pytest.mark.parametrize("spe", [32, 8])
def test_flag_mask_at_every_delay_s_edge(lib, spe):
    min_delay, sqrt_spe, seen = 1, M.isqrt(spe), set()
    for delay in (sqrt_spe, sqrt_spe + 1, spe, spe + 1, min_delay, min_delay + 1):
        for matching_target, matching_head in itertools.product((False, True), repeat=2):
            want = 0
            if delay <= M.isqrt(spe):
                want |= M.TIMELY_SOURCE
            if matching_target and delay <= spe:
                want |= M.TIMELY_TARGET
            if matching_head and delay == min_delay:
                want |= M.TIMELY_HEAD
            assert lib.arl_flag_mask(delay, sqrt_spe, spe, min_delay, int(matching_target), int(matching_head)) == want
            seen.add(want)
    assert {0, 1, 2, 3, 7} <= seen  # (TIMELY_HEAD alone cannot be: the minimum delay is within sqrt(SLOTS_PER_EPOCH))
