"""-m gpu: SSZ roots from the resident arrays -- pe_ssz_merkleize, pe_registry_set_static / _get and pe_state_roots
(k_ssz_merkle, k_ssz_validator_roots, k_ssz_pubkey_roots) -- against tests/ssz_model.py (hashlib), byte for byte: there is
no tolerance anywhere in this file.

T = 1024: the nodes one workgroup of k_ssz_merkle reduces per pass (SSZ_TILE_LOG2 in kernels.h).  The shapes
below are its edges: chunk counts around T and T^2 (one pass, two, three), registries whose uint64 lists (4 to a chunk) and
uint8 lists (32 to a chunk) end on, before and behind a chunk and a tile."""
import ctypes as C
import json

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from pos_evolution_amd import engine as E
from pos_evolution_amd._abi import pe_state_ctx
from tests import ssz_model as M

pytestmark = pytest.mark.gpu
T = 1024
INVALID, STATE = -1, pea._abi.PE_ERR_STATE            # PE_ERR_INVALID_ARG, PE_ERR_STATE (include/posevo.h)
BITS = dict(balances=E.ROOT_BALANCES, inactivity_scores=E.ROOT_INACTIVITY, previous_epoch_participation=E.ROOT_PART_PREV,
            current_epoch_participation=E.ROOT_PART_CUR, validators=E.ROOT_VALIDATORS)
WIDE_INCREMENT = 2**48   # effective_balance / increment fits the engine's 16 bits for every uint64: all 64 bits in use


def test_the_tile_is_the_kernels():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pos_evolution_amd", "csrc", "kernels.h")).read()
    assert 1 << int(re.search(r"SSZ_TILE_LOG2\s*=\s*(\d+)", text).group(1)) == T


def smallest_depth(n: int) -> int:
    return max(0, (n - 1).bit_length())


def climb(root: bytes, frm: int, to: int) -> bytes:
    for k in range(frm, to):
        root = M.H(root + M.Z[k])
    return root


# ---------------------------------------------------------------- pe_ssz_merkleize
@pytest.fixture(scope="module")
def chunk_pool():
    """T^2 + 1 random chunks, shared and never written."""
    a = np.random.default_rng(1016).integers(0, 256, size=(T * T + 1, 32), dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def roots_0_to_1100(chunk_pool):
    """merkleize(chunks[:n], smallest depth) for n = 0 .. 1100 by the model, computed once."""
    chunks = [chunk_pool[i].tobytes() for i in range(1100)]
    return [M.merkleize(chunks[:n], smallest_depth(n)) for n in range(1101)]


def check_merkleize(e, pool, n, want_small):
    d0 = smallest_depth(n)
    for depth in (d0, d0 + 1, 38):
        want = climb(want_small, d0, depth)
        got = e.ssz_merkleize(pool[:n], depth)
        assert got == want, (n, depth)
    assert e.ssz_merkleize(pool[:n], d0 + 1, mix_length=n) == M.mix_in_length(climb(want_small, d0, d0 + 1), n), n


def test_merkleize_every_count_to_1100(engine_factory, chunk_pool, roots_0_to_1100):
    e = engine_factory()
    for n in range(1101):
        check_merkleize(e, chunk_pool, n, roots_0_to_1100[n])
    # the climb used above is the model's own definition, not the engine's: a few counts through the model at every depth
    chunks = [chunk_pool[i].tobytes() for i in range(1100)]
    for n in (0, 1, 2, 3, 513, 1025, 1100):
        for depth in (smallest_depth(n) + 1, 38):
            assert e.ssz_merkleize(chunk_pool[:n], depth) == M.merkleize(chunks[:n], depth), (n, depth)


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T - 1, 2 * T + 1])
def test_merkleize_at_the_tile_edges(engine_factory, chunk_pool, n):
    e = engine_factory()
    chunks = [chunk_pool[i].tobytes() for i in range(n)]
    check_merkleize(e, chunk_pool, n, M.merkleize(chunks, smallest_depth(n)))
    # bytes in, as well as arrays
    assert e.ssz_merkleize(b"".join(chunks), 38) == M.merkleize(chunks, 38)


@pytest.mark.parametrize("n", [T * T - 1, T * T, T * T + 1])
def test_merkleize_at_the_square_of_the_tile(engine_factory, chunk_pool, n):
    """Two passes that end in one workgroup, and the first count that needs a third."""
    e = engine_factory()
    flat = chunk_pool[:n].tobytes()
    want = M.merkleize([flat[i:i + 32] for i in range(0, len(flat), 32)], smallest_depth(n))
    check_merkleize(e, chunk_pool, n, want)


def test_all_zero_chunks_give_the_zero_hash(engine_factory):
    e = engine_factory()
    zeros = np.zeros((2 * T + 1, 32), dtype=np.uint8)
    for n in (0, 1, 2, 5, T - 1, T, T + 1, 2 * T + 1):
        for depth in (smallest_depth(n), smallest_depth(n) + 1, 38, 64):
            assert e.ssz_merkleize(zeros[:n], depth) == M.Z[depth], (n, depth)
    assert e.ssz_merkleize(zeros[:0], 7, mix_length=0) == M.H(M.Z[7] + bytes(32))


def test_merkleize_refusals_leave_the_output_alone(engine_factory, chunk_pool):
    e = engine_factory()
    out = np.full(32, 0xA5, dtype=np.uint8)
    ch = np.ascontiguousarray(chunk_pool[:9])
    for n, depth in ((5, 2), (2, 0), (9, 3), (1, 65), (0, 65)):
        rc = e._lib.pe_ssz_merkleize(e._h, ch.ctypes.data, n, depth, -1, out.ctypes.data)
        assert rc == INVALID and (out == 0xA5).all(), (n, depth)
    assert e.ssz_merkleize(ch[:8], 3) == M.merkleize([c.tobytes() for c in ch[:8]], 3)   # ... and the handle still works


# ---------------------------------------------------------------- pe_state_roots
def arrays_of(reg: M.Registry):
    u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
    return dict(pubkeys=np.frombuffer(b"".join(reg.pubkeys), dtype=np.uint8).reshape(-1, 48),
                wc=np.frombuffer(b"".join(reg.withdrawal_credentials), dtype=np.uint8).reshape(-1, 32),
                eff=u64(reg.effective_balance), slashed=np.array(reg.slashed, dtype=np.uint8),
                elig=u64(reg.activation_eligibility_epoch), act=u64(reg.activation_epoch), ext=u64(reg.exit_epoch),
                wdr=u64(reg.withdrawable_epoch), bal=u64(reg.balances), sc=u64(reg.inactivity_scores),
                prev=np.array(reg.previous_epoch_participation, dtype=np.uint8),
                cur=np.array(reg.current_epoch_participation, dtype=np.uint8))


def load(e, a, materialise):
    """A registry into an engine.  materialise False: the working-state view mirrors pe_set_validators; True: the registry
    is loaded with OTHER effective balances and `slashed` values and the view of its own carries the right ones."""
    n = a["eff"].size
    flags = (1 | (a["slashed"] << 1)).astype(np.uint8)
    if materialise:
        e.set_validators(a["eff"][::-1].copy(), (flags ^ 2).astype(np.uint8))
        e.state_set_validators(a["eff"], (flags | 8).astype(np.uint8))
    else:
        e.set_validators(a["eff"], flags)
    e.registry_set_epochs(a["act"], a["ext"])
    e.state_set_balances(a["bal"], a["sc"], a["wdr"])
    e.participation_set(0, a["cur"])
    e.participation_set(1, a["prev"])
    e.registry_set_static(a["pubkeys"], a["wc"], a["elig"])
    assert e.num_validators == n and e.state_validators()[2] == materialise


def resident(e):
    """Every resident array the roots are formed from, read back."""
    return [e.state_validators()[:2], e.registry_get_epochs()[:2], e.state_get_balances()[:3], e.participation_get(0),
            e.participation_get(1), e.registry_static()[:3]]


def same(x, y):
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return np.array_equal(x, y)


def check_roots(e, reg, leaves, limit_log2=40):
    want = M.state_roots(reg, limit_log2) if leaves is None else None
    if want is None:
        want = {"balances": M.u64_list_root(reg.balances, limit_log2),
                "inactivity_scores": M.u64_list_root(reg.inactivity_scores, limit_log2),
                "previous_epoch_participation": M.u8_list_root(reg.previous_epoch_participation, limit_log2),
                "current_epoch_participation": M.u8_list_root(reg.current_epoch_participation, limit_log2),
                "validators": M.validators_root(leaves, limit_log2)}
    got = e.state_roots(E.ROOT_ALL, limit_log2, want_leaves=True)
    if leaves is not None:
        got_leaves = got.pop("validator_leaves")
        for v in range(len(leaves)):   # a failure names the validator, not only the root
            assert got_leaves[v].tobytes() == leaves[v], f"hash_tree_root(Validator) of validator {v}"
    for name in want:
        assert got[name] == want[name], name
    return want


@pytest.mark.parametrize("n", [1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 4 * T - 1, 4 * T, 4 * T + 1, 32 * T + 1, 65537])
def test_state_roots_vs_model(engine_factory, n):
    reg = M.random_registry(n, 1000 + n)
    a = arrays_of(reg)
    assert (a["bal"] >> np.uint64(56)).all() and (a["sc"] >> np.uint64(56)).all()   # the top byte of every value is in use
    assert n < 256 or (len(set(a["prev"].tolist())) == 256 and len(set(a["cur"].tolist())) == 256)
    assert (a["ext"] == np.uint64(2**64 - 1)).any() and (n < 2 or set(a["slashed"].tolist()) == {0, 1})
    leaves = reg.validator_leaves()
    for materialise in (False, True):
        e = engine_factory(effective_balance_increment=WIDE_INCREMENT)
        load(e, a, materialise)
        before = resident(e)
        want = check_roots(e, reg, leaves)
        # bit by bit: only the field asked for is written
        for name, bit in BITS.items():
            got = e.state_roots(bit)
            assert list(got) == [name] and got[name] == want[name], name
            out = pea._abi.pe_state_root_set()
            C.memset(C.byref(out), 0x5A, C.sizeof(out))
            e._check(e._lib.pe_state_roots(e._h, bit, 0, C.byref(out), None))          # limit_log2 0 = 40
            for other in BITS:
                assert bytes(getattr(out, other)) == (want[name] if other == name else b"\x5a" * 32), (name, other)
        # the smallest limit that holds the registry: other depths through the same kernels
        small = max(5, smallest_depth(n))
        check_roots(e, reg, leaves, small)
        assert e.state_validators()[2] == materialise                                  # the view is not materialised
        assert same(resident(e), before)                                               # read-only
        e.close()


def test_empty_registry(engine_factory):
    e = engine_factory()
    e.set_validators(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    e.registry_set_epochs(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    e.state_set_balances(np.zeros(0, dtype=np.uint64))
    e.registry_set_static(np.zeros((0, 48), dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8), np.zeros(0, dtype=np.uint64))
    for limit_log2 in (5, 40):
        assert e.state_roots(E.ROOT_ALL, limit_log2) == M.state_roots(M.Registry(), limit_log2)


def test_golden_vectors(engine_factory):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_ssz.py")
    spec_ = importlib.util.spec_from_file_location("generate_ssz", path)
    gen = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(gen)
    for c in json.load(open(M.GOLDEN_PATH)):
        reg = gen.from_json(c["registry"])
        if len(reg) == 0:
            continue
        e = engine_factory(effective_balance_increment=WIDE_INCREMENT)
        load(e, arrays_of(reg), False)
        got = e.state_roots(E.ROOT_ALL, c["limit_log2"], want_leaves=True)
        assert [x.tobytes().hex() for x in got.pop("validator_leaves")] == c["validator_leaves"], c["name"]
        assert {k: v.hex() for k, v in got.items()} == c["roots"], c["name"]
        e.close()


def test_stale_tail_of_a_larger_registry(engine_factory):
    """A larger registry of 0xFF everywhere, then 257 validators on the same handle: nothing beyond element n is read."""
    e = engine_factory(effective_balance_increment=WIDE_INCREMENT)
    big = 5000
    ff64, ff8 = np.full(big, 2**64 - 1, dtype=np.uint64), np.full(big, 0xFF, dtype=np.uint8)
    e.set_validators(ff64, np.full(big, 3, dtype=np.uint8))
    e.registry_set_epochs(ff64, ff64)
    e.state_set_balances(ff64, ff64, ff64)
    e.participation_set(0, ff8)
    e.participation_set(1, ff8)
    e.registry_set_static(np.full((big, 48), 0xFF, dtype=np.uint8), np.full((big, 32), 0xFF, dtype=np.uint8), ff64)
    e.state_roots()
    reg = M.random_registry(257, 77)
    load(e, arrays_of(reg), False)
    check_roots(e, reg, reg.validator_leaves())


def test_refusals_write_nothing(engine_factory):
    reg = M.random_registry(40, 5)
    a = arrays_of(reg)
    e = engine_factory(effective_balance_increment=WIDE_INCREMENT)
    out = pea._abi.pe_state_root_set()

    def refused(status, which, limit_log2=40):
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        assert e._lib.pe_state_roots(e._h, which, limit_log2, C.byref(out), None) == status, (which, limit_log2)
        assert bytes(out) == b"\x5a" * 160

    flags = (1 | (a["slashed"] << 1)).astype(np.uint8)
    e.set_validators(a["eff"], flags)
    # nothing resident but participation
    for bit in (E.ROOT_BALANCES, E.ROOT_INACTIVITY, E.ROOT_VALIDATORS, E.ROOT_ALL):
        refused(STATE, bit)
    assert e.state_roots(E.ROOT_PART_CUR | E.ROOT_PART_PREV)["current_epoch_participation"] == M.u8_list_root([0] * 40)
    e.state_set_balances(a["bal"], a["sc"], a["wdr"])
    refused(STATE, E.ROOT_VALIDATORS)                     # no epochs, no static part
    e.registry_set_epochs(a["act"], a["ext"])
    refused(STATE, E.ROOT_VALIDATORS)                     # no static part
    assert e.registry_static()[3] is False
    e.registry_set_static(a["pubkeys"], a["wc"], a["elig"])
    leaf, wc, elig, is_set = e.registry_static()
    assert is_set and np.array_equal(wc, a["wc"]) and np.array_equal(elig, a["elig"])
    assert [x.tobytes() for x in leaf] == [M.pubkey_leaf(p) for p in reg.pubkeys]
    e.participation_set(0, a["cur"])
    e.participation_set(1, a["prev"])
    check_roots(e, reg, reg.validator_leaves())
    for which in (0, 32, 0x80000001):
        refused(INVALID, which)
    for limit_log2 in (1, 4, 65, 200):
        refused(INVALID, E.ROOT_ALL, limit_log2)
    refused(INVALID, E.ROOT_ALL, 5)                       # 2^5 < 40
    check_roots(e, reg, reg.validator_leaves(), 6)
    with pytest.raises(pea.EngineError) as err:           # a static part of another size
        e.registry_set_static(a["pubkeys"][:-1], a["wc"][:-1], a["elig"][:-1])
    assert err.value.status == INVALID and e.registry_static()[3]
    e.dist_init_custom(0, 1, lambda *args: 0, lambda *args: 0)
    refused(STATE, E.ROOT_ALL)
    e.dist_destroy()
    check_roots(e, reg, reg.validator_leaves())
    # dropped where the view is: a registry of another size, a new store
    e.set_validators(a["eff"][:-1], flags[:-1])
    assert not e.registry_static()[3]
    e.set_validators(a["eff"], flags)
    e.registry_set_static(a["pubkeys"], a["wc"], a["elig"])
    e.store_init(0, 0, bytes(32))
    assert not e.registry_static()[3]
    refused(STATE, E.ROOT_VALIDATORS)


# ---------------------------------------------------------------- the roots follow the device's own writes
def roots_over_read_back(e, reg):
    """The model over what the handle reads back now (validators: over the view, the epochs and the static part of reg)."""
    eff, sflags, _ = e.state_validators()
    bal, sc, wdr, _ = e.state_get_balances()
    act, ext, _ = e.registry_get_epochs()
    now = M.Registry(pubkeys=reg.pubkeys, withdrawal_credentials=reg.withdrawal_credentials,
                     effective_balance=[int(x) for x in eff], slashed=[int(x >> 1) & 1 for x in sflags],
                     activation_eligibility_epoch=reg.activation_eligibility_epoch, activation_epoch=[int(x) for x in act],
                     exit_epoch=[int(x) for x in ext], withdrawable_epoch=[int(x) for x in wdr],
                     balances=[int(x) for x in bal], inactivity_scores=[int(x) for x in sc],
                     previous_epoch_participation=e.participation_get(1).tolist(),
                     current_epoch_participation=e.participation_get(0).tolist())
    return M.state_roots(now), now


def test_roots_follow_rewards_and_the_balance_update(engine_factory):
    from tests import rewards_model as RM
    n = 1500
    a = RM.random_registry(n, 9, 12)
    reg = M.random_registry(n, 10, M.ENGINE_MAX_EFFECTIVE_BALANCE)
    e = engine_factory()
    e.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))
    e.state_set_validators(a["eff"], a["sflags"])
    e.participation_set(1, a["participation"])
    e.state_set_balances(a["balances"], a["scores"], a["withdrawable"])
    s = arrays_of(reg)
    e.registry_set_epochs(s["act"], s["ext"])
    e.registry_set_static(s["pubkeys"], s["wc"], s["elig"])
    first = e.state_roots()
    assert first == roots_over_read_back(e, reg)[0]
    st = e.rewards_and_penalties(12, 10)
    assert st["rewards"] > 0 and st["penalties"] > 0
    second = e.state_roots()
    want, now = roots_over_read_back(e, reg)
    assert second == want and now.balances != a["balances"].tolist()
    assert second["balances"] != first["balances"] and second["inactivity_scores"] != first["inactivity_scores"]
    assert second["validators"] == first["validators"]
    n_changed, _ = e.effective_balance_updates(pea.BALANCES_RESIDENT)
    assert n_changed > 0
    third = e.state_roots(want_leaves=True)
    leaves = third.pop("validator_leaves")
    want, now = roots_over_read_back(e, reg)
    assert [x.tobytes() for x in leaves] == now.validator_leaves()
    assert third == want and third["validators"] != second["validators"] and third["balances"] == second["balances"]


class _Chain:
    """A small store with committees for one epoch, as the smoke run builds one."""

    def __init__(self, n_val, seed):
        self.n_val, self.spe, self.n_comm = n_val, 32, 64
        self.tree = synth.random_tree(96, seed, "branchy")
        self.epoch = int(self.tree.slot.max()) // self.spe + 1
        self.comm = synth.random_committees(n_val, self.n_comm, seed)
        self.eff = synth.balances(n_val, seed, mixed=True)
        self.flags = synth.validator_flags(n_val, seed, inactive_frac=0.02)
        root0 = self.tree.roots[0].tobytes()
        self.atts, self.arena, _ = synth.epoch_attestations(self.comm, self.tree, self.epoch, self.spe, seed=1, density=0.8,
                                                            parts=2, source=(0, root0))
        self.ctx = pe_state_ctx()
        self.ctx.slot = (self.epoch + 1) * self.spe
        self.ctx.chain_tip_root[:] = self.tree.roots[95].tobytes()
        self.ctx.current_justified_root[:] = root0
        self.ctx.previous_justified_root[:] = root0
        self.ctx.base_reward_per_increment = 1000

    def start(self, e):
        e.store_init(0, 0, self.tree.roots[0].tobytes())
        for i in range(1, 96):
            e.add_block(self.tree.roots[i].tobytes(), self.tree.roots[int(self.tree.parent[i])].tobytes(), int(self.tree.slot[i]))
        e.set_validators(self.eff, self.flags, synth.registry_points(e, self.n_val))
        e.set_committees(self.epoch, self.comm.offsets, self.comm.members)
        e.on_tick((self.epoch + 1) * self.spe * 12)


PART = E.ROOT_PART_PREV | E.ROOT_PART_CUR


def part_roots(e):
    return {"previous_epoch_participation": M.u8_list_root(e.participation_get(1)),
            "current_epoch_participation": M.u8_list_root(e.participation_get(0))}


def test_roots_follow_the_flag_passes_and_the_rotation(engine_factory):
    """process_attestation's flag pass writes participation on another stream: the roots are ordered behind it, outside a
    pipeline and inside an open streaming one (which the call completes)."""
    chain = _Chain(3000, 3)
    plain, piped = engine_factory(), engine_factory()
    got = {}
    for e in (plain, piped):
        chain.start(e)
        empty = e.state_roots(PART)
        assert empty == part_roots(e) and not e.participation_get(1).any()
        if e is plain:
            agg = e.aggregate(packed=(chain.atts, chain.arena))
            e.on_attestation_batch(packed=(agg["atts"], agg["out_arena"]))
            st, _ = e.process_attestation_batch(chain.ctx, packed=(agg["atts"], agg["out_arena"]))
            assert (st == 0).all()
            got[e] = e.state_roots(PART)
        else:
            with e.pipeline(lagged=True):
                agg = e.aggregate(packed=(chain.atts, chain.arena), want_aggregate_pubkeys=True)
                e.on_attestation_batch(packed=(agg["atts"], pea.RESIDENT))
                st, _ = e.process_attestation_batch(chain.ctx, packed=(agg["atts"], pea.RESIDENT))
                got[e] = e.state_roots(PART)     # completes the open pipeline
            e.drain()
            assert (st == 0).all()
            assert e.state_roots(PART) == got[e]
        want = part_roots(e)
        assert got[e] == want and got[e] != empty and e.participation_get(1).any()
    assert got[plain] == got[piped]
    for e in (plain, piped):
        e.participation_rotate()
        after = e.state_roots(PART)
        assert after == part_roots(e)
        assert after["current_epoch_participation"] == M.u8_list_root([0] * chain.n_val)
        assert after["previous_epoch_participation"] == got[e]["current_epoch_participation"]


# ---------------------------------------------------------------- a million validators
def test_million_validators_vs_model(engine_factory):
    """All five roots of a registry of 2^20 validators.  The model's side is about 17 M hashlib calls: this is the file's
    one long case, as tests/test_gpu_full_size.py's are."""
    n = 1 << 20
    rng = np.random.default_rng(20)
    u64 = lambda: rng.integers(0, 2**64, size=n, dtype=np.uint64)  # noqa: E731
    a = dict(pubkeys=rng.integers(0, 256, size=(n, 48), dtype=np.uint8), wc=rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
             eff=u64(), slashed=rng.integers(0, 2, size=n, dtype=np.uint8), elig=u64(), act=u64(), ext=u64(), wdr=u64(),
             bal=u64(), sc=u64(), prev=rng.integers(0, 256, size=n, dtype=np.uint8), cur=rng.integers(0, 256, size=n, dtype=np.uint8))
    a["ext"][::7] = np.uint64(2**64 - 1)
    e = engine_factory(effective_balance_increment=WIDE_INCREMENT)
    load(e, a, False)
    got = e.state_roots(want_leaves=True)
    leaves = got.pop("validator_leaves")
    sha = M.H
    pk = np.concatenate([a["pubkeys"], np.zeros((n, 16), dtype=np.uint8)], axis=1)
    cols = [np.zeros((n, 32), dtype=np.uint8) for _ in range(6)]
    for col, key in zip(cols, ("eff", "slashed", "elig", "act", "ext", "wdr")):
        v = a[key]
        col[:, :v.dtype.itemsize] = v.astype("<u8" if v.dtype.itemsize == 8 else np.uint8).reshape(n, 1).view(np.uint8)
    want_leaves = []
    for v in range(n):
        h01 = sha(sha(pk[v].tobytes()) + a["wc"][v].tobytes())
        h23 = sha(cols[0][v].tobytes() + cols[1][v].tobytes())
        h45 = sha(cols[2][v].tobytes() + cols[3][v].tobytes())
        h67 = sha(cols[4][v].tobytes() + cols[5][v].tobytes())
        want_leaves.append(sha(sha(h01 + h23) + sha(h45 + h67)))
    assert want_leaves[:3] == M.Registry(
        pubkeys=[a["pubkeys"][v].tobytes() for v in range(3)], withdrawal_credentials=[a["wc"][v].tobytes() for v in range(3)],
        effective_balance=a["eff"][:3].tolist(), slashed=a["slashed"][:3].tolist(),
        activation_eligibility_epoch=a["elig"][:3].tolist(), activation_epoch=a["act"][:3].tolist(),
        exit_epoch=a["ext"][:3].tolist(), withdrawable_epoch=a["wdr"][:3].tolist(), balances=[0] * 3).validator_leaves()
    bad = np.flatnonzero((leaves != np.frombuffer(b"".join(want_leaves), dtype=np.uint8).reshape(n, 32)).any(axis=1))
    assert bad.size == 0, f"hash_tree_root(Validator) differs at validators {bad[:8]}"
    assert got == {"balances": M.u64_list_root(a["bal"]), "inactivity_scores": M.u64_list_root(a["sc"]),
                   "previous_epoch_participation": M.u8_list_root(a["prev"]),
                   "current_epoch_participation": M.u8_list_root(a["cur"]), "validators": M.validators_root(want_leaves)}
