"""-m gpu: pe_process_block_operations (block_ops_kernels.hip) against the sequential loop of tests/block_ops_model.py, bit
for bit: every resident array read back (exit and withdrawable epochs, balances, the view's flags), every status and every
word of the stats.  There is no tolerance anywhere in this file.  256 = the slots of one workgroup (BLOCK_OPS_WG), 64 = a
wave; the registries hold 5, 257 or 2049 validators and the churn limit is 4, so that a handful of exits moves the queue.  At
most 17 workgroups: k_block_ops_scan sees one wave of partials here.  A block of 516 workgroups (the scan's cross-wave term, its
tile loop and the ragged last tile), n_slots at 255, 256, 257 and 512 for the call's last lane, and 300 operations for the search
over the slot offsets are tests/test_gpu_scan_tiles.py, with this file's helpers."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import pos_evolution_amd as pea
from pos_evolution_amd import engine as E
from tests import block_ops_cases as K
from tests import block_ops_model as B
from tests import registry_updates_model as M
from tests import ssz_model as SSZ

pytestmark = pytest.mark.gpu
CUR = K.CUR
PARAM_NAMES = [name for name, _ in pea._abi.pe_block_ops_params._fields_]


def abi(p):
    return {k: getattr(p, k) for k in PARAM_NAMES}


def load(e, a, cur=CUR, view=True, balances=True, keys=None):
    flags = M.view_flags(a, cur)
    e.set_validators(a["eff"], (flags & 3).astype(np.uint8))
    if view:
        e.state_set_validators(a["eff"], flags)
    e.registry_set_epochs(a["act"], a["ext"])
    if balances:
        e.state_set_balances(a["bal"], None, a["wdr"])
    if keys is not None:
        e.registry_set_static(keys[0], keys[1], a["elig"])
    return flags


def assert_registry(e, want):
    act, ext, _ = e.registry_get_epochs()
    bal, _, wdr, _ = e.state_get_balances()
    eff, flags, is_set = e.state_validators()
    assert is_set
    got = dict(act=act, ext=ext, wdr=wdr, bal=bal, eff=eff, slashed=(flags >> 1) & 1)
    for k, x in got.items():
        bad = np.flatnonzero(x != want[k])
        assert bad.size == 0, (k, int(bad[0]), int(x[bad[0]]), int(want[k][bad[0]]))


def check(e, a, proposer, ops, p, cur=CUR):
    """One call held to the loop; -> (the registry after it, statuses, stats)."""
    want, status, st = B.block_operations_sequential(a, cur, proposer, ops, p)
    got_status, got = e.process_block_operations(cur, proposer, ops, abi(p))
    assert [int(s) for s in got_status] == status
    assert got == st, (got, st)
    assert_registry(e, want)
    return want, status, st


def status_of(call, *args, **kw):
    try:
        call(*args, **kw)
    except pea.EngineError as err:
        return err.status
    return 0


def votes(tag=0, cur=CUR):
    return B.double_vote(cur - 1, tag)


# ---------------------------------------------------------------- list lengths across wave and workgroup edges
@pytest.fixture(scope="module")
def big():
    """one registry of 2049 validators for the list shapes; never written"""
    return K.registry(2049, 11, 3, False, K.params())


@pytest.mark.parametrize("length", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_list_lengths(engine_factory, big, length):
    n, p = 2049, K.params()
    rng = np.random.default_rng(length)
    i1 = sorted(int(x) for x in rng.choice(n, size=length, replace=False))
    i2 = sorted(set(i1[::2]) | {int(x) for x in rng.choice(n, size=min(n, length + 3), replace=False)})
    d1, d2 = votes()
    ops = [B.voluntary_exit(i1[0], CUR), B.attester_slashing(d1, d2, i1, i2), B.attester_slashing(*votes(1), [n - 1], [n - 1])]
    e = engine_factory()
    load(e, big)
    ops = [op for op, s in zip(ops, B.block_operations_sequential(big, CUR, 3, ops, p)[1]) if s == 0]
    _, _, st = check(e, big, 3, ops, p)
    assert st["n_invalid"] == 0 and st["n_slashed"] >= min(length, 2) // 2
    e.close()


# ---------------------------------------------------------------- intersections and bad lists
def test_intersections(engine_factory):
    n, p = 257, K.params()
    a = M.blank_registry(n, p)
    a["bal"] += np.arange(n, dtype=np.uint64)
    whole = list(range(n))
    e = engine_factory()
    load(e, a)
    # empty: invalid, nothing moves
    _, status, st = check(e, a, 0, [B.attester_slashing(*votes(), whole[0::2], whole[1::2])], p)
    assert status == [B.NOBODY_SLASHABLE] and st["n_invalid"] == 1
    # only the last element of both lists
    a, _, st = check(e, a, 0, [B.attester_slashing(*votes(), whole[0:200:2] + [256], whole[1:200:2] + [256])], p)
    assert st["n_slashed"] == 1 and a["slashed"][256] == 1
    # the whole list: everyone else
    a, _, st = check(e, a, 0, [B.attester_slashing(*votes(1), whole, whole)], p)
    assert st["n_slashed"] == 256 and st["last_exit_epoch"] - st["first_exit_epoch"] == 64
    e.close()


@pytest.mark.parametrize("n", [5, 257])
def test_bad_lists(engine_factory, n):
    p = K.params()
    a = M.blank_registry(n, p)
    whole = list(range(n))
    e = engine_factory()
    load(e, a)
    swapped = whole[:-2] + [n - 1, n - 2]
    for i1, i2 in ((swapped, whole), (whole, swapped), (whole[:-1] + [n - 2], whole), (whole, whole[:-1] + [n]), (whole + [n], whole),
                   ([], whole), (whole, [])):
        ops = [B.voluntary_exit(0, CUR), B.attester_slashing(*votes(), i1, i2), B.proposer_slashing(1, 1, b"a" * 32, 1, 1, b"b" * 32)]
        _, status, st = check(e, a, 0, ops, p)
        assert status == [0, B.BAD_INDICES, 0] and st["n_invalid"] == 1
    # the bad lists' candidates took nothing: the same validators are all still slashable
    _, _, st = check(e, a, 0, [B.attester_slashing(*votes(), whole, whole)], p)
    assert st["n_slashed"] == n
    e.close()


# ---------------------------------------------------------------- one validator in several operations
@pytest.mark.parametrize("view", [True, False])
def test_the_same_validator_in_two_slashings_and_an_exit(engine_factory, view):
    """view False: the working-state view still mirrors pe_set_validators and is materialised by the call"""
    n, p = 5, K.params()
    a = M.blank_registry(n, p)
    a["slashed"][4], a["ext"][4], a["wdr"][4] = 1, CUR + 7, CUR + 9000
    e = engine_factory()
    load(e, a, view=view)
    first, second = B.attester_slashing(*votes(), [1, 2], [1, 2, 3]), B.attester_slashing(*votes(1), [0, 2, 4], [2, 4])
    _, status, _ = check(e, a, 3, [first, second], p)
    assert status == [0, B.NOBODY_SLASHABLE]                         # 2 was taken by the first, 4 was slashed before
    second = B.attester_slashing(*votes(1), [0, 2, 4], [0, 2, 4])
    _, status, _ = check(e, a, 3, [first, second, B.voluntary_exit(2, CUR)], p)
    assert status == [0, 0, B.ALREADY_EXITING]
    _, status, _ = check(e, a, 3, [B.voluntary_exit(2, CUR), first, second, B.voluntary_exit(3, CUR)], p)
    assert status == [0, 0, 0, 0]
    e.close()


# ---------------------------------------------------------------- the proposer among the slashed
@pytest.mark.parametrize("position", [0, 2, 4])
def test_the_proposer_slashed_at_each_position(engine_factory, position):
    """five slashings, reward 62 500 000 each, penalty 1 000 000 000: with 900 000 000 the proposer's penalty is cut unless two
    rewards arrived before it"""
    n, p = 5, K.params()
    a = M.blank_registry(n, p)
    a["bal"][position] = 900_000_000
    e = engine_factory()
    load(e, a)
    _, _, st = check(e, a, position, [B.attester_slashing(*votes(), list(range(n)), list(range(n)))], p)
    assert st["n_saturated"] == (1 if position < 2 else 0) and st["proposer_rewards"] == 5 * 62_500_000
    e.close()


@pytest.mark.parametrize("at", ["first", "middle", "last"])
def test_the_proposer_among_many(engine_factory, at):
    a, proposer, ops, p = K.random_block(257, {"first": 0, "middle": 1, "last": 2}[at], c0=3, proposer_at=at)
    assert K.classes_of(a, CUR, proposer, ops, p)["proposer_" + at]
    e = engine_factory()
    load(e, a)
    check(e, a, proposer, ops, p)
    e.close()


# ---------------------------------------------------------------- the exit queue
@pytest.mark.parametrize("c0,beyond", [(3, False), (4, False), (1, True), (2, True), (5, True)])
def test_the_exit_queue(engine_factory, c0, beyond):
    """c0 of 4 already leave at E0, six fresh exits: voluntary ones and a slashing's, interleaved with a slashing of a
    validator that is already leaving (it must not advance the rank)"""
    n, p = 257, K.params()
    a = M.blank_registry(n, p)
    e0 = CUR + 1 + p.max_seed_lookahead + (3 if beyond else 0)
    a["ext"][n - c0:], a["wdr"][n - c0:] = e0, e0 + 256
    a["ext"][0], a["wdr"][0] = e0 - 1, e0 + 255
    ops = [B.voluntary_exit(10, CUR), B.voluntary_exit(200, CUR), B.attester_slashing(*votes(), [0, 64, 65], [0, 64, 65]),
           B.voluntary_exit(5, CUR - 1), B.proposer_slashing(9, 130, b"a" * 32, 9, 130, b"b" * 32)]
    e = engine_factory()
    load(e, a)
    a, _, st = check(e, a, 1, ops, p)
    assert st["n_exits_initiated"] == 6 and st["n_slashed"] == 4
    assert st["first_exit_epoch"] == e0 + (1 if c0 >= 4 else 0) and st["last_exit_epoch"] == st["first_exit_epoch"] + (c0 % 4 + 5) // 4
    check(e, a, 1, [B.voluntary_exit(7, CUR)], p)                    # the queue's end is what the first call wrote
    e.close()


# ---------------------------------------------------------------- invalid blocks, refusals
def test_an_invalid_operation_in_the_middle(engine_factory):
    a, proposer, ops, p = K.random_block(257, 5, c0=3, valid=False)
    e = engine_factory()
    load(e, a)
    _, status, st = check(e, a, proposer, ops, p)
    assert st["n_invalid"] and status[-1] == B.NOBODY_SLASHABLE and 0 in status
    valid = [op for op, s in zip(ops, status) if s == 0]
    _, _, st = check(e, a, proposer, valid, p)
    assert st["n_invalid"] == 0 and st["n_slashed"] > 0
    e.close()


def test_every_status(engine_factory):
    p = K.params()
    a = M.blank_registry(8, p)
    a["act"][1], a["act"][2] = CUR + 1, CUR - 255
    a["ext"][3], a["wdr"][3] = CUR + 9, CUR + 9 + 256
    a["slashed"][4], a["ext"][4], a["wdr"][4] = 1, CUR + 5, CUR + 8000
    d1, d2 = votes()
    root = lambda x: bytes([x]) * 32  # noqa: E731
    ops = [B.attester_slashing(d1, d1, [0], [0]), B.attester_slashing(d1, d2, [0], [0], sig=False), B.attester_slashing(d1, d2, [0], [5]),
           B.attester_slashing(d1, d2, [4], [4]), B.proposer_slashing(1, 0, root(1), 2, 0, root(2)),
           B.proposer_slashing(1, 0, root(1), 1, 0, root(1)), B.proposer_slashing(1, 9, root(1), 1, 9, root(2)),
           B.proposer_slashing(1, 4, root(1), 1, 4, root(2)), B.proposer_slashing(1, 0, root(1), 1, 0, root(2), sig=False),
           B.voluntary_exit(8, 0), B.voluntary_exit(1, 0), B.voluntary_exit(3, 0), B.voluntary_exit(0, CUR + 1), B.voluntary_exit(2, 0),
           B.voluntary_exit(0, CUR, sig=False), B.voluntary_exit(0, CUR), B.voluntary_exit(0, CUR)]
    e = engine_factory()
    load(e, a)
    _, status, _ = check(e, a, 7, ops, p)
    assert sorted(set(status)) == [0] + list(range(64, 74))
    e.close()


def test_the_refusals(engine_factory):
    n, p = 257, K.params()
    a = M.blank_registry(n, p)
    ops = [B.attester_slashing(*votes(), [1, 2, 3], [2, 3]), B.voluntary_exit(9, CUR)]
    e = engine_factory()
    load(e, a, balances=False)
    assert status_of(e.process_block_operations, CUR, 0, ops, abi(p)) == pea._abi.PE_ERR_STATE
    e.state_set_balances(a["bal"], None, a["wdr"])
    # a range that runs past n_indices, handed over as the wrapper packs it
    arr, flat = E.pack_block_ops(ops)
    arr[0].indices_2_length = 3
    status, st, params = np.zeros(2, dtype=np.int32), pea._abi.pe_block_ops_stats(), e.block_ops_params(**abi(p))
    rc = e._lib.pe_process_block_operations(e._h, CUR, 0, C.addressof(arr), 2, flat.ctypes.data, flat.size, C.byref(params),
                                            status.ctypes.data, C.byref(st))
    assert rc == pea._abi.PE_ERR_INVALID_ARG
    for bad_p, proposer, cur in ((p, n, CUR), (K.params(min_slashing_penalty_quotient=0), 0, CUR), (p, 0, M.FAR - 8192),
                                 (K.params(min_validator_withdrawability_delay=M.FAR - CUR - 5), 0, CUR)):
        with pytest.raises(ValueError):
            B.block_operations_sequential(a, cur, proposer, ops, bad_p)
        assert status_of(e.process_block_operations, cur, proposer, ops, abi(bad_p)) == pea._abi.PE_ERR_INVALID_ARG
    assert_registry(e, a)                                            # none of them wrote
    _, _, st = check(e, a, 0, ops, p)                                # the same handle goes on
    assert st["n_slashed"] == 2 and st["n_exits_initiated"] == 3
    e.close()


# ---------------------------------------------------------------- chains
def test_two_calls_and_the_calls_that_follow(engine_factory):
    """slashings, then exits, as a block's two calls; then pe_process_slashings half a vector later penalises exactly the
    validators slashed here, and pe_state_roots hashes what the calls left"""
    n, p = 257, K.params()
    a = K.registry(n, 21, 3, True, p)
    rng = np.random.default_rng(4)
    pk, wc = rng.integers(0, 256, size=(n, 48), dtype=np.uint8), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    ops = [B.attester_slashing(*votes(), list(range(0, 120)), list(range(60, 200))), B.proposer_slashing(3, 201, b"x" * 32, 3, 201, b"y" * 32)]
    ops = [op for op, s in zip(ops, B.block_operations_sequential(a, CUR, 2, ops, p)[1]) if s == 0]
    e = engine_factory()
    load(e, a, keys=(pk, wc))
    before = a
    a, _, st1 = check(e, a, 2, ops, p)
    exits = [B.voluntary_exit(v, CUR) for v in range(200, 257)]
    exits = [op for op, s in zip(exits, B.block_operations_sequential(a, CUR, 2, exits, p)[1]) if s == 0]
    a, _, st2 = check(e, a, 2, exits, p)
    assert st1["n_slashed"] > 10 and st2["n_exits_initiated"] > 4 and st2["first_exit_epoch"] >= st1["last_exit_epoch"]
    roots = e.state_roots(E.ROOT_VALIDATORS | E.ROOT_BALANCES)
    leaves = [SSZ.validator_root(pk[v].tobytes(), wc[v].tobytes(), int(a["eff"][v]), int(a["slashed"][v]), int(a["elig"][v]),
                                 int(a["act"][v]), int(a["ext"][v]), int(a["wdr"][v])) for v in range(n)]
    assert roots == {"validators": SSZ.validators_root(leaves), "balances": SSZ.u64_list_root([int(x) for x in a["bal"]])}
    later = CUR + p.epochs_per_slashings_vector // 2
    flags = e.state_validators()[1]
    assert np.array_equal(flags, B.view_slashed_flags(M.view_flags(before, CUR), a["slashed"]))
    bal, sst = M.slashings_sequential(a, flags, later, st1["slashed_balance"], 3, p.epochs_per_slashings_vector)
    assert e.process_slashings(later, st1["slashed_balance"], 3, p.epochs_per_slashings_vector) == sst
    assert sst["n_penalised"] == st1["n_slashed"]
    assert np.array_equal(e.state_get_balances()[0], bal)
    newly = (a["slashed"] != 0) & (before["slashed"] == 0)
    assert int(newly.sum()) == st1["n_slashed"] and not (bal != a["bal"])[~newly].any() and (bal != a["bal"]).sum() > 10
    e.close()


# ---------------------------------------------------------------- the Python layer
def state_of(a, cur, slots_per_epoch, slashings):
    validators = [SimpleNamespace(effective_balance=int(a["eff"][v]), slashed=bool(a["slashed"][v]), activation_epoch=int(a["act"][v]),
                                  exit_epoch=int(a["ext"][v]), withdrawable_epoch=int(a["wdr"][v])) for v in range(a["eff"].size)]
    cp = SimpleNamespace(epoch=0, root=bytes(32))
    return SimpleNamespace(slot=slots_per_epoch * cur + 3, validators=validators, balances=[int(x) for x in a["bal"]],
                           slashings=list(slashings), current_epoch_participation=[0] * len(validators),
                           previous_epoch_participation=[0] * len(validators), current_justified_checkpoint=cp,
                           previous_justified_checkpoint=cp)


def registry_of(state, a):
    out = M.copy_registry(a)
    for k, name in (("ext", "exit_epoch"), ("wdr", "withdrawable_epoch"), ("slashed", "slashed")):
        out[k] = np.array([int(getattr(v, name)) for v in state.validators], dtype=out[k].dtype)
    out["bal"] = np.array(state.balances, dtype=np.uint64)
    return out


def test_the_forkchoice_mirror(engine_factory):
    from pos_evolution_amd import forkchoice as fc
    n, p = 5, K.params()
    a = M.blank_registry(n, p)
    e = engine_factory()
    e.set_validators(a["eff"], np.ones(n, dtype=np.uint8))
    state = state_of(a, CUR, int(e.cfg.slots_per_epoch), [0] * 8192)
    data = lambda root: fc.AttestationData(1, 0, root, fc.Checkpoint(CUR - 2, bytes(32)), fc.Checkpoint(CUR - 1, bytes(32)))  # noqa: E731
    slashing = fc.AttesterSlashing(fc.IndexedAttestation([1, 3], data(b"a" * 32)), fc.IndexedAttestation([0, 1, 3], data(b"b" * 32)))
    with pytest.raises(AssertionError):
        fc.process_attester_slashing(state, slashing, proposer_index=2, **abi(p))          # not bound
    fc.bind_state(e, state, bytes(32), 1000)
    same = fc.AttesterSlashing(slashing.attestation_1, slashing.attestation_1)
    for bad in (dict(attester_slashing=slashing, signature_valid=False), dict(attester_slashing=same)):
        with pytest.raises(AssertionError):
            fc.process_attester_slashing(state, proposer_index=2, **bad, **abi(p))
        got = registry_of(state, a)
        assert all(np.array_equal(got[k], a[k]) for k in M.FIELDS) and not any(state.slashings)
    op = B.attester_slashing(E.attestation_data_bytes(fc._data_row(slashing.attestation_1.data)),
                             E.attestation_data_bytes(fc._data_row(slashing.attestation_2.data)), [1, 3], [0, 1, 3])
    want, _, st = B.block_operations_sequential(a, CUR, 2, [op], p)
    fc.process_attester_slashing(state, slashing, proposer_index=2, **abi(p))
    got = registry_of(state, a)
    assert all(np.array_equal(got[k], want[k]) for k in M.FIELDS) and state._last_block_ops_stats == st
    assert state.slashings[CUR % 8192] == st["slashed_balance"] == 64 * M.ETH and sum(state.slashings) == 64 * M.ETH
    exit_ = SimpleNamespace(message=SimpleNamespace(validator_index=4, epoch=CUR))
    fc.process_voluntary_exit(state, exit_, **abi(p))
    with pytest.raises(AssertionError):
        fc.process_voluntary_exit(state, exit_, **abi(p))
    header = lambda tag: SimpleNamespace(message=SimpleNamespace(slot=7, proposer_index=0, tag=tag))  # noqa: E731
    fc.process_proposer_slashing(state, SimpleNamespace(signed_header_1=header(1), signed_header_2=header(2)),
                                 hash_tree_root=lambda h: bytes([h.tag]) * 32, proposer_index=2, **abi(p))
    want, status, _ = B.block_operations_sequential(want, CUR, 2, [B.voluntary_exit(4, CUR), B.proposer_slashing(7, 0, b"\1" * 32, 7, 0, b"\2" * 32)], p)
    got = registry_of(state, a)
    assert status == [0, 0] and all(np.array_equal(got[k], want[k]) for k in M.FIELDS)
    e.close()


def test_the_slashers_evidence_is_acted_on(engine_factory):
    """find_attester_slashings' output through attester_slashing_ops_from_evidence: exactly the validators the slasher named
    are slashed, on the handle that found them"""
    from oracle import spec
    from tests.scenario import new_world, slot_committee_members
    w = new_world(64, "minimal", engine_factory=engine_factory)
    anchor = w.store.justified_checkpoint.root
    w.tick_to_slot(1, offset=spec.SECONDS_PER_SLOT - 1)
    blk_a, blk_b = w.block(anchor, 1, graffiti=b"a"), w.block(anchor, 1, graffiti=b"b")
    w.tick_to_slot(3)
    xs = slot_committee_members(w.store, 2)
    fc, eng = w.fc, w.mirror.engine
    eng.slasher_enable(8, 64)
    assert fc.find_attester_slashings(w.mirror, w.attestation_for(xs, blk_a, 2)) == []
    named = sorted(xs)[:len(xs) - 1]
    evidence = fc.find_attester_slashings(w.mirror, w.attestation_for(named, blk_b, 2))
    assert evidence and sorted(v for s in evidence for v in s.attestation_1.attesting_indices) == named
    ops = fc.attester_slashing_ops_from_evidence(evidence)
    assert len(ops) == len(named) and all(op["i1"] == op["i2"] and len(op["i1"]) == 1 for op in ops)
    n, p = eng.num_validators, K.params()
    a = M.blank_registry(n, p)
    cur = 5
    flags = M.view_flags(a, cur)
    eng.state_set_validators(a["eff"], flags)
    eng.registry_set_epochs(a["act"], a["ext"])
    eng.state_set_balances(a["bal"], None, a["wdr"])
    p = K.params(shard_committee_period=0)
    want, status, st = B.block_operations_sequential(a, cur, 0, ops, p)
    got_status, got = eng.process_block_operations(cur, 0, ops, abi(p))
    assert [int(s) for s in got_status] == status == [0] * len(ops) and got == st
    assert_registry(eng, want)
    assert np.flatnonzero(want["slashed"]).tolist() == named
