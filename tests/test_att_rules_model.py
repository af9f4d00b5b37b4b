"""tests/att_rules_model.py pinned to oracle/spec.py: for every row of the boundary matrix (tests/att_rules_cases.py) the
spec's validate_on_attestation and process_attestation run on a spec.Store / spec.BeaconState of the same world, and
  * accept / reject equals the model's status == 0,
  * the participation flags the spec set, and the array it set them in, equal the model's mask and `which`,
  * the model's status names the assert the spec raised at: the raising function is read off the traceback, the assert
    inside it is found by evaluating the function's asserts in the order of its text, with the spec's own helpers.
This is where the expected values of tests/test_gpu_att_rules.py come from."""
import traceback

import pytest

from oracle import spec
from tests import att_rules_cases as C
from tests import att_rules_model as M


@pytest.fixture(scope="module")
def pinned():
    w = C.world()
    with C.preset():
        genesis_state = C.spec_genesis_state()
        store = spec.get_forkchoice_store(*_anchor(genesis_state))
        for name, parent, slot in w.chain:
            store.blocks[spec.Root(w.R[name])] = spec.BeaconBlock(
                slot=slot, parent_root=spec.Root(w.R[parent]) if parent else spec.ZERO_ROOT)
        yield w, store, genesis_state


def _anchor(state):
    block = spec.BeaconBlock(slot=0, state_root=spec.hash_tree_root(state))
    return state, block


def _attestation(r):
    data = spec.AttestationData(slot=r["slot"], index=r["index"], beacon_block_root=spec.Root(r["beacon_block_root"]),
                                source=spec.Checkpoint(r["source"][0], spec.Root(r["source"][1])),
                                target=spec.Checkpoint(r["target"][0], spec.Root(r["target"][1])))
    return spec.Attestation(aggregation_bits=[bool(b) for b in r["bits"]], data=data, signature_valid=r["sig_valid"])


def _raising_function(exc):
    return traceback.extract_tb(exc.__traceback__)[-1].name


def _fc_assert(store, att, from_block):
    """The first failing assert of validate_on_attestation (A.4), in text order."""
    d, t = att.data, att.data.target
    if not from_block:
        cur = spec.compute_epoch_at_slot(spec.get_current_slot(store))
        prev = cur - 1 if cur > spec.GENESIS_EPOCH else spec.GENESIS_EPOCH
        if t.epoch not in [cur, prev]:
            return M.EPOCH_TIME, "validate_target_epoch_against_current_time"
    f = "validate_on_attestation"
    if not t.epoch == spec.compute_epoch_at_slot(d.slot):
        return M.EPOCH_SLOT, f
    if t.root not in store.blocks:
        return M.UNKNOWN_TARGET, f
    if d.beacon_block_root not in store.blocks:
        return M.UNKNOWN_BLOCK, f
    if not store.blocks[d.beacon_block_root].slot <= d.slot:
        return M.BLOCK_AFTER_SLOT, f
    if not t.root == spec.get_ancestor(store, d.beacon_block_root, spec.compute_start_slot_at_epoch(t.epoch)):
        return M.TARGET_NOT_ANCESTOR, f
    if not spec.get_current_slot(store) >= d.slot + 1:
        return M.SLOT_NOT_PAST, f
    return M.OK, None


def _state_assert(state, att):
    """The first failing assert of process_attestation (pe:724-730) and A.9, in text order."""
    d = att.data
    f = "process_attestation"
    if d.target.epoch not in (spec.get_previous_epoch(state), spec.get_current_epoch(state)):
        return M.EPOCH_TIME, f
    if not d.target.epoch == spec.compute_epoch_at_slot(d.slot):
        return M.EPOCH_SLOT, f
    if not d.slot + spec.MIN_ATTESTATION_INCLUSION_DELAY <= state.slot <= d.slot + spec.SLOTS_PER_EPOCH:
        return M.INCLUSION, f
    if not d.index < spec.get_committee_count_per_slot(state, d.target.epoch):
        return M.INDEX_RANGE, f
    if not len(att.aggregation_bits) == len(spec.get_beacon_committee(state, d.slot, d.index)):
        return M.BITS_LENGTH, f
    justified = state.current_justified_checkpoint if d.target.epoch == spec.get_current_epoch(state) \
        else state.previous_justified_checkpoint
    if not d.source == justified:
        return M.SOURCE, "get_attestation_participation_flag_indices"
    indexed = spec.get_indexed_attestation(state, att)
    if not spec.is_valid_indexed_attestation(state, indexed):  # pe:736: one assert, two statuses
        return (M.EMPTY if not indexed.attesting_indices else M.BAD_SIGNATURE), f
    return M.OK, None


def _spec_state(w, genesis_state, sc):
    state = genesis_state  # one registry for the whole module: only the fields below change between scenarios
    state.slot = sc.slot
    # block_roots: the state's own chain = the ancestry of its latest block
    state.block_roots = {}
    root = sc.tip
    while root is not None:
        parent, slot = w.blocks[root]
        state.block_roots[slot] = spec.Root(root)
        root = parent
    state.current_justified_checkpoint = spec.Checkpoint(sc.current_justified[0], spec.Root(sc.current_justified[1]))
    state.previous_justified_checkpoint = spec.Checkpoint(sc.previous_justified[0], spec.Root(sc.previous_justified[1]))
    return state


def _rows():
    w = C.world()
    return [pytest.param(si, ri, id=f"{sc['name']} / {ri}: {r['tag']}")
            for si, sc in enumerate(w.scenarios) for ri, r in enumerate(sc["rows"])]


@pytest.mark.parametrize("si,ri", _rows())
def test_row_against_the_spec(pinned, si, ri):
    w, store, genesis_state = pinned
    sc = w.scenarios[si]
    r = sc["rows"][ri]
    att = _attestation(r)
    cc = C.committee_ctx(sc["time"], resident=False)

    # ---- fork-choice side: validate_on_attestation
    store.time = sc["time"]
    want = M.fork_choice_status(r, w.blocks, sc["time"] // spec.SECONDS_PER_SLOT, cc)
    raised = None
    try:
        spec.validate_on_attestation(store, att, r["from_block"])
    except AssertionError as e:
        raised = e
    code, fn = _fc_assert(store, att, r["from_block"])
    assert (raised is None) == (code == M.OK)
    if raised is not None:
        assert _raising_function(raised) == fn
        assert want == code
    else:
        # past A.4 the model answers for get_indexed_attestation's committee (A.6): every epoch has a table here, the
        # bits have the committee's length and at least one is set, so all that is left is the flat committee id
        # and, for three rows, get_indexed_attestation (bits[i] for every member) and is_valid_indexed_attestation (A.7)
        target_state = _spec_state(w, genesis_state, sc["state"])
        expect = M.OK
        try:
            com = spec.get_beacon_committee(target_state, r["slot"], r["index"])
            assert com == w.members_of(r["target"][0], M.flat_committee(r, cc))
            try:
                indexed = spec.get_indexed_attestation(target_state, att)
                if not spec.is_valid_indexed_attestation(target_state, indexed):
                    expect = M.EMPTY if not indexed.attesting_indices else M.BAD_SIGNATURE
            except IndexError:
                expect = M.BITS_LENGTH
        except AssertionError:
            expect = M.INDEX_RANGE
        assert want == expect

    # ---- state side: process_attestation
    state = _spec_state(w, genesis_state, sc["state"])
    state.current_epoch_participation = [0] * C.N_VAL
    state.previous_epoch_participation = [0] * C.N_VAL
    want, mask, which = M.state_status(r, w.blocks, sc["state"], cc)
    raised = None
    try:
        spec.process_attestation(state, att)
    except AssertionError as e:
        raised = e
    code, fn = _state_assert(state, att)
    assert (raised is None) == (code == M.OK) == (want == M.OK)
    assert want == code
    parts = (state.current_epoch_participation, state.previous_epoch_participation)
    if raised is not None:
        assert _raising_function(raised) == fn
        assert not any(parts[0]) and not any(parts[1])
    else:
        com = spec.get_beacon_committee(state, r["slot"], r["index"])
        attesters = {v for v, b in zip(com, r["bits"]) if b}
        assert com == w.members_of(r["target"][0], M.flat_committee(r, cc))
        for v in range(C.N_VAL):
            assert parts[which][v] == (mask if v in attesters else 0)
        assert not any(parts[1 - which])


def test_every_targeted_status_occurs_in_its_scenario():
    w = C.world()
    for sc in w.scenarios:
        for resident in (False, True):
            run = M.Run(C.N_VAL, w.increments, w.brpi)
            out = run.batch(sc["rows"], w.blocks, sc["time"] // 12, sc["state"], C.committee_ctx(sc["time"], resident),
                            w.members_of)
            assert sc["want_status"] <= set(out["status"]), sc["name"]
            assert sc["want_pstatus"] <= set(out["pstatus"]), sc["name"]
            assert out["status"].count(M.OK) >= 3 and out["pstatus"].count(M.OK) >= 3   # plain valid rows
    state_masks = {m for sc in w.scenarios[2:] for m in
                   M.Run(C.N_VAL, w.increments, w.brpi).batch(sc["rows"], w.blocks, sc["time"] // 12, sc["state"],
                                                              C.committee_ctx(sc["time"], False), w.members_of)["mask"]}
    assert {0, 1, 2, 3, 7} <= state_masks
    # rows the state scenarios add only where the chain has a committee slot for them: each at least once, refused as meant
    for tag, status in (("source: current-epoch row with the previous justified checkpoint", M.SOURCE),
                        ("source: previous-epoch row with the current justified checkpoint", M.SOURCE),
                        ("flat committee id = n_committees", M.INDEX_RANGE)):
        hits = [M.state_status(r, w.blocks, sc["state"], C.committee_ctx(sc["time"], False))[0]
                for sc in w.scenarios[2:] for r in sc["rows"] if r["tag"] == tag]
        assert hits and all(h == status for h in hits), tag
    for delay in (0, 1, 2, 5, 6, 31, 32, 33):
        assert any(r["tag"] == f"inclusion delay {delay}" for sc in w.scenarios[2:] for r in sc["rows"]), delay


def test_first_accepted_row_of_a_committee_earns_the_flag():
    """pe:745-749 in batch order: in every state scenario the committee of (S - 1, index 1) is attested twice, wrong head
    first -- the second row earns TIMELY_HEAD alone for the validators both rows name."""
    w = C.world()
    sc = w.scenarios[4]
    run = M.Run(C.N_VAL, w.increments, w.brpi)
    out = run.batch(sc["rows"], w.blocks, sc["time"] // 12, sc["state"], C.committee_ctx(sc["time"], False), w.members_of)
    i = next(k for k, r in enumerate(sc["rows"]) if r["tag"] == "first wins: first row, wrong head")
    first, second = sc["rows"][i], sc["rows"][i + 1]
    assert (out["mask"][i], out["mask"][i + 1]) == (3, 7) and out["pstatus"][i] == out["pstatus"][i + 1] == 0
    com = w.members_of(first["target"][0], M.flat_committee(first, C.committee_ctx(sc["time"], False)))
    both = [v for v, a, b in zip(com, first["bits"], second["bits"]) if a and b]
    only2 = [v for v, a, b in zip(com, first["bits"], second["bits"]) if b and not a]
    assert both and only2
    assert out["numerator"][i + 1] == sum(w.increments[v] * w.brpi * 14 for v in both) + \
        sum(w.increments[v] * w.brpi * 54 for v in only2)
