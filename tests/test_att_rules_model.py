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


# ---------------------------------------------------------------- order inside a batch: tests/lmd_flag_cases.py
# The model's extensions -- committees of differing sizes, a table that is no partition, equivocating indices, the slot of
# the winning row -- pinned by running the spec's own on_attestation and process_attestation, row after row, over every
# batch of tests/lmd_flag_cases.py.  The world's committees are hand-made, so get_beacon_committee answers from its
# tables; everything that decides order (update_latest_messages, the flag loop) is the spec's text.
def _lmd_flag_cases(w):
    from tests import lmd_flag_cases as L

    for k in (2, 3, 5):
        for rot in range(k):
            for inter in (False, True):
                yield f"equal epochs k={k} rotation {rot} interleaved={inter}", L.equal_epochs(w, k, rot, inter)[0]
    for variant in ("sequence", "later first", "earlier first"):
        yield f"stored message, {variant}", L.stored_message(w, variant)
    for later_first in (True, False):
        for inter in (False, True):
            yield f"two tables, later first={later_first} interleaved={inter}", L.two_tables(w, later_first, inter)
    for between in (False, True):
        yield f"equivocating, between={between}", L.equivocating(w, between)
    for r, orders in L.FLAG_ORDERS.items():
        for masks in orders:
            for rot in range(r):
                for inter in (False, True):
                    yield f"flag rounds {masks} rotation {rot} interleaved={inter}", L.flag_rounds(w, masks, rot, inter)
    for at in (False, True):
        yield f"straddle at_threshold={at}", L.straddle(w, at)
    rows, groups = L.voided_group(w)
    yield "voided group", [("batch", groups)]


@pytest.mark.parametrize("hot,n_val,overlapping", [(64, 4096, False), (129, 4100, False), (65, 4096, True), (1, 4096, True)])
def test_order_cases_against_the_spec(monkeypatch, hot, n_val, overlapping):
    from tests import lmd_flag_cases as L
    from tests.scenario import genesis

    w = L.world(hot, n_val, overlapping)
    with C.preset():
        assert spec.SLOTS_PER_EPOCH == L.SPE
        anchor_state, block = genesis(8)   # the store's anchor; the state the rows are processed on is another object
        genesis_state, _ = genesis(8)
        rewards = []
        monkeypatch.setattr(spec, "get_beacon_committee",
                            lambda st, slot, index: list(w.members_of(slot // L.SPE, (slot % L.SPE) * L.CPS + index)))
        monkeypatch.setattr(spec, "get_committee_count_per_slot", lambda st, ep: L.CPS)
        monkeypatch.setattr(spec, "get_base_reward", lambda st, i: w.increments[i] * w.brpi)
        monkeypatch.setattr(spec, "get_beacon_proposer_index", lambda st: 0)
        monkeypatch.setattr(spec, "increase_balance", lambda st, i, delta: rewards.append(delta))
        monkeypatch.setattr(spec, "VOTE_EXPIRY_SLOTS", 200)   # the variant that records the slot of a latest message
        denominator = (spec.WEIGHT_DENOMINATOR - spec.PROPOSER_WEIGHT) * spec.WEIGHT_DENOMINATOR // spec.PROPOSER_WEIGHT
        n_cases = 0
        for name, steps in _lmd_flag_cases(w):
            n_cases += 1
            store = spec.get_forkchoice_store(anchor_state, block)
            for bname, parent, slot in w.chain:
                store.blocks[spec.Root(w.R[bname])] = spec.BeaconBlock(
                    slot=slot, parent_root=spec.Root(w.R[parent]) if parent else spec.ZERO_ROOT)
            clock = L.S0
            state = _spec_state(w, genesis_state, w.sc[clock])
            state.current_epoch_participation = [0] * n_val
            state.previous_epoch_participation = [0] * n_val
            monkeypatch.setattr(spec, "store_target_checkpoint_state",
                                lambda store, target: store.checkpoint_states.__setitem__(target, state))
            model = M.Run(n_val, w.increments, w.brpi)
            for si, step in enumerate(steps):
                if step[0] == "mark":
                    store.equivocating_indices.update(step[1])
                    model.equivocating.update(step[1])
                    continue
                if step[0] == "tick":
                    clock = L.S1
                    state = _spec_state(w, genesis_state, w.sc[clock])
                    state.previous_epoch_participation = state.current_epoch_participation
                    state.current_epoch_participation = [0] * n_val
                    model.part = ([0] * n_val, model.part[0])
                    continue
                store.time = clock * spec.SECONDS_PER_SLOT
                want = model.batch(step[1], w.blocks, clock, w.sc[clock], w.committee_ctx(clock, False), w.members_of)
                for i, r in enumerate(step[1]):
                    where = f"{name}, step {si}, row {i} ({r['tag']})"
                    att = _attestation(r)
                    if r["overlap"]:   # an aggregate whose members share a bit never verifies (A.8)
                        att.signature_valid = False
                    try:
                        spec.on_attestation(store, att)
                        accepted = True
                    except AssertionError:
                        accepted = False
                    assert accepted == (want["status"][i] == M.OK), where
                for i, r in enumerate(step[1]):
                    where = f"{name}, step {si}, row {i} ({r['tag']})"
                    att = _attestation(r)
                    if r["overlap"]:
                        att.signature_valid = False
                    before = (list(state.current_epoch_participation), list(state.previous_epoch_participation))
                    del rewards[:]
                    try:
                        spec.process_attestation(state, att)
                        accepted = True
                    except AssertionError:
                        accepted = False
                    assert accepted == (want["pstatus"][i] == M.OK), where
                    after = (state.current_epoch_participation, state.previous_epoch_participation)
                    paid = sum(w.increments[v] * w.brpi * weight
                               for a, b in zip(before, after) for v in range(n_val) if a[v] != b[v]
                               for f, weight in enumerate(M.FLAG_WEIGHTS) if (b[v] & ~a[v]) >> f & 1)
                    assert want["numerator"][i] == paid, where
                    assert rewards == ([want["numerator"][i] // denominator] if accepted else []), where
                got = {int(v): (int(m.epoch), bytes(m.root)) for v, m in store.latest_messages.items()}
                assert got == model.latest, f"{name}, step {si}: latest messages"
                assert {int(v): int(s) for v, s in store.__dict__.get("latest_message_slots", {}).items()} == model.slots, \
                    f"{name}, step {si}: slots of the latest messages"
                assert list(state.current_epoch_participation) == model.part[0], f"{name}, step {si}"
                assert list(state.previous_epoch_participation) == model.part[1], f"{name}, step {si}"
            assert model.latest, name
        assert n_cases > 60


def test_order_cases_do_what_they_claim():
    """The first of the competing rows gives the message and the winner moves with the rotation; a later row of a flag
    round pays less than it would alone; equivocating validators and a voided group leave nothing."""
    from tests import lmd_flag_cases as L

    for overlapping in (False, True):
        w = L.world(65, 4096, overlapping)
        v = L.specials(w.n_val)[0]
        for k in (2, 3, 5):
            winners = set()
            for rot in range(k):
                for inter in (False, True):
                    steps, first = L.equal_epochs(w, k, rot, inter)
                    model = M.Run(w.n_val, w.increments, w.brpi)
                    out = L.replay(model, w, steps, False)
                    assert set(out[0]["status"]) == {M.OK} and set(out[0]["pstatus"]) == {M.OK}
                    assert model.latest[v] == (2, first["beacon_block_root"]) and model.slots[v] == first["slot"]
                    winners.add(model.latest[v][1])
            assert len(winners) == k
        for masks in ([1, 3, 7], [7, 3, 1], [1, 1, 3, 3, 7], [7, 3, 3, 1, 1]):
            for rot in range(len(masks)):
                steps = L.flag_rounds(w, masks, rot, False)
                model = M.Run(w.n_val, w.increments, w.brpi)
                out = L.replay(model, w, steps, False)[0]
                assert sorted(out["mask"]) == sorted(masks) and set(out["pstatus"]) == {M.OK}
                alone = [M.apply_flags([0] * w.n_val, [x for x, b in zip(w.members_of(2, r["slot"] % L.SPE), r["bits"]) if b],
                                       m, w.increments, w.brpi) for r, m in zip(steps[0][1], out["mask"])]
                assert out["numerator"][0] == alone[0] and all(a <= b for a, b in zip(out["numerator"], alone))
                assert any(a < b for a, b in zip(out["numerator"][1:], alone[1:]))
                assert model.part[0][v] == 7 if 7 in masks else 3
        model = M.Run(w.n_val, w.increments, w.brpi)
        L.replay(model, w, L.equivocating(w, False), False)
        assert v not in model.latest and model.part[0][v]
        model = M.Run(w.n_val, w.increments, w.brpi)
        L.replay(model, w, L.equivocating(w, True), False)
        assert model.latest[v][0] == 1
    w = L.world(64)
    rows, groups = L.voided_group(w)
    model = M.Run(w.n_val, w.increments, w.brpi)
    out = L.replay(model, w, [("batch", groups)], True)[0]
    assert out["status"] == [M.OK, M.BAD_SIGNATURE, M.OK, M.OK] and out["pstatus"] == out["status"]
    for at in (False, True):
        model = M.Run(w.n_val, w.increments, w.brpi)
        L.replay(model, w, L.straddle(w, at), False)
        one = w.committees[1][L.ONE][0]
        assert model.latest[one] == (1, w.R["P35"]) and model.latest[w.committees[1][L.P127][0]] == (1, w.R["P35"])
