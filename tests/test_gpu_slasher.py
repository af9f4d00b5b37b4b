"""-m gpu: slashing detection on the device (pe_slasher_*, slash_kernels.hip) against the sequential model
(tests/slasher_model.py), whose every comparison is the reference's is_slashable_attestation_data (pe:1134-1143).
Per call: statuses, the number of pieces of evidence and the evidence MULTISET (ids resolved to the 128 data bytes)
equal the model's, and the records read back equal the model's history for every epoch of the window."""
from collections import Counter

import numpy as np
import pytest

import pos_evolution_amd as pea
from oracle import spec
from pos_evolution_amd import _abi, synth
from tests import slasher_model as sm
from tests.scenario import new_world, slot_committee_members
from tests.test_slasher_model import SPE, make_rows, random_history

pytestmark = pytest.mark.gpu
NONE32 = 0xFFFFFFFF


class Pair:
    """An engine with its slasher enabled and the model, fed the same calls and compared after each."""

    def __init__(self, engine_factory, n_val, history, max_data, comm_of_epoch, spe=SPE, only=None, engine=None):
        self.n_val, self.H = n_val, history
        if engine is None:
            engine = engine_factory(slots_per_epoch=spe, max_committee_tables=16)
            engine.store_init(0, 0, bytes([7]) * 32)
            engine.set_validators(np.full(n_val, 32 * 10**9, dtype=np.uint64), np.ones(n_val, dtype=np.uint8))
        self.e = engine
        self.model = sm.SlasherModel(n_val, history, max_data, spe, only=only)
        for epoch, comm in comm_of_epoch.items():
            self.set_committees(epoch, comm)
        self.e.slasher_enable(history, max_data)
        self._data = {}

    def set_committees(self, epoch, comm):
        self.e.set_committees(epoch, comm.offsets, comm.members)
        self.model.set_committees(epoch, comm.offsets, comm.members)

    def resolve(self, epoch, data_id):
        key = (int(epoch), int(data_id))
        if key not in self._data:
            self._data[key] = self.e.slasher_data(*key).tobytes()[:128]
        return self._data[key]

    def evidence_multiset(self, evidence):
        self._data = {}  # ids are per epoch slot: a slot that was reused hands them out again
        return Counter((int(ev["validator"]), int(ev["kind"]), self.resolve(ev["target_epoch_1"], ev["id_1"]),
                        self.resolve(ev["target_epoch_2"], ev["id_2"])) for ev in evidence)

    def ingest(self, atts, arena, w, cap=1 << 16, apply=False, engine_packed=None, sample=None):
        want_status, want_ev = self.model.ingest(atts, arena, w)
        status, ev = self.e.slasher_ingest(packed=engine_packed or (atts, arena), current_epoch=w, cap=cap, apply=apply)
        assert status.tolist() == want_status
        got = self.evidence_multiset(ev)
        if sample is not None:   # the model follows a sample of the registry: inside it the comparison is exact
            got = Counter({k: c for k, c in got.items() if k[0] in sample})
        else:
            assert self.e.slasher_found == len(want_ev)
        if cap >= self.e.slasher_found:
            assert got == Counter(want_ev)
        else:
            assert len(ev) == cap and not (got - Counter(want_ev))   # at most cap, each a member of the model's multiset
        return status, ev, want_ev

    def check_records(self, validators=None):
        w = self.model.W
        for epoch in range(max(0, w - self.H + 1), w + 1):
            src, ids = self.e.slasher_records(epoch)
            want = self.model.records_of(epoch) if validators is None else None
            for v in (range(self.n_val) if validators is None else validators):
                ws, wb = want[v] if want is not None else (
                    (self.model.records[v][epoch][0].source.epoch, self.model.records[v][epoch][1])
                    if epoch in self.model.records.get(v, {}) else (None, None))
                if ws is None:
                    assert src[v] == NONE32 and ids[v] == NONE32, (epoch, v)
                else:
                    assert int(src[v]) == ws and self.resolve(epoch, ids[v]) == wb, (epoch, v)


def flat_comm(n_val, n_epochs, seed=3):
    return {e: synth.random_committees(n_val, SPE, seed + e) for e in range(n_epochs)}


def first_member(comm, c=0):
    return int(comm.members[comm.offsets[c]])


@pytest.mark.parametrize("seed,history", [(1, 12), (2, 12), (3, 5), (4, 7)])
def test_random_histories_equal_the_model(engine_factory, seed, history):
    """>= 8 epochs, several calls per epoch, host bits; H = 5 and 7 slide the window over reused slots."""
    n_val, n_epochs = 48, 10
    comm_of_epoch, calls = random_history(seed, n_val, n_epochs)
    p = Pair(engine_factory, n_val, history, 1 << 12, comm_of_epoch)
    kinds = Counter()
    for w, votes in calls:
        atts, arena = make_rows(votes, comm_of_epoch, n_val)
        _, ev, _ = p.ingest(atts, arena, w)
        kinds.update(int(k) for k in ev["kind"])
        p.check_records()
    assert kinds[_abi.PE_SLASH_DOUBLE] and kinds[_abi.PE_SLASH_SURROUND]


def test_many_new_votes_of_one_validator_in_one_call(engine_factory):
    """More new votes of one validator in a call than the kernel holds in registers: seven different votes for one target
    epoch and votes for six further epochs, in one batch -- the later passes see the records of the earlier ones."""
    n_val = 32
    comm = flat_comm(n_val, 12)
    same = {e: comm[0] for e in range(12)}   # one shuffling for every epoch: the validator sits in committee 0 throughout
    p = Pair(engine_factory, n_val, 16, 64, same)
    v = first_member(comm[0])
    votes = [(9, 8, 0, salt, [v]) for salt in range(7)]
    votes += [(e, s, 0, 0, [v]) for e, s in ((11, 1), (10, 2), (8, 3), (7, 4), (6, 6), (5, 0))]
    votes += [(9, 8, 0, 0, [v]), (11, 1, 0, 5, [v])]
    atts, arena = make_rows(votes, same, n_val)
    _, ev, want = p.ingest(atts, arena, 11)
    assert len(want) > 10
    p.check_records()
    _, ev, want = p.ingest(atts, arena, 11)      # everything again: the recorded votes are silent, the others are not
    p.check_records()


def test_two_votes_in_one_batch_first_is_recorded(engine_factory):
    n_val = 32
    comm = flat_comm(n_val, 4)
    v = first_member(comm[2])
    for order in ((0, 1), (1, 0)):
        p = Pair(engine_factory, n_val, 8, 16, comm)
        votes = [(2, 1, 0, salt, [v]) for salt in order]
        atts, arena = make_rows(votes, comm, n_val)
        _, ev, _ = p.ingest(atts, arena, 2)
        assert len(ev) == 1 and ev[0]["kind"] == _abi.PE_SLASH_DOUBLE and ev[0]["validator"] == v
        assert p.resolve(2, ev[0]["id_1"]) == sm.data_bytes(atts[0])    # d1 = the first in batch order
        assert p.resolve(2, ev[0]["id_2"]) == sm.data_bytes(atts[1])
        src, ids = p.e.slasher_records(2)
        assert p.resolve(2, ids[v]) == sm.data_bytes(atts[0])
        p.check_records()


def test_surround_both_directions(engine_factory):
    n_val = 32
    same = {e: synth.random_committees(n_val, SPE, 9) for e in range(10)}
    v = first_member(same[0])
    outer, inner = (8, 2, 0, 0, [v]), (7, 3, 0, 0, [v])
    for first, second in ((outer, inner), (inner, outer)):
        # across calls
        p = Pair(engine_factory, n_val, 16, 16, same)
        a1, ar1 = make_rows([first], same, n_val)
        a2, ar2 = make_rows([second], same, n_val)
        p.ingest(a1, ar1, 8)
        _, ev, _ = p.ingest(a2, ar2, 8)
        assert len(ev) == 1 and ev[0]["kind"] == _abi.PE_SLASH_SURROUND
        assert (int(ev[0]["target_epoch_1"]), int(ev[0]["target_epoch_2"])) == (8, 7)   # d1 surrounds
        p.check_records()
        # inside one call, across two target epochs
        p = Pair(engine_factory, n_val, 16, 16, same)
        atts, arena = make_rows([first, second], same, n_val)
        _, ev, _ = p.ingest(atts, arena, 8)
        assert len(ev) == 1 and (int(ev[0]["target_epoch_1"]), int(ev[0]["target_epoch_2"])) == (8, 7)
        p.check_records()


def test_a_vote_doubled_and_surrounding_yields_both_kinds(engine_factory):
    n_val = 32
    same = {e: synth.random_committees(n_val, SPE, 11) for e in range(10)}
    v = first_member(same[0])
    p = Pair(engine_factory, n_val, 16, 16, same)
    p.ingest(*make_rows([(7, 3, 0, 0, [v]), (8, 7, 0, 0, [v])], same, n_val), 8)
    _, ev, _ = p.ingest(*make_rows([(8, 2, 0, 1, [v])], same, n_val), 8)
    assert sorted(int(k) for k in ev["kind"]) == [_abi.PE_SLASH_DOUBLE, _abi.PE_SLASH_SURROUND]
    p.check_records()


def test_window(engine_factory):
    n_val = 32
    same = {e: synth.random_committees(n_val, SPE, 13) for e in range(16)}
    v = first_member(same[0])
    p = Pair(engine_factory, n_val, 5, 16, same)          # H = 5: not a power of two
    p.ingest(*make_rows([(3, 2, 0, 0, [v])], same, n_val), 3)
    status, ev, _ = p.ingest(*make_rows([(4, 3, 0, 0, [v]), (3, 1, 0, 1, [v])], same, n_val)[:2], 3)
    assert status.tolist() == [_abi.PE_SLASH_FUTURE_TARGET, 0] and len(ev) == 1
    p.check_records()
    # a decreasing current_epoch fails and changes nothing
    recs = [p.e.slasher_records(e) for e in range(0, 4)]
    with pytest.raises(pea.EngineError) as err:
        p.e.slasher_ingest(packed=make_rows([(2, 0, 0, 3, [v])], same, n_val), current_epoch=2)
    assert err.value.status == -1
    assert p.model.ingest(*make_rows([(2, 0, 0, 3, [v])], same, n_val), 2) is None
    for (s0, i0), (s1, i1) in zip(recs, [p.e.slasher_records(e) for e in range(0, 4)]):
        assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    # TOO_OLD: 3 + 5 <= 8; the record of epoch 3 has left the window, its slot (3 mod 5) is reused by epoch 8:
    # (1, 8) would surround (2, 3) -- no evidence
    status, ev, _ = p.ingest(*make_rows([(3, 2, 0, 0, [v]), (8, 1, 0, 0, [v])], same, n_val), 8)
    assert status.tolist() == [_abi.PE_SLASH_TOO_OLD, 0] and len(ev) == 0
    p.check_records()
    src, ids = p.e.slasher_records(3)
    assert (src == NONE32).all()
    # ... while a record still inside the window does: (6, 7) inside (1, 8)
    _, ev, _ = p.ingest(*make_rows([(7, 6, 0, 0, [v])], same, n_val), 8)
    assert len(ev) == 1 and ev[0]["kind"] == _abi.PE_SLASH_SURROUND
    p.check_records()
    # a jump of more than H epochs clears everything
    _, ev, _ = p.ingest(*make_rows([(15, 0, 0, 0, [v])], same, n_val), 15)
    assert len(ev) == 0
    p.check_records()


def test_an_index_that_wraps_a_64_bit_sum_names_no_committee(engine_factory):
    """The boundary matrix's own world (tests/att_rules_cases.py: 32 slots per epoch, two committees per slot): the position
    (slot % 32) * 2 + (2^64 - 6) at slot % 32 = 3 is 2^64, not committee 0 -- the row is refused and leaves no record."""
    from types import SimpleNamespace

    from tests import att_rules_cases as C
    from tests import att_rules_model as M
    from tests.test_gpu_att_rules import _pack, wrap_rows

    w = C.world()
    sc, rows = wrap_rows(w)
    cc = C.committee_ctx(sc["time"], resident=False)
    want = [M.INDEX_RANGE if M.flat_committee(r, cc) >= C.CPS * C.SPE else M.OK for r in rows]
    assert want == [M.OK, M.INDEX_RANGE]
    epoch = rows[0]["target"][0]
    assert all(r["target"][0] == epoch for r in rows)
    comm = SimpleNamespace(offsets=np.arange(0, C.N_VAL + 1, C.SIZE, dtype=np.uint32),
                           members=np.array([v for c in w.committees[epoch] for v in c], dtype=np.uint32))
    p = Pair(engine_factory, C.N_VAL, 4, 16, {epoch: comm}, spe=C.SPE)
    status, ev, _ = p.ingest(*_pack(rows), epoch)   # (and equal to the slasher's own model)
    assert status.tolist() == want and len(ev) == 0
    p.check_records()


def test_table_full(engine_factory):
    n_val = 32
    comm = flat_comm(n_val, 4)
    p = Pair(engine_factory, n_val, 8, 2, comm)           # D = 2
    members = comm[1].members[comm[1].offsets[0]:comm[1].offsets[1]]
    votes = [(1, 0, 0, salt, [int(members[0])]) for salt in range(4)] + [(1, 0, 0, 1, [int(members[1])])]
    status, ev, _ = p.ingest(*make_rows(votes, comm, n_val), 1)
    assert status.tolist() == [0, 0, _abi.PE_SLASH_TABLE_FULL, _abi.PE_SLASH_TABLE_FULL, 0]
    assert len(ev) == 1
    p.check_records()


def test_cap_below_found(engine_factory):
    n_val = 64
    comm = flat_comm(n_val, 4)
    p = Pair(engine_factory, n_val, 8, 16, comm)
    members = [int(v) for v in comm[2].members[comm[2].offsets[1]:comm[2].offsets[2]]]
    assert len(members) >= 6
    votes = [(2, 1, 1, 0, members), (2, 1, 1, 1, members)]
    _, ev, want = p.ingest(*make_rows(votes, comm, n_val), 2, cap=3)
    assert p.e.slasher_found == len(members) == len(want) and len(ev) == 3
    p.check_records()                                      # the history is updated all the same
    _, ev, want = p.ingest(*make_rows([(2, 1, 1, 2, members)], comm, n_val), 2, cap=0)
    assert p.e.slasher_found == len(members) and len(ev) == 0


def test_ingest_before_enable_is_a_state_error(engine_factory):
    e = engine_factory(slots_per_epoch=SPE)
    e.store_init(0, 0, bytes([7]) * 32)
    e.set_validators(np.full(16, 32 * 10**9, dtype=np.uint64), np.ones(16, dtype=np.uint8))
    comm = flat_comm(16, 1)
    e.set_committees(0, comm[0].offsets, comm[0].members)
    with pytest.raises(pea.EngineError) as err:
        e.slasher_ingest(packed=make_rows([(0, 0, 0, 0, [1])], comm, 16), current_epoch=0)
    assert err.value.status == _abi.PE_ERR_STATE
    e.slasher_enable(4, 4)
    e.slasher_disable()
    with pytest.raises(pea.EngineError) as err:
        e.slasher_ingest(packed=make_rows([(0, 0, 0, 0, [1])], comm, 16), current_epoch=0)
    assert err.value.status == _abi.PE_ERR_STATE


def unaggregated_epoch(comm, epoch, parts=3, seed=5, double_from=None):
    """One epoch's attestations in `parts` partial aggregates per committee; double_from: committees whose last part
    votes for another head (their members of that part double-vote against an earlier call)."""
    tree = synth.random_tree(8, 1, "branchy")
    tree.slot[:] = np.minimum(tree.slot, epoch * SPE)
    atts, arena, _ = synth.epoch_attestations(comm, tree, epoch, SPE, seed=seed, density=0.9, parts=parts,
                                              source=(max(epoch - 1, 0), None))
    return atts, arena


def test_resident_bits_equal_host_bits(engine_factory):
    """PE_BITS_RESIDENT after a pe_aggregate of unaggregated rows = the host-bits call over the same groups."""
    n_val = 256
    comm = {e: synth.random_committees(n_val, SPE * 2, 20 + e) for e in range(4)}
    p = Pair(engine_factory, n_val, 8, 256, comm)
    a1, ar1 = unaggregated_epoch(comm[1], 1, seed=5)
    p.ingest(a1, ar1, 1)
    # epoch 1 again with other heads for some committees (double votes), and epoch 2: unaggregated, through pe_aggregate
    a2, ar2 = unaggregated_epoch(comm[1], 1, seed=6)
    agg = p.e.aggregate(packed=(a2, ar2))
    rows, out_arena = np.ascontiguousarray(agg["atts"]), np.ascontiguousarray(agg["out_arena"])
    assert agg["n_groups"] < len(a2)
    _, ev, want = p.ingest(rows, out_arena, 2, engine_packed=(rows, pea.RESIDENT))
    assert len(want) > 0
    p.check_records()


def test_inside_an_open_pipeline(engine_factory):
    """The call is synchronous: inside a pipeline it first completes the outstanding work and gives the same outputs."""
    n_val = 256
    comm = {e: synth.random_committees(n_val, SPE * 2, 30 + e) for e in range(4)}
    p = Pair(engine_factory, n_val, 8, 256, comm)
    a1, ar1 = unaggregated_epoch(comm[1], 1, seed=7)
    a2, ar2 = unaggregated_epoch(comm[1], 1, seed=8)
    p.ingest(a1, ar1, 1)
    with p.e.pipeline():
        agg = p.e.aggregate(packed=(a2, ar2))              # enqueued, not complete
        rows = agg["atts"]                                 # host-derived: complete at return
        want_status, want_ev = p.model.ingest(a2, ar2, 1)
        status, ev = p.e.slasher_ingest(packed=(a2, ar2), current_epoch=1, cap=1 << 16)
        assert status.tolist() == want_status and p.e.slasher_found == len(want_ev) > 0
        assert p.evidence_multiset(ev) == Counter(want_ev)
    assert agg["n_groups"] == len(rows)
    p.check_records()


def test_apply_equals_on_attester_slashing(engine_factory):
    """PE_SLASH_APPLY on a tree where the masked votes change the head (the K8 shape, tests/fc_scenarios.py): flags,
    per-block weights and head against (1) a twin engine that received pe_on_attester_slashing once per piece of evidence and
    (2) the oracle Store after spec.on_attester_slashing over find_attester_slashings' output."""
    worlds = []
    for _ in range(2):
        w = new_world(64, "minimal", engine_factory=engine_factory)
        anchor = w.store.justified_checkpoint.root
        w.tick_to_slot(1, offset=spec.SECONDS_PER_SLOT - 1)
        a = w.block(anchor, 1, graffiti=b"a")
        b = w.block(anchor, 1, graffiti=b"b")
        w.tick_to_slot(3)
        xs = slot_committee_members(w.store, 2)
        ys = slot_committee_members(w.store, 1)[:5]
        w.vote(xs, a, 2)
        w.vote(ys, b, 1)
        assert w.head() == a
        worlds.append((w, a, b, xs, ys))
    (w, a, b, xs, ys), (w2, _, _, _, _) = worlds
    fc, eng = w.fc, w.mirror.engine
    eng.slasher_enable(8, 64)
    first = w.attestation_for(xs, a, 2)
    assert fc.find_attester_slashings(w.mirror, first) == []
    eq = sorted(xs)[:len(xs) - 2]
    assert len(xs) - len(eq) < len(ys)
    slashings = fc.find_attester_slashings(w.mirror, w.attestation_for(eq, b, 2), apply=True)
    assert slashings and sorted(v for s in slashings for v in s.attestation_1.attesting_indices) == eq
    # (2) the oracle: every returned object passes the pyspec's handler
    for s in slashings:
        spec.on_attester_slashing(w.store, s)
    assert w.store.equivocating_indices == set(eq) == w.mirror.equivocating_indices
    assert w.head() == b
    w.check()
    # (1) the twin: pe_on_attester_slashing once per piece of evidence (one validator on both sides)
    for s in slashings:
        for v in s.attestation_1.attesting_indices:
            fc.on_attester_slashing(w2.mirror, fc.AttesterSlashing(fc.IndexedAttestation([v], s.attestation_1.data),
                                                                   fc.IndexedAttestation([v], s.attestation_2.data)))
    eng2 = w2.mirror.engine
    assert np.array_equal(eng.validator_flags(), eng2.validator_flags())
    assert (eng.validator_flags()[eq] & _abi.PE_VAL_EQUIVOCATING).all()
    assert eng.get_head() == eng2.get_head() == bytes(b)
    assert np.array_equal(eng.get_weights(), eng2.get_weights())
    # the checkpoint export sees it, and a later flag upload keeps it (as after pe_mark_equivocating)
    assert np.array_equal(eng.export_state()["flags"], eng2.export_state()["flags"])
    w.mirror.set_justified_state(w.store.checkpoint_states[w.store.justified_checkpoint])
    assert (eng.validator_flags()[eq] & _abi.PE_VAL_EQUIVOCATING).all() and eng.get_head() == bytes(b)


def test_at_size_placed_slashings_are_exactly_the_ones_found(engine_factory):
    """1 048 576 validators in 2048 committees of 512 (the configs[3] shape), H = 64, three epochs; ~1 % double voters and
    ~0.1 % surrounders placed by construction.  The validators with evidence are exactly the placed ones; on a seeded sample
    of 4096 validators plus all the placed ones the evidence equals the model's (inside the sample the comparison is exact:
    the sample bounds what is left to construction, it is not a tolerance)."""
    n_val, n_comm, spe, H = 1 << 20, 2048, 32, 64
    rng = np.random.Generator(np.random.PCG64(2024))
    epochs = (10, 11, 12)
    comm = {e: synth.random_committees(n_val, n_comm, 40 + e) for e in epochs}
    placed = rng.choice(n_val, size=n_val // 100 + n_val // 1000, replace=False)
    doublers, surrounders = placed[:n_val // 100], placed[n_val // 100:]
    sample = set(int(v) for v in rng.choice(n_val, size=4096, replace=False)) | set(int(v) for v in placed)
    p = Pair(engine_factory, n_val, H, 8192, comm, spe=spe, only=sample)
    is_d = np.zeros(n_val, dtype=bool)
    is_s = np.zeros(n_val, dtype=bool)
    is_d[doublers] = True
    is_s[surrounders] = True
    cps = n_comm // spe

    def rows_of(epoch, source, salt, pick):
        """one row per committee with the members `pick` selects (committees with none: no row)"""
        c_ = comm[epoch]
        atts, bit_rows, k = np.zeros(n_comm, dtype=synth.ATT_DTYPE), [], 0
        for c in range(n_comm):
            members = c_.members[c_.offsets[c]:c_.offsets[c + 1]]
            bits = pick(members)
            if not bits.any():
                continue
            a = atts[k]
            k += 1
            a["slot"], a["index"] = epoch * spe + c // cps, c % cps
            a["beacon_block_root"] = np.frombuffer(spec.sha256(b"head%d" % salt), dtype=np.uint8)
            a["source_epoch"], a["source_root"] = source, np.frombuffer(spec.sha256(b"src%d" % source), dtype=np.uint8)
            a["target_epoch"], a["target_root"] = epoch, np.frombuffer(spec.sha256(b"tgt%d" % epoch), dtype=np.uint8)
            a["flags"] = 1
            bit_rows.append(bits)
        atts = np.ascontiguousarray(atts[:k])
        arena, offs, nb = synth.pack_bit_rows(bit_rows)
        atts["bits_offset"], atts["n_bits"] = offs, nb
        return atts, arena

    found = set()
    for e in epochs[:2]:                                       # honest epochs: source = e - 1
        _, ev, _ = p.ingest(*rows_of(e, e - 1, 0, lambda m: np.ones(m.size, dtype=bool)), e, sample=sample)
        assert p.e.slasher_found == 0
    # epoch 12: the surrounders vote (9, 12) instead of (11, 12) -- it surrounds their (10, 11); everyone else is honest,
    # and the double voters then vote for another head as well
    e = epochs[2]
    _, ev, _ = p.ingest(*rows_of(e, e - 1, 0, lambda m: ~is_s[m]), e, sample=sample)
    assert p.e.slasher_found == 0
    _, ev, _ = p.ingest(*rows_of(e, e - 3, 0, lambda m: is_s[m]), e, sample=sample, cap=1 << 15)
    assert p.e.slasher_found == len(surrounders) and (ev["kind"] == _abi.PE_SLASH_SURROUND).all()
    found |= set(int(v) for v in ev["validator"])
    _, ev, _ = p.ingest(*rows_of(e, e - 1, 1, lambda m: is_d[m]), e, sample=sample, cap=1 << 15)
    assert p.e.slasher_found == len(doublers) and (ev["kind"] == _abi.PE_SLASH_DOUBLE).all()
    found |= set(int(v) for v in ev["validator"])
    assert found == set(int(v) for v in placed)
    p.check_records(validators=sorted(sample)[::16])
