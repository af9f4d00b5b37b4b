"""-m gpu: pe_slasher_ingest over rows in device memory -- (PE_ROWS_RESIDENT, PE_BITS_RESIDENT): the groups of the last
pe_aggregate over DeviceRows, judged, given their AttestationData ids and turned into the scan's rows and lists on the device
(slash_kernels.hip: k_slash_rows_*, k_slash_lists_*).

The specification is the sequential model (tests/slasher_model.py) fed the aggregate's out_atts / out_arena; the model's
per-epoch tables are in order of first appearance, so the ids THEMSELVES are held to it: slasher_data(epoch, i) must be the
model's i-th data.  Where a twin handle is named it takes the host-row route (out_atts with PE_BITS_RESIDENT) over the same
calls, and raw evidence (ids included), records and data bytes must be equal."""
from collections import Counter

import numpy as np
import pytest

import pos_evolution_amd as pea
from pos_evolution_amd import _abi, synth
from tests import slasher_model as sm
from tests.test_gpu_slasher import NONE32, Pair, first_member, unaggregated_epoch
from tests.test_slasher_model import SPE, make_rows

pytestmark = pytest.mark.gpu
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT
INVALID_ARG = -1   # PE_ERR_INVALID_ARG (include/posevo.h)


def _dev_rows(atts):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(atts).view(np.uint8).reshape(-1).copy()).cuda()
    return pea.DeviceRows(t.data_ptr(), len(atts), keep=t)


def _engine(engine_factory, n_val):
    e = engine_factory(slots_per_epoch=SPE, max_committee_tables=16)
    e.store_init(0, 0, bytes([7]) * 32)
    e.set_validators(np.full(n_val, 32 * 10**9, dtype=np.uint64), np.ones(n_val, dtype=np.uint8))
    return e


def _concat(*batches):
    """(atts, arena) batches -> one batch: the bit offsets of the later ones move behind the earlier arenas"""
    atts, arenas, at = [], [], 0
    for a, ar in batches:
        a = a.copy()
        a["bits_offset"] += at
        at += len(ar)
        atts.append(a)
        arenas.append(ar)
    return np.ascontiguousarray(np.concatenate(atts)), np.ascontiguousarray(np.concatenate(arenas))


def slash_data_hash(data128: bytes) -> int:
    """The twin of slash_kernels.hip's slash_data_hash: the 32 little-endian words folded in order."""
    h = 0x85EBCA6B
    for w in np.frombuffer(data128, dtype="<u4"):
        h ^= int(w)
        h = (h * 0x9E3779B1) & 0xFFFFFFFF
        h ^= h >> 15
    return h


class Rows:
    """One handle on the device-row route with its model, optionally a twin handle on the host-row route; both are fed
    the same calls and compared after each."""

    def __init__(self, engine_factory, n_val, history, max_data, comm, twin=True):
        self.comm = dict(comm)
        self.p = Pair(None, n_val, history, max_data, comm, engine=_engine(engine_factory, n_val))
        self.t = Pair(None, n_val, history, max_data, comm, engine=_engine(engine_factory, n_val)) if twin else None
        self.e, self.model = self.p.e, self.p.model
        self.epoch = 0

    def engines(self):
        return [self.e] + ([self.t.e] if self.t else [])

    def tick(self, epoch):
        """the store's clock into `epoch`: the resident mode resolves against the tables of it and of the one before"""
        self.epoch = epoch
        for e in self.engines():
            e.on_tick((epoch * SPE + SPE - 1) * int(e.cfg.seconds_per_slot))

    def aggregate(self, e, atts, arena, device):
        keep = _dev_rows(atts) if device else None
        agg = e.aggregate(packed=(keep, arena) if device else (atts, arena))
        return agg, np.ascontiguousarray(agg["atts"]), np.ascontiguousarray(agg["out_arena"]), keep

    def ingest(self, atts, arena, w, route="dev", cap=1 << 16, apply=False, slack=3):
        """-> (status, evidence, the model's evidence, the groups)"""
        if route == "dev":   # the model knows the tables the resident mode resolves: the clock's epoch and the one before
            self.model.committees = {}
            for ep in (self.epoch, self.epoch - 1):
                if ep in self.comm:
                    self.model.set_committees(ep, self.comm[ep].offsets, self.comm[ep].members)
        else:
            for ep, c in self.comm.items():
                self.model.set_committees(ep, c.offsets, c.members)
        agg, rows, out_arena, keep = self.aggregate(self.e, atts, arena, route == "dev")
        ng = agg["n_groups"]
        assert ng == len(rows)
        want_status, want_ev = self.model.ingest(rows, out_arena, w)
        if route == "dev":
            status, ev = self.e.slasher_ingest(packed=(RR, RES), cap_rows=len(atts) + slack, current_epoch=w, cap=cap, apply=apply)
            assert len(status) == len(atts) + slack and not status[ng:].any()
        else:
            status, ev = self.e.slasher_ingest(packed=(rows, RES), current_epoch=w, cap=cap, apply=apply)
        del keep
        assert status[:ng].tolist() == want_status
        assert self.e.slasher_found == len(want_ev)
        assert self.p.evidence_multiset(ev) == Counter(want_ev)
        self.p.check_records()
        self.check_ids()
        if self.t is not None:
            _, rows_t, _, _ = self.aggregate(self.t.e, atts, arena, False)
            assert np.array_equal(rows_t, rows)
            status_t, ev_t = self.t.e.slasher_ingest(packed=(rows_t, RES), current_epoch=w, cap=cap, apply=apply)
            assert status_t.tolist() == status[:ng].tolist()
            assert sorted(map(tuple, ev_t.tolist())) == sorted(map(tuple, ev.tolist())), "raw evidence: the ids themselves"
            self.check_twin()
        return status[:ng], ev, want_ev, rows

    def check_ids(self, e=None):
        """slasher_data(epoch, i) is the i-th data of the epoch in order of first appearance, and there is no further one"""
        e = e or self.e
        for epoch, table in self.model.tables.items():
            for i, b in enumerate(table):
                assert e.slasher_data(epoch, i).tobytes()[:128] == b, (epoch, i)
            with pytest.raises(pea.EngineError):
                e.slasher_data(epoch, len(table))

    def check_twin(self):
        w = self.model.W
        for epoch in range(max(0, w - self.p.H + 1), w + 1):
            (s0, i0), (s1, i1) = self.e.slasher_records(epoch), self.t.e.slasher_records(epoch)
            assert np.array_equal(s0, s1) and np.array_equal(i0, i1), epoch
        self.check_ids(self.t.e)


def _epoch(comm, epoch, seed, source, parts=3):
    """tests.test_gpu_slasher.unaggregated_epoch with a source epoch of the caller's choosing"""
    tree = synth.random_tree(8, 1, "branchy")
    tree.slot[:] = np.minimum(tree.slot, epoch * SPE)
    atts, arena, _ = synth.epoch_attestations(comm, tree, epoch, SPE, seed=seed, density=0.9, parts=parts, source=(source, None))
    return atts, arena


def test_equals_the_host_row_route(engine_factory):
    """Unaggregated epochs through DeviceRows -> aggregate -> (ROWS_RESIDENT, RESIDENT) against the twin on out_atts: epoch 1;
    epoch 1 again with other heads (double votes) beside epoch 2 in ONE batch (two epoch slots in a call); then epoch 3 with
    source 0, which surrounds the (1, 2) votes of the call before (two epochs hold no surround: s1 < s2 < t2 < t1)."""
    n_val = 256
    comm = {e: synth.random_committees(n_val, SPE * 2, 20 + e) for e in range(5)}
    r = Rows(engine_factory, n_val, 8, 256, comm)
    r.tick(1)
    a1 = unaggregated_epoch(comm[1], 1, seed=5)
    _, ev, _, rows = r.ingest(*a1, 1)
    assert len(rows) < len(a1[0]) and len(ev) == 0
    r.tick(2)
    batch = _concat(unaggregated_epoch(comm[1], 1, seed=6), unaggregated_epoch(comm[2], 2, seed=7))
    _, ev, _, rows = r.ingest(*batch, 2)
    assert set(rows["target_epoch"].tolist()) == {1, 2}
    kinds = Counter(int(k) for k in ev["kind"])
    assert kinds[_abi.PE_SLASH_DOUBLE] > 0
    r.tick(3)
    _, ev, _, _ = r.ingest(*_epoch(comm[3], 3, seed=8, source=0), 3)
    kinds.update(int(k) for k in ev["kind"])
    assert kinds[_abi.PE_SLASH_SURROUND] > 0


def test_ids_are_first_appearance_order_across_tiles(engine_factory):
    """2048 groups in one aggregate -- eight tiles of the id pass, eight workgroups of the others -- over two epoch slots
    in shuffled order; half of their data is already in the slots from an earlier call.  The ids equal the twin's and the
    model's order of first appearance."""
    n_val, n_comm = 2048, 1024
    comm = {e: synth.random_committees(n_val, n_comm, 50 + e) for e in (1, 2)}
    r = Rows(engine_factory, n_val, 4, 1500, comm)
    rng = np.random.Generator(np.random.PCG64(17))

    def votes(epoch, cs):
        out = []
        for c in cs:
            members = comm[epoch].members[comm[epoch].offsets[c]:comm[epoch].offsets[c + 1]]
            out.append((epoch, epoch - 1, int(c), 0, [int(v) for v in members[:1 + int(c) % 2]]))
        return out

    r.tick(2)
    first = votes(2, range(0, n_comm, 2)) + votes(1, range(1, n_comm, 2))
    r.ingest(*make_rows([first[i] for i in rng.permutation(len(first))], comm, n_val), 2)
    both = votes(2, range(n_comm)) + votes(1, range(n_comm))
    both = [both[i] for i in rng.permutation(len(both))]
    _, ev, _, rows = r.ingest(*make_rows(both, comm, n_val), 2)
    assert len(rows) == 2048 >= 1100 and len(ev) == 0
    assert len(r.model.tables[1]) == len(r.model.tables[2]) == n_comm


def test_table_full(engine_factory):
    """D = 4 and a slot that holds 3: of 3 new data and 1 known one, the known one and the first new one get ids, the other
    two read TABLE_FULL -- with every group that carries their data; a later call finds the slot at 4.  Equal data in two
    groups (they differ in the bit length) share one id, or are full together."""
    n_val = 64
    comm = {e: synth.random_committees(n_val, SPE, 60 + e) for e in (0, 1)}
    r = Rows(engine_factory, n_val, 4, 4, comm)
    r.tick(1)
    v = [first_member(comm[1], c) for c in range(SPE)]
    r.ingest(*make_rows([(1, 0, 0, salt, [v[0]]) for salt in range(3)], comm, n_val), 1)
    votes = [(1, 0, 1, 3, [v[1]]), (1, 0, 1, 3, [v[1]]), (1, 0, 0, 1, [v[0]]), (1, 0, 2, 4, [v[2]]), (1, 0, 2, 4, [v[2]]),
             (1, 0, 3, 5, [v[3]])]
    atts, arena = make_rows(votes, comm, n_val)
    # rows 1 and 4: the data of rows 0 and 3 with eight more bits than the committee has -- groups of their own
    longer = []
    for k in (1, 4):
        size = int(atts[k]["n_bits"])
        bits = np.unpackbits(arena[int(atts[k]["bits_offset"]):][:(size + 7) // 8], bitorder="little")[:size].astype(bool)
        longer.append(np.concatenate([bits, np.zeros(8, dtype=bool)]))
    extra, offs, nb = synth.pack_bit_rows(longer)
    atts["bits_offset"][[1, 4]] = offs + len(arena)
    atts["n_bits"][[1, 4]] = nb
    arena = np.concatenate([arena, extra])
    full = _abi.PE_SLASH_TABLE_FULL
    status, _, _, rows = r.ingest(atts, arena, 1)
    assert len(rows) == 6 and status.tolist() == [0, 0, 0, full, full, full]
    status, _, _, _ = r.ingest(*make_rows([(1, 0, 4, 6, [v[4]]), (1, 0, 1, 3, [v[1]])], comm, n_val), 1)
    assert status.tolist() == [full, 0] and len(r.model.tables[1]) == 4


def test_hash_collisions(engine_factory):
    """D = 8, so 16 table entries: eight data whose keys meet in ONE entry under the kernel's hash (picked by running its
    twin over candidate heads) resolve to eight ids and back; then again as known data."""
    n_val = 64
    comm = {e: synth.random_committees(n_val, SPE, 70 + e) for e in (0, 1)}
    v = first_member(comm[1], 0)
    picked, salt = [], 0
    while len(picked) < 8:
        atts, _ = make_rows([(1, 0, 0, salt, [v])], comm, n_val)
        if slash_data_hash(sm.data_bytes(atts[0])) & 15 == 5:
            picked.append(salt)
        salt += 1
    r = Rows(engine_factory, n_val, 4, 8, comm)
    r.tick(1)
    votes = [(1, 0, 0, s, [v]) for s in picked]
    status, ev, _, _ = r.ingest(*make_rows(votes, comm, n_val), 1)
    assert status.tolist() == [0] * 8 and len(ev) == 7 and len(r.model.tables[1]) == 8
    status, ev, _, _ = r.ingest(*make_rows(votes[::-1], comm, n_val), 1)
    assert status.tolist() == [0] * 8


def test_window(engine_factory):
    """H = 3: slots are reused as current_epoch advances by one and by more than H; the window statuses come before a
    missing table; a target inside the window but older than the store's previous epoch has no table in this mode."""
    n_val = 32
    same = synth.random_committees(n_val, SPE, 13)
    comm = {e: same for e in range(16)}
    v = first_member(same, 0)
    r = Rows(engine_factory, n_val, 3, 16, comm, twin=False)
    for epoch in (3, 4, 5):   # by one: epoch 5 takes the slot of epoch 2 (empty), epoch 6 below that of epoch 3
        r.tick(epoch)
        status, ev, _, _ = r.ingest(*make_rows([(epoch, epoch - 1, 0, 0, [v]), (epoch - 1, epoch - 2, 0, 0, [v])], comm, n_val), epoch)
        assert status.tolist() == [0, 0] and len(ev) == 0
    r.tick(6)
    votes = [(6, 2, 0, 0, [v]),      # surrounds (3, 4) and (4, 5); (2, 3) has left the window
             (7, 6, 0, 0, [v]),      # future: before "no table" (epoch 7 is neither current nor previous)
             (3, 2, 0, 1, [v]),      # 3 + 3 <= 6: too old, before "no table"
             (4, 3, 0, 1, [v])]      # inside the window, older than the previous epoch: no table in this mode
    status, ev, _, _ = r.ingest(*make_rows(votes, comm, n_val), 6)
    assert status.tolist() == [0, _abi.PE_SLASH_FUTURE_TARGET, _abi.PE_SLASH_TOO_OLD, sm.NO_COMMITTEE_TABLE]
    assert sorted(int(k) for k in ev["kind"]) == [_abi.PE_SLASH_SURROUND] * 2
    assert (r.e.slasher_records(3)[0] == NONE32).all()
    r.tick(12)                       # by more than H: every slot is cleared; (0, 12) finds nothing to surround
    status, ev, _, _ = r.ingest(*make_rows([(12, 0, 0, 0, [v])], comm, n_val), 12)
    assert status.tolist() == [0] and len(ev) == 0 and list(r.model.tables) == [12]


def test_mixed_routes_continue_one_sequence_of_ids(engine_factory):
    """Host rows, device rows, host rows again, device rows again on ONE handle against a twin on host rows throughout;
    slasher_data answers after every switch (check_ids in every step), new and known data on either side of each."""
    n_val = 64
    comm = {e: synth.random_committees(n_val, SPE, 80 + e) for e in (0, 1, 2)}
    r = Rows(engine_factory, n_val, 4, 32, comm)
    r.tick(2)
    v = {e: [first_member(comm[e], c) for c in range(SPE)] for e in (1, 2)}

    def call(salts, cs):
        return make_rows([(e, e - 1, c, s, [v[e][c]]) for e in (2, 1) for c in cs for s in salts], comm, n_val)

    found = 0
    for route, salts, cs in (("host", (0,), (0, 1, 2)), ("dev", (0, 1), (1, 2, 3)), ("host", (1, 2), (0, 3, 4)),
                             ("dev", (0, 2, 3), (0, 4, 5)), ("dev", (3,), (5, 6))):
        _, ev, _, _ = r.ingest(*call(salts, cs), 2, route=route)
        found += len(ev)
    assert found > 0 and len(r.model.tables[1]) == len(r.model.tables[2]) > 12


def test_a_failing_call_changes_nothing(engine_factory):
    n_val = 64
    comm = {e: synth.random_committees(n_val, SPE, 90 + e) for e in (0, 1, 2, 3)}
    r = Rows(engine_factory, n_val, 4, 32, comm)
    v = [first_member(comm[1], c) for c in range(SPE)]
    fresh = _engine(engine_factory, n_val)
    fresh.slasher_enable(4, 32)
    with pytest.raises(pea.EngineError) as err:    # no aggregate over device rows on the handle
        fresh.slasher_ingest(packed=(RR, RES), cap_rows=4, current_epoch=1)
    assert err.value.status == _abi.PE_ERR_STATE
    r.tick(1)
    r.ingest(*make_rows([(1, 0, c, 0, [v[c]]) for c in range(3)], comm, n_val), 1)

    def refused(want, **kw):
        with pytest.raises(pea.EngineError) as err:
            r.e.slasher_ingest(**kw)
        assert err.value.status == want
        r.p.check_records()
        r.check_ids()
        r.check_twin()

    atts, arena = make_rows([(1, 0, c, 1, [v[c]]) for c in range(4)], comm, n_val)
    keep = _dev_rows(atts)
    r.e.aggregate(packed=(keep, arena))
    refused(_abi.PE_ERR_CAPACITY, packed=(RR, RES), cap_rows=3, current_epoch=1)
    refused(INVALID_ARG, packed=(RR, arena), cap_rows=4, current_epoch=1)
    refused(INVALID_ARG, packed=(RR, RES), cap_rows=4, current_epoch=0)   # a smaller current_epoch, as today
    # a source epoch that does not fit 32 bits fails the whole call
    bad = atts.copy()
    bad["source_epoch"][2] = 2**32 - 1
    keep = _dev_rows(bad)
    r.e.aggregate(packed=(keep, arena))
    refused(INVALID_ARG, packed=(RR, RES), cap_rows=4, current_epoch=1)
    # the clock moves into another epoch between aggregate and ingest
    keep = _dev_rows(atts)
    r.e.aggregate(packed=(keep, arena))
    r.tick(2)
    refused(_abi.PE_ERR_STATE, packed=(RR, RES), cap_rows=4, current_epoch=1)
    # ... and the handle goes on as if none of it had happened
    status, ev, _, _ = r.ingest(atts, arena, 2)
    assert status.tolist() == [0] * 4 and len(ev) == 3


def test_apply_marks_the_equivocating_validators(engine_factory):
    """PE_SLASH_APPLY over device rows: the validator flags and the next head equal the twin's."""
    n_val = 64
    comm = {e: synth.random_committees(n_val, SPE, 100 + e) for e in (0, 1)}
    r = Rows(engine_factory, n_val, 4, 32, comm)
    r.tick(1)
    members = [int(x) for x in comm[1].members[comm[1].offsets[0]:comm[1].offsets[1]]]
    r.ingest(*make_rows([(1, 0, 0, 0, members)], comm, n_val), 1, apply=True)
    _, ev, _, _ = r.ingest(*make_rows([(1, 0, 0, 1, members[:3])], comm, n_val), 1, apply=True)
    assert len(ev) == 3
    fl, fl_t = r.e.validator_flags(), r.t.e.validator_flags()
    assert np.array_equal(fl, fl_t)
    assert sorted(np.nonzero(fl & _abi.PE_VAL_EQUIVOCATING)[0].tolist()) == sorted(members[:3])
    assert r.e.get_head() == r.t.e.get_head()


def test_more_new_votes_of_one_validator_than_a_pass_holds(engine_factory):
    """Six different data for one committee in one batch, one validator in all of them (a partition admits no other way
    into six groups): more than SLASH_NV new votes reach the unchanged scan through device-built rows and lists."""
    n_val = 32
    comm = {e: synth.random_committees(n_val, SPE, 110 + e) for e in (0, 1, 2)}
    r = Rows(engine_factory, n_val, 8, 64, comm)
    r.tick(2)
    v, u = first_member(comm[2], 0), first_member(comm[1], 0)
    votes = [(2, 1, 0, salt, [v]) for salt in range(6)] + [(1, 0, 0, salt, [u]) for salt in range(5)]
    votes = [votes[i] for i in (0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5)]
    _, ev, want, _ = r.ingest(*make_rows(votes, comm, n_val), 2)
    assert len(want) >= 9
    r.ingest(*make_rows(votes[::-1], comm, n_val), 2)
