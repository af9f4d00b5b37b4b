"""CPU: the sequential slasher model (tests/slasher_model.py) against the reference's is_slashable_attestation_data
(pe:1134-1143) applied to ALL pairs of votes.  The model keeps one record per validator and target epoch, so it does not
find every slashable pair -- but while the history spans fewer than H epochs it finds every slashable VALIDATOR."""
import numpy as np
import pytest

from oracle import spec
from pos_evolution_amd import synth
from tests import slasher_model as sm

SPE = 8


def make_rows(votes, comm_of_epoch, n_val):
    """votes: list of (target epoch, source epoch, committee id, salt, voters) -> (ATT_DTYPE rows, arena)."""
    atts = np.zeros(len(votes), dtype=synth.ATT_DTYPE)
    bit_rows = []
    for k, (epoch, source, c, salt, voters) in enumerate(votes):
        comm = comm_of_epoch[epoch]
        cps = (comm.offsets.size - 1) // SPE
        members = comm.members[comm.offsets[c]:comm.offsets[c + 1]]
        a = atts[k]
        a["slot"], a["index"] = epoch * SPE + c // cps, c % cps
        a["beacon_block_root"] = np.frombuffer(spec.sha256(b"head%d" % salt), dtype=np.uint8)
        a["source_epoch"], a["source_root"] = source, np.frombuffer(spec.sha256(b"src%d" % source), dtype=np.uint8)
        a["target_epoch"], a["target_root"] = epoch, np.frombuffer(spec.sha256(b"tgt%d" % epoch), dtype=np.uint8)
        a["flags"] = 1
        bit_rows.append(np.isin(members, np.asarray(sorted(voters), dtype=np.uint32)))
    arena, offs, nb = synth.pack_bit_rows(bit_rows)
    atts["bits_offset"], atts["n_bits"] = offs, nb
    return atts, arena


def random_history(seed, n_val=48, n_epochs=10, n_comm=SPE):
    """Calls of random votes over n_epochs epochs: honest votes (source = epoch - 1, one head), double votes (another
    head for the same committee) and surround votes (sources far back or far ahead) injected."""
    rng = np.random.Generator(np.random.PCG64(seed))
    comm_of_epoch = {e: synth.random_committees(n_val, n_comm, seed * 100 + e) for e in range(n_epochs)}
    calls = []
    for w in range(n_epochs):
        for _ in range(int(rng.integers(1, 4))):
            votes = []
            for _ in range(int(rng.integers(1, 6))):
                epoch = int(rng.integers(max(0, w - 3), w + 1))
                c = int(rng.integers(0, n_comm))
                comm = comm_of_epoch[epoch]
                members = comm.members[comm.offsets[c]:comm.offsets[c + 1]]
                voters = members[rng.random(members.size) < 0.6]
                kind = rng.random()
                if kind < 0.6:
                    source, salt = max(epoch - 1, 0), 0
                elif kind < 0.8:
                    source, salt = max(epoch - 1, 0), int(rng.integers(1, 3))       # another head: a double vote
                else:
                    source, salt = int(rng.integers(0, epoch + 1)), 0               # another span: may surround
                votes.append((epoch, source, c, salt, [int(v) for v in voters]))
            calls.append((w, votes))
    return comm_of_epoch, calls


def all_pairs_slashable(votes_of, n_val):
    out = set()
    for v in range(n_val):
        ds = votes_of[v]
        if any(spec.is_slashable_attestation_data(ds[i], ds[j]) for i in range(len(ds)) for j in range(len(ds)) if i != j):
            out.add(v)
    return out


@pytest.mark.parametrize("seed", range(12))
def test_model_finds_every_slashable_validator(seed):
    n_val, n_epochs = 48, 10
    comm_of_epoch, calls = random_history(seed, n_val, n_epochs)
    model = sm.SlasherModel(n_val, history=n_epochs + 2, max_data=1 << 20, slots_per_epoch=SPE)
    for e, comm in comm_of_epoch.items():
        model.set_committees(e, comm.offsets, comm.members)
    votes_of = [[] for _ in range(n_val)]
    found = set()
    n_kinds = {sm.DOUBLE: 0, sm.SURROUND: 0}
    for w, votes in calls:
        atts, arena = make_rows(votes, comm_of_epoch, n_val)
        status, evidence = model.ingest(atts, arena, w)
        assert status == [0] * len(votes)
        for k, (_, _, _, _, voters) in enumerate(votes):
            for v in voters:
                votes_of[v].append(sm.data_of(atts[k]))
        by_bytes = {sm.data_bytes(r): sm.data_of(r) for r in atts}
        for v, kind, b1, b2 in evidence:
            n_kinds[kind] += 1
            # the stated argument order satisfies the reference's function
            d1 = by_bytes.get(b1) or next(d for d, b in model.records[v].values() if b == b1)
            d2 = by_bytes.get(b2) or next(d for d, b in model.records[v].values() if b == b2)
            assert spec.is_slashable_attestation_data(d1, d2)
            assert (kind == sm.DOUBLE) == (d1.target.epoch == d2.target.epoch)
            if kind == sm.SURROUND:
                assert d1.source.epoch < d2.source.epoch and d2.target.epoch < d1.target.epoch
        found |= model.slashed(evidence)
    assert found == all_pairs_slashable(votes_of, n_val)
    assert found, "the scenario injected nothing"
    assert n_kinds[sm.DOUBLE] and n_kinds[sm.SURROUND]


def _one(model, comm, epoch, source, salt, voters, w):
    atts, arena = make_rows([(epoch, source, 0, salt, voters)], {epoch: comm}, model.n_val)
    return model.ingest(atts, arena, w), atts


def test_the_two_casper_conditions_by_hand():
    """pe:1128: no two votes with the same target epoch; no vote whose span (source, target) surrounds another's."""
    n_val = 8
    comm = synth.random_committees(n_val, SPE, 1)
    v = int(comm.members[comm.offsets[0]])
    model = sm.SlasherModel(n_val, history=16, max_data=16, slots_per_epoch=SPE)
    for e in range(10):
        model.set_committees(e, comm.offsets, comm.members)
    # h(t1) == h(t2): two different votes for target epoch 5
    (st, ev), a1 = _one(model, comm, 5, 4, 0, [v], 5)
    assert st == [0] and ev == []
    (st, ev), a2 = _one(model, comm, 5, 4, 1, [v], 5)
    assert ev == [(v, sm.DOUBLE, sm.data_bytes(a1[0]), sm.data_bytes(a2[0]))]
    (st, ev), _ = _one(model, comm, 5, 4, 0, [v], 5)                 # the recorded vote again: nothing
    assert ev == []
    # h(s1) < h(s2) < h(t2) < h(t1): (2, 8) surrounds (3, 7), whichever arrives first
    model1 = sm.SlasherModel(n_val, history=16, max_data=16, slots_per_epoch=SPE)
    for e in range(10):
        model1.set_committees(e, comm.offsets, comm.members)
    (st, ev), inner = _one(model1, comm, 7, 3, 0, [v], 8)
    assert ev == []
    (st, ev), outer = _one(model1, comm, 8, 2, 0, [v], 8)
    assert ev == [(v, sm.SURROUND, sm.data_bytes(outer[0]), sm.data_bytes(inner[0]))]
    model2 = sm.SlasherModel(n_val, history=16, max_data=16, slots_per_epoch=SPE)
    for e in range(10):
        model2.set_committees(e, comm.offsets, comm.members)
    (st, ev), outer = _one(model2, comm, 8, 2, 0, [v], 8)
    (st, ev), inner = _one(model2, comm, 7, 3, 0, [v], 8)
    assert ev == [(v, sm.SURROUND, sm.data_bytes(outer[0]), sm.data_bytes(inner[0]))]
    # equal sources or equal targets are not a surround
    (st, ev), _ = _one(model2, comm, 6, 2, 0, [v], 8)
    assert ev == []


def test_window_and_statuses():
    n_val = 8
    comm = synth.random_committees(n_val, SPE, 2)
    v = int(comm.members[comm.offsets[0]])
    model = sm.SlasherModel(n_val, history=5, max_data=1, slots_per_epoch=SPE)
    for e in range(20):
        model.set_committees(e, comm.offsets, comm.members)
    (st, ev), _ = _one(model, comm, 3, 2, 0, [v], 3)
    (st, ev), _ = _one(model, comm, 4, 3, 0, [v], 3)
    assert st == [sm.FUTURE_TARGET]
    (st, ev), _ = _one(model, comm, 3, 2, 1, [v], 3)
    assert st == [sm.TABLE_FULL] and ev == []
    assert model.ingest(*make_rows([], {}, n_val), 2) is None     # the epoch may not decrease
    (st, ev), _ = _one(model, comm, 3, 2, 0, [v], 8)                # 3 + 5 <= 8
    assert st == [sm.TOO_OLD]
    assert model.records_of(3)[v] == (None, None)
    (st, ev), _ = _one(model, comm, 8, 1, 0, [v], 8)                # would surround (2, 3), which has left the window
    assert st == [0] and ev == []
