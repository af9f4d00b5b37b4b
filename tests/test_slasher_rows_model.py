"""CPU: the premise of ingesting GROUPS (pe_slasher_ingest over the resident aggregate, PE_ROWS_RESIDENT) instead of the
rows they were formed from -- in the sequential model alone (tests/slasher_model.py): over random unaggregated epochs with
planted double and surround votes, the aggregated groups find the same set of slashed VALIDATORS as the unaggregated rows.
(Aggregation changes the order in which a validator's votes of one call meet its history, so the pieces of evidence may pair
up differently; who is slashable does not depend on it.)  And the build's resource log: the kernels of the route hold no
scratch."""
import os
import re

import numpy as np
import pytest

from pos_evolution_amd import synth
from tests import slasher_model as sm
from tests.test_slasher_model import SPE, make_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def aggregate(atts, arena):
    """pe_aggregate's grouping in plain Python: rows with equal AttestationData and bit length form one group, in order of
    first appearance; its bits are the OR of the members'."""
    order, bits_of = [], {}
    for row in atts:
        key = (sm.data_bytes(row), int(row["n_bits"]))
        nb, off = int(row["n_bits"]), int(row["bits_offset"])
        bits = np.unpackbits(arena[off:off + (nb + 7) // 8], bitorder="little")[:nb].astype(bool)
        if key not in bits_of:
            order.append((key, row))
            bits_of[key] = bits
        else:
            bits_of[key] = bits_of[key] | bits
    out = np.zeros(len(order), dtype=atts.dtype)
    for g, (_, row) in enumerate(order):
        out[g] = row
    out_arena, offs, nb = synth.pack_bit_rows([bits_of[key] for key, _ in order])
    out["bits_offset"], out["n_bits"] = offs, nb
    return out, out_arena


def unaggregated_calls(seed, n_val, n_epochs, n_comm=SPE, parts=3):
    """Per epoch one call: every committee attests in `parts` partial aggregates (a partition of its voters); some parts vote
    for another head (double votes against the other parts' voters of an earlier or later call -- and inside the call when a
    voter is planted in two parts), some with a source far back (their span surrounds earlier votes)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    comm_of_epoch = {e: synth.random_committees(n_val, n_comm, seed * 100 + e) for e in range(n_epochs)}
    calls = []
    for w in range(1, n_epochs):
        votes = []
        for epoch in (w, w - 1):                       # the current epoch, and late votes for the one before
            comm = comm_of_epoch[epoch]
            for c in range(n_comm):
                members = comm.members[comm.offsets[c]:comm.offsets[c + 1]]
                part_of = rng.integers(0, parts, size=members.size)
                for p in range(parts):
                    voters = [int(v) for v in members[part_of == p]]
                    if not voters or (epoch != w and rng.random() < 0.7):
                        continue
                    kind = rng.random()
                    source, salt = max(epoch - 1, 0), 0
                    if kind < 0.15:
                        salt = int(rng.integers(1, 3))                      # another head
                        if rng.random() < 0.5:
                            voters.append(int(members[int(rng.integers(0, members.size))]))   # ... also from another part
                    elif kind < 0.25:
                        source = int(rng.integers(0, epoch + 1))            # another span: may surround
                    votes.append((epoch, source, c, salt, sorted(set(voters))))
        calls.append((w, [votes[i] for i in rng.permutation(len(votes))]))
    return comm_of_epoch, calls


@pytest.mark.parametrize("seed", range(6))
def test_groups_find_the_same_slashed_validators_as_their_rows(seed):
    n_val, n_epochs = 64, 8
    comm_of_epoch, calls = unaggregated_calls(seed, n_val, n_epochs)
    models = [sm.SlasherModel(n_val, history=n_epochs + 2, max_data=1 << 20, slots_per_epoch=SPE) for _ in range(2)]
    for m in models:
        for e, comm in comm_of_epoch.items():
            m.set_committees(e, comm.offsets, comm.members)
    slashed = [set(), set()]
    kinds = set()
    fewer = False
    for w, votes in calls:
        atts, arena = make_rows(votes, comm_of_epoch, n_val)
        groups, out_arena = aggregate(atts, arena)
        fewer |= len(groups) < len(atts)
        for k, (rows, bits) in enumerate(((atts, arena), (groups, out_arena))):
            status, evidence = models[k].ingest(rows, bits, w)
            assert status == [0] * len(rows)
            slashed[k] |= models[k].slashed(evidence)
            kinds |= {ev[1] for ev in evidence}
        assert slashed[0] == slashed[1], w
    assert slashed[0] and kinds == {sm.DOUBLE, sm.SURROUND} and fewer


def test_the_python_aggregate_is_the_union_per_data():
    comm = {1: synth.random_committees(16, SPE, 3)}
    members = [int(v) for v in comm[1].members[comm[1].offsets[0]:comm[1].offsets[1]]]
    assert len(members) >= 2
    atts, arena = make_rows([(1, 0, 0, 0, members[:1]), (1, 0, 0, 1, members), (1, 0, 0, 0, members[1:])], comm, 16)
    groups, out_arena = aggregate(atts, arena)
    assert len(groups) == 2 and sm.data_bytes(groups[0]) == sm.data_bytes(atts[0])
    nb = int(groups[0]["n_bits"])
    bits = np.unpackbits(out_arena[int(groups[0]["bits_offset"]):][:(nb + 7) // 8], bitorder="little")[:nb]
    assert bits.all() and nb == len(members)


def test_row_kernels_are_built_without_scratch():
    """The library's build writes the compiler's resource usage of slash_kernels.hip: none of the kernels that form the scan's
    rows, ids and lists may spill, and only the two single-workgroup scans hold LDS (one word per wave)."""
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "slash_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("the library has not been built here (make writes the log)")
    blocks = {b.split()[0]: b for b in re.split(r"remark: [^\n]*Function Name: ", open(log).read())[1:]}
    names = ["k_slash_rows_check", "k_slash_rows_lookup", "k_slash_rows_ids", "k_slash_rows_emit", "k_slash_lists_count",
             "k_slash_lists_scan", "k_slash_lists_fill", "k_slash_lists_sort", "k_slash_table_build"]
    for name in names:
        blk = [b for k, b in blocks.items() if name in k]
        assert len(blk) == 1, name
        assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk[0]).group(1) == "0", name
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk[0]).group(1))
        assert lds == (16 if name in ("k_slash_rows_ids", "k_slash_lists_scan") else 0), name
