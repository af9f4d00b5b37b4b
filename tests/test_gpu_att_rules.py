"""-m gpu: attestation validation held to the spec at every inequality's edge.  The boundary matrix of
tests/att_rules_cases.py -- whose expected values are tests/att_rules_model.py's, pinned row by row to oracle/spec.py by
tests/test_att_rules_model.py -- through every implementation of the rules:
  host        rows in host memory, synchronous calls (engine_attest.cpp)
  resident    rows in device memory (PE_ROWS_RESIDENT): k_att_validate_fc / k_att_validate_state, synchronous
  pipelined   the same inside one pipeline
  paired      a streaming step whose fork-choice kernels go out as block ranges of the next step's row kernels
              (pair_kernels.hip); the launch counters confirm that the paired form ran
Everything is compared for equality: statuses of both sides, counts, reward numerators, latest messages, both
participation arrays.  And get_indexed_attestation (A.6) beyond 2048 members, up to the kernel's 8192."""
import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from pos_evolution_amd._abi import PE_ATT_FLAG_FROM_BLOCK, PE_ATT_FLAG_SIGNATURE_VALID, PE_ERR_CAPACITY, pe_state_ctx
from tests import att_rules_cases as C
from tests import att_rules_model as M

pytestmark = pytest.mark.gpu
NONE32 = 0xFFFFFFFF
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT
ROUTES = ("host", "resident", "pipelined", "paired")
N_FILLER = 3


def _pack(rows):
    atts = np.zeros(len(rows), dtype=synth.ATT_DTYPE)
    for i, r in enumerate(rows):
        a = atts[i]
        a["slot"], a["index"] = r["slot"], r["index"]
        a["beacon_block_root"] = np.frombuffer(r["beacon_block_root"], np.uint8)
        a["source_epoch"], a["source_root"] = r["source"][0], np.frombuffer(r["source"][1], np.uint8)
        a["target_epoch"], a["target_root"] = r["target"][0], np.frombuffer(r["target"][1], np.uint8)
        a["flags"] = (PE_ATT_FLAG_SIGNATURE_VALID if r["sig_valid"] else 0) | (PE_ATT_FLAG_FROM_BLOCK if r["from_block"] else 0)
    arena, offs, nb = synth.pack_bit_rows([np.array(r["bits"], dtype=bool) for r in rows])
    atts["bits_offset"], atts["n_bits"] = offs, nb
    return atts, arena


def _engine(w, sc):
    e = pea.Engine(max_committee_tables=8)
    e.store_init(0, 0, w.R["g"])
    for name, parent, slot in w.chain[1:]:
        e.add_block(w.R[name], w.R[parent], slot)
    e.set_validators(np.array(w.balances, dtype=np.uint64), np.ones(C.N_VAL, dtype=np.uint8))
    offsets = np.arange(0, C.N_VAL + 1, C.SIZE, dtype=np.uint32)
    cur = sc["time"] // 12 // C.SPE
    for ep in sorted(C.EPOCHS, key=lambda x: x in (cur, max(cur - 1, 0))):   # the clock's two epochs last: most recently used
        e.set_committees(ep, offsets, np.array([v for c in w.committees[ep] for v in c], dtype=np.uint32))
    e.on_tick(sc["time"])
    return e


def _ctx(w, sc):
    s = sc["state"]
    ctx = pe_state_ctx()
    ctx.slot = s.slot
    ctx.chain_tip_root[:] = s.tip
    ctx.current_justified_epoch, ctx.previous_justified_epoch = s.current_justified[0], s.previous_justified[0]
    ctx.current_justified_root[:] = s.current_justified[1]
    ctx.previous_justified_root[:] = s.previous_justified[1]
    ctx.base_reward_per_increment = w.brpi
    return ctx


def _dev_rows(atts):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(atts).view(np.uint8).reshape(-1).copy()).cuda()
    return pea.DeviceRows(t.data_ptr(), len(atts), keep=t)


def _dev_arena(arena):
    import torch

    t = torch.from_numpy(arena.copy()).cuda()
    return pea.DeviceArena(t.data_ptr(), t.numel(), keep=t)


def _resident_calls(e, atts, arena, ctx, head):
    agg = e.aggregate(packed=(atts, arena), want_aggregate_pubkeys=False)
    status, _, count = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))
    if head:
        e.get_head_async()
    pst, num = e.process_attestation_batch(ctx, packed=(RR, RES), cap=len(atts))
    return agg, status, count, pst, num


def _run(e, route, batches, ctx):
    """-> per batch (status, count, pstatus, numerators), each of the batch's length (groups form in row order: every row
    of the matrix has AttestationData of its own)."""
    out = []
    if route == "host":
        for rows in batches:
            atts, arena = _pack(rows)
            agg = e.aggregate(packed=(atts, arena), want_aggregate_pubkeys=False)
            assert agg["n_groups"] == len(rows) and np.array_equal(agg["group_of"], np.arange(len(rows)))
            status, _, count = e.on_attestation_batch(packed=(agg["atts"], agg["out_arena"]))
            pst, num = e.process_attestation_batch(ctx, packed=(agg["atts"], agg["out_arena"]))
            out.append((status.copy(), count.copy(), pst.copy(), num.copy()))
        return out
    raw = []
    if route == "paired":
        e.set_pipeline_lag(2)
        e.profile_enable(True)
        e.profile_reset()
    for rows in batches:
        atts, arena = _pack(rows)
        d_rows = _dev_rows(atts)
        if route == "resident":
            raw.append(_resident_calls(e, d_rows, arena, ctx, head=False))
        elif route == "pipelined":
            with e.pipeline():
                r = _resident_calls(e, d_rows, _dev_arena(arena), ctx, head=False)
            raw.append(r)
        else:
            with e.pipeline(lagged=True):
                r = _resident_calls(e, d_rows, _dev_arena(arena), ctx, head=True)
            raw.append(r)
    if route == "paired":
        e.drain()
        ln = {k: v["launches"] for k, v in e.profile().items()}
        e.profile_enable(False)
        n = len(batches)
        # every step but the last had its validate / LMD / votes / tree launched inside the next step's row kernels
        assert all(ln[p] == n - 1 for p in ("pair_ingest_validate", "pair_plan_lmd", "pair_members_votes", "pair_union_tree")), ln
        assert ln["lmd"] == 1 and ln["votes"] == 1 and ln["tree"] == 1, ln
    for rows, (agg, status, count, pst, num) in zip(batches, raw):
        n = len(rows)
        assert int(agg["n_groups"]) == n and np.array_equal(np.asarray(agg["group_of"])[:n], np.arange(n))
        out.append((np.array(status[:n]), np.array(count[:n]), np.array(pst[:n]), np.array(num[:n])))
    return out


@pytest.fixture(scope="module")
def world():
    return C.world()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("si", range(2 + len(C.STATE_SLOTS)), ids=lambda si: C.world().scenarios[si]["name"].replace(" ", "_"))
def test_boundary_matrix_equals_the_model(world, si, route):
    w = world
    sc = w.scenarios[si]
    rows = sc["rows"]
    # the paired route needs a next step to pair with: the batch's first rows again, accepted or refused as before -- the
    # model replays that second batch too, on what the first one left behind
    batches = [rows, rows[:N_FILLER]] if route == "paired" else [rows]
    cc = C.committee_ctx(sc["time"], resident=(route != "host"))
    model = M.Run(C.N_VAL, w.increments, w.brpi)
    want = [model.batch(b, w.blocks, sc["time"] // 12, sc["state"], cc, w.members_of) for b in batches]
    e = _engine(w, sc)
    try:
        got = _run(e, route, batches, _ctx(w, sc))
        for k, (wnt, (status, count, pst, num)) in enumerate(zip(want, got)):
            tags = [f"{k}/{i} {r['tag']} (slot {r['slot']}, index {r['index']})" for i, r in enumerate(batches[k])]
            bad = [(t, int(a), b) for t, a, b in zip(tags, status, wnt["status"]) if a != b]
            assert not bad, ("on_attestation status (row, engine, model)", bad)
            bad = [(t, int(a), b) for t, a, b in zip(tags, pst, wnt["pstatus"]) if a != b]
            assert not bad, ("process_attestation status (row, engine, model)", bad)
            assert [int(x) for x in count] == wnt["count"]
            bad = [(t, int(a), b, m) for t, a, b, m in zip(tags, num, wnt["numerator"], wnt["mask"]) if a != b]
            assert not bad, ("reward numerator (row, engine, model, model's flag mask)", bad)
        assert sc["want_status"] <= {int(x) for x in got[0][0]} and sc["want_pstatus"] <= {int(x) for x in got[0][2]}
        ep, blk = e.latest_messages()
        want_ep = np.zeros(C.N_VAL, dtype=np.uint64)
        want_blk = np.full(C.N_VAL, NONE32, dtype=np.uint32)
        for v, (epoch, root) in model.latest.items():
            want_ep[v], want_blk[v] = epoch, e.block_index_of(root)
        assert model.latest, "the scenario installs votes"
        assert np.array_equal(blk, want_blk), "latest messages: blocks"
        assert np.array_equal(ep[want_blk != NONE32], want_ep[want_blk != NONE32]), "latest messages: epochs"
        assert np.array_equal(e.participation_get(0), np.array(model.part[0], dtype=np.uint8)), "current_epoch_participation"
        assert np.array_equal(e.participation_get(1), np.array(model.part[1], dtype=np.uint8)), "previous_epoch_participation"
    finally:
        e.close()


BITS_ROUTES = ("host bits", "resident bits", "device rows")


@pytest.mark.parametrize("route", BITS_ROUTES)
def test_no_bit_set_and_a_false_verdict_answers_by_route(world, route):
    """The one row the model refuses (is_valid_indexed_attestation is ONE assert, A.7; att_rules_model._indexed_status): no
    bit set AND a false signature verdict.  Host rows over bits in host memory test emptiness first; host rows over
    PE_BITS_RESIDENT and device rows (PE_ROWS_RESIDENT) ask the verdict first.  A known difference between the routes
    (DESIGN.md 7), pinned here on both sides so that no change moves it unseen; the rows beside it are accepted everywhere."""
    w = world
    sc = w.scenarios[0]
    b = C._Batch(w, sc["state"])
    b.add("valid", 59, 0, "A59", 1, "A32")
    b.add("no bit set, signature verdict false", 57, 0, "A57", 1, "A32", bits=[0] * C.SIZE, sig_valid=False)
    b.add("valid", 58, 1, "A58", 1, "A32")
    rows = b.done()
    want = M.EMPTY if route == "host bits" else M.BAD_SIGNATURE
    atts, arena = _pack(rows)
    ctx = _ctx(w, sc)
    e = _engine(w, sc)
    try:
        if route == "host bits":
            status, _, count = e.on_attestation_batch(packed=(atts, arena))
            pst, num = e.process_attestation_batch(ctx, packed=(atts, arena))
        elif route == "resident bits":
            agg = e.aggregate(packed=(atts, arena), want_aggregate_pubkeys=False)
            assert agg["n_groups"] == len(rows) and np.array_equal(agg["group_of"], np.arange(len(rows)))
            status, _, count = e.on_attestation_batch(packed=(agg["atts"], RES))
            pst, num = e.process_attestation_batch(ctx, packed=(agg["atts"], RES))
        else:
            agg, status, count, pst, num = _resident_calls(e, _dev_rows(atts), arena, ctx, head=False)
            assert int(agg["n_groups"]) == len(rows)
        assert [int(x) for x in status[:3]] == [M.OK, want, M.OK]
        assert [int(x) for x in pst[:3]] == [M.OK, want, M.OK]
        assert int(num[1]) == 0 and int(num[0]) > 0 and int(num[2]) > 0
        assert [int(x) for x in count[:3]] == [rows[0]["popcount"], 0, rows[2]["popcount"]]
    finally:
        e.close()


def wrap_rows(w):
    """-> (scenario, [a plain valid row, the row whose position wraps a 64-bit sum onto committee 0]) of state.slot 69."""
    sc = next(sc for sc in w.scenarios if sc["name"] == "state.slot 69")
    return sc, [next(r for r in sc["rows"] if r["tag"] == tag) for tag in ("valid", C.WRAP_TAG)]


def test_indexed_attestation_of_an_index_that_wraps_a_64_bit_sum(world):
    """pe_get_indexed_attestations (A.6) asks only for the position to exist: (slot % 32) * 2 + (2^64 - 6) at slot % 32 = 3
    is 2^64, not committee 0."""
    w = world
    sc, rows = wrap_rows(w)
    cc = C.committee_ctx(sc["time"], resident=False)
    want = [M.INDEX_RANGE if M.flat_committee(r, cc) >= C.CPS * C.SPE else M.OK for r in rows]
    assert want == [M.OK, M.INDEX_RANGE]
    e = _engine(w, sc)
    try:
        status, off, idx = e.get_indexed_attestations(packed=_pack(rows))
        assert [int(x) for x in status] == want
        com = w.members_of(rows[0]["target"][0], M.flat_committee(rows[0], cc))
        assert list(off) == [0, rows[0]["popcount"], rows[0]["popcount"]]
        assert [int(v) for v in idx] == sorted(v for v, b in zip(com, rows[0]["bits"]) if b)
    finally:
        e.close()


# ---------------------------------------------------------------- A.6 beyond 2048 members
@pytest.fixture(scope="module")
def big_engine():
    e = pea.Engine()
    e.store_init(0, 0, bytes(32))
    e.set_validators(synth.balances(3 * 8193, 31), np.ones(3 * 8193, dtype=np.uint8))
    yield e
    e.close()


def _one_committee(e, epoch, size, density, seed):
    """A table whose committee 0 has `size` members (a random permutation) and whose other 31 are empty."""
    rng = np.random.Generator(np.random.PCG64(seed))
    members = rng.permutation(3 * size).astype(np.uint32)[:size]
    offsets = np.full(33, size, dtype=np.uint32)
    offsets[0] = 0
    e.set_committees(epoch, offsets, members)
    bits = np.ones(size, dtype=bool) if density == 1.0 else rng.random(size) < density
    row = pea.AttRow(epoch * 32, 0, bytes(32), 0, bytes(32), epoch, bytes(32), bits.astype(np.uint8))
    return members, bits, row


@pytest.mark.parametrize("density", [1.0, 0.5])
@pytest.mark.parametrize("size", [2049, 4096, 4097, 8191, 8192])
def test_indexed_attestation_of_a_committee_beyond_2048_members(big_engine, size, density):
    """k_indexed_attestations compacts and bitonic-sorts up to 8192 members in LDS: every bit set (at 4096 and 8192 the
    count is a power of two and nothing is padded) and about half of them."""
    e = big_engine
    members, bits, row = _one_committee(e, 5, size, density, seed=size)
    status, off, idx = e.get_indexed_attestations([row])
    assert list(status) == [0] and list(off) == [0, int(bits.sum())]
    assert np.array_equal(idx, np.sort(members[bits]))


def test_a_committee_of_8193_is_refused_and_the_handle_works_on(big_engine):
    e = big_engine
    _, _, row = _one_committee(e, 6, 8193, 1.0, seed=1)
    with pytest.raises(pea.EngineError) as err:
        e.get_indexed_attestations([row])
    assert err.value.status == PE_ERR_CAPACITY
    members, bits, row = _one_committee(e, 7, 2500, 0.5, seed=2)
    status, off, idx = e.get_indexed_attestations([row])
    assert list(status) == [0] and np.array_equal(idx, np.sort(members[bits]))
