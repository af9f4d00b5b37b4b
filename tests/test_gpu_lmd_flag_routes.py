"""-m gpu: update_latest_messages (pe:1435-1441) and the flag loop of process_attestation (pe:745-749) held to the spec
where the order of rows inside one batch decides the outcome, on every route the engine has for them.  The batches are
tests/lmd_flag_cases.py's; the expected values are tests/att_rules_model.py's, which tests/test_att_rules_model.py pins to
oracle/spec.py on the same batches.  Everything is compared for equality: the epoch, block and (on an engine with vote
expiry) slot of every latest message, both participation arrays, every row's statuses, count and reward numerator.

  host-atomic           host rows, partition tables, a registry so large that 8 x (bits of a table's rows) < validators:
                        k_lmd<0> / k_lmd<1>, the atomicMax on (epoch + 1, 0xFFFFFFFE - order) and its settled key
  host-validator-major  the same rows plus full rows of filler committees, so that 8 x bits >= validators:
                        k_lmd_validator_major
  host-overlapping      a table in which the special validators sit in two committees: no partition, so the atomic LMD
                        kernels and one flag round per row
  resident, pipelined, paired   rows in device memory, as tests/test_gpu_att_rules.py drives them: lmd_vm_tables_body and
                        launch_participation_tables; the paired form is confirmed by the launch counters
The flag pass of the three host routes is k_participation, one launch per (round, table)."""
import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from pos_evolution_amd._abi import PE_ATT_FLAG_SIGNATURE_VALID
from pos_evolution_amd.engine import _ptr
from tests import att_rules_model as M
from tests import lmd_flag_cases as L
from tests import test_gpu_att_rules as TA

pytestmark = pytest.mark.gpu
NONE32 = 0xFFFFFFFF
HOST_ROUTES = ("host-atomic", "host-validator-major", "host-overlapping")
RESIDENT_ROUTES = ("resident", "pipelined", "paired")
ROUTES = HOST_ROUTES + RESIDENT_ROUTES
EXPIRY = 200


def _world(route, hot, n_val=4096):
    # 8 x 712 bits (five rows of 65 and three of 129 members on one table) must stay below the registry's size
    return L.world(hot, 2 * n_val if route == "host-atomic" else n_val, overlapping=(route == "host-overlapping"))


def _engine(w, expiry):
    e = pea.Engine(max_committee_tables=8, vote_expiry_slots=EXPIRY if expiry else 0)
    e.store_init(0, 0, w.R["g"])
    for name, parent, slot in w.chain[1:]:
        e.add_block(w.R[name], w.R[parent], slot)
    e.set_validators(np.array(w.balances, dtype=np.uint64), np.ones(w.n_val, dtype=np.uint8))
    for ep in (3, 1, 2):
        com = w.committees[ep]
        offsets = np.cumsum([0] + [len(c) for c in com]).astype(np.uint32)
        e.set_committees(ep, offsets, np.array([v for c in com for v in c], dtype=np.uint32))
    e.on_tick(L.S0 * 12)
    return e


def _slots(e):
    out = np.zeros(e.num_validators, dtype=np.uint32)
    e._check(e._lib.pe_get_latest_message_slots(e._h, _ptr(out), e.num_validators))
    return out


def _table_bits(rows):
    out = {}
    for r in rows:
        out[r["target"][0]] = out.get(r["target"][0], 0) + r["n_bits"]
    return out


def _for_route(route, w, rows, clock):
    """The batch as the route takes it, with the selection of engine_attest.cpp (8 x bits of a table's rows against the
    registry's size) asserted on the rows themselves."""
    if route == "host-validator-major":
        rows = rows + w.fillers(clock, {r["target"][0] for r in rows})
        assert all(8 * b >= w.n_val for b in _table_bits(rows).values()), _table_bits(rows)
    elif route == "host-atomic":
        assert all(8 * b < w.n_val for b in _table_bits(rows).values()), _table_bits(rows)
    return rows


def _compare_state(e, w, model, expiry, what):
    name_of_index = {e.block_index_of(r): n for n, r in w.R.items()}
    name_of_index[NONE32] = "none"
    ep, blk = e.latest_messages()
    want_ep = np.zeros(w.n_val, dtype=np.uint64)
    want_blk = np.full(w.n_val, NONE32, dtype=np.uint32)
    want_slot = np.zeros(w.n_val, dtype=np.uint32)
    for v, (epoch, root) in model.latest.items():
        want_ep[v], want_blk[v], want_slot[v] = epoch, e.block_index_of(root), model.slots[v]
    bad = [(int(v), name_of_index.get(int(blk[v]), int(blk[v])), name_of_index[int(want_blk[v])])
           for v in np.nonzero(blk != want_blk)[0]]
    assert not bad, (what, "latest message: block (validator, engine, model)", bad[:8])
    has = want_blk != NONE32
    bad = [(int(v), int(ep[v]), int(want_ep[v])) for v in np.nonzero((ep != want_ep) & has)[0]]
    assert not bad, (what, "latest message: epoch (validator, engine, model)", bad[:8])
    if expiry:
        got = _slots(e)
        bad = [(int(v), int(got[v]), int(want_slot[v])) for v in np.nonzero((got != want_slot) & has)[0]]
        assert not bad, (what, "latest message: slot of the winning row (validator, engine, model)", bad[:8])
    for which, label in ((0, "current_epoch_participation"), (1, "previous_epoch_participation")):
        got, want = e.participation_get(which), np.array(model.part[which], dtype=np.uint8)
        bad = [(int(v), int(got[v]), int(want[v])) for v in np.nonzero(got != want)[0]]
        assert not bad, (what, label + " (validator, engine, model)", bad[:8])


def _compare_rows(rows, got, want, what):
    status, count, pst, num = got
    for label, a, b in (("on_attestation status", status, want["status"]), ("count", count, want["count"]),
                        ("process_attestation status", pst, want["pstatus"]), ("reward numerator", num, want["numerator"])):
        bad = [(i, r["tag"], int(x), y, m) for i, (r, x, y, m) in enumerate(zip(rows, a, b, want["mask"])) if int(x) != y]
        assert not bad, (what, label + " (row, tag, engine, model, model's flag mask)", bad)


def _check(route, w, steps, expiry, what):
    """One fresh handle: the steps through the route, the model beside it.  Consecutive batches go out in ONE stream of
    calls (on the pipelined routes: back to back), and everything is compared where that stream ends."""
    what = f"{route}, hot committee of {w.hot}, {what}"
    resident = route in RESIDENT_ROUTES
    model = M.Run(w.n_val, w.increments, w.brpi)
    e = _engine(w, expiry)
    try:
        clock, pending = L.S0, []

        def flush():
            if not pending:
                return
            batches = [_for_route(route, w, rows, clock) for rows in pending]
            if route == "paired":   # a last step for the one before it to pair with
                ep, vote = (2, "T64") if clock == L.S0 else (3, "T69")
                batches.append([w.row(clock, "pairing step", ep, 0, vote, bits=[1] * len(w.committees[ep][0]))])
            cc = w.committee_ctx(clock, resident)
            want = [model.batch(b, w.blocks, clock, w.sc[clock], cc, w.members_of) for b in batches]
            got = TA._run(e, route if resident else "host", batches, TA._ctx(w, w.scenario(clock)))
            for k, (b, g, wnt) in enumerate(zip(batches, got, want)):
                _compare_rows(b, g, wnt, f"{what}, batch {k} of {len(batches)}")
            _compare_state(e, w, model, expiry, what)
            del pending[:]

        for step in steps:
            if step[0] == "batch":
                pending.append(step[1])
                continue
            flush()
            if step[0] == "mark":
                e.mark_equivocating(np.array(sorted(set(step[1])), dtype=np.uint64))
                model.equivocating.update(step[1])
            else:
                assert step[0] == "tick"
                clock = L.S1
                e.on_tick(clock * 12)
                e.participation_rotate()
                model.part = ([0] * w.n_val, model.part[0])
        flush()
        assert model.latest
    finally:
        e.close()
    return model


# ---------------------------------------------------------------- 1 (and 7): equal epochs, the first row wins
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("hot,k,n_val", [(1, 2, 4096), (1, 5, 4096), (63, 3, 4096), (64, 5, 4096), (65, 2, 4096),
                                         (65, 5, 4096), (129, 3, 4096), (64, 3, 4100)])
def test_equal_epochs_first_row_wins(route, hot, k, n_val):
    """k rows of one target epoch name the special validators and vote for different blocks: every rotation, alone and
    among rows of other committees (positions 0 and 7, 3 and 4, ...); vote expiry on, so the slot is the winner's too."""
    w = _world(route, hot, n_val)
    v = L.specials(w.n_val)[0]
    winners = set()
    for rot in range(k):
        for inter in (False, True):
            steps, first = L.equal_epochs(w, k, rot, inter)
            model = _check(route, w, steps, True, f"equal epochs, k = {k}, rotation {rot}, interleaved = {inter}")
            assert model.latest[v][1] == first["beacon_block_root"]
            winners.add(model.latest[v][1])
    assert len(winners) == k   # the winner moved with the order


# ---------------------------------------------------------------- 2 (and 7): against the stored message
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("hot", [1, 64, 65, 129])
def test_against_the_stored_message(route, hot):
    w = _world(route, hot)
    v = L.specials(w.n_val)[0]
    for variant in ("sequence", "later first", "earlier first"):
        model = _check(route, w, L.stored_message(w, variant), True, f"stored message, {variant}")
        assert model.latest[v] == ((3, w.R["T69"]) if variant == "sequence" else (2, w.R["T68"]))
        if variant == "sequence" and len(L.seams(w.size["hot3"])) > 1:   # a seam validator the epoch-3 row does not name
            assert model.latest[w.committees[3][L.HOT3][L.seams(w.size["hot3"])[1]]][0] < 3


# ---------------------------------------------------------------- 3: two tables in one batch
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("hot", [63, 64, 129])
def test_two_tables_in_one_batch(route, hot):
    w = _world(route, hot)
    v = L.specials(w.n_val)[0]
    for later_first in (True, False):
        for inter in (False, True):
            model = _check(route, w, L.two_tables(w, later_first, inter), False,
                           f"two tables, later epoch first = {later_first}, interleaved = {inter}")
            assert model.latest[v][0] == 2 and model.part[0][v] == 7 and model.part[1][v] == 2
            if not (w.overlapping and inter):   # there a row of the second committee names the validator first
                assert model.latest[v][1] == w.R["T69"]


# ---------------------------------------------------------------- 4: equivocating validators
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("hot", [1, 65])
def test_equivocating_validators(route, hot):
    w = _world(route, hot)
    v = L.specials(w.n_val)[0]
    model = _check(route, w, L.equivocating(w, between=False), False, "equivocating, marked before the batch")
    assert v not in model.latest and model.part[0][v]
    model = _check(route, w, L.equivocating(w, between=True), False, "equivocating, marked between two batches")
    assert model.latest[v] == (1, w.R["P34"])


# ---------------------------------------------------------------- 5: a voided group
@pytest.mark.parametrize("route", RESIDENT_ROUTES)
@pytest.mark.parametrize("hot", L.SIZES)
def test_voided_group(route, hot):
    """Two rows of equal data whose bits overlap: one group, voided through its gate word -- no message, no flags, and
    the groups around it (one on the same committee, one on another, one on another table) as the model has them."""
    w = _world(route, hot)
    rows, groups = L.voided_group(w)
    group_of = [0, 1, 2, 1, 3]
    what = f"{route}, hot committee of {hot}, voided group on a committee of {w.size['hot2']}"
    model = M.Run(w.n_val, w.increments, w.brpi)
    pairing = [w.row(L.S0, "pairing step", 2, 0, "T64", bits=[1] * 160)]
    want = model.batch(groups, w.blocks, L.S0, w.sc[L.S0], w.committee_ctx(L.S0, True), w.members_of)
    assert want["status"][1] == M.BAD_SIGNATURE and want["pstatus"][1] == M.BAD_SIGNATURE
    e = _engine(w, False)
    try:
        ctx = TA._ctx(w, w.scenario(L.S0))
        if route == "paired":
            e.set_pipeline_lag(2)
            e.profile_enable(True)
            e.profile_reset()
        raw = []
        for batch in ([rows, pairing] if route == "paired" else [rows]):
            atts, arena = TA._pack(batch)
            if route == "resident":
                raw.append(TA._resident_calls(e, TA._dev_rows(atts), arena, ctx, head=False))
            else:
                with e.pipeline(lagged=(route == "paired")):
                    raw.append(TA._resident_calls(e, TA._dev_rows(atts), TA._dev_arena(arena), ctx, head=(route == "paired")))
        if route == "paired":
            e.drain()
            ln = {k: v["launches"] for k, v in e.profile().items()}
            e.profile_enable(False)
            assert all(ln[p] == 1 for p in ("pair_ingest_validate", "pair_plan_lmd", "pair_members_votes", "pair_union_tree")), ln
            model.batch(pairing, w.blocks, L.S0, w.sc[L.S0], w.committee_ctx(L.S0, True), w.members_of)
        agg, status, count, pst, num = raw[0]
        assert int(agg["n_groups"]) == 4 and list(np.asarray(agg["group_of"])[:5]) == group_of, what
        _compare_rows(groups, (status[:4], count[:4], pst[:4], num[:4]), want, what)
        _compare_state(e, w, model, False, what)
    finally:
        e.close()


# ---------------------------------------------------------------- 6: flag rounds
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("hot,r", [(1, 3), (63, 2), (64, 5), (65, 3), (129, 5), (129, 1)])
def test_flag_rounds(route, hot, r):
    """r rows on one committee with overlapping bit sets and nested flag masks, ascending and descending, every rotation;
    alone, and among rows of a second committee and of a second table."""
    w = _world(route, hot)
    for masks in L.FLAG_ORDERS[r]:
        for rot in range(r):
            for inter in (False, True):
                _check(route, w, L.flag_rounds(w, masks, rot, inter), False,
                       f"flag rounds, masks {masks}, rotation {rot}, interleaved = {inter}")


# ---------------------------------------------------------------- the selection between the two host LMD kernels
def test_either_side_of_the_validator_major_threshold():
    """8 x 511 = 4096 - 8 takes the atomic kernels, 8 x 512 = 4096 the validator-major one: the same messages."""
    w = L.world(64, 4096)
    left = _check("host", w, L.straddle(w, at_threshold=False), True, "511 bits on one table")
    right = _check("host", w, L.straddle(w, at_threshold=True), True, "512 bits on one table")
    assert left.latest == right.latest and left.slots == right.slots


# ---------------------------------------------------------------- 8: more rows of one committee than 16 bits count
def test_65537_rows_of_one_committee_in_one_call():
    """Host rows: 65537 accepted rows name one member of one committee with one mask, which is 65537 flag rounds.  The
    first pays in full, every later one nothing, and the byte is the mask."""
    w = L.world(1, 4096)   # HOT2 has 63 members
    n = 65537
    row = w.row(L.S0, "again and again", 2, L.HOT2, "T68", bits=[1 if i == 5 else 0 for i in range(63)])
    v = w.committees[2][L.HOT2][5]
    one, arena = TA._pack([row])
    atts = np.repeat(one, n)
    assert atts["flags"][0] == PE_ATT_FLAG_SIGNATURE_VALID and atts.dtype == synth.ATT_DTYPE
    e = _engine(w, False)
    try:
        pst, num = e.process_attestation_batch(TA._ctx(w, w.scenario(L.S0)), packed=(atts, arena))
        assert not pst.any()
        full = w.increments[v] * w.brpi * (14 + 26)
        paid = [(int(i), int(num[i])) for i in np.nonzero(num)[0]]
        assert paid == [(0, full)], ("rows that were paid (row, numerator); the model pays row 0 alone", paid[:8], full)
        want = np.zeros(w.n_val, dtype=np.uint8)
        want[v] = 3
        assert np.array_equal(e.participation_get(0), want) and not e.participation_get(1).any()
    finally:
        e.close()
