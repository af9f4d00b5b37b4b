"""-m gpu: pe_verify_resident -- every group of the resident aggregate decided by the pairing check from the points the signed
aggregate left in device memory, and the device-row handlers acting on that verdict.

Everything is valid or invalid BY CONSTRUCTION (no pairing is computed in Python): validator v holds the key sk_v G1 with
sk_v = A + v B (synth.registry_points), message j is the point h_j G2, and a row's signature is (sum of the sk of its set bits)
h_j G2 -- or something else where the case says so.  Every signature and message point is d G2 for a known d, built with the
engine's own g2_sum over the table 2^i G2; tests/verify_resident_model.py turns the scalars into the expected verdict
(e(key G1, h G2) e(-G1, sig G2) == 1  <=>  key h - sig == 0 mod r) and into the expected row of the rule table.

Shape: 512 validators in 64 committees of 8, two a slot.  More than 64 groups: the same committees attest again with another
source root (another AttestationData, hence another group)."""
import functools

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import g2
from pos_evolution_amd import _abi
from pos_evolution_amd._abi import pe_state_ctx
from tests import helpers as H
from tests import verify_resident_model as vm
from tests import wire_cases as wc
from tests import wire_model as wm
from tests.test_gpu_g2 import _off_subgroup_point
from tests.test_gpu_resident_rows import _dev_rows

pytestmark = pytest.mark.gpu
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT
R = vm.R_ORDER
N_VAL, N_COMM, SPE, SIZE = 512, 64, 32, 8
A, B = 0x1234567, 0x89ABCDE                                   # sk_v = A + v B: synth.registry_points' progression
MSG = [(0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 * (j + 1) + 97 * j) % R for j in range(4)]
D = 0xD00DFEEDFACE                                            # the cancelling pair: sig_a + D G2, sig_b - D G2
P_FIELD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
WIRE_H = wc.BASE_K["g2"]                                      # the base point of tests/wire_cases.py as a message point
BAD_SIGNATURE = 12                                            # PE_ATT_BAD_SIGNATURE
INVALID_ARG = -1                                               # PE_ERR_INVALID_ARG


@functools.lru_cache(maxsize=None)
def _table():
    pts, cur = [], g2.G2
    for _ in range(255):
        pts.append(cur)
        cur = g2.double(cur)
    return np.frombuffer(b"".join(g2.to_bytes192(p) for p in pts), dtype=np.uint8).reshape(-1, 192).copy()


@pytest.fixture(scope="module")
def tool(engine_factory):
    return engine_factory(device=0)


def _g2_points(tool, scalars):
    """(n, 192) uint8: d G2 for every d (0: the identity), by the engine's G2 sum over the doublings of G2."""
    idx, off = [], [0]
    for d in scalars:
        d %= R
        idx += [i for i in range(255) if (d >> i) & 1]
        off.append(len(idx))
    if not idx:
        idx = [0]
    return tool.g2_sum(_table(), np.array(off, dtype=np.uint32), index=np.array(idx, dtype=np.uint32)).copy()


def _world(engine_factory, seed=7):
    e = engine_factory(device=0)
    tree = synth.random_tree(96, seed, "branchy")
    H.load_tree(e, tree)
    e.set_validators(synth.balances(N_VAL, seed, mixed=True), synth.validator_flags(N_VAL, seed), synth.registry_points(e, N_VAL, A, B))
    epoch = int(tree.slot.max()) // SPE + 1
    comm = synth.random_committees(N_VAL, N_COMM, seed)
    e.set_committees(epoch, comm.offsets, comm.members)
    e.on_tick((epoch + 1) * SPE * 12)
    ctx = pe_state_ctx()
    ctx.slot = (epoch + 1) * SPE
    ctx.chain_tip_root[:] = tree.roots[tree.roots.shape[0] - 1].tobytes()
    ctx.current_justified_root[:] = tree.roots[0].tobytes()
    ctx.previous_justified_root[:] = tree.roots[0].tobytes()
    ctx.base_reward_per_increment = 777
    return dict(e=e, tree=tree, comm=comm, epoch=epoch, ctx=ctx)


def _members(w, committee, bits):
    c = w["comm"]
    return c.members[c.offsets[committee]:c.offsets[committee + 1]][np.asarray(bits, dtype=bool)]


def _sk_sum(w, committee, bits):
    m = _members(w, committee, bits)
    return (len(m) * A + int(m.astype(np.int64).sum()) * B) % R


def _bits(*positions):
    b = np.zeros(SIZE, dtype=bool)
    b[list(positions)] = True
    return b


class Rows:
    """The rows of one aggregate: add(group key, committee, bits, signature scalar, message index); rows of one (committee,
    variant) share their AttestationData and therefore their group."""

    def __init__(self, w):
        self.w, self.spec = w, []

    def add(self, committee, variant, bits, dlog, msg):
        self.spec.append((committee, variant, np.asarray(bits, dtype=bool), dlog, msg))
        return len(self.spec) - 1

    def build(self, tool, order=None):
        w, spec = self.w, self.spec if order is None else [self.spec[i] for i in order]
        atts, arena = H.committee_attestations(w["comm"], w["tree"], w["epoch"], [s[0] for s in spec], [s[2] for s in spec])
        for i, s in enumerate(spec):
            atts["source_root"][i, 31] ^= s[1]
        pts = _g2_points(tool, [s[3] if s[3] is not None else 0 for s in spec])
        return atts, arena, tool.g2_compress(pts).copy(), np.array([s[4] for s in spec], dtype=np.uint32)


def _standard(w, n_groups, forge=True):
    """n_groups groups of one or two rows; odd groups forged (their first row signs the next message); with five groups or more
    groups 0 and 2 carry the cancelling pair.  -> (Rows, [vm.Group per group])."""
    rows, model = Rows(w), []
    for g in range(n_groups):
        c, variant, j = g % N_COMM, g // N_COMM, g % len(MSG)
        parts = [_bits(0, 1, 2, 3, 4, 5, 6)] if g % 3 == 0 else [_bits(0, 1, 2, 3, 4), _bits(5, 6)]
        key, sig = 0, 0
        for k, bits in enumerate(parts):
            s = _sk_sum(w, c, bits)
            signed = MSG[(j + 1) % len(MSG)] if (forge and g % 2 == 1 and k == 0) else MSG[j]
            d = s * signed % R
            if forge and n_groups >= 5 and k == len(parts) - 1 and g in (0, 2):
                d = (d + (D if g == 0 else -D)) % R
            rows.add(c, variant, bits, d, j)
            key, sig = key + s, sig + d
        model.append(vm.Group(key=key % R, h=MSG[j], sig=sig % R))
    return rows, model


def _signed(e, atts, arena, sigs, check_subgroup=False, want_pk=True):
    return e.aggregate_signed(sigs, packed=(_dev_rows(atts), arena), compressed=True, check_subgroup=check_subgroup,
                              want_aggregate_pubkeys=want_pk)


def _group_order(agg, n_rows):
    """first input row of every device-formed group, in group order."""
    gof = np.asarray(agg["group_of"][:n_rows])
    return [int(np.flatnonzero(gof == g)[0]) for g in range(agg["n_groups"])]


def _msg_points(tool):
    return _g2_points(tool, MSG)


# ------------------------------------------------------------------ layout edges, and agreement with the host-staged route
@pytest.mark.parametrize("n_groups", [1, 3, 4, 5, 16, 17, 64, 65, 256, 257])
def test_layout_edges_by_construction_and_against_fast_aggregate_verify(engine_factory, tool, n_groups):
    """1, 3 | 4 | 5: four groups per Miller wave; 16 | 17: the lane pairs of one prepare wave; 64 | 65: a prepare workgroup;
    256 | 257: the settle's workgroup.  Valid and forged groups alternate."""
    w = _world(engine_factory)
    e = w["e"]
    rows, model = _standard(w, n_groups)
    atts, arena, sigs, msg_of_row = rows.build(tool)
    agg = _signed(e, atts, arena, sigs)
    assert agg["n_groups"] == n_groups                      # rows are in group order: device group g is group g
    msgs = _msg_points(tool)
    got = e.verify_resident(msgs, point_of_row=msg_of_row, apply=False)
    want = [vm.decide(m)[0] for m in model]
    assert got.tolist() == want
    assert set(want) == ({0, 1} if n_groups > 1 else {1})
    st = e._profile_verify_resident_stats()
    assert {k: st[k] for k in vm.ROWS} == {k: v for k, v in vm.stats(model).items() if k in vm.ROWS}
    assert st["groups"] == n_groups and st["subgroup_pass"] == 1
    # the route a caller had before: indices from the unions, signatures decompressed again, everything uploaded
    status, off, idx = e.get_indexed_attestations(packed=(agg["atts"], agg["out_arena"]))
    assert (status == 0).all()
    sig192, dst = e.g2_decompress(agg["sig96c"])
    assert (dst == 0).all()
    per_group = msgs[[g % len(MSG) for g in range(n_groups)]]
    assert e.fast_aggregate_verify(idx, off, per_group, sig192).tolist() == got.tolist()


# ------------------------------------------------------------------ the rule table
def _rule_table_rows(w, subgroup_member_scalar=None, wire_cases=()):
    """One group per row of the table (except 'no committee', which an aggregate with pubkeys cannot hold: see
    test_an_aggregate_with_a_group_without_committee_fails), honest groups between them; then one honest group per case of
    `wire_cases` signing WIRE_H G2, whose message point (index 8 + k) the caller replaces by the case's bytes.
    -> (Rows, model, extras)."""
    rows, model, note = Rows(w), [], {}

    def honest(c, j=0, parts=((0, 1, 2), (3, 4))):
        key = sig = 0
        for p in parts:
            s = _sk_sum(w, c, _bits(*p))
            rows.add(c, 0, _bits(*p), s * MSG[j] % R, j)
            key, sig = key + s, sig + s * MSG[j]
        model.append(vm.Group(key=key % R, h=MSG[j], sig=sig % R))
        return len(model) - 1

    honest(0)
    note["bad_message_off_curve"] = honest(1, j=1)        # its message point is replaced below: own point indices 4, 5, 6
    note["bad_message_non_canonical"] = honest(2, j=2)
    # overlapping members: the same bits twice
    s = _sk_sum(w, 3, _bits(0, 1))
    rows.add(3, 0, _bits(0, 1), s * MSG[0] % R, 0)
    rows.add(3, 0, _bits(0, 1), s * MSG[0] % R, 0)
    model.append(vm.Group(key=s, h=MSG[0], sig=2 * s * MSG[0] % R, overlap=True))
    honest(4, j=3)
    # a member whose signature does not decode (its bytes are replaced below)
    s0, s1 = _sk_sum(w, 5, _bits(0, 1)), _sk_sum(w, 5, _bits(2))
    rows.add(5, 0, _bits(0, 1), s0 * MSG[1] % R, 1)
    note["undecodable_row"] = rows.add(5, 0, _bits(2), s1 * MSG[1] % R, 1)
    model.append(vm.Group(key=(s0 + s1) % R, h=MSG[1], sig=s0 * MSG[1] % R, bad_member=True))
    # a member outside G2 (its bytes are replaced below)
    s0, s1 = _sk_sum(w, 6, _bits(0, 1)), _sk_sum(w, 6, _bits(2))
    rows.add(6, 0, _bits(0, 1), s0 * MSG[2] % R, 2)
    note["off_subgroup_row"] = rows.add(6, 0, _bits(2), s1 * MSG[2] % R, 2)
    note["off_subgroup_group"] = len(model)
    model.append(vm.Group(key=(s0 + s1) % R, h=MSG[2], sig=s0 * MSG[2] % R))   # bad_member / sig_in_g2 set by the caller
    # all-zero bits: the identity key (and the identity signature: the first matching row names it)
    rows.add(7, 0, _bits(), 0, 0)
    model.append(vm.Group(key=0, h=MSG[0], sig=0))
    # an identity aggregate signature from a member and its negation
    s0 = _sk_sum(w, 8, _bits(0, 1))
    rows.add(8, 0, _bits(0, 1), s0 * MSG[3] % R, 3)
    rows.add(8, 0, _bits(2, 3), -s0 * MSG[3] % R, 3)
    model.append(vm.Group(key=(s0 + _sk_sum(w, 8, _bits(2, 3))) % R, h=MSG[3], sig=0))
    # an identity message point: own point index 7
    note["identity_message"] = honest(9, j=0)
    honest(10, j=1)
    for k, c in enumerate(wire_cases):
        key = _sk_sum(w, 11 + k, _bits(0, 1, 2))
        rows.add(11 + k, 0, _bits(0, 1, 2), key * WIRE_H % R, 8 + k)
        note["wire", c.name] = len(model)
        model.append(vm.Group(key=key, h=WIRE_H, sig=key * WIRE_H % R))
    return rows, model, note


def _rule_table_call(engine_factory, tool, check_subgroup, wire_cases=()):
    """The rule table decided by one pe_verify_resident; -> (verdicts, model, note, stats)."""
    w = _world(engine_factory)
    e = w["e"]
    rows, model, note = _rule_table_rows(w, wire_cases=wire_cases)
    atts, arena, sigs, msg_of_row = rows.build(tool)
    sigs[note["undecodable_row"]] = 0                       # no compression flag: malformed
    sigs[note["off_subgroup_row"]] = np.frombuffer(g2.compress(_off_subgroup_point()), dtype=np.uint8)
    g_off = note["off_subgroup_group"]
    if check_subgroup:
        model[g_off].bad_member = True                      # the leg leaves it out and counts it
    else:
        model[g_off].sig_in_g2 = False                      # it enters the sum: the call's own pass finds the aggregate
    # points 0..3 = MSG; 4: off its curve; 5: unused; 6: not canonical; 7: the identity
    msgs = np.concatenate([_msg_points(tool), np.zeros((4 + len(wire_cases), 192), dtype=np.uint8)])
    for k, c in enumerate(wire_cases):
        msgs[8 + k] = np.frombuffer(c.enc, dtype=np.uint8)
        if c.expect == wm.BAD:
            model[note["wire", c.name]].bad_message = True
        elif c.expect == wm.INFINITY:
            model[note["wire", c.name]].h = 0
    good = g2.mul(MSG[1], g2.G2)
    msgs[4] = np.frombuffer(g2.to_bytes192((good[0], ((good[1][0] + 1) % P_FIELD, good[1][1]))), dtype=np.uint8)
    msgs[5] = msgs[0]
    nc = bytearray(g2.to_bytes192(g2.mul(MSG[2], g2.G2)))
    x_c0 = int.from_bytes(nc[48:96], "big") + P_FIELD      # the same residue, not reduced: fits 48 bytes, no flag bits there
    assert x_c0 < 1 << 384
    nc[48:96] = x_c0.to_bytes(48, "big")
    msgs[6] = np.frombuffer(bytes(nc), dtype=np.uint8)
    msgs[7] = np.frombuffer(g2.to_bytes192(None), dtype=np.uint8)
    agg = _signed(e, atts, arena, sigs, check_subgroup=check_subgroup)
    first = _group_order(agg, len(atts))
    assert agg["n_groups"] == len(model)
    point = msg_of_row.copy()
    for key, idx in (("bad_message_off_curve", 4), ("bad_message_non_canonical", 6), ("identity_message", 7)):
        g = note[key]
        point[[i for i in range(len(atts)) if agg["group_of"][i] == g]] = idx
        if idx == 7:
            model[g].h = 0
        else:
            model[g].bad_message = True
    assert first == sorted(first)
    got = e.verify_resident(msgs, point_of_row=point, apply=False)
    return got, model, note, e._profile_verify_resident_stats()


@pytest.mark.parametrize("check_subgroup", [False, True])
def test_every_row_of_the_rule_table(engine_factory, tool, check_subgroup):
    got, model, note, st = _rule_table_call(engine_factory, tool, check_subgroup)
    assert got.tolist() == [vm.decide(m)[0] for m in model]
    want = vm.stats(model, subgroup_pass=not check_subgroup)
    assert st == {**want, "no_committee": 0}
    for row in ("bad_message", "overlap", "bad_member", "empty_key", "identity_signature", "identity_message", "pairing"):
        assert st[row] >= 1, row
    assert st["not_g2"] == (0 if check_subgroup else 1) and st["bad_message"] == 2


def test_every_wire_case_on_the_message_point(engine_factory, tool):
    """k_bls_resident_prepare decodes the message point with wire_load_g2 (wire_points.h): every case of tests/wire_cases.py
    as the message point of an honest group behind the rule table's own groups, whose verdicts must not move.  A bad encoding is
    row 2 of the table (verdict 2), every spelling of infinity the identity message (0), bit 5 on x.c1 changes nothing (1)."""
    cases = wc.cases("g2")
    got, model, note, st = _rule_table_call(engine_factory, tool, False, wire_cases=cases)
    want = [vm.decide(m)[0] for m in model]
    by_class = {wc.SAME: 1, wm.INFINITY: 0, wm.BAD: 2}
    for c in cases:
        assert want[note["wire", c.name]] == by_class[c.expect], c.name
    seen = [(c.name, int(got[note["wire", c.name]]), by_class[c.expect]) for c in cases]
    print(seen)
    assert not [s for s in seen if s[1] != s[2]]
    assert got.tolist() == want
    assert st == {**vm.stats(model, subgroup_pass=True), "no_committee": 0}
    assert st["bad_message"] == 2 + sum(c.expect == wm.BAD for c in cases)
    assert st["identity_message"] == 1 + sum(c.expect == wm.INFINITY for c in cases)


def test_an_aggregate_with_a_group_without_committee_fails(engine_factory, tool):
    """PE_BLS_UNDECIDED is the verdict of a group whose status_agg is not 0.  An aggregate that asks for pubkeys -- the only kind
    this call accepts -- fails as a whole when it holds such a group, so no completed aggregate shows the verdict today; the
    kernel keeps the row and the model test pins it.  Here: that aggregate fails, and the call then refuses the handle."""
    w = _world(engine_factory)
    e = w["e"]
    rows, _ = _standard(w, 4, forge=False)
    atts, arena, sigs, _ = rows.build(tool)
    atts["index"][2] = N_COMM                                # a flat committee id beyond the table
    with pytest.raises(pea.EngineError):
        _signed(e, atts, arena, sigs)
    with pytest.raises(pea.EngineError) as err:
        e.verify_resident(_msg_points(tool), apply=False)
    assert err.value.status == _abi.PE_ERR_STATE


# ------------------------------------------------------------------ message points
def test_message_points_by_row_by_group_and_in_device_memory(engine_factory, tool):
    import torch

    w = _world(engine_factory)
    e = w["e"]
    n_groups = 21
    rows, model = _standard(w, n_groups)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(rows.spec))
    atts, arena, sigs, msg_of_row = rows.build(tool, order=perm)          # groups form in order of first appearance
    agg = _signed(e, atts, arena, sigs)
    first = _group_order(agg, len(atts))
    spec_group = []                                                       # device group -> group of _standard
    count = 0
    starts = []
    for g in range(n_groups):
        starts.append(count)
        count += 1 if g % 3 == 0 else 2
    for r in first:
        spec_group.append(max(g for g in range(n_groups) if starts[g] <= perm[r]))
    want = [vm.decide(model[g])[0] for g in spec_group]
    assert 0 in want and 1 in want
    # shuffled points, several rows sharing one
    shuffle = np.array([2, 0, 3, 1])
    msgs = _msg_points(tool)
    shuffled = np.empty_like(msgs)
    shuffled[shuffle] = msgs                                             # point j now lies at shuffle[j]
    assert e.verify_resident(shuffled, point_of_row=shuffle[msg_of_row], apply=False).tolist() == want
    # NULL point_of_row: one point per group, in the device-formed order
    per_group = msgs[[g % len(MSG) for g in spec_group]]
    assert e.verify_resident(per_group, apply=False).tolist() == want
    # device memory: 16-byte aligned (read in place), and off by 8 bytes (copied)
    flat = np.ascontiguousarray(per_group).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(8, dtype=np.uint8), flat, np.zeros(8, dtype=np.uint8)])).cuda()
    t16 = torch.from_numpy(flat.copy()).cuda()
    assert t16.data_ptr() % 16 == 0 and (t.data_ptr() + 8) % 16 == 8
    assert e.verify_resident(pea.DeviceArena(t16.data_ptr(), flat.size, keep=t16), apply=False).tolist() == want
    assert e.verify_resident(pea.DeviceArena(t.data_ptr() + 8, flat.size, keep=t), apply=False).tolist() == want


# ------------------------------------------------------------------ the handlers act on the computed verdict
def test_handlers_reject_exactly_the_forged_groups(engine_factory, tool):
    n_groups = N_COMM
    worlds = [_world(engine_factory) for _ in range(3)]                   # apply | verdicts only | never verified
    rows, model = _standard(worlds[0], n_groups)
    atts, arena, sigs, msg_of_row = rows.build(tool)
    msgs = _msg_points(tool)
    want = np.array([vm.decide(m)[0] for m in model])
    forged = want != 1
    assert forged.any() and (~forged).any()
    out = []
    for k, w in enumerate(worlds):
        e = w["e"]
        agg = _signed(e, atts, arena, sigs)
        assert agg["n_groups"] == n_groups
        if k < 2:
            assert e.verify_resident(msgs, point_of_row=msg_of_row, apply=(k == 0)).tolist() == want.tolist()
        if k == 0:                                                        # twice is harmless
            assert e.verify_resident(msgs, point_of_row=msg_of_row, apply=True).tolist() == want.tolist()
        status, _, _ = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))
        pst, num = e.process_attestation_batch(w["ctx"], packed=(RR, RES), cap=len(atts))
        out.append((status[:n_groups].copy(), pst[:n_groups].copy(), num[:n_groups].copy()))
    (st_a, pst_a, num_a), (st_v, pst_v, num_v), (st_n, pst_n, num_n) = out
    # without apply, and without the call: the statuses of today
    assert (st_n == 0).all() and (pst_n == 0).all()
    assert np.array_equal(st_v, st_n) and np.array_equal(pst_v, pst_n) and np.array_equal(num_v, num_n)
    # with apply: PE_ATT_BAD_SIGNATURE for exactly the forged groups
    assert np.array_equal(st_a, np.where(forged, BAD_SIGNATURE, 0)) and np.array_equal(pst_a, np.where(forged, BAD_SIGNATURE, 0))
    assert (num_a[forged] == 0).all() and np.array_equal(num_a[~forged], num_n[~forged])
    # ... and nothing of theirs moved: no latest message, no participation flag
    ea, en = worlds[0]["e"], worlds[2]["e"]
    (ep_a, blk_a), (ep_n, blk_n) = ea.latest_messages(), en.latest_messages()
    part_a, part_n = [ea.participation_get(i) for i in (0, 1)], [en.participation_get(i) for i in (0, 1)]
    voted_forged = np.zeros(N_VAL, dtype=bool)
    for g in np.flatnonzero(forged):
        voted_forged[_members(worlds[0], g % N_COMM, _bits(0, 1, 2, 3, 4, 5, 6))] = True
    assert (blk_a[voted_forged] == 0xFFFFFFFF).all() and (blk_n[voted_forged] != 0xFFFFFFFF).any()
    assert np.array_equal(blk_a[~voted_forged], blk_n[~voted_forged]) and np.array_equal(ep_a[~voted_forged], ep_n[~voted_forged])
    for pa, pn in zip(part_a, part_n):
        assert (pa[voted_forged] == 0).all() and np.array_equal(pa[~voted_forged], pn[~voted_forged])
    assert any((pn[voted_forged] != 0).any() for pn in part_n)

    class _Store:
        engine = worlds[1]["e"]
    from pos_evolution_amd import forkchoice
    assert forkchoice.verify_resident_attestations(_Store, [bytes(m) for m in msgs], point_of_row=msg_of_row) == \
        [bool(v == 1) for v in want]
    status, _, _ = _Store.engine.on_attestation_batch(packed=(RR, RES), cap=len(atts))
    assert np.array_equal(status[:n_groups] == BAD_SIGNATURE, forged)


# ------------------------------------------------------------------ the signed aggregate's own outputs
def test_signed_aggregate_outputs_are_unchanged(engine_factory, tool):
    """The leg that keeps the points gives the bytes of the leg that does not: out_signatures96 and sig_status against a twin
    handle that asks for no pubkeys (null keep pointers: the parent's launch), and both against the closed forms -- the aggregate
    key of the union's members (synth.registry_closed_form) and the compressed sum of the rows' known multiples of G2."""
    wa, wb = _world(engine_factory), _world(engine_factory)
    rows, model, note = _rule_table_rows(wa)
    atts, arena, sigs, _ = rows.build(tool)
    sigs[note["undecodable_row"]] = 0
    sigs[note["off_subgroup_row"]] = np.frombuffer(g2.compress(_off_subgroup_point()), dtype=np.uint8)
    for check in (False, True):
        kept = _signed(wa["e"], atts, arena, sigs, check_subgroup=check, want_pk=True)
        plain = _signed(wb["e"], atts, arena, sigs, check_subgroup=check, want_pk=False)
        n = kept["n_groups"]
        assert n == plain["n_groups"] == len(model)
        assert np.array_equal(kept["sig96c"], plain["sig96c"]) and np.array_equal(kept["sig_status"], plain["sig_status"])
        assert np.array_equal(kept["atts"], plain["atts"]) and np.array_equal(kept["out_arena"], plain["out_arena"])
        want_status = np.zeros(len(atts), dtype=np.int32)
        want_status[note["undecodable_row"]] = 1
        if check:
            want_status[note["off_subgroup_row"]] = 3
        assert kept["sig_status"].tolist() == want_status.tolist()
        bits = kept["bits"]
        for g in range(n):
            c = int((kept["atts"][g]["slot"] % SPE) * (N_COMM // SPE) + kept["atts"][g]["index"])
            assert kept["aggpk96"][g].tobytes() == synth.registry_closed_form(_members(wa, c, bits[g]), A, B), g
            if g != note["off_subgroup_group"] or check:
                assert kept["sig96c"][g].tobytes() == g2.compress(g2.mul(model[g].sig, g2.G2) if model[g].sig else None), g


# ------------------------------------------------------------------ error returns
def test_error_returns_write_nothing_and_a_valid_call_follows(engine_factory, tool):
    w = _world(engine_factory)
    e = w["e"]
    rows, model = _standard(w, 9)
    atts, arena, sigs, msg_of_row = rows.build(tool)
    atts0, arena0, sigs0, msg_of_row0 = atts, arena, sigs, msg_of_row               # this epoch's rows, for the second world
    msgs = _msg_points(tool)
    want = [vm.decide(m)[0] for m in model]
    dev = _dev_rows(atts)

    def refused(status, **kw):
        with pytest.raises(pea.EngineError) as err:
            e.verify_resident(kw.pop("msgs", msgs), **{"point_of_row": msg_of_row, "apply": True, **kw})
        assert err.value.status == status, (err.value.status, status)

    def valid_call_follows():
        _signed(e, atts, arena, sigs)
        assert e.verify_resident(msgs, point_of_row=msg_of_row, apply=False).tolist() == want

    per_group = msgs[[g % len(MSG) for g in range(len(model))]]
    by_group = dict(point_of_row=None, msgs=per_group)
    refused(_abi.PE_ERR_STATE, **by_group)                                           # no aggregate at all
    valid_call_follows()
    e.aggregate(packed=(dev, arena), want_aggregate_pubkeys=True)                    # an unsigned aggregate
    refused(_abi.PE_ERR_STATE, **by_group)
    valid_call_follows()
    e.aggregate_signed(sigs, packed=(atts, arena), want_aggregate_pubkeys=True)      # host rows
    refused(_abi.PE_ERR_STATE, **by_group)
    valid_call_follows()
    _signed(e, atts, arena, sigs, want_pk=False)                                     # aggregate pubkeys not requested
    refused(_abi.PE_ERR_STATE, **by_group)
    valid_call_follows()
    # PE_ERR_INVALID_ARG / PE_ERR_CAPACITY: nothing written, nothing applied -- the handlers afterwards accept every group
    _signed(e, atts, arena, sigs)
    bad = msg_of_row.copy()
    bad[3] = len(msgs)
    refused(INVALID_ARG, point_of_row=bad)                               # a point_of_row entry out of range
    refused(INVALID_ARG, point_of_row=None, msgs=msgs[:4])               # too few points for nine groups
    refused(_abi.PE_ERR_CAPACITY, cap=len(model) - 1)                                # cap below the group count
    sentinel = np.full(16, 77, dtype=np.int32)
    rc = e._lib.pe_verify_resident(e._h, msgs.ctypes.data, len(msgs), None, _abi.PE_VERIFY_APPLY, 8,
                                   sentinel.ctypes.data_as(_abi.C.POINTER(_abi.C.c_int32)))
    assert rc == INVALID_ARG and (sentinel == 77).all()
    status, _, _ = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))
    assert (status[:len(model)] == 0).all()
    assert e.verify_resident(msgs, point_of_row=msg_of_row, apply=False).tolist() == want
    # a tick between the aggregate and the call: the rule of PE_ROWS_RESIDENT
    e.set_committees(w["epoch"] + 1, w["comm"].offsets, w["comm"].members)          # the next epoch's table, for the call after
    _signed(e, atts, arena, sigs)
    e.on_tick((w["epoch"] + 2) * SPE * 12)
    refused(_abi.PE_ERR_STATE)
    rows_next, _ = _standard(dict(w, epoch=w["epoch"] + 1), 9)                       # the same groups, one epoch later
    atts, arena, sigs, msg_of_row = rows_next.build(tool)
    valid_call_follows()
    # pe_dist_init_custom active
    w2 = _world(engine_factory)
    _signed(w2["e"], atts0, arena0, sigs0)
    assert w2["e"].verify_resident(msgs, point_of_row=msg_of_row0, apply=False).tolist() == want
    w2["e"].dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    with pytest.raises(pea.EngineError) as err:
        w2["e"].verify_resident(msgs, point_of_row=msg_of_row0, apply=False)
    assert err.value.status == _abi.PE_ERR_STATE
    w2["e"].dist_destroy()
    _signed(w2["e"], atts0, arena0, sigs0)
    assert w2["e"].verify_resident(msgs, point_of_row=msg_of_row0, apply=False).tolist() == want
