"""-m gpu: pe_verify_resident_data -- the resident aggregate verified over the signing root of ITS OWN AttestationData: signing
roots, hash_to_curve and the pairing check on the device, from the rows where they lie.

The world is tests/test_gpu_verify_resident.py's (512 validators, 64 committees of 8, sk_v = A + v B).  Signatures here are TRUE
signatures over the specification's message: a row's is (sum of the sk of its set bits) * hash_to_g2(model signing root), with
tests/att_signing_model.py for the root and tests/hash_to_curve_model.py for the point and the multiplication -- so a VALID
verdict means the engine hashed the same 32 bytes to the same point.  Python pays ~0.3 s per signature: at most six groups, every
point and signature computed once per module and shared."""
import functools

import numpy as np
import pytest

import pos_evolution_amd as pea
from oracle import g2
from pos_evolution_amd import _abi, forkchoice
from tests import att_signing_model as am
from tests import hash_to_curve_model as hm
from tests import helpers as H
from tests.test_gpu_resident_rows import _dev_rows
from tests.test_gpu_verify_resident import BAD_SIGNATURE, N_COMM, R, SPE, _bits, _group_order, _signed, _sk_sum, _world

pytestmark = pytest.mark.gpu
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT
PREV, CUR = am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT
ALL, HEAD, TAIL = _bits(0, 1, 2, 3, 4, 5, 6), _bits(0, 1, 2, 3, 4), _bits(5, 6)


@functools.lru_cache(maxsize=None)
def _point(message: bytes):
    return hm.hash_to_g2(message, hm.ETH2_DST)


@functools.lru_cache(maxsize=None)
def _signature(message: bytes, sk: int) -> bytes:
    """sk * H(message), compressed"""
    return g2.compress(hm.curve_mul(sk % R, _point(message)))


class Group:
    """One group: a committee's attestation (variant: another source root, hence another AttestationData) in `parts` rows.
    epoch_shift 1: the target is the epoch after the world's.  message(row) -> the 32 bytes the members sign; default: the
    model's signing root of the row under (fork_epoch, PREV, CUR)."""

    def __init__(self, committee, parts=(ALL,), variant=0, epoch_shift=0, message=None):
        self.committee, self.parts, self.variant, self.epoch_shift, self.message = committee, parts, variant, epoch_shift, message


def _build(w, groups, fork_epoch):
    """-> (atts, arena, compressed signatures, model roots per group)"""
    comms = [g.committee for g in groups for _ in g.parts]
    atts, arena = H.committee_attestations(w["comm"], w["tree"], w["epoch"], comms, [p for g in groups for p in g.parts])
    sigs, roots, i = [], [], 0
    for g in groups:
        for bits in g.parts:
            atts["source_root"][i, 31] ^= g.variant
            atts["slot"][i] += SPE * g.epoch_shift
            atts["target_epoch"][i] += g.epoch_shift                 # the target root stays: the tree ends before either epoch
            root = am.signing_root(atts[i], fork_epoch, PREV, CUR)
            signed = g.message(atts[i]) if g.message else root
            sigs.append(_signature(signed, _sk_sum(w, g.committee, bits)))
            i += 1
        roots.append(root)
    return atts, arena, np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(-1, 96).copy(), roots


def _other_domain(fork_epoch):
    return lambda row: am.signing_root(row, fork_epoch, CUR, PREV)


def _one_field_off(fork_epoch):
    def message(row):
        other = {name: row[name] for name in am.FIELDS}
        other["source_epoch"] = int(row["source_epoch"]) + 1
        return am.signing_root(other, fork_epoch, PREV, CUR)
    return message


def _four(fork_epoch=0):
    """honest in one row | honest in two rows | signed under the other domain | signed over data one field off"""
    return [Group(0), Group(1, parts=(HEAD, TAIL)), Group(2, message=_other_domain(fork_epoch)),
            Group(3, message=_one_field_off(fork_epoch))], [1, 1, 0, 0]


def _roots_array(roots):
    return np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(-1, 32)


def test_by_construction(engine_factory):
    w = _world(engine_factory)
    e = w["e"]
    groups, want = _four()
    atts, arena, sigs, roots = _build(w, groups, 0)
    agg = _signed(e, atts, arena, sigs)
    assert agg["n_groups"] == 4
    verdict, got_roots = e.verify_resident_data(0, PREV, CUR, apply=False)
    assert verdict.tolist() == want
    assert np.array_equal(got_roots, _roots_array(roots))
    st = e._profile_verify_resident_stats()
    assert st["groups"] == 4 and st["pairing"] == 4 and st["bad_message"] == 0 and st["subgroup_pass"] == 1
    # every row takes the previous domain once the fork lies beyond its target: the honest groups no longer verify, the group
    # that signed under the swapped pair does
    verdict, got_roots = e.verify_resident_data(2**64 - 1, PREV, CUR, apply=False)
    assert verdict.tolist() == [0, 0, 1, 0]
    assert np.array_equal(got_roots, _roots_array([am.signing_root(atts[i], 2**64 - 1, PREV, CUR) for i in (0, 1, 3, 4)]))

    class _Store:
        engine = e
    assert forkchoice.verify_resident_attestation_data(_Store, 0, PREV, CUR) == [True, True, False, False]


def test_fork_boundary(engine_factory):
    w = _world(engine_factory)
    e = w["e"]
    cur_epoch = w["epoch"] + 1
    e.set_committees(cur_epoch, w["comm"].offsets, w["comm"].members)
    e.on_tick(((cur_epoch + 1) * SPE - 1) * 12)                       # the last slot of the store's current epoch
    groups = [Group(0), Group(1, epoch_shift=1)]                      # targets: the store's previous | current epoch
    atts, arena, sigs, roots = _build(w, groups, cur_epoch)
    assert atts["target_epoch"].tolist() == [cur_epoch - 1, cur_epoch]
    assert roots[0] == am.sm.H(am.attestation_data_root(atts[0]) + PREV) and roots[1] == am.sm.H(am.attestation_data_root(atts[1]) + CUR)
    agg = _signed(e, atts, arena, sigs)
    assert agg["n_groups"] == 2
    verdict, got_roots = e.verify_resident_data(cur_epoch, PREV, CUR, apply=False)
    assert verdict.tolist() == [1, 1] and np.array_equal(got_roots, _roots_array(roots))
    verdict, got_roots = e.verify_resident_data(cur_epoch, CUR, PREV, apply=False)
    assert verdict.tolist() == [0, 0]
    assert np.array_equal(got_roots, _roots_array([am.signing_root(a, cur_epoch, CUR, PREV) for a in atts]))
    # one epoch either way and exactly one group changes its domain
    assert e.verify_resident_data(cur_epoch + 1, PREV, CUR, apply=False)[0].tolist() == [1, 0]
    assert e.verify_resident_data(cur_epoch - 1, PREV, CUR, apply=False)[0].tolist() == [0, 1]


@pytest.mark.parametrize("n_groups", [1, 4, 5])
def test_against_the_three_call_route(engine_factory, n_groups):
    """A wave of the Miller loop holds four groups.  Odd groups are signed under the other domain."""
    w = _world(engine_factory)
    e = w["e"]
    groups = [Group(g, message=_other_domain(0) if g % 2 else None) for g in range(n_groups)]
    atts, arena, sigs, roots = _build(w, groups, 0)
    dev = _dev_rows(atts)
    agg = e.aggregate_signed(sigs, packed=(dev, arena), compressed=True, want_aggregate_pubkeys=True)
    first = _group_order(agg, len(atts))
    assert agg["n_groups"] == n_groups and first == list(range(n_groups))
    # the route it replaces, device memory to device memory: roots of the first rows -> points -> verdicts
    import torch
    buf = torch.zeros(32 * n_groups + 192 * n_groups, dtype=torch.uint8, device="cuda")
    d_roots = pea.DeviceArena(buf.data_ptr(), 32 * n_groups, keep=buf)
    d_points = pea.DeviceArena(buf.data_ptr() + 32 * n_groups, 192 * n_groups, keep=buf)
    e.attestation_signing_roots(pea.DeviceRows(dev.ptr, n_groups, keep=dev), 0, PREV, CUR, out=d_roots)
    e.hash_to_g2((d_roots, 32), out=d_points)
    before = e.verify_resident(d_points, apply=False)
    stats_before = e._profile_verify_resident_stats()
    assert before.tolist() == [1 - g % 2 for g in range(n_groups)]
    verdict, got_roots = e.verify_resident_data(0, PREV, CUR, apply=False)
    assert np.array_equal(verdict, before) and e._profile_verify_resident_stats() == stats_before
    assert np.array_equal(got_roots, _roots_array(roots))
    assert np.array_equal(buf[:32 * n_groups].cpu().numpy().reshape(-1, 32), got_roots)
    # the shared workspace is intact: the caller's points decide as before, and so does the call itself
    assert np.array_equal(e.verify_resident(d_points, apply=False), before) and e._profile_verify_resident_stats() == stats_before
    host_points = e.hash_to_g2(_roots_array(roots))
    assert np.array_equal(e.verify_resident(host_points, apply=False), before)
    assert np.array_equal(e.verify_resident_data(0, PREV, CUR, apply=False, want_roots=False)[0], before)


def test_apply_reaches_the_handlers(engine_factory):
    groups, want = _four()
    forged = np.array(want) != 1
    out = []
    for apply in (True, False):
        w = _world(engine_factory)
        e = w["e"]
        atts, arena, sigs, _ = _build(w, groups, 0)
        _signed(e, atts, arena, sigs)
        assert e.verify_resident_data(0, PREV, CUR, apply=apply)[0].tolist() == want
        if apply:                                                     # twice is harmless
            assert e.verify_resident_data(0, PREV, CUR, apply=True)[0].tolist() == want
        status, _, _ = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))
        pst, num = e.process_attestation_batch(w["ctx"], packed=(RR, RES), cap=len(atts))
        out.append((status[:4].copy(), pst[:4].copy(), num[:4].copy()))
    (st_a, pst_a, num_a), (st_v, pst_v, num_v) = out
    assert (st_v == 0).all() and (pst_v == 0).all()                   # without PE_VERIFY_APPLY sig_valid is unchanged
    assert np.array_equal(st_a, np.where(forged, BAD_SIGNATURE, 0)) and np.array_equal(pst_a, np.where(forged, BAD_SIGNATURE, 0))
    assert (num_a[forged] == 0).all() and np.array_equal(num_a[~forged], num_v[~forged])


def test_unchanged_around_it(engine_factory):
    w = _world(engine_factory)
    e = w["e"]
    groups, want = _four()
    atts, arena, sigs, roots = _build(w, groups, 0)
    dom = e._attester_domains(0, PREV, CUR)

    def refused(status, call=None):
        with pytest.raises(pea.EngineError) as err:
            (call or (lambda: e.verify_resident_data(0, PREV, CUR)))()
        assert err.value.status == status, (err.value.status, status)

    def valid_call_follows():
        _signed(e, atts, arena, sigs)
        assert e.verify_resident_data(0, PREV, CUR, apply=False)[0].tolist() == want

    refused(_abi.PE_ERR_STATE)                                        # no aggregate at all
    valid_call_follows()
    e.aggregate(packed=(_dev_rows(atts), arena), want_aggregate_pubkeys=True)      # an unsigned aggregate
    refused(_abi.PE_ERR_STATE)
    valid_call_follows()
    e.aggregate_signed(sigs, packed=(atts, arena), want_aggregate_pubkeys=True)    # host rows
    refused(_abi.PE_ERR_STATE)
    valid_call_follows()
    # zero rows: pe_aggregate_signed forms no resident aggregate from them, and both calls say so alike
    e.aggregate_signed(sigs[:0], packed=(atts[:0], arena), want_aggregate_pubkeys=True)
    refused(_abi.PE_ERR_STATE)
    refused(_abi.PE_ERR_STATE, lambda: e.verify_resident(np.zeros((1, 192), np.uint8)))
    valid_call_follows()
    # a group without a committee: an aggregate that asks for pubkeys fails as a whole (tests/test_gpu_verify_resident.py), so
    # no completed aggregate holds one; the call refuses the handle as pe_verify_resident does
    bad = atts.copy()
    bad["index"][2] = N_COMM
    with pytest.raises(pea.EngineError):
        _signed(e, bad, arena, sigs)
    refused(_abi.PE_ERR_STATE)
    valid_call_follows()
    # errors write nothing and apply nothing
    verdict, out_roots = np.full(8, 77, dtype=np.int32), np.full(8 * 32, 0x77, dtype=np.uint8)
    raw = lambda d, flags, cap: e._lib.pe_verify_resident_data(e._h, d, flags, cap, verdict.ctypes.data, out_roots.ctypes.data)
    assert raw(None, _abi.PE_VERIFY_APPLY, 8) == _abi.PE_ERR_INVALID_ARG              # NULL dom
    assert raw(_abi.C.byref(dom), _abi.PE_VERIFY_APPLY | 2, 8) == _abi.PE_ERR_INVALID_ARG   # unknown flags
    assert raw(_abi.C.byref(dom), _abi.PE_VERIFY_APPLY, 3) == _abi.PE_ERR_CAPACITY    # cap below the four groups
    assert (verdict == 77).all() and (out_roots == 0x77).all()
    status, _, _ = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))
    assert (status[:4] == 0).all()
    # cap above the groups: the entries past them read 0
    assert raw(_abi.C.byref(dom), 0, 6) == _abi.PE_OK
    assert verdict.tolist() == want + [0, 0, 77, 77]
    assert np.array_equal(out_roots[:128].reshape(4, 32), _roots_array(roots)) and (out_roots[128:192] == 0).all() and (out_roots[192:] == 0x77).all()
    # a tick between the aggregate and the call: the rule of PE_ROWS_RESIDENT
    e.set_committees(w["epoch"] + 1, w["comm"].offsets, w["comm"].members)
    _signed(e, atts, arena, sigs)
    e.on_tick((w["epoch"] + 2) * SPE * 12)
    refused(_abi.PE_ERR_STATE)


def test_an_open_pipeline_is_completed_not_refused(engine_factory):
    w = _world(engine_factory)
    e = w["e"]
    groups, want = _four()
    atts, arena, sigs, roots = _build(w, groups, 0)
    dev = _dev_rows(atts)
    with e.pipeline():
        e.aggregate_signed(sigs, packed=(dev, arena), compressed=True, want_aggregate_pubkeys=True)
        verdict, got_roots = e.verify_resident_data(0, PREV, CUR, apply=False)
        assert verdict.tolist() == want and np.array_equal(got_roots, _roots_array(roots))
