"""CPU: the model of the block operations (tests/block_ops_model.py) against itself and against what already stands: the
sequential loop -- the specification -- is held to the closed form the kernels compute on seeded random registries whose
classes are counted; is_slashable_attestation_data is the reference's text; initiate_validator_exit agrees with the
registry updates' ejections."""
import numpy as np
import pytest

from tests import block_ops_cases as K
from tests import block_ops_model as B
from tests import registry_updates_model as M


def assert_same(got, want):
    (ga, gs, gt), (wa, ws, wt) = got, want
    assert gs == ws
    assert gt == wt
    for k in M.FIELDS:
        assert np.array_equal(ga[k], wa[k]), k


@pytest.mark.parametrize("knobs", K.GRID, ids=lambda k: "-".join(str(v) for v in k.values()))
def test_the_loop_is_the_closed_form(knobs):
    a, proposer, ops, p = K.random_block(**knobs)
    before = M.copy_registry(a)
    want = B.block_operations_sequential(a, K.CUR, proposer, ops, p)
    assert_same(B.block_operations_closed_form(a, K.CUR, proposer, ops, p), want)
    assert all(np.array_equal(a[k], before[k]) for k in M.FIELDS)       # neither form writes its input
    if want[2]["n_invalid"]:
        assert all(np.array_equal(want[0][k], before[k]) for k in M.FIELDS)
    else:
        assert knobs["valid"] and len(ops) > 0


def test_every_class_occurred():
    """a condition on the generator's output, not a tolerance: the grid above shows each class at least once"""
    seen = dict.fromkeys(K.CLASSES, 0)
    for knobs in K.GRID:
        a, proposer, ops, p = K.random_block(**knobs)
        for name, hit in K.classes_of(a, K.CUR, proposer, ops, p).items():
            seen[name] += bool(hit)
    assert all(seen.values()), seen


def test_slashable_data_is_the_references_text():
    """double votes and surround votes at their boundaries, through oracle.spec, and the model's wrapper decides nothing"""
    from oracle import spec
    d = lambda s, t, tag=0: B.att_data(source_epoch=s, target_epoch=t, block_root=bytes([tag]) * 32)  # noqa: E731
    cases = [(d(3, 5), d(3, 5), False),            # the same data
             (d(3, 5), d(3, 5, 1), True),          # double vote: same target, other data
             (d(3, 5), d(4, 5), True),             # ... other source
             (d(2, 6), d(3, 5), True),             # surround
             (d(3, 5), d(2, 6), False),            # surrounded: the argument order matters
             (d(3, 6), d(3, 5), False),            # equal sources
             (d(2, 5), d(3, 5, 1), True),          # equal targets: a double vote whatever the sources
             (d(2, 6), d(3, 6, 1), True),
             (d(2, 6), d(3, 7), False)]
    for d1, d2, want in cases:
        assert B.slashable_data(d1, d2) is want
    c1, c2 = spec.Checkpoint(2, spec.Root(bytes(32))), spec.Checkpoint(6, spec.Root(bytes(32)))
    c3, c4 = spec.Checkpoint(3, spec.Root(bytes(32))), spec.Checkpoint(5, spec.Root(bytes(32)))
    mk = lambda s, t: spec.AttestationData(slot=0, index=0, beacon_block_root=spec.Root(bytes(32)), source=s, target=t)  # noqa: E731
    assert spec.is_slashable_attestation_data(mk(c1, c2), mk(c3, c4)) and not spec.is_slashable_attestation_data(mk(c3, c4), mk(c1, c2))


@pytest.mark.parametrize("limit,c0,beyond,n_eject", [(1, 0, False, 3), (4, 3, False, 6), (4, 4, False, 5), (4, 2, True, 9),
                                                     (3, 5, True, 7), (2, 0, True, 1)])
def test_initiate_validator_exit_is_the_registry_updates_ejection(limit, c0, beyond, n_eject):
    """exit_queue_case's ejected validators, handed over as voluntary exits in index order, get the epochs the ejection gives"""
    cur = 400
    a, rp = M.exit_queue_case(200, cur, limit, c0, beyond, n_eject, interleave=True)
    want, st = M.registry_updates_sequential(a, cur, cur - 2, rp)
    ejected = np.flatnonzero(want["ext"] != a["ext"])
    assert ejected.size == n_eject == st["n_ejected"]
    p = B.BlockParams(min_per_epoch_churn_limit=limit)
    got, status, bst = B.block_operations_sequential(a, cur, 0, [B.voluntary_exit(int(v), cur) for v in ejected], p)
    assert status == [0] * n_eject
    assert np.array_equal(got["ext"], want["ext"]) and np.array_equal(got["wdr"], want["wdr"])
    assert (bst["first_exit_epoch"], bst["last_exit_epoch"], bst["churn_limit"]) == (st["first_exit_epoch"], st["last_exit_epoch"],
                                                                                    st["churn_limit"])


def test_the_statuses_in_their_order():
    p = K.params()
    a = M.blank_registry(8, p)
    a["act"][1] = K.CUR + 1
    a["act"][2] = K.CUR - 255
    a["ext"][3], a["wdr"][3] = K.CUR + 9, K.CUR + 9 + 256
    a["slashed"][4], a["ext"][4], a["wdr"][4] = 1, K.CUR + 5, K.CUR + 8000
    d1, d2 = B.double_vote(K.CUR - 1)
    root = lambda x: bytes([x]) * 32  # noqa: E731
    ops = [B.attester_slashing(d1, d1, [0], [0]), B.attester_slashing(d1, d2, [], [0]), B.attester_slashing(d1, d2, [1, 1], [1]),
           B.attester_slashing(d1, d2, [0, 8], [0]), B.attester_slashing(d1, d2, [0], [0], sig=False),
           B.attester_slashing(d1, d2, [0], [5]), B.attester_slashing(d1, d2, [4], [4]),
           B.proposer_slashing(1, 0, root(1), 2, 0, root(2)), B.proposer_slashing(1, 0, root(1), 1, 5, root(2)),
           B.proposer_slashing(1, 0, root(1), 1, 0, root(1)), B.proposer_slashing(1, 9, root(1), 1, 9, root(2)),
           B.proposer_slashing(1, 4, root(1), 1, 4, root(2)), B.proposer_slashing(1, 0, root(1), 1, 0, root(2), sig=False),
           B.voluntary_exit(8, 0), B.voluntary_exit(1, 0), B.voluntary_exit(3, 0), B.voluntary_exit(0, K.CUR + 1),
           B.voluntary_exit(2, 0), B.voluntary_exit(0, K.CUR, sig=False), B.voluntary_exit(0, K.CUR),
           B.voluntary_exit(0, K.CUR)]
    want = [B.NOT_SLASHABLE_DATA, B.BAD_INDICES, B.BAD_INDICES, B.BAD_INDICES, B.BAD_SIGNATURE, B.NOBODY_SLASHABLE,
            B.NOBODY_SLASHABLE, B.HEADER_MISMATCH, B.HEADER_MISMATCH, B.HEADER_MISMATCH, B.BAD_INDICES,
            B.PROPOSER_NOT_SLASHABLE, B.BAD_SIGNATURE, B.BAD_INDICES, B.NOT_ACTIVE, B.ALREADY_EXITING, B.EXIT_EPOCH_FUTURE,
            B.TOO_YOUNG, B.BAD_SIGNATURE, B.OK, B.ALREADY_EXITING]
    for form in (B.block_operations_sequential, B.block_operations_closed_form):
        out, status, st = form(a, K.CUR, 7, ops, p)
        assert status == want and st["n_invalid"] == len(ops) - 1
        assert all(np.array_equal(out[k], a[k]) for k in M.FIELDS)


def test_the_refusals():
    p = K.params()
    a = M.blank_registry(8, p)
    d1, d2 = B.double_vote(K.CUR - 1)
    ops = [B.attester_slashing(d1, d2, [1, 2], [1, 2])]
    for form in (B.block_operations_sequential, B.block_operations_closed_form):
        for cur, proposer, q, big in ((K.CUR, 8, p, False), (K.CUR, 0, K.params(min_slashing_penalty_quotient=0), False),
                                      (K.CUR, 0, K.params(whistleblower_reward_quotient=0), False),
                                      (M.FAR - 8192, 0, p, False), (K.CUR, 0, K.params(min_validator_withdrawability_delay=M.FAR - K.CUR - 5), False),
                                      (K.CUR, 0, p, True)):
            b = M.copy_registry(a)
            if big:
                b["eff"][:] = 2**63
            with pytest.raises(ValueError):
                form(b, cur, proposer, ops, q)
