"""The synchronous BLS calls on ONE handle, each after another call has left the shared workspace at a different size.

pe_pairing_check, pe_verify_resident and the fallback of pe_batch_verify lay their scratch out in d_bls; pe_batch_verify in d_batch;
the three phases of pe_verify_signatures in d_verify, one after the other from offset 0.  The edge tests of each call run it on a
handle of its own kind; here one handle runs them interleaved, small after large and large after small, and every verdict,
status and aggregate equals what a fresh handle returns for that call alone -- and the models' answers, through the helpers of
the calls' own tests.
"""
import numpy as np
import pytest

from oracle.g1 import R_ORDER
from tests import test_gpu_batch_verify as tb
from tests import test_gpu_bls_verify as tp
from tests import test_gpu_verify_resident as tr
from tests import test_gpu_verify_signatures as ts
from tests import verify_resident_model as rm
from tests.test_gpu_verify_resident import tool  # noqa: F401  (the fixture: a handle that makes G2 points)

pytestmark = pytest.mark.gpu


def _pair_groups(verdicts):
    """Groups of two pairs e(G1, s G2) e(G1, (t - s) G2): valid where t = 0."""
    return [(tp._points([1, 1], [tp.FULL + g, (1 - v - tp.FULL - g) % R_ORDER]), v) for g, v in enumerate(verdicts)]


def _resident(engine_factory, tool):
    """A handle with a 3-group resident signed aggregate; -> (world, message points, point_of_row, the model's verdicts)."""
    w = tr._world(engine_factory)
    rows, model = tr._standard(w, 3)
    atts, arena, sigs, msg_of_row = rows.build(tool)
    assert tr._signed(w["e"], atts, arena, sigs)["n_groups"] == 3
    return w, tr._msg_points(tool), msg_of_row, [rm.decide(m)[0] for m in model]


def _batch_pool(n):
    dlogs = [(3 + 2 * i, 5 + 7 * i, (3 + 2 * i) * (5 + 7 * i) % R_ORDER) for i in range(n)]
    return [tb._group(*d) for d in dlogs], dlogs


def _signatures(e, sizes, spoil=None):
    case = ts.Case(sizes)
    if spoil is not None:
        case.spoil(spoil)
    n = len(case.members)
    verdict, status, group, _ = case.run(e, ts._scalars(n, seed=n), k=3)   # (asserts the model's answer, aggregates included)
    return verdict, status, group, case.agg.tobytes()


def test_interleaved_calls_on_one_handle_equal_fresh_handles(engine_factory, tool):  # noqa: F811
    w, msgs, msg_of_row, want_resident = _resident(engine_factory, tool)
    e = w["e"]
    fresh = lambda: engine_factory(device=0)
    groups, dlogs = _batch_pool(9)
    forged, forged_dlogs = tb._spoil(groups, dlogs, [6])

    def pairing(x, verdicts):
        a, b, off, want = tp._call(_pair_groups(verdicts))
        got = x.pairing_check(a, b, off).tolist()
        assert got == want.tolist()
        return got

    def batch(x, gs, ds, c=None):
        if c is not None:
            x._profile_batch_set_chunk(c)
        return tb._check(x, gs, ds, tb._scalars(len(gs), seed=len(gs)))   # (asserts the model's and the per-group path's answer)

    got = []
    got.append(pairing(e, [1]))                                                      # 1
    got.append(e.verify_resident(msgs, point_of_row=msg_of_row, apply=False).tolist())  # 2
    got.append(pairing(e, [1, 0, 1, 0, 0]))                                          # 3: d_bls grows under the resident layout
    got.append(e.verify_resident(msgs, point_of_row=msg_of_row, apply=False).tolist())  # 4: ... which is bound again, smaller
    got.append(batch(e, groups[:2], dlogs[:2]))                                      # 5
    got.append(batch(e, forged, forged_dlogs, c=4))                                  # 6: the fallback reuses d_bls (verify_pairs_run)
    got.append(_signatures(e, [1, 3]))                                               # 7
    got.append(_signatures(e, [5, 1, 4], spoil=7))                                   # 8: sums, locate and aggregate re-bind d_verify
    assert got[1] == got[3] == want_resident and set(want_resident) == {0, 1}
    assert got[5][0] == [0 if i == 6 else 1 for i in range(9)] and got[5][1]["rechecked"] > 0
    assert got[7][0] == [0 if j == 7 else 1 for j in range(10)] and got[7][2] == [1, 1, 0]

    w2, msgs2, msg_of_row2, _ = _resident(engine_factory, tool)
    alone = [
        pairing(fresh(), [1]),
        w2["e"].verify_resident(msgs2, point_of_row=msg_of_row2, apply=False).tolist(),
        pairing(fresh(), [1, 0, 1, 0, 0]),
        None,
        batch(fresh(), groups[:2], dlogs[:2]),
        batch(fresh(), forged, forged_dlogs, c=4),
    ]
    alone[3] = alone[1]
    for sizes, spoil in (([1, 3], None), ([5, 1, 4], 7)):
        x = fresh()
        x.set_validators(np.full(ts.N_VAL, 32 * 10 ** 9, dtype=np.uint64), np.ones(ts.N_VAL, dtype=np.uint8),
                         tr.synth.registry_points(x, ts.N_VAL))
        alone.append(_signatures(x, sizes, spoil))
    assert got == alone
