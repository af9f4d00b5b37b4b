"""-m gpu: get_head's tree kernel against the C oracle at the edges of its launch shapes (fc_kernels.hip: k_tree<1024, 1 / 2 /
4 / 8>, the lean <512, 4> / <512, 8> of pipelined calls, k_pair_union_tree of streaming steps), on the structured trees and
cases of tests/tree_shapes.py: the justified root inside the tree, a heavier subtree outside it, ties at non-zero weights
that only the root rank breaks, a boost that turns a tie into a win, dead heavy subtrees, thousands of children under one
parent.  Votes go in through on_attestation; everything is compared with ==.  Then k_votes' ragged tails.

What these cases catch, measured on the MI355X against single-line mutants of tree_body (never committed):
  scan2's store `i <= n` -> `i < n`        every case at 1023, 1025, 2047, 2049, 4095, 4097, 8191 (weights and heads)
  scan2's full-shape store removed         every case at 1024, 2048, 4096, 8192, and all six paired-tree tests
  rank term dropped from `best`            star_no_votes, star_tie, late_fork_tie at all 11 sizes, comb_three_ties at 7
  `i < j_end` -> `<=` in the final test     two_subtrees_justified_leaf and comb_three_ties at all 11 sizes
  `i > justified_pos` -> `>=` (g_item)      two_subtrees_justified_B and comb_three_ties at all 11 sizes, all paired tests
  viability bit dropped from the final     nothing, and nothing can: a non-viable item has par = NONE32, so it is never a
  test; `<= j_end` in the g_item line      best child, its g is 1 and its count never 0; the other only touches counters
                                           at positions >= j_end, which the final test does not read
(tests/test_gpu_ffg_sums.py: stride halved fails every n >= 4096, slashed test removed every n >= 63.)"""
import functools
import hashlib

import numpy as np
import pytest

import pos_evolution_amd.synth as synth
from oracle import cport
from tests import helpers as H
from tests import tree_shapes as TS

pytestmark = pytest.mark.gpu
NONE32 = 0xFFFFFFFF
SIZES = [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]
N32 = 4096
N_COMM = 64


@functools.lru_cache(maxsize=None)
def _references(n):
    """[(case, oracle head, oracle weights)] of one size: computed once, shared, never written to."""
    bal, flags = TS.registry(N32)
    out = []
    for case in TS.cases(n, N32):
        t = case.tree
        head_o, w_o = cport.get_head(t.parent.copy(), case.leaf_ok, t.roots, case.vote, bal, flags, case.justified, case.boost)
        TS.check_claims(case, head_o, [int(x) for x in w_o], bal, flags)
        w_o.setflags(write=False)
        out.append((case, head_o, w_o))
    return out


@pytest.fixture(scope="module")
def shape_engine(engine_factory):
    e = engine_factory(max_committee_tables=4)
    bal, flags = TS.registry(N32)
    e.store_init(0, 0, b"\x01" * 32)
    e.set_validators(bal, flags)
    return e, synth.random_committees(N32 + TS.N_BIG, N_COMM, 7)


def _load_case(e, comm, case, loaded=None):
    """The case's tree, leaf tests, votes (through on_attestation), justified root and boost in the engine's store.
    `loaded`: what the previous case left there.  Loading a tree is one ABI call per block, so a case that differs from
    the previous one only by MORE votes or by the boost keeps the store and hands in the new votes alone (a validator's
    first message is recorded whatever the epoch; nothing is ever taken back, hence the superset rule)."""
    t = case.tree
    jroot = t.roots[case.justified].tobytes()
    good, bad, fin = (1, jroot), (2, jroot), (0, t.roots[0].tobytes())
    prev = loaded.get("case") if loaded is not None else None
    keep = (prev is not None and prev.tree is t and prev.justified == case.justified
            and np.array_equal(prev.leaf_ok, case.leaf_ok)
            and np.array_equal(case.vote[prev.vote != NONE32], prev.vote[prev.vote != NONE32]))
    if keep:
        fresh = np.where(prev.vote == NONE32, case.vote, NONE32).astype(np.uint32)
        assert np.array_equal(H.install_votes(e, t, comm, fresh), fresh)
    else:
        H.load_tree(e, t, [((good if ok else bad), fin) for ok in case.leaf_ok])
        assert np.array_equal(H.install_votes(e, t, comm, case.vote), case.vote)
        e.set_checkpoints(good, fin)    # epoch 1 != GENESIS: the leaf test is live; finalized stays at genesis
    e.set_proposer_boost(t.roots[case.boost].tobytes() if case.boost != NONE32 else bytes(32))
    assert np.array_equal(e.latest_messages()[1], case.vote)
    if loaded is not None:
        loaded["case"] = case
        loaded["loads"] = loaded.get("loads", 0) + (0 if keep else 1)


@pytest.mark.parametrize("n", SIZES)
def test_get_head_at_the_shape_edges_vs_oracle(shape_engine, n):
    """Every case of tests/tree_shapes.py at one block count: per-block weights and head of the synchronous call
    (k_votes<2>, k_tree<1024, PER>) and of a call inside a plain and inside a lagged pipeline (k_votes<1>; the lean
    k_tree<512, 4> / <512, 8> from 1025 to 4096 blocks) against cport.get_head with the case's justified and boost
    index.  All mismatches of a size are reported together.
    Case 6's middle tie lies where the halves of the launch shape meet at 1023 / 1024, 2047 / 2048, 4095 / 4096 and
    8191 / 8192 blocks; at 1025, 2049 and 4097 the comb's spine ends before the middle of the next shape, and the tie sits
    at the spine's middle level instead (tree_shapes.comb_tie_levels)."""
    e, comm = shape_engine
    wrong, loaded = [], {}
    for case, head_o, w_o in _references(n):
        want = case.tree.roots[head_o].tobytes()
        _load_case(e, comm, case, loaded)
        if not np.array_equal(e.get_weights(), w_o):
            wrong.append((case.name, "sync weights"))
        if e.get_head() != want:
            wrong.append((case.name, "sync head"))
        for lagged in (False, True):
            with e.pipeline(lagged=lagged):
                got = e.get_head()
            e.drain()
            if got != want:
                wrong.append((case.name, "lagged" if lagged else "pipelined", "head"))
            if not np.array_equal(e.last_weights(), w_o):
                wrong.append((case.name, "lagged" if lagged else "pipelined", "weights"))
    assert loaded["loads"] == 7          # star x 3 and late_fork x 2 share a store
    assert not wrong, "%d blocks: " % n + "; ".join(" ".join(w) for w in wrong)


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("name", ["two_subtrees_justified_B", "comb_three_ties"])
@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_paired_tree_of_a_streaming_step_vs_oracle(shape_engine, n, name):
    """The head of a streaming step over rows in device memory is held back and runs as block 0 of k_pair_union_tree<1024, 1>
    / <512, 4, true> / <512, 8, true> beside the bitfield union of the NEXT step's aggregate (engine_pair.cpp): head and
    per-block weights of that launch against the oracle, at the block counts that fill those shapes exactly.
    The profile counts the bracket around the pair, which also covers its fall-back of two separate launches; that the
    pair itself ran follows from launch_pair_union_tree (pair_kernels.hip), which declines only an aggregate without
    groups or a tree beyond 4096 blocks -- both asserted here -- and from the stand-alone tree and votes kernels counting
    zero launches."""
    import pos_evolution_amd as pea

    e, comm = shape_engine
    case, head_o, w_o = next(r for r in _references(n) if r[0].name == name)
    _load_case(e, comm, case)
    n_val, spe = N32 + TS.N_BIG, 32
    ep = int(case.tree.slot.max()) // spe + 3                      # install_votes left the clock at this epoch's start
    off, mem = e.compute_committees(ep, hashlib.sha256(b"shapes").digest(), n_val, 32, 10)
    anchor = synth.Tree(case.tree.roots[:1], case.tree.parent[:1], case.tree.slot[:1])
    steps = []
    for k in range(2):   # rows that are only ever aggregated (no on_attestation: the votes stay the case's)
        atts, arena, bit_rows = synth.epoch_attestations(synth.Committees(off, mem), anchor, ep, spe, seed=k, density=0.9,
                                                         parts=2)
        ta, tb = _dev(atts), _dev(arena)
        steps.append((pea.DeviceRows(ta.data_ptr(), len(atts), keep=ta), pea.DeviceArena(tb.data_ptr(), tb.numel(), keep=tb),
                      sum(int(np.sum(b)) for b in bit_rows)))
    e.profile_enable(True)
    e.profile_reset()
    with e.pipeline(lagged=True):
        agg0 = e.aggregate(packed=steps[0][:2])
        head = e.get_head_async()                                  # held: votes + tree wait for the next aggregate
    with e.pipeline(lagged=True):
        agg1 = e.aggregate(packed=steps[1][:2])                    # ... and go out paired with its row kernels
    e.drain()
    ln = {k: v["launches"] for k, v in e.profile().items()}
    e.profile_enable(False)
    assert bytes(head) == case.tree.roots[head_o].tobytes()
    assert np.array_equal(e.last_weights(), w_o)
    for agg, (_, _, n_set) in zip((agg0, agg1), steps):
        assert agg["n_groups"] == 32 and int(agg["count"].sum()) == n_set   # parts of a committee are disjoint
    assert n <= 4096 and ln["pair_union_tree"] == 1 and ln["pair_members_votes"] == 1, ln
    assert ln["tree"] == 0 and ln["votes"] == 0 and ln["bits_union"] == 1, ln


# ---------------------------------------------------------------- k_votes tails
def _tail_world(n_val):
    tree = synth.random_tree(40, 40, "bushy")
    bal = synth.balances(n_val, 40, True)
    flags = synth.validator_flags(n_val, 40, inactive_frac=0.005, slashed_frac=0.01)
    vote = synth.zipf_votes(n_val, 40, 40, recent=8)
    # the ragged tail counts, with balances nothing else has
    bal[-3:] = np.array([77, 78, 79], dtype=np.uint64) * np.uint64(10**9)
    flags[-3:] = 1
    vote[-3:] = [39, 38, 39]
    return tree, bal, flags, vote, synth.random_committees(n_val, N_COMM, 40)


@pytest.mark.parametrize("n_val", [200003, (1 << 20) + 1])
def test_votes_ragged_tail_vs_oracle(engine_factory, n_val):
    """k_votes where the validator count is no multiple of 4.  200003: 50001 quads on the capped grid of 64 workgroups,
    the ragged last quad is the SECOND in-flight quad (u = 1) of its lane.  2^20 + 1: 128 workgroups x 2 quads per lane cover
    2^20 exactly, the one validator left is a second trip of lane 0 alone."""
    tree, bal, flags, vote, comm = _tail_world(n_val)
    e = engine_factory()
    H.load_tree(e, tree)
    e.set_validators(bal, flags)
    installed = H.install_votes(e, tree, comm, vote)
    assert (installed[-3:] == vote[-3:]).all()
    head_o, w_o = cport.get_head(tree.parent.copy(), np.ones(40, dtype=np.uint8), tree.roots, installed, bal, flags, 0, NONE32)
    assert np.array_equal(e.get_weights(), w_o)
    assert e.get_head() == tree.roots[head_o].tobytes()
    with e.pipeline():                 # k_votes<1>: one quad in flight
        assert e.get_head() == tree.roots[head_o].tobytes()
    e.drain()
    assert np.array_equal(e.last_weights(), w_o)


def test_votes_ragged_tail_with_vote_expiry_vs_oracle(engine_factory):
    """The vote-expiry variant (vote_expiry_slots = 20) over the same 200003 validators: the slot table is read by the same
    ragged quads.  The clock stands 40 slots after the attested epoch's start: votes cast in its first 20 slots (0 .. 19) have
    expired."""
    n_val, spe, eta = 200003, 32, 20
    tree, bal, flags, vote, comm = _tail_world(n_val)
    E = int(tree.slot.max()) // spe + 1
    now = E * spe + 40
    e = engine_factory(vote_expiry_slots=eta)
    H.load_tree(e, tree)
    e.set_validators(bal, flags)
    installed = H.install_votes(e, tree, comm, vote, now_slot=now)
    cps = N_COMM // spe
    slot_of = np.zeros(n_val, dtype=np.int64)
    for c in range(N_COMM):
        slot_of[comm.members[comm.offsets[c]:comm.offsets[c + 1]]] = E * spe + c // cps
    alive = installed.copy()
    alive[slot_of + eta < now] = NONE32
    n_alive, n_inst = int((alive != NONE32).sum()), int((installed != NONE32).sum())
    assert n_inst // 4 < n_alive < 3 * n_inst // 4
    head_o, w_o = cport.get_head(tree.parent.copy(), np.ones(40, dtype=np.uint8), tree.roots, alive, bal, flags, 0, NONE32)
    assert np.array_equal(e.get_weights(), w_o)
    assert e.get_head() == tree.roots[head_o].tobytes()
