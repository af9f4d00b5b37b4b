"""CPU: the claim pe_prune rests on, held to the oracle without the engine -- re-rooting the block table at the finalized
root and remapping the latest messages (tests/prune_model.py) is unobservable to get_head.

L0 (oracle/spec.py, the reference's own text) computes the head and every block's weight on the UNPRUNED store; the C oracle
computes them on the model's pruned arrays.  The heads must be the same root and the weights of every kept block equal."""
import os

import numpy as np
import pytest

from oracle import cport, spec
from tests import prune_model as pm
from tests.scenario import new_world, slot_committee_members
from tests.test_oracle_cport import flatten_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_world(seed, n_blocks):
    rng = np.random.default_rng(seed)
    w = new_world(64, "minimal", PROPOSER_SCORE_BOOST=int(rng.choice([40, 70])))
    st = w.store.checkpoint_states[w.store.justified_checkpoint]
    for i, v in enumerate(st.validators):  # mixed balances, a few inactive / slashed validators
        v.effective_balance = int(rng.integers(16, 33)) * 10**9
        if i % 13 == 0:
            v.exit_epoch = 0
        if i % 17 == 0:
            v.slashed = True
    roots = [w.store.justified_checkpoint.root]
    slot = 0
    while len(roots) < n_blocks:
        slot += 1
        w.tick_to_slot(slot, offset=int(rng.integers(0, spec.SECONDS_PER_SLOT)))
        for _ in range(int(rng.integers(1, 3))):  # one or two blocks per slot: side branches off recent blocks
            parent = roots[int(rng.integers(max(0, len(roots) - 4), len(roots)))]
            if w.store.blocks[parent].slot < slot and len(roots) < n_blocks:
                roots.append(w.block(parent, slot, graffiti=bytes([len(roots)])))
        a_slot = slot - 1
        cand = [r for r in roots[-8:] if w.store.blocks[r].slot <= a_slot]
        if cand:  # about half of the slot's committee votes: some validators never get a message
            voters = slot_committee_members(w.store, a_slot)
            w.vote(voters[: 1 + len(voters) // 2], cand[int(rng.integers(0, len(cand)))], a_slot)
        if slot == 9:
            w.store.equivocating_indices.update(slot_committee_members(w.store, 2)[:3])
    return w, roots, rng


def _descendants(parent, i):
    keep = {i}
    for k in range(i + 1, len(parent)):
        if int(parent[k]) in keep:
            keep.add(k)
    return sorted(keep)


@pytest.mark.parametrize("seed,n_blocks", [(0, 48), (1, 48), (2, 33), (3, 48), (4, 17), (5, 48), (6, 40), (7, 48)])
def test_pruned_arrays_give_the_unpruned_head_and_weights(seed, n_blocks):
    w, _, rng = _random_world(seed, n_blocks)
    store = w.store
    r_list, idx, parent, leaf_ok, root_bytes, vote, bal, flags, boost = flatten_store(store)
    assert len(r_list) == n_blocks <= 48 and len(bal) == 64
    assert (vote == pm.NONE32).any() and (flags & 4).any()
    # a finalized root with something beside and above it, and a justified root in its subtree
    inner = [i for i in range(1, n_blocks) if len(_descendants(parent, i)) >= 3]
    fin = int(inner[int(rng.integers(0, len(inner)))])
    sub = _descendants(parent, fin)
    just = int(sub[int(rng.integers(0, min(len(sub), 3)))])
    state = store.checkpoint_states[store.justified_checkpoint]
    # epoch GENESIS_EPOCH: filter_block_tree's leaf test passes for every block, so the whole subtree competes
    store.finalized_checkpoint = spec.Checkpoint(spec.GENESIS_EPOCH, r_list[fin])
    store.justified_checkpoint = spec.Checkpoint(spec.GENESIS_EPOCH, r_list[just])
    store.checkpoint_states[store.justified_checkpoint] = state
    head_l0 = spec.get_head(store)

    m = pm.index_map(parent, fin)
    keep, parent_new = pm.prune_parent(parent, m)
    assert [int(i) for i in keep] == sub and m[fin] == 0 and parent_new[0] == pm.NONE32
    assert all(parent_new[k] < k for k in range(1, len(keep)))          # still parents first
    vote_new, remapped, orphaned = pm.remap_votes(vote, m)
    assert orphaned == int(np.count_nonzero((vote != pm.NONE32) & ~np.isin(vote, keep)))
    assert remapped + orphaned + int(np.count_nonzero(vote == pm.NONE32)) == len(vote)  # fin > 0: every kept index moves
    boost_new = pm.NONE32 if boost == pm.NONE32 or m[boost] == pm.PRUNED else int(m[boost])
    # the C oracle knows "no message" only: an orphaned message weighs on nothing, which is what PRUNED means to k_votes
    vote_c = np.where(vote_new == pm.PRUNED, pm.NONE32, vote_new).astype(np.uint32)
    head, weights = cport.get_head(parent_new, leaf_ok[keep], root_bytes[keep], vote_c, bal, flags, int(m[just]), boost_new,
                                   slots_per_epoch=spec.SLOTS_PER_EPOCH, boost_percent=spec.PROPOSER_SCORE_BOOST)
    assert r_list[int(keep[head])] == head_l0
    for k, i in enumerate(keep):
        assert int(weights[k]) == spec.get_latest_attesting_balance(store, r_list[int(i)]), (k, int(i))


def test_second_prune_is_the_identity_and_left_over_marks_stay():
    parent = np.array([pm.NONE32, 0, 1, 1, 2, 3, 2, 6], dtype=np.uint32)
    m = pm.index_map(parent, 2)
    assert m.tolist() == [pm.PRUNED, pm.PRUNED, 0, pm.PRUNED, 1, pm.PRUNED, 2, 3]
    vote = np.array([0, 3, 2, 4, 7, pm.NONE32, pm.PRUNED, 9], dtype=np.uint32)  # 9: no index of the table, left alone
    out, remapped, orphaned = pm.remap_votes(vote, m)
    assert out.tolist() == [pm.PRUNED, pm.PRUNED, 0, 1, 3, pm.NONE32, pm.PRUNED, 9] and (remapped, orphaned) == (3, 2)
    keep, parent_new = pm.prune_parent(parent, m)
    assert parent_new.tolist() == [pm.NONE32, 0, 0, 2]
    m2 = pm.index_map(parent_new, 0)
    assert m2.tolist() == [0, 1, 2, 3]
    out2, r2, o2 = pm.remap_votes(out, m2)
    assert out2.tolist() == out.tolist() and (r2, o2) == (0, 0)


def test_remap_kernel_is_built_without_scratch():
    """The library's build writes the compiler's resource usage of the fork-choice kernels; k_votes_remap must not spill."""
    import re
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "fc_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("the library has not been built here (make writes the log)")
    blk = [b for b in re.split(r"remark: [^\n]*Function Name: ", open(log).read())[1:] if "k_votes_remap" in b.split()[0]]
    assert len(blk) == 1
    assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk[0]).group(1) == "0"
    assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk[0]).group(1)) <= 64   # static LDS: the two counters
