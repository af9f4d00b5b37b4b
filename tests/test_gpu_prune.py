"""-m gpu: pe_prune -- the block table re-rooted at the finalized root, the latest messages remapped on the device
(k_votes_remap), held to the C oracle on the test's own UNPRUNED arrays, to tests/prune_model.py element for element, and to
a never-pruned twin handle fed the same calls."""
import hashlib

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import cport
from pos_evolution_amd import _abi
from pos_evolution_amd.engine import EngineError, _ptr, _root
from tests import prune_model as pm

pytestmark = pytest.mark.gpu

NONE32, PRUNED = pm.NONE32, pm.PRUNED
SPE, N_COMM = 32, 64
ZERO = bytes(32)
RR, RES = pea.ROWS_RESIDENT, pea.RESIDENT


# ---------------------------------------------------------------- helpers
def _status(fn, *a, **k):
    try:
        fn(*a, **k)
    except EngineError as err:
        return err.status
    return 0


def _set_lm(e, epoch, block, slot=None):
    ep = np.ascontiguousarray(epoch, dtype=np.uint64)
    bi = np.ascontiguousarray(block, dtype=np.uint32)
    sl = None if slot is None else np.ascontiguousarray(slot, dtype=np.uint32)
    e._check(e._lib.pe_set_latest_messages(e._h, ep.size, _ptr(ep), _ptr(bi), _ptr(sl)))


def _checkpoints_by_hand(e, root):
    """finalized = justified = best_justified = (0, root): epoch GENESIS_EPOCH keeps every leaf viable.  (best_justified
    too: pe_prune refuses while a known best-justified root lies outside the finalized subtree.)"""
    e.set_checkpoints((0, root), (0, root))
    e._check(e._lib.pe_set_best_justified(e._h, 0, _root(root)))


def _lm_slots(e):
    out = np.zeros(max(e.num_validators, 1), dtype=np.uint32)
    e._check(e._lib.pe_get_latest_message_slots(e._h, _ptr(out), e.num_validators))
    return out[:e.num_validators]


def _eq(a, b):
    """export_state dictionaries (nested dicts / tuples / arrays / scalars) compared value for value."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_eq(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _dev_packed(atts, arena):
    ta, tb = _dev(atts), _dev(arena)
    return pea.DeviceRows(ta.data_ptr(), len(atts), keep=ta), pea.DeviceArena(tb.data_ptr(), tb.numel(), keep=tb)


class Full:
    """The test's own, never pruned arrays: every block ever inserted, in insertion order."""

    def __init__(self, tree):
        self.roots = [tree.roots[i].tobytes() for i in range(len(tree.parent))]
        self.parent = [int(p) for p in tree.parent]
        self.slot = [int(s) for s in tree.slot]
        self.pj = [(0, ZERO)] * len(self.roots)
        self.pf = [(0, ZERO)] * len(self.roots)
        self.idx = {r: i for i, r in enumerate(self.roots)}

    def add(self, root, parent_idx, slot, pj=(0, ZERO), pf=(0, ZERO)):
        self.idx[root] = len(self.roots)
        self.roots.append(root); self.parent.append(parent_idx); self.slot.append(slot); self.pj.append(pj); self.pf.append(pf)
        return len(self.roots) - 1

    def tree(self):
        return synth.Tree(np.frombuffer(b"".join(self.roots), dtype=np.uint8).reshape(-1, 32).copy(),
                          np.array(self.parent, dtype=np.uint64).astype(np.uint32), np.array(self.slot, dtype=np.uint64))

    def head(self, e, vote_block, bal, flags):
        """(head root, weights) of the C oracle on the unpruned arrays under the engine's present checkpoints."""
        sc = e.store_scalars()
        j, f = sc["justified"], sc["finalized"]
        leaf = np.array([(j[0] == 0 or self.pj[i] == j) and (f[0] == 0 or self.pf[i] == f) for i in range(len(self.roots))],
                        dtype=np.uint8)
        t = self.tree()
        vb = np.where(vote_block == PRUNED, NONE32, vote_block).astype(np.uint32)  # the oracle knows "no message" only
        h, w = cport.get_head(t.parent, leaf, t.roots, vb, bal, flags, self.idx[j[1]], NONE32)
        return self.roots[h], w


def _check_head(e, full, vote_block, bal, flags):
    want, w_o = full.head(e, vote_block, bal, flags)
    assert e.get_head() == want
    w = e.get_weights()
    for i in range(e.num_blocks):   # matched by root: every block the handle still holds
        assert int(w[i]) == int(w_o[full.idx[e.block_root_at(i)]]), i
    return want


def _load(e, tree, bal, flags, equiv=()):
    e.store_init(0, int(tree.slot[0]), tree.roots[0].tobytes())
    for i in range(1, len(tree.parent)):
        e.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]))
    e.set_validators(bal, flags)
    if len(equiv):
        e.mark_equivocating(np.asarray(equiv, dtype=np.uint64))


def _world(engine_factory, n_engines=2, n_blocks=300, n_val=1027, seed=5, **cfg):
    """A branchy tree, a mixed registry with a few equivocators, the committee tables of the clock's current epoch E and of
    E - 1, the clock at the last slot of E."""
    tree = synth.random_tree(n_blocks, seed, "branchy")
    bal = synth.balances(n_val, seed, mixed=True)
    flags = synth.validator_flags(n_val, seed, inactive_frac=0.02, slashed_frac=0.02)
    equiv = np.arange(7, n_val, 97)
    E = int(tree.slot.max()) // SPE + 1
    comm = {E - 1: synth.random_committees(n_val, N_COMM, seed), E: synth.random_committees(n_val, N_COMM, seed + 1)}
    engines = []
    for _ in range(n_engines):
        e = engine_factory(**cfg)
        _load(e, tree, bal, flags, equiv)
        for ep, c in comm.items():
            e.set_committees(ep, c.offsets, c.members)
        e.on_tick(((E + 1) * SPE - 1) * 12)
        engines.append(e)
    flags_eq = flags.copy()
    flags_eq[equiv] |= 4
    tip = int(np.argmax(tree.slot))
    return dict(engines=engines, tree=tree, full=Full(tree), bal=bal, flags=flags_eq, E=E, comm=comm, tip=tip,
                vote_epoch=np.zeros(n_val, dtype=np.uint64), vote_block=np.full(n_val, NONE32, dtype=np.uint32))


def _batch(w, epoch, tree, seed, vote_recent, density=0.8):
    return synth.epoch_attestations(w["comm"][epoch], tree, epoch, SPE, seed=seed, density=density, vote_recent=vote_recent)[:2]


def _apply(w, epoch, atts, arena, engines=None):
    """on_attestation_batch over host rows on every engine (equal statuses), then on the test's own latest messages."""
    sts = [e.on_attestation_batch(packed=(atts, arena))[0] for e in (engines or w["engines"])]
    for s in sts[1:]:
        assert np.array_equal(s, sts[0])
    _track(w, epoch, atts, arena, sts[0])
    return sts[0]


def _track(w, epoch, atts, arena, status):
    ok = status == 0
    comm = w["comm"][epoch]
    pos = ((atts["slot"] % SPE) * (N_COMM // SPE) + atts["index"]).astype(np.int64)
    blk = np.array([w["full"].idx[r.tobytes()] for r in atts["beacon_block_root"]], dtype=np.uint32)
    cport.update_latest_messages(comm.offsets[pos][ok], atts["n_bits"][ok], atts["bits_offset"][ok], atts["target_epoch"][ok],
                                 blk[ok], arena, comm.members, w["flags"], w["vote_epoch"], w["vote_block"])


def _kept_tree(full, fin):
    """The finalized root's subtree as a tree of its own (model arrays): rows built over it name kept blocks only."""
    t = full.tree()
    m = pm.index_map(t.parent, fin)
    keep, parent_new = pm.prune_parent(t.parent, m)
    return synth.Tree(t.roots[keep].copy(), parent_new, t.slot[keep].copy()), m, keep


def _finalize_by_hand(w, engines, depth_slot):
    """finalized = justified = (0, the main chain's block at depth_slot)."""
    fin = synth.ancestor_at(w["tree"], w["tip"], depth_slot)
    for e in engines:
        _checkpoints_by_hand(e, w["full"].roots[fin])
    return fin


def _expect_lm(e, full, vote_block):
    """The engine's latest-message blocks the unpruned vote_block array stands for: by root, PRUNED where the block is gone."""
    to_e = np.full(len(full.roots), PRUNED, dtype=np.uint32)
    for i in range(e.num_blocks):
        to_e[full.idx[e.block_root_at(i)]] = i
    out = vote_block.copy()
    named = vote_block < len(full.roots)
    out[named] = to_e[vote_block[named]]
    return out


# ---------------------------------------------------------------- 1. equivalence after a prune
def test_head_weights_statuses_and_messages_after_a_prune(engine_factory):
    w = _world(engine_factory)
    e, twin = w["engines"]
    full, tree, E, tip = w["full"], w["tree"], w["E"], w["tip"]
    bal, flags = w["bal"], w["flags"]
    st = _apply(w, E - 1, *_batch(w, E - 1, tree, 1, vote_recent=300))   # votes all over the tree: ancestors, side branches
    assert (st == 0).sum() > N_COMM // 2
    for x in (e, twin):
        _check_head(x, full, w["vote_block"], bal, flags)
    # finalized and justified advance through on_block: two competing blocks whose post-states carry the new checkpoints
    fin, just = synth.ancestor_at(tree, tip, 4 * SPE), synth.ancestor_at(tree, tip, 5 * SPE)
    pj, pf = (5, full.roots[just]), (4, full.roots[fin])
    new = {}

    def on_block(name, parent_idx):
        root = hashlib.sha256(b"prune-new-" + name).digest()
        slot = full.slot[parent_idx] + 1
        for x in (e, twin):
            x.on_block(root, full.roots[parent_idx], slot, pj, pf)
        new[name] = full.add(root, parent_idx, slot, pj, pf)
        for x in (e, twin):
            _check_head(x, full, w["vote_block"], bal, flags)

    on_block(b"a", tip)
    on_block(b"b", int(tree.parent[tip]))
    assert e.store_scalars()["finalized"] == pf and e.store_scalars()["justified"] == pj
    kept, m, keep = _kept_tree(full, fin)
    _, want_remapped, want_orphaned = pm.remap_votes(w["vote_block"], m)
    stats = e.prune()
    assert stats == dict(blocks_before=len(full.roots), blocks_after=len(keep), votes_remapped=want_remapped,
                         votes_orphaned=want_orphaned)
    assert want_orphaned > 0 and want_remapped > 0 and 1 < len(keep) < len(full.roots)
    assert [e.block_root_at(i) for i in range(e.num_blocks)] == [full.roots[i] for i in keep]
    assert _status(e.last_weights) == _abi.PE_ERR_STATE          # dropped until the next head computation
    _check_head(e, full, w["vote_block"], bal, flags)
    assert e.last_weights().size == len(keep)
    # further blocks and a batch that names kept blocks only
    on_block(b"c", new[b"a"])
    on_block(b"d", new[b"b"])
    on_block(b"e", new[b"c"])
    kept, _, _ = _kept_tree(full, fin)
    for seed in (2, 3):
        st = _apply(w, E, *_batch(w, E, kept, seed, vote_recent=12, density=0.6))
        assert (st == 0).sum() > N_COMM // 2
        heads = {_check_head(x, full, w["vote_block"], bal, flags) for x in (e, twin)}
        assert len(heads) == 1
    ep_e, bl_e = e.latest_messages()
    ep_t, bl_t = twin.latest_messages()
    assert np.array_equal(bl_t, w["vote_block"]) and np.array_equal(ep_t, w["vote_epoch"])   # the twin IS the unpruned store
    assert np.array_equal(ep_e, ep_t)
    assert np.array_equal(bl_e, _expect_lm(e, full, bl_t))
    assert (bl_e == PRUNED).any() and ((bl_e != PRUNED) & (bl_e != NONE32)).any()


# ---------------------------------------------------------------- 2. kernel shape edges
def _shape_tree(kind):
    """-> (parent list, finalized index).  two: the smallest table, the new root a leaf.  chain: the full LDS map, a
    mid-chain root.  sib_mid: the root has siblings before and behind it in insertion order and the three subtrees interleave,
    so the map is no shift.  sib_leaf: the same tree re-rooted at a leaf in the middle of the insertion order."""
    if kind == "two":
        return [NONE32, 0], 1
    if kind == "chain":
        return [NONE32] + list(range(8191)), 8000
    rng = np.random.default_rng(11)
    parent = [NONE32, 0, 1, 1, 1]
    for i in range(5, 40):
        parent.append(int(rng.integers(2, i)))
    if kind == "sib_mid":
        return parent, 3
    leaves = [i for i in range(5, 35) if i not in parent]
    return parent, leaves[len(leaves) // 2]


def _depth_tree(parent, salt):
    slot = [0] * len(parent)
    for i in range(1, len(parent)):
        slot[i] = slot[parent[i]] + 1
    return synth.Tree(synth.make_roots(len(parent), salt), np.array(parent, dtype=np.uint64).astype(np.uint32),
                      np.array(slot, dtype=np.uint64))


GRID_PASS = 256 * 256 * 4   # REMAP_MAX_WG x REMAP_WG x 4 validators: what one pass of launch_votes_remap's capped grid covers
SHAPE_CASES = [(kind, v) for kind in ("two", "sib_mid", "sib_leaf") for v in (1, 3, 5, 255, 1024, 1027)] + \
              [("sib_mid", GRID_PASS + 40003), ("chain", 1027), ("chain", GRID_PASS + 40003)]


@pytest.mark.parametrize("kind,n_val", SHAPE_CASES)
def test_remap_kernel_shape_edges_vs_model(engine_factory, kind, n_val):
    parent, fin = _shape_tree(kind)
    tree = _depth_tree(parent, kind.encode())
    n_old = len(parent)
    expiry = 6 if n_val in (5, 1027) else 0           # vote_slot exists only under the vote-expiry variant
    e = engine_factory(vote_expiry_slots=expiry)
    bal = synth.balances(n_val, 3, mixed=True)
    flags = synth.validator_flags(n_val, 3, inactive_frac=0.02)
    _load(e, tree, bal, flags)
    m = pm.index_map(tree.parent, fin)
    kept = np.nonzero(m != PRUNED)[0]
    anc, a = [], fin
    while parent[a] != NONE32:
        a = parent[a]
        anc.append(a)
    on_path = set(anc)
    side = np.array([i for i in range(n_old) if m[i] == PRUNED and i not in on_path] or anc, dtype=np.uint32)
    rng = np.random.default_rng(n_val + n_old)
    # every validator draws one of: no message, a kept block, a pruned ancestor, a pruned side branch (the ancestors again where
    # the tree has none), a mark left over from an earlier prune; the first five validators take the five kinds in turn
    cat = rng.integers(0, 5, size=n_val)
    cat[:5] = np.arange(5)[:n_val] if n_val < 5 else np.arange(5)
    vote = np.full(n_val, NONE32, dtype=np.uint32)
    vote[cat == 1] = rng.choice(kept, size=int((cat == 1).sum()))
    vote[cat == 2] = rng.choice(np.array(anc, dtype=np.uint32), size=int((cat == 2).sum()))
    vote[cat == 3] = rng.choice(side, size=int((cat == 3).sum()))
    vote[cat == 4] = PRUNED
    epoch = rng.integers(0, 9, size=n_val).astype(np.uint64)
    slots = rng.integers(1, 1000, size=n_val).astype(np.uint32)
    _set_lm(e, epoch, vote, slots)
    ep0, bl0 = e.latest_messages()
    assert np.array_equal(bl0, vote) and np.array_equal(ep0[vote != NONE32], epoch[vote != NONE32])   # (epoch, PRUNED) is accepted
    sl0 = _lm_slots(e)
    _checkpoints_by_hand(e, tree.roots[fin].tobytes())
    want, want_remapped, want_orphaned = pm.remap_votes(vote, m)
    stats = e.prune()
    assert stats == dict(blocks_before=n_old, blocks_after=len(kept), votes_remapped=want_remapped, votes_orphaned=want_orphaned)
    if kind in ("two", "sib_leaf"):
        assert stats["blocks_after"] == 1
    ep1, bl1 = e.latest_messages()
    assert np.array_equal(bl1, want)                      # element for element
    assert np.array_equal(ep1, ep0)                       # vote_key: a message keeps its epoch
    assert np.array_equal(_lm_slots(e), sl0)              # vote_slot under vote_expiry_slots (zeros without)
    if expiry:
        assert np.array_equal(sl0, slots)
    else:   # and the head: the oracle on the unpruned arrays, started at the finalized root
        vb = np.where(vote == PRUNED, NONE32, vote).astype(np.uint32)
        head_o, w_o = cport.get_head(tree.parent, np.ones(n_old, dtype=np.uint8), tree.roots, vb, bal, flags, fin, NONE32)
        assert e.get_head() == tree.roots[head_o].tobytes()
        assert np.array_equal(e.get_weights(), w_o[kept])


# ---------------------------------------------------------------- 3. no-op and idempotence
def test_prune_at_block_zero_changes_nothing_and_a_second_prune_is_that(engine_factory):
    w = _world(engine_factory, n_engines=1, n_blocks=120, n_val=515)
    e, = w["engines"]
    _apply(w, w["E"] - 1, *_batch(w, w["E"] - 1, w["tree"], 1, vote_recent=120))
    before = e.export_state()
    assert e.prune() == dict(blocks_before=120, blocks_after=120, votes_remapped=0, votes_orphaned=0)
    assert _eq(e.export_state(), before)
    fin = _finalize_by_hand(w, [e], 40)
    first = e.prune()
    assert first["blocks_after"] < 120 and first["votes_orphaned"] > 0
    after = e.export_state()
    n = first["blocks_after"]
    assert e.prune() == dict(blocks_before=n, blocks_after=n, votes_remapped=0, votes_orphaned=0)
    assert _eq(e.export_state(), after)
    assert e.block_root_at(0) == w["full"].roots[fin]
    _check_head(e, w["full"], w["vote_block"], w["bal"], w["flags"])


# ---------------------------------------------------------------- 4. a store that outlives its table
def test_twenty_thousand_blocks_through_a_table_of_8192(engine_factory):
    """A chain with a two-block side branch every 50 blocks, one chain block per slot; every block's post-state carries the
    checkpoints of two / one epochs before its own, so on_block keeps raising the finalized checkpoint; prune() every 1024
    blocks.  The C oracle takes all 20 000 blocks, so every comparison is on the full unpruned arrays."""
    n_total, n_val = 20000, 4096
    e = engine_factory()
    # a library without pe_prune fills its table: the test then fails where it should, with PE_ERR_CAPACITY from on_block
    prune = getattr(e, "prune", lambda: None)
    bal = synth.balances(n_val, 9, mixed=True)
    flags = synth.validator_flags(n_val, 9, inactive_frac=0.01)
    roots = synth.make_roots(n_total, b"long")
    anchor = synth.Tree(roots[:1], np.array([NONE32], dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    full = Full(anchor)
    e.store_init(0, 0, full.roots[0])
    e.set_validators(bal, flags)
    e.on_tick(30000 * 12 + 11)
    chain = {0: 0}                       # slot -> full index of the chain's block
    rng = np.random.default_rng(4)
    vote_block = np.full(n_val, NONE32, dtype=np.uint32)     # by FULL index
    k, slot, checks = 1, 0, 0

    def put(parent_idx, s):
        nonlocal k
        ep = s // SPE
        je, fe = max(ep - 1, 0), max(ep - 2, 0)
        pj, pf = (je, full.roots[chain[je * SPE]]), (fe, full.roots[chain[fe * SPE]])
        root = roots[k].tobytes()
        e.on_block(root, full.roots[parent_idx], s, pj, pf)    # raises on PE_ERR_CAPACITY
        i = full.add(root, parent_idx, s, pj, pf)
        k += 1
        assert e.num_blocks < 8192
        if k % 1024 == 0:
            prune()
            assert e.num_blocks < 8192
        return i

    while k < n_total:
        slot += 1
        chain[slot] = put(chain[slot - 1], slot)
        if slot % 50 == 0 and k + 2 <= n_total:
            put(put(chain[slot - 1], slot), slot + 1)
        if k // 2000 > checks:
            checks = k // 2000
            assert np.array_equal(e.latest_messages()[1], _expect_lm(e, full, vote_block))   # the old messages, remapped by root
            # fresh latest messages on the last forty blocks (all descend from the finalized root), a few validators without
            vote_block = rng.integers(len(full.roots) - 40, len(full.roots), size=n_val).astype(np.uint32)
            vote_block[rng.random(n_val) < 0.05] = NONE32
            _set_lm(e, np.full(n_val, slot // SPE, dtype=np.uint64), _expect_lm(e, full, vote_block))
            want, _ = full.head(e, vote_block, bal, flags)
            assert e.get_head() == want
    assert checks == 10 and len(full.roots) == n_total


# ---------------------------------------------------------------- 5. rejections
def test_calls_that_name_pruned_blocks_are_rejected_and_change_nothing(engine_factory):
    w = _world(engine_factory, n_engines=1, n_blocks=200, n_val=515)
    e, = w["engines"]
    full, tree, E = w["full"], w["tree"], w["E"]
    _apply(w, E - 1, *_batch(w, E - 1, tree, 1, vote_recent=200))
    fin = _finalize_by_hand(w, [e], 100)
    kept, m, keep = _kept_tree(full, fin)
    e.prune()
    before = e.export_state()
    # attestations of epoch E whose beacon_block_root is a pruned block (one inserted before the finalized root: an ancestor
    # or a side branch) under a target that is still there
    old = synth.Tree(tree.roots[:fin].copy(), tree.parent[:fin].copy(), tree.slot[:fin].copy())
    atts, arena = _batch(w, E, old, 7, vote_recent=8)
    atts["target_root"] = np.frombuffer(full.roots[fin], dtype=np.uint8)
    st = e.on_attestation_batch(packed=(atts, arena))[0]
    assert (st == _abi.PE_ATT_UNKNOWN_BEACON_BLOCK_ROOT).all()
    assert _eq(e.export_state(), before)
    atts_t = atts.copy()                              # ... and with the pruned block as the target as well
    atts_t["target_root"] = atts_t["beacon_block_root"]
    assert (e.on_attestation_batch(packed=(atts_t, arena))[0] == _abi.PE_ATT_UNKNOWN_TARGET_ROOT).all()
    assert _eq(e.export_state(), before)
    # ... the same rows resident on the device: the device look-up tables were rebuilt
    agg = e.aggregate(packed=_dev_packed(atts, arena))
    st_r = e.on_attestation_batch(packed=(RR, RES), cap=len(atts))[0]
    assert agg["n_groups"] == len(atts) and np.array_equal(st_r, st)
    assert _eq(e.export_state(), before)
    # ... and rows on kept blocks still pass, through both paths (then the store does change)
    atts_k, arena_k = _batch(w, E, kept, 8, vote_recent=8)
    e.aggregate(packed=_dev_packed(atts_k, arena_k))
    st_k = e.on_attestation_batch(packed=(RR, RES), cap=len(atts_k))[0]
    assert (st_k[atts_k["slot"] < (E + 1) * SPE - 1] == 0).all()
    before = e.export_state()
    # on_block under a pruned parent
    gone = int(np.nonzero(m == PRUNED)[0][-1])
    assert _status(e.on_block, hashlib.sha256(b"orphan").digest(), full.roots[gone], full.slot[gone] + 1) == _abi.PE_ERR_UNKNOWN_PARENT
    assert _eq(e.export_state(), before)
    # a justified root outside the finalized subtree: two children of one block
    kids = {}
    for i in range(1, e.num_blocks):
        kids.setdefault(int(before["parent"][i]), []).append(i)
    inner, sib = next(v for v in kids.values() if len(v) >= 2)[:2]
    e.set_checkpoints((0, e.block_root_at(sib)), (0, e.block_root_at(inner)))
    before = e.export_state()
    assert _status(e.prune) == _abi.PE_ERR_STATE
    assert _eq(e.export_state(), before)
    # an unknown finalized root
    e.set_checkpoints((0, e.block_root_at(inner)), (0, hashlib.sha256(b"nowhere").digest()))
    assert _status(e.prune) == _abi.PE_ERR_UNKNOWN_ROOT
    # a handle that exchanges with other ranks
    _checkpoints_by_hand(e, e.block_root_at(inner))
    e.dist_init_custom(0, 1, lambda b, c, s: 0, lambda s_, r_, nb, st_: 0)
    before = e.export_state()
    assert _status(e.prune) == _abi.PE_ERR_STATE
    assert _eq(e.export_state(), before)


def test_prune_before_store_init_is_a_state_error(engine_factory):
    assert _status(engine_factory().prune) == _abi.PE_ERR_STATE


# ---------------------------------------------------------------- 6. pipelines
def test_prune_between_streaming_steps_with_heads_outstanding(engine_factory):
    w = _world(engine_factory)
    e, twin = w["engines"]
    full, tree, E = w["full"], w["tree"], w["E"]
    fin = _finalize_by_hand(w, [e, twin], 150)
    kept, m, keep = _kept_tree(full, fin)
    assert e.set_pipeline_lag(2) is None and twin.set_pipeline_lag(2) is None
    steps = [_batch(w, E - 1, tree, 1, vote_recent=300), _batch(w, E - 1, tree, 2, vote_recent=300),
             _batch(w, E, kept, 3, vote_recent=12), _batch(w, E, kept, 4, vote_recent=12)]
    epochs = [E - 1, E - 1, E, E]
    out = {id(e): [], id(twin): []}

    def step(x, k):
        atts, arena = steps[k]
        with x.pipeline(lagged=True):
            x.aggregate(packed=_dev_packed(atts, arena))
            status, _, _ = x.on_attestation_batch(packed=(RR, RES), cap=len(atts))
            head = x.get_head_async()
        out[id(x)].append((status, head))

    for x in (e, twin):
        step(x, 0)
        step(x, 1)
    stats = e.prune()                     # completes both steps first: their heads are roots of the pre-prune table
    assert stats["blocks_after"] == len(keep) and stats["votes_orphaned"] > 0
    for x in (e, twin):
        step(x, 2)
        step(x, 3)
        x.drain()
    for k in range(4):
        (st_e, head_e), (st_t, head_t) = out[id(e)][k], out[id(twin)][k]
        assert np.array_equal(st_e, st_t), k
        _track(w, epochs[k], *steps[k], st_e)
        want, _ = full.head(twin, w["vote_block"], w["bal"], w["flags"])
        assert bytes(head_e) == bytes(head_t) == want, k
    assert np.array_equal(e.latest_messages()[1], _expect_lm(e, full, twin.latest_messages()[1]))
    _check_head(e, full, w["vote_block"], w["bal"], w["flags"])


# ---------------------------------------------------------------- 7. checkpoint and resume
def test_export_import_round_trips_a_pruned_store(engine_factory):
    w = _world(engine_factory, n_engines=1, n_blocks=200, n_val=515)
    e, = w["engines"]
    full, tree, E = w["full"], w["tree"], w["E"]
    atts, arena = _batch(w, E - 1, tree, 1, vote_recent=200, density=0.5)
    _apply(w, E - 1, atts, arena)
    fin = _finalize_by_hand(w, [e], 100)
    kept, m, keep = _kept_tree(full, fin)
    e.prune()
    st = e.export_state()
    assert (st["lm_block"] == PRUNED).any()
    e2 = engine_factory()
    e2.import_state(st, w["bal"])
    assert _eq(e2.export_state(), st)
    assert e2.get_head() == e.get_head() == _check_head(e, full, w["vote_block"], w["bal"], w["flags"])
    assert np.array_equal(e2.get_weights(), e.get_weights())
    # a later vote of an EQUAL epoch is still refused for a validator whose message was orphaned: every validator attests
    # for E - 1 again, on kept blocks; the messages of E - 1 stay, orphaned ones included, the others are new
    orphaned = st["lm_block"] == PRUNED
    atts2, arena2 = _batch(w, E - 1, kept, 9, vote_recent=12, density=1.0)
    st2 = _apply(w, E - 1, atts2, arena2, engines=[e, e2])
    assert (st2 == 0).sum() > N_COMM // 2
    for x in (e, e2):
        ep, bl = x.latest_messages()
        assert (bl[orphaned] == PRUNED).all() and (ep[orphaned] == E - 1).all()
        assert np.array_equal(bl, _expect_lm(x, full, w["vote_block"])) and np.array_equal(ep, w["vote_epoch"])
    assert (e.latest_messages()[1] != st["lm_block"]).any()        # ... and validators without a message got one
    assert _eq(e2.export_state(), e.export_state())


def test_block_zero_of_a_pruned_store_keeps_its_own_checkpoints_across_import(engine_factory):
    """Block 0 after the prune is a leaf whose post-state checkpoints differ from the store's: not viable, and still the head
    (get_head returns the justified root when nothing below it is viable).  The round trip must reproduce exactly that."""
    e = engine_factory()
    roots = synth.make_roots(3, b"leaf0")
    x, y = hashlib.sha256(b"x").digest(), hashlib.sha256(b"y").digest()
    e.store_init(0, 0, roots[0].tobytes())
    e.add_block(roots[1].tobytes(), roots[0].tobytes(), 40)
    e.add_block(roots[2].tobytes(), roots[1].tobytes(), 170, (3, x), (2, y))
    bal = synth.balances(9, 1, mixed=True)
    e.set_validators(bal, np.ones(9, dtype=np.uint8))
    _set_lm(e, np.full(9, 4), np.array([2, 1, 0, 2, 2, 1, NONE32, 2, 0], dtype=np.uint32))
    e.on_tick(200 * 12)
    r2 = roots[2].tobytes()
    e.set_checkpoints((5, r2), (4, r2))
    assert e.prune() == dict(blocks_before=3, blocks_after=1, votes_remapped=4, votes_orphaned=4)
    st = e.export_state()
    assert (int(st["post_justified_epoch"][0]), st["post_justified_root"][0].tobytes()) == (3, x)
    assert (int(st["post_finalized_epoch"][0]), st["post_finalized_root"][0].tobytes()) == (2, y)
    e2 = engine_factory()
    e2.import_state(st, bal)
    assert _eq(e2.export_state(), st)                      # block 0's own checkpoints, not the anchor's
    assert e2.get_head() == e.get_head() == r2
    assert np.array_equal(e2.get_weights(), e.get_weights()) and int(e.get_weights()[0]) == int(bal[[0, 3, 4, 7]].sum())


# ---------------------------------------------------------------- 8. the slasher's history
def test_slasher_history_is_untouched_by_a_prune(engine_factory):
    w = _world(engine_factory, n_engines=1, n_blocks=120, n_val=515)
    e, = w["engines"]
    E = w["E"]
    e.slasher_enable(4)
    atts, arena = _batch(w, E - 1, w["tree"], 1, vote_recent=120)
    st, _ = e.slasher_ingest(packed=(atts, arena), current_epoch=E)
    assert (st == 0).any()
    src0, ids0 = (a.copy() for a in e.slasher_records(E - 1))
    assert (ids0 != NONE32).any()
    _finalize_by_hand(w, [e], 60)
    assert e.prune()["blocks_after"] < 120
    src1, ids1 = e.slasher_records(E - 1)
    assert np.array_equal(src0, src1) and np.array_equal(ids0, ids1)
