"""Structured block trees and get_head cases for the tree kernel's shape edges (plain Python + numpy; no engine, no oracle).

The builders return (synth.Tree, names): exactly n blocks, parents before children in insertion order, roots from
synth.make_roots (a builder may hand the n roots out to its blocks in an order of its choosing, where a case needs a
certain root to rank above another).  The engine lays a tree out in DFS pre-order with the children of a block in insertion
order; preorder() restates that rule so that a case can aim at a position.

cases(n) builds the cases of tests/test_gpu_tree_shapes.py on those trees (eight kinds, ten Case objects: the star tie,
the late fork and the dead subtree come with a variant each), for a registry of n32 validators at
32 ETH followed by four at 2048 ETH, all active.  Every case names what it claims about the head (`head`: the block, or
`head_in`: the set it lies in); the CPU tests hold the C oracle to the definition on them and check the claims, the GPU tests
hold the kernel to the C oracle."""
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np

import pos_evolution_amd.synth as synth

NONE32 = 0xFFFFFFFF
ETH = 10**9
N_BIG = 4                 # validators at BIG_BALANCE behind the n32 ordinary ones
BIG_BALANCE = 2048 * ETH


# ---------------------------------------------------------------- layout
def preorder(parent):
    """(pos_of[i], size[i]) of the DFS pre-order, children in insertion order: the subtree of i is [pos, pos + size)."""
    n = len(parent)
    children = [[] for _ in range(n)]
    for i in range(1, n):
        children[int(parent[i])].append(i)
    pos = np.zeros(n, dtype=np.int64)
    size = np.ones(n, dtype=np.int64)
    order, stack = [], [0]
    while stack:
        b = stack.pop()
        pos[b] = len(order)
        order.append(b)
        stack.extend(reversed(children[b]))
    for b in reversed(order[1:]):
        size[int(parent[b])] += size[b]
    return pos, size


def shape_capacity(n):
    """Items of the launch shape the host picks for n blocks: lanes x items per lane (1024 x 1 / 2 / 4 / 8; the lean
    512 x 4 and 512 x 8 of pipelined calls hold the same counts)."""
    return 1024 if n <= 1024 else 2048 if n <= 2048 else 4096 if n <= 4096 else 8192


def _tree(parent, roots):
    n = len(parent)
    slot = np.zeros(n, dtype=np.uint64)
    for i in range(1, n):
        assert parent[i] < i
        slot[i] = slot[parent[i]] + 1
    p = np.array(parent, dtype=np.uint64).astype(np.uint32)
    p[0] = NONE32
    return synth.Tree(np.ascontiguousarray(roots), p, slot)


def _key(roots, i):
    return roots[i].tobytes()


def _swap(roots, i, j):
    roots[[i, j]] = roots[[j, i]]


# ---------------------------------------------------------------- shapes
def star(n):
    """anchor -> J -> n - 2 leaves: every leaf competes for the one best-child slot of J.  The lowest-ranked root among
    the leaves sits on the LAST leaf (pre-order position n - 1).  names: J, leaves, low, high."""
    assert n >= 5
    roots = synth.make_roots(n, b"star%d" % n)
    leaves = list(range(2, n))
    low = min(leaves, key=lambda i: _key(roots, i))
    _swap(roots, low, n - 1)
    high = max(leaves, key=lambda i: _key(roots, i))
    return _tree([0, 0] + [1] * (n - 2), roots), SimpleNamespace(J=1, leaves=leaves, low=n - 1, high=high)


def comb(n, spine_wins=(), spine_loses=()):
    """A spine S[0] (anchor) .. S[m] in which S[k] has, besides S[k + 1], the leaf child L[k] (k < m); an even n hangs one
    more block under S[m].  At odd levels the leaf is inserted before the spine child, at even levels behind it, so the
    leaves of even levels lie at the far end of the pre-order and insertion index != position.  spine_wins / spine_loses:
    levels k at which the root of S[k + 1] must rank above / below the root of L[k].  names: spine, leaf, tip, m."""
    m = (n - 1) // 2
    assert m >= 6
    roots = synth.make_roots(n, b"comb%d" % n)
    parent, spine, leaf = [0], [0], []
    for k in range(m):
        first_is_leaf = k % 2 == 1
        a, b = len(parent), len(parent) + 1
        parent += [spine[k], spine[k]]
        leaf.append(a if first_is_leaf else b)
        spine.append(b if first_is_leaf else a)
    tip = spine[m]
    if len(parent) < n:
        parent.append(spine[m])
        tip = len(parent) - 1
    assert len(parent) == n
    for k in list(spine_wins) + list(spine_loses):
        s, l = spine[k + 1], leaf[k]
        if (_key(roots, s) > _key(roots, l)) != (k in spine_wins):
            _swap(roots, s, l)
    return _tree(parent, roots), SimpleNamespace(spine=spine, leaf=leaf, tip=tip, m=m)


def late_fork(n):
    """A chain 0 .. n - 3 whose tip has the two children n - 2 and n - 1: the deciding items are the last two positions
    (pos + size == n).  The higher root sits on n - 2, so that "the last position" is the wrong answer to a tie.
    names: a (= n - 2, higher root), b (= n - 1)."""
    assert n >= 5
    roots = synth.make_roots(n, b"fork%d" % n)
    if _key(roots, n - 2) < _key(roots, n - 1):
        _swap(roots, n - 2, n - 1)
    return _tree([0] + list(range(n - 2)) + [n - 3], roots), SimpleNamespace(a=n - 2, b=n - 1)


def _two_bushes(n, top, first, second, seed, salt):
    """Blocks first / second under `top`, the rest alternately into the bush below either (parent: one of the last 8 blocks
    of that bush): the two are inserted interleaved, the pre-order puts all of first's bush in front of second's."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent = [0] + list(range(top))            # chain 0 .. top
    assert len(parent) == first and second == first + 1
    parent += [top, top]
    sides = ([first], [second])
    for i in range(second + 1, n):
        side = sides[(i - second - 1) % 2]
        parent.append(side[int(rng.integers(max(0, len(side) - 8), len(side)))])
        side.append(i)
    return _tree(parent, synth.make_roots(n, salt + b"%d" % n)), sides[0], sides[1]


def two_subtrees(n):
    """anchor -> A, B, each the root of a bushy subtree of about n / 2 blocks, inserted interleaved; B's subtree holds the
    last pre-order positions (its interval ends at n).  names: A, B, in_A, in_B (descendants), leaf_A (a leaf below A)."""
    assert n >= 9
    tree, sa, sb = _two_bushes(n, 0, 1, 2, 1000 + n, b"two")
    return tree, SimpleNamespace(A=1, B=2, in_A=sa[1:], in_B=sb[1:], leaf_A=sa[-1])


def dead_heavy(n):
    """anchor -> J -> V, H: H's subtree (about half the blocks, the last pre-order positions) is the heavy one of a case
    and has no viable leaf, V's is light and viable.  names: J, V, H, in_V, in_H (descendants)."""
    assert n >= 10
    tree, sv, sh = _two_bushes(n, 1, 2, 3, 2000 + n, b"dead")
    return tree, SimpleNamespace(J=1, V=2, H=3, in_V=sv[1:], in_H=sh[1:])


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    tree: synth.Tree
    leaf_ok: np.ndarray               # (n,) u8: the leaf test of filter_block_tree, per block
    vote: np.ndarray                  # (n_val,) u32 latest-message block, NONE32 = none
    justified: int
    boost: int = NONE32
    head: Optional[int] = None        # the block the case claims for the head ...
    head_in: Optional[frozenset] = None   # ... or the set it claims it lies in
    notes: dict = field(default_factory=dict)


def registry(n32=4096):
    """(balances u64, flags u8): n32 validators at 32 ETH, then N_BIG at BIG_BALANCE; all active."""
    bal = np.concatenate([np.full(n32, 32 * ETH, dtype=np.uint64), np.full(N_BIG, BIG_BALANCE, dtype=np.uint64)])
    return bal, np.ones(n32 + N_BIG, dtype=np.uint8)


def proposer_score(bal, flags, spe=32, percent=40, increment=ETH):
    """get_proposer_score: committee_weight = (active // SLOTS_PER_EPOCH) * (total_active_balance // active); 40 %."""
    act = (flags & 1) != 0
    num = int(act.sum())
    total = max(increment, int(bal[act].astype(object).sum()))
    return ((num // spe) * (total // num) * percent) // 100 if num else 0


class _Votes:
    """Hands the ordinary validators out in index order."""

    def __init__(self, n32):
        self.vote = np.full(n32 + N_BIG, NONE32, dtype=np.uint32)
        self.n32, self.next = n32, 0

    def give(self, block, count):
        assert self.next + count <= self.n32
        self.vote[self.next:self.next + count] = block
        self.next += count

    def spread(self, blocks, count):
        for k in range(count):
            self.give(blocks[k % len(blocks)], 1)

    def big(self, k, block):
        self.vote[self.n32 + k] = block


def _targets(blocks, seed):
    """Up to 24 vote targets inside a bush: its last block and a seeded choice of the others."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pick = rng.choice(len(blocks), size=min(23, len(blocks) - 1), replace=False) if len(blocks) > 1 else []
    return [blocks[-1]] + [blocks[int(i)] for i in pick if blocks[int(i)] != blocks[-1]]


def cases_two_subtrees(n, n32=4096):
    """1: justified = B while A's subtree, outside it, carries three times the votes: the head lies inside B.
    2: justified = a leaf below A (blocks of B's subtree follow it in pre-order): the head is that leaf."""
    tree, s = two_subtrees(n)
    v = _Votes(n32)
    v.spread(_targets(s.in_A, n), 3 * (n32 // 4))
    v.spread(_targets(s.in_B, n + 1), n32 // 4)
    ok = np.ones(n, dtype=np.uint8)
    return [Case("two_subtrees_justified_B", tree, ok, v.vote, s.B, head_in=frozenset(s.in_B)),
            Case("two_subtrees_justified_leaf", tree, ok, v.vote, s.leaf_A, head=s.leaf_A)]


def cases_star(n, n32=4096):
    """3: no votes: the highest root among n - 2 children.  4: two children at the same non-zero weight (one big validator
    each), one of them the lowest-ranked root at the last position: the other wins.  5: the boost on the lowest-ranked one,
    worth less than the one vote it has: it wins."""
    tree, s = star(n)
    ok = np.ones(n, dtype=np.uint8)
    other = s.leaves[len(s.leaves) // 2]
    assert other != s.low
    v = _Votes(n32)
    v.big(0, s.low)
    v.big(1, other)
    return [Case("star_no_votes", tree, ok, _Votes(n32).vote, s.J, head=s.high),
            Case("star_tie", tree, ok, v.vote, s.J, head=other),
            Case("star_tie_boost", tree, ok, v.vote, s.J, boost=s.low, head=s.low)]


def comb_tie_levels(n, s, pos):
    """(first level below the justified S[1], the level whose parent lies in the first half of the launch shape and whose
    spine child in the second -- where the spine does not reach that far, the middle level --, last level)."""
    half = shape_capacity(n) // 2
    mid = [k for k in range(2, s.m - 1) if pos[s.spine[k]] < half <= pos[s.spine[k + 1]]]
    return 1, (mid[0] if mid else s.m // 2), s.m - 1


def cases_comb(n, n32=4096):
    """6: justified = S[1], whose sibling leaf L[0] (outside) is the heaviest block of the tree.  At three levels the leaf
    weighs exactly what the spine child's subtree weighs; the spine's root wins the first two, the leaf's the last: the head
    is the last leaf L[m - 1]."""
    probe, s = comb(n)
    pos, _ = preorder(probe.parent)
    k1, k2, k3 = comb_tie_levels(n, s, pos)
    assert k1 < k2 < k3
    tree, s = comb(n, spine_wins=(k1, k2), spine_loses=(k3,))
    c = max(1, n32 // 64)
    v = _Votes(n32)
    v.give(s.tip, c)
    v.give(s.leaf[k3], c)
    v.give(s.leaf[k2], 2 * c)
    v.give(s.leaf[k1], 4 * c)
    v.give(s.leaf[0], 20 * c)
    return [Case("comb_three_ties", tree, np.ones(n, dtype=np.uint8), v.vote, s.spine[1], head=s.leaf[k3],
                 notes=dict(levels=(k1, k2, k3)))]


def cases_late_fork(n, n32=4096):
    """7: equal votes on the last two blocks: the higher root (n - 2) wins; one more validator on the other: it wins."""
    tree, s = late_fork(n)
    ok = np.ones(n, dtype=np.uint8)
    v = _Votes(n32)
    v.give(s.a, 5)
    v.give(s.b, 5)
    tie = v.vote.copy()
    v.give(s.b, 1)
    return [Case("late_fork_tie", tree, ok, tie, 1, head=s.a),
            Case("late_fork_one_more", tree, ok, v.vote, 1, head=s.b)]


def cases_dead_heavy(n, n32=4096):
    """8: below the justified J the heavy child H has no viable leaf, the light child V has: the head lies below V.  With
    every leaf below J failing the leaf test the head is J itself."""
    tree, s = dead_heavy(n)
    v = _Votes(n32)
    v.spread(_targets(s.in_H, n), 3 * (n32 // 4))
    v.spread(_targets(s.in_V, n + 1), n32 // 4)
    ok = np.ones(n, dtype=np.uint8)
    ok[[s.H] + s.in_H] = 0
    none = np.zeros(n, dtype=np.uint8)
    none[0] = 1
    return [Case("dead_heavy", tree, ok, v.vote, s.J, head_in=frozenset(s.in_V)),
            Case("dead_everything", tree, none, v.vote, s.J, head=s.J)]


def check_claims(case, head, weights, bal, flags):
    """What a case says about itself, against the reference's answer."""
    assert case.justified > 0
    if case.head is not None:
        assert head == case.head, case.name
    if case.head_in is not None:
        assert head in case.head_in, case.name
    s = proposer_score(bal, flags)
    if case.name == "two_subtrees_justified_B":     # the sibling subtree outside the justified one is the heavier
        assert weights[1] >= 2 * weights[2] > 0
    if case.name in ("star_tie", "star_tie_boost"):
        low, other = case.tree.roots.shape[0] - 1, int(case.vote[-N_BIG + 1])
        assert bytes(case.tree.roots[low]) < bytes(case.tree.roots[other])
        assert 0 < s < BIG_BALANCE                  # the boost is worth less than the one vote either has
        boosted = s if case.boost != NONE32 else 0
        assert weights[other] == BIG_BALANCE and weights[low] == BIG_BALANCE + boosted
    if case.name == "comb_three_ties":
        tree, names = comb(case.tree.roots.shape[0])
        for k in case.notes["levels"]:
            assert weights[names.spine[k + 1]] == weights[names.leaf[k]] > 0, k
        assert weights[names.leaf[0]] > weights[names.spine[1]]
    if case.name == "late_fork_tie":
        n = case.tree.roots.shape[0]
        assert weights[n - 2] == weights[n - 1] > 0
    if case.name == "dead_heavy":
        assert weights[3] > weights[2] > 0             # H outweighs V


CASE_BUILDERS = (cases_two_subtrees, cases_star, cases_comb, cases_late_fork, cases_dead_heavy)


def cases(n, n32=4096):
    return [c for build in CASE_BUILDERS for c in build(n, n32)]
