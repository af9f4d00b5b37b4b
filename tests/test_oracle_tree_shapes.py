"""CPU: the reference of tests/test_gpu_tree_shapes.py pinned first.  On the structured trees of tests/tree_shapes.py, with
the justified root inside the tree, the C oracle's get_head equals the definition-level restatement of
tests/test_oracle_properties.py (head and every weight), and every case is what it claims to be; plus generated worlds
that also draw the justified block."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle import cport
from tests import tree_shapes as TS
from tests.test_oracle_properties import definition_get_head, worlds

NONE32 = 0xFFFFFFFF
N32 = 256      # a small registry keeps the definition's per-vote walk quick; the cases scale their votes with it


def test_builders_build_what_they_say():
    for n in (13, 16, 37, 64, 1023, 1025):
        for build in (TS.star, TS.comb, TS.late_fork, TS.two_subtrees, TS.dead_heavy):
            tree, names = build(n)
            assert tree.roots.shape == (n, 32) and tree.parent.shape == (n,) and tree.slot.shape == (n,)
            assert len({bytes(r) for r in tree.roots}) == n
            assert tree.parent[0] == NONE32 and (tree.parent[1:] < np.arange(1, n)).all()
            assert (tree.slot[1:] == tree.slot[tree.parent[1:]] + 1).all()
        pos, size = TS.preorder(TS.two_subtrees(n)[0].parent)
        assert pos[2] + size[2] == n and pos[2] == 1 + size[1]           # B's interval ends the pre-order
        assert (np.sort(pos) == np.arange(n)).all() and not (pos == np.arange(n)).all()
        tree, s = TS.late_fork(n)
        assert bytes(tree.roots[s.a]) > bytes(tree.roots[s.b])
        tree, s = TS.star(n)
        assert all(bytes(tree.roots[s.low]) <= bytes(tree.roots[i]) <= bytes(tree.roots[s.high]) for i in s.leaves)
        tree, s = TS.comb(n, spine_wins=(1, 3), spine_loses=(2,))
        for k in (1, 2, 3):
            assert (bytes(tree.roots[s.spine[k + 1]]) > bytes(tree.roots[s.leaf[k]])) == (k != 2)
    # the middle tie level of the comb lies where the launch shape's halves meet, wherever the spine reaches that far
    for n in (1023, 1024, 2047, 2048, 4095, 4096, 8191, 8192):
        tree, s = TS.comb(n)
        pos, _ = TS.preorder(tree.parent)
        _, k2, _ = TS.comb_tie_levels(n, s, pos)
        half = TS.shape_capacity(n) // 2
        assert pos[s.spine[k2]] < half <= pos[s.spine[k2 + 1]], n


@pytest.mark.parametrize("n", [17, 32, 64])
def test_c_oracle_equals_the_definition_on_the_structured_cases(n):
    bal, flags = TS.registry(N32)
    all_cases = TS.cases(n, N32)
    assert len(all_cases) == 10
    for case in all_cases:
        t = case.tree
        head_c, w_c = cport.get_head(t.parent.copy(), case.leaf_ok, t.roots, case.vote, bal, flags, case.justified,
                                     case.boost)
        head_d, w_d = definition_get_head([int(p) for p in t.parent], case.leaf_ok, t.roots, case.vote, bal, flags,
                                          case.justified, case.boost)
        assert [int(x) for x in w_c] == w_d, case.name
        assert head_c == head_d, case.name
        TS.check_claims(case, head_c, w_d, bal, flags)


@st.composite
def worlds_with_justified(draw):
    """worlds() of tests/test_oracle_properties.py plus a justified block anywhere in the tree."""
    wd = draw(worlds())
    return wd + (draw(st.integers(0, len(wd[0]) - 1)),)


@settings(max_examples=150, deadline=None)
@given(worlds_with_justified())
def test_c_oracle_get_head_equals_the_definition_from_any_justified_block(wd):
    parent, leaf_ok, roots, vote, bal, flags, boost, justified = wd
    if len(set(roots)) != len(roots):
        return
    head_d, w_d = definition_get_head(parent, leaf_ok, roots, vote, bal, flags, justified, boost)
    r = np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(-1, 32)
    head_c, w_c = cport.get_head(np.array(parent, dtype=np.uint32), np.array(leaf_ok, dtype=np.uint8), r,
                                 np.array(vote, dtype=np.uint32), np.array(bal, dtype=np.uint64),
                                 np.array(flags, dtype=np.uint8), justified, boost)
    assert [int(x) for x in w_c] == w_d
    assert head_c == head_d
