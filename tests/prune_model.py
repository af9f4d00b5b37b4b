"""An own-words model of pe_prune (plain Python + numpy; no engine, no oracle): which blocks stay when the block table is
re-rooted at the finalized root, the map old insertion index -> new one, and what becomes of the latest messages.

The kept blocks are the finalized root and its descendants, in their relative insertion order; everything else goes.  A
latest message on a removed block keeps its epoch and names PRUNED instead of a block; NONE32 (no message), PRUNED (left
over from an earlier prune) and any other value that is no index of the old table stay as they are."""
import numpy as np

NONE32 = 0xFFFFFFFF
PRUNED = 0xFFFFFFFE


def index_map(parent, fin):
    """map[i] = new index of block i, PRUNED where it goes.  parent: insertion-order parent indices (parents first)."""
    n = len(parent)
    m = np.full(n, PRUNED, dtype=np.uint32)
    kept = 0
    for i in range(int(fin), n):
        if i == fin or (int(parent[i]) != NONE32 and m[int(parent[i])] != PRUNED):
            m[i] = kept
            kept += 1
    return m


def prune_parent(parent, m):
    """The kept blocks' parent array under the new indices (the root's parent is NONE32)."""
    keep = np.nonzero(m != PRUNED)[0]
    out = np.array([NONE32 if k == 0 else m[int(parent[i])] for k, i in enumerate(keep)], dtype=np.uint32)
    return keep, out


def remap_votes(vote_block, m):
    """-> (new vote_block, remapped, orphaned): remapped = kept under another index, orphaned = block removed now."""
    v = np.asarray(vote_block, dtype=np.uint32)
    out = v.copy()
    named = v < len(m)
    out[named] = m[v[named]]
    orphaned = int(np.count_nonzero(out[named] == PRUNED))
    remapped = int(np.count_nonzero((out[named] != PRUNED) & (out[named] != v[named])))
    return out, remapped, orphaned
