"""Shared builders for the differential tests (engine vs oracle on identical seeded inputs)."""
import numpy as np

import pos_evolution_amd.synth as synth
from oracle import cport, g1

NONE32 = 0xFFFFFFFF
ZERO = bytes(32)


def load_tree(engine, tree, leaf_cp=None, genesis_time=0):
    """store_init + add_block for a synthetic tree; leaf_cp[i] = (justified, finalized) checkpoint tuples."""
    engine.store_init(genesis_time, int(tree.slot[0]), tree.roots[0].tobytes())
    for i in range(1, tree.roots.shape[0]):
        j, f = leaf_cp[i] if leaf_cp is not None else ((0, tree.roots[0].tobytes()), (0, tree.roots[0].tobytes()))
        engine.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]), j, f)


def oracle_points(n, a=0x1234567, b=0x89ABCDE):
    """(n, 96) u8 with P_i = A + i*B (closed-form sums)."""
    A = g1.mul(a, g1.G)
    B = g1.mul(b, g1.G)
    return cport.g1_arith_progression(g1.to_bytes96(A), g1.to_bytes96(B), n), (a, b)


def closed_form_sum(indices, a, b):
    """sum_{i in S} (A + i*B) = (|S|*a + (sum i)*b) * G."""
    idx = [int(i) for i in indices]
    k = (len(idx) * a + sum(idx) * b) % g1.R_ORDER
    return g1.to_bytes96(g1.mul(k, g1.G))


def att_device_rows(atts, comm, slots_per_epoch):
    """Flat per-attestation arrays the C oracle consumes, from ATT_DTYPE rows + a committee table."""
    n_comm = comm.offsets.size - 1
    cps = n_comm // slots_per_epoch
    pos = (atts["slot"] % slots_per_epoch) * cps + atts["index"]
    member_off = comm.offsets[pos.astype(np.int64)]
    return member_off.astype(np.uint32), atts["n_bits"].astype(np.uint32), atts["bits_offset"].astype(np.uint32)


def install_votes(e, tree, comm, vote, now_slot=None):
    """Drive `vote` into the engine through on_attestation batches; returns the vote table actually installed
    (validators whose Zipf block fails validate_on_attestation keep no message).  Committee c attests in slot
    E * 32 + c // (committees per slot) of the epoch E behind the tree's last slot; the clock is set to now_slot
    (default: the first slot of epoch E + 2)."""
    n_comm = comm.offsets.size - 1
    spe = 32
    cps = n_comm // spe
    # every attestation: slot = 31 of the block's epoch or later so block.slot <= slot; use a single far epoch
    E = int(tree.slot.max()) // spe + 1
    e.set_committees(E, comm.offsets, comm.members)
    e.on_tick(((E + 2) * spe if now_slot is None else now_slot) * 12)
    # equivocators' votes are dropped by update_latest_messages (pe:1438): the caller accounts for that
    atts_list, bits_list = [], []
    installed = np.full(vote.shape[0], NONE32, dtype=np.uint32)
    for c in range(n_comm):
        mem = comm.members[comm.offsets[c]:comm.offsets[c + 1]]
        v = vote[mem]
        for blk in np.unique(v[v != NONE32]):
            blk = int(blk)
            a = np.zeros(1, dtype=synth.ATT_DTYPE)[0]
            a["slot"], a["index"] = E * spe + c // cps, c % cps
            a["beacon_block_root"] = tree.roots[blk]
            a["target_epoch"] = E
            a["target_root"] = tree.roots[synth.ancestor_at(tree, blk, E * spe)]
            a["source_root"] = tree.roots[0]
            a["flags"] = 3   # signature valid | is_from_block (no wall-clock epoch check, pe:1423)
            atts_list.append(a)
            bits_list.append(v == blk)
            installed[mem[v == blk]] = blk
    if not atts_list:   # nobody votes: nothing to hand in
        return installed
    atts = np.array(atts_list, dtype=synth.ATT_DTYPE)
    arena, offs, nb = synth.pack_bit_rows(bits_list)
    atts["bits_offset"], atts["n_bits"] = offs, nb
    status, _, _ = e.on_attestation_batch(packed=(atts, arena))
    assert (status == 0).all(), np.unique(status)
    return installed


def closed_form_sums(index_sets, a, b):
    """closed_form_sum for many sets at once: |S|*A + (sum i)*B, from the doublings of A and of B computed once (a few
    additions per set where a double-and-add per set costs hundreds).  -> list of 96-byte encodings."""
    sets = [np.asarray(s, dtype=np.int64).reshape(-1) for s in index_sets]
    counts = [int(s.size) for s in sets]
    sums = [int(s.sum()) for s in sets]
    dbl_a, dbl_b = [g1.mul(a, g1.G)], [g1.mul(b, g1.G)]
    for table, top in ((dbl_a, max(counts, default=0)), (dbl_b, max(sums, default=0))):
        while (1 << len(table)) <= top:
            table.append(g1.double(table[-1]))
    memo = {}

    def times(n, table):
        acc, i = None, 0
        while n:
            if n & 1:
                acc = g1.add(acc, table[i])
            n >>= 1
            i += 1
        return acc

    out = []
    for c, s in zip(counts, sums):
        if (c, s) not in memo:
            memo[(c, s)] = g1.to_bytes96(g1.add(times(c, dbl_a), times(s, dbl_b)))
        out.append(memo[(c, s)])
    return out


def ragged_committees(sizes, n_val, seed, slots_per_epoch=32):
    """A committee table whose first len(sizes) committees have exactly the given sizes, in that order, padded with empty
    committees to a multiple of slots_per_epoch.  Members: the head of a seeded permutation of the registry [0, n_val) --
    nobody sits in two committees (a partition, as the resident-row path requires)."""
    sizes = [int(s) for s in sizes]
    total = sum(sizes)
    assert total <= n_val
    pad = -len(sizes) % slots_per_epoch
    offsets = np.concatenate([[0], np.cumsum(sizes + [0] * pad)]).astype(np.uint32)
    members = np.random.Generator(np.random.PCG64(seed)).permutation(n_val)[:total].astype(np.uint32)
    return synth.Committees(offsets, members)


def committee_attestations(comm, tree, epoch, committees, bit_rows, slots_per_epoch=32):
    """One pe_attestation row per entry: row i attests for committee committees[i] of `epoch` with the bits bit_rows[i]
    (n_bits = len(bit_rows[i]), whatever the committee's size), voting for the tree's last block with a consistent FFG
    target.  -> (atts, arena)."""
    cps = (comm.offsets.size - 1) // slots_per_epoch
    blk = tree.roots.shape[0] - 1
    assert int(tree.slot[blk]) <= epoch * slots_per_epoch
    atts = np.zeros(len(committees), dtype=synth.ATT_DTYPE)
    c = np.asarray(committees, dtype=np.uint64)
    atts["slot"], atts["index"] = epoch * slots_per_epoch + c // cps, c % cps
    atts["beacon_block_root"] = tree.roots[blk]
    atts["source_epoch"], atts["source_root"] = 0, tree.roots[0]
    atts["target_epoch"], atts["target_root"] = epoch, tree.roots[synth.ancestor_at(tree, blk, epoch * slots_per_epoch)]
    atts["flags"] = 1
    arena, offs, nb = synth.pack_bit_rows(bit_rows)
    atts["bits_offset"], atts["n_bits"] = offs, nb
    return atts, arena
