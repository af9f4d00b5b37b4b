#!/usr/bin/env python
"""Times pe_verify_resident against the route a caller had before it, on one handle, alternated in one process.

One pe_aggregate_signed over device rows (compressed signatures, aggregate pubkeys requested) per shape:
    configs[3]'s step   8192 rows -> 2048 groups (four partial aggregates per committee)
    8192 groups         8192 rows -> 8192 groups (every committee attests to four different AttestationData)
Then, host to host, three alternated rounds after a warm-up of each:
    resident   pe_verify_resident(message points, point_of_row): the points are taken where the aggregate left them
    staged     pe_g2_decompress(out_signatures96), then pe_pairing_check over (out_aggpk96, H(m)), (-g1, signature) -- the two
               library calls, the interleaving of their inputs and the identity rule a caller applies to the result
Even groups are valid by construction (signature = (sum of the signers' sk) h G2), odd ones are off by one G2; both routes'
verdicts are compared with the construction before anything is timed.  Each shape is taken twice: after a leg without
PE_SIG_CHECK_SUBGROUP (the call then runs its own subgroup pass over the aggregate signatures, which the staged route never does)
and after a leg with it (the pass is skipped: both routes then do the same work).  Every single time is printed, then the medians.

    python examples/verify_resident_timing.py [--rounds 3] [--out profiles/verify_resident_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
import pos_evolution_amd.synth as synth  # noqa: E402
from oracle import g1, g2  # noqa: E402

R = g1.R_ORDER
A, B = 0x1234567, 0x89ABCDE      # synth.registry_points: validator v holds (A + v B) G1
H_SCALAR = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R
N_COMM, SPE, SIZE = 2048, 32, 32


def g2_multiples(e, scalars):
    """(n, 192) uint8: d G2 for every d, by the engine's G2 sum over the doublings of G2."""
    pts, cur = [], g2.G2
    for _ in range(255):
        pts.append(cur)
        cur = g2.double(cur)
    table = np.frombuffer(b"".join(g2.to_bytes192(p) for p in pts), dtype=np.uint8).reshape(-1, 192).copy()
    idx, off = [], [0]
    for d in scalars:
        idx += [i for i in range(255) if (d >> i) & 1]
        off.append(len(idx))
    return e.g2_sum(table, np.array(off, dtype=np.uint32), index=np.array(idx or [0], dtype=np.uint32)).copy()


def world():
    import torch

    n_val = N_COMM * SIZE
    e = pea.Engine(device=0)
    tree = synth.random_tree(96, 3, "branchy")
    e.store_init(0, 0, tree.roots[0].tobytes())
    for i in range(1, 96):
        e.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]))
    e.set_validators(synth.balances(n_val, 3, mixed=True), synth.validator_flags(n_val, 3), synth.registry_points(e, n_val, A, B))
    epoch = int(tree.slot.max()) // SPE + 1
    comm = synth.random_committees(n_val, N_COMM, 3)
    e.set_committees(epoch, comm.offsets, comm.members)
    e.on_tick((epoch + 1) * SPE * 12)
    atts, arena, bit_rows = synth.epoch_attestations(comm, tree, epoch, SPE, seed=3, density=0.9, parts=4,
                                                     source=(0, tree.roots[0].tobytes()))
    return e, torch, comm, atts, arena, bit_rows


def shape(e, torch, comm, atts, arena, bit_rows, split, check_subgroup):
    """split: every row of a committee gets an AttestationData of its own (8192 groups) instead of sharing one (2048)."""
    atts = atts.copy()
    if split:
        atts["source_root"][:, 31] ^= (np.arange(len(atts)) % 4).astype(np.uint8)
    group_key = np.arange(len(atts)) if split else np.arange(len(atts)) // 4
    sk = []
    for i, bits in enumerate(bit_rows):
        m = comm.members[comm.offsets[i // 4]:comm.offsets[i // 4 + 1]][bits]
        sk.append((len(m) * A + int(m.astype(np.int64).sum()) * B) % R)
    first_row = {int(k): i for i, k in reversed(list(enumerate(group_key)))}
    dlog = [(s * H_SCALAR + (1 if (group_key[i] & 1) and first_row[int(group_key[i])] == i else 0)) % R for i, s in enumerate(sk)]
    sigs = e.g2_compress(g2_multiples(e, dlog)).copy()
    t = torch.from_numpy(np.ascontiguousarray(atts).view(np.uint8).reshape(-1).copy()).cuda()
    rows = pea.DeviceRows(t.data_ptr(), len(atts), keep=t)
    agg = e.aggregate_signed(sigs, packed=(rows, arena), compressed=True, check_subgroup=check_subgroup,
                             want_aggregate_pubkeys=True)
    n_groups = agg["n_groups"]
    want = np.array([0 if (g & 1) else 1 for g in range(n_groups)], dtype=np.int32)
    empty = np.array([not b.any() for b in agg["bits"]])
    want[empty] = 0
    return agg, n_groups, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e, torch, comm, atts, arena, bit_rows = world()
    msg = g2_multiples(e, [H_SCALAR])
    neg_g1 = np.frombuffer(g1.to_bytes96(g1.neg(g1.G)), dtype=np.uint8)
    por = np.zeros(len(atts), dtype=np.uint32)
    say("device: %s" % torch.cuda.get_device_name(0))
    for split, check_subgroup in ((False, False), (True, False), (False, True), (True, True)):
        agg, n_groups, want = shape(e, torch, comm, atts, arena, bit_rows, split, check_subgroup)
        say("the leg %s PE_SIG_CHECK_SUBGROUP: the call %s its own subgroup pass over the aggregates"
            % (("ran with", "skips") if check_subgroup else ("ran without", "runs")))

        def resident():
            return e.verify_resident(msg, point_of_row=por, apply=False)

        def staged():
            sig192, _ = e.g2_decompress(agg["sig96c"])
            p1 = np.empty((2 * n_groups, 96), dtype=np.uint8)
            p1[0::2], p1[1::2] = agg["aggpk96"], neg_g1
            p2 = np.empty((2 * n_groups, 192), dtype=np.uint8)
            p2[0::2], p2[1::2] = msg[0], sig192
            v = e.pairing_check(p1, p2, np.arange(0, 2 * n_groups + 1, 2, dtype=np.uint32))
            # FastAggregateVerify's own rule, which the caller applies: no signer or an identity signature never verifies
            v[((agg["aggpk96"][:, 0] & 0x40) != 0) | ((sig192[:, 0] & 0x40) != 0)] = 0
            return v

        for name, fn in (("resident", resident), ("staged", staged)):     # warm-up, and the verdicts
            got = fn()
            assert np.array_equal(got, want), (name, int((got != want).sum()))
        say("%d rows -> %d groups (%d valid by construction); both routes give the construction's verdicts"
            % (len(atts), n_groups, int(want.sum())))
        times = {"resident": [], "staged": []}
        for r in range(max(1, args.rounds)):
            for name, fn in (("resident", resident), ("staged", staged)):
                t0 = time.perf_counter()
                fn()
                times[name].append(1e3 * (time.perf_counter() - t0))
                say("  round %d  %-8s %8.3f ms" % (r + 1, name, times[name][-1]))
        a, b = float(np.median(times["resident"])), float(np.median(times["staged"]))
        say("  median    resident %8.3f ms   staged %8.3f ms   difference %+.3f ms (%s)"
            % (a, b, a - b, "resident is faster" if a < b else "resident is NOT faster"))
        say("  stats of the last resident call: %s" % e._profile_verify_resident_stats())
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
