#!/usr/bin/env python3
"""One synchronous device-row pe_aggregate (aggregate pubkeys wanted) at a chosen participation, host clock around the call:
what the threshold of the complement's sparse route (G1_SPARSE_MAX) costs or saves where groups sit near it.

    python tools/g1_sparse_timing.py [--density 0.90] [--validators 1048576] [--committees 2048] [--parts 4] [--reps 30]

The handle reads POSEVO_G1_SPARSE when it is created, so one process times one setting: run it once per setting (0 = the dense
complement route, 1 = the default threshold, 16 / 64 / 128 = that threshold) and alternate the settings.  Prints the setting,
the participation, how many groups went by complement, how many of those have at most 16 / 64 / 128 absentees, and the
median / minimum / maximum of `reps` calls after 5 warm-ups.  Needs a GPU."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, default=0.90)
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--committees", type=int, default=2048)
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.init()
    import pos_evolution_amd as pea
    import pos_evolution_amd.synth as synth
    from bench_legs.workload import epoch_attestations

    spe = 32
    e = pea.Engine(device=0)
    tree = synth.random_tree(64, 4, "bushy")
    e.store_init(0, 0, tree.roots[0].tobytes())
    for i in range(1, 64):
        e.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]))
    V = a.validators
    e.set_validators(synth.balances(V, 4), synth.validator_flags(V, 4, inactive_frac=0.0), synth.registry_points(e, V))
    ep = int(tree.slot.max()) // spe + 1
    off, mem = e.compute_committees(ep, hashlib.sha256(b"g1-sparse-timing").digest(), V, a.committees, 90)
    comm = synth.Committees(off, mem)
    e.on_tick((ep + 1) * spe * 12)
    atts, arena = epoch_attestations(comm, tree, ep, spe, seed=4, density=a.density, parts=a.parts,
                                     source=(0, tree.roots[0].tobytes()), vote_recent=8, vote_seed=4)
    t_rows = torch.from_numpy(atts.view(np.uint8).reshape(-1).copy()).cuda()
    t_bits = torch.from_numpy(arena.copy()).cuda()
    rows = pea.DeviceRows(t_rows.data_ptr(), len(atts), keep=t_rows)
    bits = pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)
    torch.cuda.synchronize()
    times = []
    for r in range(a.reps + 5):
        t0 = time.perf_counter()
        agg = e.aggregate(packed=(rows, bits), want_aggregate_pubkeys=True)
        n = agg["n_groups"]
        if r >= 5:
            times.append((time.perf_counter() - t0) * 1e3)
    absent = np.array([int(x["n_bits"]) for x in agg["atts"][:n]]) - np.asarray(agg["count"][:n]).astype(np.int64)
    _, n_cmpl = e.profile_committee_sums()
    print(f"POSEVO_G1_SPARSE={os.environ.get('POSEVO_G1_SPARSE', '(unset: 1)')} density {a.density} groups {n} by_complement {n_cmpl} "
          f"absentees<=16/64/128: {int((absent <= 16).sum())}/{int((absent <= 64).sum())}/{int((absent <= 128).sum())} "
          f"ms median {statistics.median(times):.4f} min {min(times):.4f} max {max(times):.4f} ({a.reps} calls)")
    e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
