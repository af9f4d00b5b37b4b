#!/usr/bin/env python
"""Times the sync committee calls on one GPU at V validators (default 1 048 576), as the host wall clock around the synchronous
calls, the median of at least 20 after a warm-up.

  (a) pe_sync_committee_compute, size 512, 90 rounds, over all V validators: every effective balance at 32 ETH, and every one at
      1 ETH against a 32 ETH maximum (1 acceptance in 32); with the candidates examined.
  (b) pe_process_sync_aggregate with PE_SYNC_VERIFY | PE_SYNC_APPLY for n = 1 and n = 32 blocks, about 95 % of the committee
      signing -- against the route a caller had before the call existed, timed in the same process, the two alternating:
      pe_state_get_balances, the rewards on the host, pe_state_set_balances, and pe_hash_to_g2 + pe_g2_decompress +
      pe_fast_aggregate_verify over a participants' list built on the host.  Both routes' balances and verdicts are compared
      before anything is printed.

    python examples/sync_committee_timing.py [--validators V] [--calls N] [--json PATH]

Registry keys are sk_v = A + v B (synth.registry_points), so the participants' aggregate signature is one scalar multiple of H(m)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
import pos_evolution_amd.synth as synth  # noqa: E402
from oracle import g2  # noqa: E402
from pos_evolution_amd.engine import SYNC_APPLY, SYNC_CURRENT, SYNC_VERIFY  # noqa: E402
from tests import hash_to_curve_model as hm  # noqa: E402
from tests import sync_committee_model as M  # noqa: E402

ETH = 10**9
A, B = 0x1234567, 0x89ABCDE
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
DOMAIN = bytes([7, 0, 0, 0]) + hashlib.sha256(b"fork").digest()[:28]


def median_ms(times):
    return dict(median_ms=float(np.median(times)) * 1e3, min_ms=min(times) * 1e3, calls=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="write the figures to this file")
    args = ap.parse_args()
    n_val, calls = args.validators, max(20, args.calls)
    e = pea.Engine(device=0)
    flags = np.ones(n_val, dtype=np.uint8)
    full = np.full(n_val, 32 * ETH, dtype=np.uint64)
    e.set_validators(full, flags, synth.registry_points(e, n_val, A, B))
    out = dict(validators=n_val, method="host wall clock around the synchronous calls, median after warm-up", warmup=args.warmup)

    # ---- (a) sampling
    seeds = [hashlib.sha256(b"period-%d" % k).digest() for k in range(args.warmup + calls)]
    for name, bal in (("32 ETH", full), ("1 ETH", np.full(n_val, ETH, dtype=np.uint64))):
        e.state_set_validators(bal, flags)
        times, tries = [], []
        for i, seed in enumerate(seeds):
            t0 = time.perf_counter()
            _, _, tr = e.sync_committee_compute(seed, n_val, 90, 32 * ETH, 512)
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                times.append(dt)
                tries.append(tr)
        out["compute " + name] = dict(median_ms(times), candidates_median=int(np.median(tries)), candidates_max=int(max(tries)))
        r = out["compute " + name]
        print(f"pe_sync_committee_compute, {n_val} validators at {name}, size 512, 90 rounds: median of {calls}: "
              f"{r['median_ms']:8.3f} ms  min {r['min_ms']:8.3f} ms  candidates examined: median {r['candidates_median']}, "
              f"max {r['candidates_max']}")

    # ---- (b) one block's aggregate, and 32
    e.state_set_validators(full, flags)
    members, _, _ = e.sync_committee_compute(seeds[0], n_val, 90, 32 * ETH, 512)
    members = [int(v) for v in members]
    e.sync_committee_rotate()
    assert e.sync_committee_get(SYNC_CURRENT)[0].tolist() == members
    total = 32 * ETH * n_val
    pr, qr = M.reward_scalars(total, 512)
    rng = np.random.default_rng(3)
    start = rng.integers(0, 33 * ETH, size=n_val, dtype=np.uint64)
    for n in (1, 32):
        aggs = []
        for b in range(n):
            positions = [p for p in range(512) if rng.random() < 0.95]
            bits = bytearray(64)
            for p in positions:
                bits[p // 8] |= 1 << (p % 8)
            root = hashlib.sha256(b"block-%d" % b).digest()
            sk = sum(A + members[p] * B for p in positions) % R
            sig = g2.compress(hm.curve_mul(sk, hm.hash_to_g2(M.signing_root(root, DOMAIN), hm.ETH2_DST)))
            aggs.append(dict(bits=bytes(bits), signature=sig, block_root=root, domain=DOMAIN, proposer_index=int(rng.integers(0, n_val))))

        def device_route():
            res = e.process_sync_aggregate(aggs, total, SYNC_VERIFY | SYNC_APPLY)
            return res["verdict"].tolist()

        def host_route():
            bal = e.state_get_balances()[0]
            work = {v: int(bal[v]) for v in members + [a["proposer_index"] for a in aggs]}   # only the balances it touches
            M.process_sync_aggregates(work, members, [(a["bits"], a["proposer_index"]) for a in aggs], pr, qr)
            bal[list(work)] = np.array(list(work.values()), dtype=np.uint64)
            e.state_set_balances(bal)
            index, offsets = [], [0]
            for a in aggs:
                index += M.participants(members, a["bits"])
                offsets.append(len(index))
            points = e.hash_to_g2([M.signing_root(a["block_root"], a["domain"]) for a in aggs])
            sig192, status = e.g2_decompress(np.frombuffer(b"".join(a["signature"] for a in aggs), dtype=np.uint8))
            assert not status.any()
            return e.fast_aggregate_verify(index, offsets, points, sig192).tolist()

        times = {"device": [], "host": []}
        final, verdicts = {}, {}
        for i in range(args.warmup + calls):
            for name, route in (("device", device_route), ("host", host_route)):      # alternating, from the same balances
                e.state_set_balances(start)
                t0 = time.perf_counter()
                verdicts[name] = route()
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times[name].append(dt)
                final[name] = e.state_get_balances()[0]
        assert verdicts["device"] == verdicts["host"] == [1] * n, verdicts
        assert np.array_equal(final["device"], final["host"]), "the two routes' balances differ"
        for name, label in (("device", "pe_process_sync_aggregate (VERIFY | APPLY)"),
                            ("host", "balances down, host rewards, balances up, three-call verify")):
            out[f"aggregate n={n} {name}"] = r = median_ms(times[name])
            print(f"n = {n:2d}  {label:60s} median of {calls}: {r['median_ms']:9.3f} ms   min {r['min_ms']:9.3f} ms")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    e.close()


if __name__ == "__main__":
    main()
