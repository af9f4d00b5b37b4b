#!/usr/bin/env python
"""Times pe_batch_verify against the per-group path (pe_fast_aggregate_verify's pairing products: pe_pairing_check over the
pairs (pk, H(m)), (-g1, sig)) on the same inputs, on one GPU, host to host.

    python examples/batch_verify_timing.py [--rounds N] [--groups 2048,8192,32768] [--chunks 2,5,11] [--out FILE]

Per size: valid groups by construction (64 distinct ones, tiled); one warm-up call of everything, then ROUNDS rounds in one
process, each timing the per-group call and the batch call at every chunk size c in turn (alternated, so that a drift of the
box's clock meets both alike).  Every timed call's verdicts are checked.  Last: an all-invalid batch of 8192 groups, the
fallback's ceiling (top-level check, every chunk value exponentiated, every group rechecked).  Every single time is printed:
"faster" may be said only where every batch run beat every per-group run."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from oracle import g1, g2  # noqa: E402
from oracle.g1 import R_ORDER  # noqa: E402
from tests import pairing_model as pm  # noqa: E402
from tests.batch_verify_model import CHUNK  # noqa: E402  (the engine's default c)

NEG_G1 = np.frombuffer(g1.to_bytes96(g1.neg(g1.G)), dtype=np.uint8)


def make(n_groups, valid, distinct=64):
    rng = np.random.default_rng(13)
    pk, msg, sig = [], [], []
    for _ in range(distinct):
        a = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        b = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        pk.append(g1.to_bytes96(g1.mul(a, g1.G)))
        msg.append(g2.to_bytes192(g2.mul(b, g2.G2)))
        sig.append(g2.to_bytes192(g2.mul((a * b + (0 if valid else 1)) % R_ORDER, g2.G2)))
    reps = -(-n_groups // distinct)
    tile = lambda rows, w: np.frombuffer(b"".join(rows) * reps, dtype=np.uint8).reshape(-1, w)[:n_groups].copy()
    return tile(pk, 96), tile(msg, 192), tile(sig, 192)


def per_group_args(pk, msg, sig):
    n = len(pk)
    a = np.zeros((2 * n, 96), np.uint8)
    b = np.zeros((2 * n, 192), np.uint8)
    a[0::2], a[1::2] = pk, NEG_G1
    b[0::2], b[1::2] = msg, sig
    return a, b, np.arange(0, 2 * n + 1, 2, dtype=np.uint32)


def timed(fn, want):
    t0 = time.perf_counter()
    got = fn()
    t = time.perf_counter() - t0
    assert (got == want).all(), "verdicts differ from the construction"
    return 1e3 * t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--groups", default="2048,8192,32768")
    ap.add_argument("--chunks", default="2,5,11")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    chunks = [int(v) for v in args.chunks.split(",")]
    rounds = max(3, args.rounds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e = pea.Engine(device=0)
    m2, fe = pm.fp_products_per_lane(2)
    say("dependent Fp products per lane: per group %d + %d = %d; a chunk of c groups %s + %d once per call"
        % (m2, fe, m2 + fe, ", ".join("c=%d: %d (%.0f per group)" % (c, pm.fp_products_per_lane(c + 1)[0],
                                                                    pm.fp_products_per_lane(c + 1)[0] / c) for c in chunks), fe))
    for n in [int(v) for v in args.groups.split(",")]:
        pk, msg, sig = make(n, True)
        pa, pb, off = per_group_args(pk, msg, sig)
        calls = [("per-group", lambda: e.pairing_check(pa, pb, off))]
        for c in chunks:
            def batch(c=c):
                e._profile_batch_set_chunk(c)
                return e.batch_verify(pk, msg, sig)       # scalars drawn by the engine: the production mode
            calls.append(("batch c=%d" % c, batch))
        times = {name: [] for name, _ in calls}
        for name, fn in calls:                            # warm-up: arenas, code objects
            timed(fn, 1)
        for _ in range(rounds):
            for name, fn in calls:
                times[name].append(timed(fn, 1))
        stats = e._profile_batch_stats()
        assert stats["top_exps"] == 1 and stats["fallback_exps"] == 0 and stats["rechecked"] == 0
        base = times["per-group"]
        for name, _ in calls:
            t = times[name]
            say("groups %5d valid  %-11s %s ms  median %8.3f  x%.2f of per-group  %s"
                % (n, name, " ".join("%8.3f" % v for v in t), float(np.median(t)), float(np.median(base)) / float(np.median(t)),
                   "" if name == "per-group" else ("every run faster" if max(t) < min(base) else
                                                   "every run slower" if min(t) > max(base) else "runs overlap")))
    n = 8192
    pk, msg, sig = make(n, False)
    pa, pb, off = per_group_args(pk, msg, sig)
    e._profile_batch_set_chunk(CHUNK)
    timed(lambda: e.batch_verify(pk, msg, sig), 0)
    t = [timed(lambda: e.batch_verify(pk, msg, sig), 0) for _ in range(rounds)]
    b = [timed(lambda: e.pairing_check(pa, pb, off), 0) for _ in range(rounds)]
    stats = e._profile_batch_stats()
    assert stats["rechecked"] == n and stats["fallback_exps"] == stats["chunks"]
    say("groups %5d ALL INVALID  batch c=%d (fallback: %d chunk values, %d groups rechecked) %s ms  median %8.3f;  per-group %s ms"
        % (n, CHUNK, stats["fallback_exps"], stats["rechecked"], " ".join("%8.3f" % v for v in t), float(np.median(t)),
           " ".join("%8.3f" % v for v in b)))
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
