#!/usr/bin/env python
"""Times pe_hash_to_g2 -- the message points H(m) from 32-byte signing roots -- beside the verification it feeds, on one GPU, in
one process.

    python examples/hash_to_g2_timing.py [--rounds N] [--sizes 8192,32768] [--out FILE]

Per size n: n distinct roots; one warm-up call of everything, then ROUNDS rounds, each timing in turn (alternated, so that a
drift of the box's clock meets all alike)
    hash host    pe_hash_to_g2, roots in host memory, points back to host memory (192 n bytes cross)
    hash device  pe_hash_to_g2, roots and points in device memory (nothing crosses)
    fast_agg     pe_fast_aggregate_verify of n groups of one key
    batch        pe_batch_verify of the same n groups
The groups verify by construction with message points of known discrete logarithm (64 distinct, tiled): what is timed is the
verification's shape, not these roots' signatures.  Four of the device's points are held to tests/hash_to_curve_model.py, and
the two routes to each other.  Every single time is printed; the summary line gives H(m) per second (best of the device route)
and its ratio to the faster verification's groups per second."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from oracle import g1, g2  # noqa: E402
from oracle.g1 import R_ORDER  # noqa: E402
from tests import hash_to_curve_model as hm  # noqa: E402


def groups(n, distinct=64):
    rng = np.random.default_rng(13)
    pk, msg, sig = [], [], []
    for _ in range(distinct):
        a = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        b = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        pk.append(g1.to_bytes96(g1.mul(a, g1.G)))
        msg.append(g2.to_bytes192(g2.mul(b, g2.G2)))
        sig.append(g2.to_bytes192(g2.mul(a * b % R_ORDER, g2.G2)))
    reps = -(-n // distinct)
    tile = lambda rows, w: np.frombuffer(b"".join(rows) * reps, dtype=np.uint8).reshape(-1, w)[:n].copy()
    return tile(pk, 96), tile(msg, 192), tile(sig, 192)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="8192,32768")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.init()
    for n in (int(v) for v in args.sizes.split(",")):
        e = pea.Engine(device=0)
        roots = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)
        pk, msg, sig = groups(n)
        e.set_validators(np.full(n, 32 * 10 ** 9, dtype=np.uint64), np.ones(n, dtype=np.uint8), pk)
        index, off = np.arange(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32)
        t_roots = torch.from_numpy(roots.reshape(-1).copy()).cuda()
        t_out = torch.zeros(192 * n, dtype=torch.uint8, device="cuda")
        d_roots = (pea.DeviceArena(t_roots.data_ptr(), 32 * n, keep=t_roots), 32)
        d_out = pea.DeviceArena(t_out.data_ptr(), 192 * n, keep=t_out)
        calls = {
            "hash host": lambda: e.hash_to_g2(roots),
            "hash device": lambda: e.hash_to_g2(d_roots, out=d_out),
            "fast_agg": lambda: e.fast_aggregate_verify(index, off, msg, sig),
            "batch": lambda: e.batch_verify(pk, msg, sig),
        }
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                t, out = timed(fn)
                times[k].append(t)
                if k == "hash host":
                    host_pts = out
                elif k in ("fast_agg", "batch"):
                    assert (out == 1).all(), "verdicts differ from the construction"
        assert np.array_equal(t_out.cpu().numpy().reshape(n, 192), host_pts), "the two routes differ"
        for i in (0, 1, n // 2, n - 1):
            assert bytes(host_pts[i]) == g2.to_bytes192(hm.hash_to_g2(bytes(roots[i]))), "a point differs from the model"
        for k, ts in times.items():
            say("n %6d  %-12s %s ms  min %9.3f  median %9.3f" % (n, k, " ".join("%9.3f" % t for t in ts), min(ts),
                                                                  float(np.median(ts))))
        h = n / (1e-3 * min(times["hash device"]))
        v = n / (1e-3 * min(min(times["fast_agg"]), min(times["batch"])))
        say("n %6d  H(m)/s %.0f (device route, best run; host route %.0f)   verified groups/s %.0f (the faster of the two "
            "calls, best run)   ratio H(m)/s : groups/s = %.2f" % (n, h, n / (1e-3 * min(times["hash host"])), v, h / v))
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
