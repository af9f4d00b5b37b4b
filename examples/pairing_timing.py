#!/usr/bin/env python
"""Times pe_pairing_check on one GPU at the shape of one pe_aggregate_signed step: G groups of two pairs (aggregate key and
message point, -g1 and signature), G = 8192 and 2048; one warm-up call, then the median of several timed calls (host to host:
upload, three launches, download).  Half of the groups are valid by construction, half are not; the verdicts are compared
before anything is printed.

    python examples/pairing_timing.py [--calls N] [--groups 8192,2048]

Reported per shape: ms per call, pairings/s, and the fraction of the 12 x 32 Fp product ceiling -- the one DESIGN.md reports
pe_g2_sum against (2^20 mixed adds x 36 products in 1.19 ms = 0.55 of it, i.e. 57.7 G products/s).  The Fp products per group
are counted from the op tables the kernels run (tests/pairing_model.fp_products_per_lane): products per lane on the group's
critical path, times the 12 working lanes of its 16-lane row."""
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

CEILING = 2 ** 20 * 36 / 1.19e-3 / 0.55   # Fp products per second (k_g2_accumulate's row)


def groups(n_groups, distinct=32):
    """Two pairs per group: (a G1, b G2), (-G1, a b G2) is valid; every other group has its last scalar off by one."""
    rng = np.random.default_rng(12)
    rows1, rows2, want = [], [], []
    neg = g1.to_bytes96(g1.neg(g1.G))
    for i in range(distinct):
        a = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        b = int.from_bytes(rng.bytes(32), "big") % R_ORDER
        ok = i % 2 == 0
        rows1.append(g1.to_bytes96(g1.mul(a, g1.G)) + neg)
        rows2.append(g2.to_bytes192(g2.mul(b, g2.G2)) + g2.to_bytes192(g2.mul((a * b + (0 if ok else 1)) % R_ORDER, g2.G2)))
        want.append(1 if ok else 0)
    reps = -(-n_groups // distinct)
    p1 = np.frombuffer(b"".join(rows1) * reps, dtype=np.uint8).reshape(-1, 96)[:2 * n_groups].copy()
    p2 = np.frombuffer(b"".join(rows2) * reps, dtype=np.uint8).reshape(-1, 192)[:2 * n_groups].copy()
    return p1, p2, np.arange(0, 2 * n_groups + 1, 2, dtype=np.uint32), np.array((want * reps)[:n_groups], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--groups", default="8192,2048")
    args = ap.parse_args()
    e = pea.Engine(device=0)
    miller, fe = pm.fp_products_per_lane(2)
    per_group = 12 * (miller + fe)
    print("Fp products per group of two pairs: %d per lane on the critical path (Miller loop %d, final exponentiation %d), "
          "%d over the 12 working lanes" % (miller + fe, miller, fe, per_group))
    for n_groups in [int(v) for v in args.groups.split(",")]:
        p1, p2, off, want = groups(n_groups)
        got = e.pairing_check(p1, p2, off)     # warm-up
        assert np.array_equal(got, want), "verdicts differ from the construction"
        times = []
        for _ in range(max(3, args.calls)):
            t0 = time.perf_counter()
            e.pairing_check(p1, p2, off)
            times.append(time.perf_counter() - t0)
        t = float(np.median(times))
        print("groups %5d x 2 pairs: %8.3f ms per call (min %.3f, max %.3f over %d calls)  %9.0f pairings/s  "
              "%.2f of the 12 x 32 product ceiling" % (n_groups, 1e3 * t, 1e3 * min(times), 1e3 * max(times), len(times),
                                                       2 * n_groups / t, n_groups * per_group / t / CEILING))
    e.close()


if __name__ == "__main__":
    main()
