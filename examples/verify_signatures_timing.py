#!/usr/bin/env python
"""Times pe_verify_signatures against the work it shares with pe_aggregate_signatures and against the only other route to the
same verdicts (one two-pair pairing check per signature), on one GPU, host to host.

    python examples/verify_signatures_timing.py [--rounds N] [--committees 2048] [--size 512] [--out FILE]

Inputs by construction: 16384 registry keys (a + v b) G1, ONE message point H = h G2, signatures (a + v b) h G2; the epoch's
committees x size members walk the 16384 validators round and round (the arithmetic per member is that of distinct ones; the
registry rows and signature bytes repeat every 32 committees).  One warm-up call of everything, then ROUNDS rounds in one process,
the calls alternated.  Every timed call's verdicts are checked.  The per-signature route is timed at 32768 signatures and SCALED
to the epoch's count: it is labelled so."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
import pos_evolution_amd.synth as synth  # noqa: E402
from oracle import g1, g2  # noqa: E402
from oracle.g1 import R_ORDER  # noqa: E402
from tests import verify_signatures_model as vm  # noqa: E402

A, B, H, N_VAL, N_PAIRING = 0x1234567, 0x89ABCDE, 0x9E3779B97F4A7C15, 16384, 32768


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--committees", type=int, default=2048)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rounds, n_groups, total = max(3, args.rounds), args.committees, args.committees * args.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e = pea.Engine(device=0)
    keys = synth.registry_points(e, N_VAL, a=A, b=B)
    e.set_validators(np.full(N_VAL, 32 * 10 ** 9, dtype=np.uint64), np.ones(N_VAL, dtype=np.uint8), keys)
    table = synth.signature_points(e, N_VAL, a=A * H % R_ORDER, b=B * H % R_ORDER)
    signer = (np.arange(total, dtype=np.uint64) % N_VAL).astype(np.uint32)
    sig = table[signer].copy()
    off = np.arange(0, total + 1, args.size, dtype=np.uint32)
    msg = np.tile(np.frombuffer(g2.to_bytes192(g2.mul(H, g2.G2)), dtype=np.uint8), (n_groups, 1))
    k = e._profile_verify_stats()["k"] or vm.STRIPE
    (g2_exec, g2_useful), (g1_exec, g1_useful) = vm.fp_products_per_point(k)
    say("Fp products per lane at k = %d, counted from the code: per signature %.0f executed (%.0f useful; per-point scale %d), "
        "per key %.0f executed (%.0f useful; per-point scale %d); wave maximum of additions per plane %.2f (G2) %.2f (G1) of %d"
        % (k, g2_exec, g2_useful, 64 * (vm.G2_DBL + vm.G2_ADD), g1_exec, g1_useful, 64 * (vm.G1_DBL + vm.G1_ADD),
           vm.wave_max_adds(k, 32), vm.wave_max_adds(k, 64), k))

    def spoiled(every):
        """one invalid member (its neighbour's signature) in every `every`-th committee"""
        bad = sig.copy()
        first = np.arange(0, n_groups, every) * args.size
        bad[first] = table[(signer[first] + 1) % N_VAL]
        return bad, len(first)

    bad_1pc, n_1pc = spoiled(100)
    bad_all, n_all = spoiled(1)

    def verify(s, failed):
        verdict, _, group, _ = e.verify_signatures(s, signer, off, msg)
        st = e._profile_verify_stats()
        assert int(verdict.sum()) == total - failed and int((group == 1).sum()) == n_groups - failed
        assert st["failed_groups"] == failed and st["rechecked"] == failed * args.size
        return st

    def aggregate():
        _, status, bad = e.aggregate_signatures(sig, off, check_subgroup=True)
        assert not bad.any()

    m = min(N_PAIRING, total)
    pa = np.zeros((2 * m, 96), np.uint8)
    pb = np.zeros((2 * m, 192), np.uint8)
    pa[0::2], pa[1::2] = keys[signer[:m]], np.frombuffer(g1.to_bytes96(g1.neg(g1.G)), dtype=np.uint8)
    pb[0::2], pb[1::2] = msg[0], e.g2_decompress(table)[0][signer[:m]]
    poff = np.arange(0, 2 * m + 1, 2, dtype=np.uint32)

    def per_signature():
        assert (e.pairing_check(pa, pb, poff) == 1).all()

    calls = [("verify_signatures, all valid", lambda: verify(sig, 0), 1.0),
             ("aggregate_signatures + subgroup check", aggregate, 1.0),
             ("per-signature pairing, %d signatures, SCALED x%.0f" % (m, total / m), per_signature, total / m),
             ("verify_signatures, 1 invalid in %d committees" % n_1pc, lambda: verify(bad_1pc, n_1pc), 1.0),
             ("verify_signatures, 1 invalid in all %d committees" % n_all, lambda: verify(bad_all, n_all), 1.0)]
    times = {name: [] for name, _, _ in calls}
    for name, fn, _ in calls:
        fn()                                               # warm-up: buffers, code objects
    for _ in range(rounds):
        for name, fn, scale in calls:
            times[name].append(ms(fn)[0] * scale)
    say("%d signatures in %d committees of %d, engine-drawn scalars, host to host, ms per call:" % (total, n_groups, args.size))
    base = float(np.median(times[calls[0][0]]))
    for name, _, _ in calls:
        t = times[name]
        say("  %-58s %s  median %10.3f  x%.2f of the all-valid call" % (name, " ".join("%10.3f" % v for v in t), float(np.median(t)),
                                                                     float(np.median(t)) / base))
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
