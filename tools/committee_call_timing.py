#!/usr/bin/env python3
"""Call time of the synchronous pe_compute_committees at 1 M validators WITH pubkeys loaded (tools/active_set_timing.py loads
none, so no committee sums are built there): 25 calls back to back over three epochs, median / min / max of the last 20.

    python tools/committee_call_timing.py [label]        (POSEVO_COMMITTEE_SUMS=0: without the sums).  Needs a GPU."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch

    torch.cuda.init()
    import pos_evolution_amd as pea
    from oracle import cport, g1

    n = 1 << 20
    pts = cport.g1_arith_progression(g1.to_bytes96(g1.mul(0x1234567, g1.G)), g1.to_bytes96(g1.mul(0x89ABCDE, g1.G)), n)
    e = pea.Engine(device=0)
    e.set_validators(np.full(n, 32 * 10**9, dtype=np.uint64), np.ones(n, dtype=np.uint8), pts)
    seed = hashlib.sha256(b"call-time").digest()
    ts = []
    for i in range(25):
        t0 = time.perf_counter()
        e.compute_committees(5 + (i % 3), seed, n, 2048, 90, want_result=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts[5:])
    print(sys.argv[1] if len(sys.argv) > 1 else "", json.dumps({"compute_committees_1M_call_ms_median": round(ts[len(ts) // 2], 4),
                                                                "min": round(ts[0], 4), "max": round(ts[-1], 4)}))
    e.close()


if __name__ == "__main__":
    main()
