#!/usr/bin/env python
"""Times pe_state_roots on one GPU: each of the five per-validator field roots of BeaconState at V validators (default
1 048 576), the median of at least 20 calls after a warm-up, with the hashes per second that makes; and in the same run the
single-core hashlib time of tests/ssz_model.py for the same data, as the host baseline.  The roots of both sides are
compared before anything is printed.

    python examples/state_roots_timing.py [--validators V] [--calls N] [--no-host]
    POSEVO_SSZ_TILE_LOG2=9 python examples/state_roots_timing.py --no-host     # another tile of k_ssz_merkle

Hash counts: a list of c chunks costs c - 1 + (nodes paired with a zero hash) on the device, about c; hash_tree_root of a
Validator costs 7 (its pubkey leaf is formed once, when the static part is set), so `validators` is about 8 V."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from pos_evolution_amd import engine as E  # noqa: E402
from tests import ssz_model as M  # noqa: E402

FIELDS = [("balances", E.ROOT_BALANCES), ("inactivity_scores", E.ROOT_INACTIVITY),
          ("previous_epoch_participation", E.ROOT_PART_PREV), ("current_epoch_participation", E.ROOT_PART_CUR),
          ("validators", E.ROOT_VALIDATORS)]


def device_hashes(name: str, n: int) -> int:
    """Nodes k_ssz_merkle computes for n validators (every level's ceil), plus 7 per validator for `validators`."""
    chunks = {"balances": (n + 3) // 4, "inactivity_scores": (n + 3) // 4, "previous_epoch_participation": (n + 31) // 32,
              "current_epoch_participation": (n + 31) // 32, "validators": n}[name]
    total, m = 0, chunks
    while m > 1:
        m = (m + 1) // 2
        total += m
    return total + (7 * n if name == "validators" else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the hashlib baseline (tens of seconds at 1 M validators)")
    args = ap.parse_args()
    n, calls = args.validators, max(20, args.calls)
    rng = np.random.default_rng(8)
    u64 = lambda: rng.integers(0, 2**64, size=n, dtype=np.uint64)  # noqa: E731
    a = dict(pubkeys=rng.integers(0, 256, size=(n, 48), dtype=np.uint8), wc=rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
             eff=rng.integers(0, 33, size=n, dtype=np.uint64) * np.uint64(10**9), slashed=rng.integers(0, 2, size=n, dtype=np.uint8),
             elig=u64(), act=u64(), ext=u64(), wdr=u64(), bal=u64(), sc=u64(),
             prev=rng.integers(0, 256, size=n, dtype=np.uint8), cur=rng.integers(0, 256, size=n, dtype=np.uint8))
    e = pea.Engine(device=0)
    e.set_validators(a["eff"], (1 | (a["slashed"] << 1)).astype(np.uint8))
    e.registry_set_epochs(a["act"], a["ext"])
    e.state_set_balances(a["bal"], a["sc"], a["wdr"])
    e.participation_set(0, a["cur"])
    e.participation_set(1, a["prev"])
    t0 = time.perf_counter()
    e.registry_set_static(a["pubkeys"], a["wc"], a["elig"])
    t_static = time.perf_counter() - t0
    print(f"validators {n}  tile_log2 {os.environ.get('POSEVO_SSZ_TILE_LOG2', 'default')}  "
          f"registry_set_static (upload + {n} pubkey leaves) {t_static * 1e3:.2f} ms")
    got = {}
    for name, bit in FIELDS + [("all five", E.ROOT_ALL)]:
        for _ in range(args.warmup):
            e.state_roots(bit)
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            r = e.state_roots(bit)
            times.append(time.perf_counter() - t0)
        got.update(r)
        med = float(np.median(times))
        hashes = sum(device_hashes(f, n) for f, b in FIELDS if b & bit)
        print(f"  {name:30s} median of {calls}: {med * 1e3:8.3f} ms   min {min(times) * 1e3:8.3f} ms   "
              f"{hashes:9d} hashes   {hashes / med / 1e9:6.3f} G hashes/s")
    if args.no_host:
        e.close()
        return
    # the host baseline: the model, one core, the same data
    t0 = time.perf_counter()
    want = {"balances": M.u64_list_root(a["bal"]), "inactivity_scores": M.u64_list_root(a["sc"])}
    t_u64 = time.perf_counter() - t0
    t0 = time.perf_counter()
    want["previous_epoch_participation"] = M.u8_list_root(a["prev"])
    want["current_epoch_participation"] = M.u8_list_root(a["cur"])
    t_u8 = time.perf_counter() - t0
    t0 = time.perf_counter()
    reg = M.Registry(pubkeys=[a["pubkeys"][v].tobytes() for v in range(n)], withdrawal_credentials=[a["wc"][v].tobytes() for v in range(n)],
                     effective_balance=a["eff"].tolist(), slashed=a["slashed"].tolist(), activation_eligibility_epoch=a["elig"].tolist(),
                     activation_epoch=a["act"].tolist(), exit_epoch=a["ext"].tolist(), withdrawable_epoch=a["wdr"].tolist(),
                     balances=[0] * n)
    want["validators"] = M.validators_root(reg.validator_leaves())
    t_val = time.perf_counter() - t0
    assert got == want, "device and model roots differ"
    print(f"  hashlib, one core: the two uint64 lists {t_u64:.2f} s, the two uint8 lists {t_u8:.2f} s, validators {t_val:.2f} s "
          f"(total {t_u64 + t_u8 + t_val:.2f} s); roots equal")
    e.close()


if __name__ == "__main__":
    main()
