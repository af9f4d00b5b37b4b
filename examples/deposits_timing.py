"""pe_process_deposits at 1 M resident validators against the route a caller had before it: download the resident arrays
through the _get calls, look the pubkeys up in a host dict, apply, re-upload through pe_set_validators and the _set calls.

Three batches: 16 deposits (a block: 14 top-ups, 2 new keys), 4 096 top-ups, 4 096 new keys with proofs = NULL (genesis /
replay).  Both routes run on the same handle pair in one process, alternated, REPS times each; the host dict alone (lookups
and appends, no transfer, no signature check) is timed too.  The index build is reported separately: it is paid once per handle.

    python examples/deposits_timing.py [n_validators] > profiles/deposits_timing.txt

New keys are real: secret keys a + i b, keys (a + i b) G1, one message point M = m G2 and signatures (a + i b) M, formed by
repeated addition (oracle/g1.py, oracle/g2.py: test infrastructure, not the product)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pos_evolution_amd as pea  # noqa: E402
from oracle import g1, g2  # noqa: E402
from oracle.g1 import R_ORDER  # noqa: E402
from pos_evolution_amd.engine import DEPOSIT_DTYPE  # noqa: E402

ETH, FAR = 10**9, 2**64 - 1
REPS = 3
MSG = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R_ORDER


def real_keys(count):
    a, b = 0x1F2E3D4C5B6A7988, 0xABCDEF
    pks = g1.synthetic_points(count, a, b)
    sigs = g2.synthetic_points(count, a * MSG % R_ORDER, b * MSG % R_ORDER)
    return [g1.compress(p) for p in pks], [g2.compress(s) for s in sigs]


class Host:
    """The registry as a caller holds it, and the route through the host."""

    def __init__(self, n, rng):
        self.pubkeys = np.frombuffer(rng.bytes(48 * n), dtype=np.uint8).reshape(n, 48).copy()
        self.wc = np.zeros((n, 32), dtype=np.uint8)
        self.index = {self.pubkeys[i].tobytes(): i for i in range(n)}

    def load(self, e, n):
        eff = np.full(n, 32 * ETH, dtype=np.uint64)
        e.set_validators(eff, np.ones(n, dtype=np.uint8))
        e.state_set_validators(eff, np.full(n, 9, dtype=np.uint8))
        e.registry_set_epochs(np.zeros(n, dtype=np.uint64), np.full(n, FAR, dtype=np.uint64))
        e.state_set_balances(np.full(n, 32 * ETH, dtype=np.uint64))
        e.registry_set_static(self.pubkeys, self.wc, np.zeros(n, dtype=np.uint64))

    def dict_alone(self, rows, valid):
        """Lookups, top-ups and appends on host arrays that are already there: no transfer, no signature check."""
        index, n = self.index, len(self.index)
        added, topups = [], []
        for r, ok in zip(rows, valid):
            v = index.get(r["pubkey"].tobytes())
            if v is None:
                if ok:
                    index[r["pubkey"].tobytes()] = n + len(added)
                    added.append(r)
            else:
                topups.append((v, int(r["amount"])))
        for r in added:                      # leave the dict as it was: the next repetition sees the same registry
            del index[r["pubkey"].tobytes()]
        return added, topups

    def round_trip(self, e, rows, valid):
        """download -> dict -> apply -> re-upload: what a deposit cost a handle before pe_process_deposits."""
        eff, flags, _ = e.state_validators()
        act, ext, _ = e.registry_get_epochs()
        bal, score, wdr, _ = e.state_get_balances()
        _, wc, elig, _ = e.registry_static()
        cur, prev = e.participation_get(0), e.participation_get(1)
        added, topups = self.dict_alone(rows, valid)
        for v, amount in topups:
            bal[v] += np.uint64(amount)
        k = len(added)
        amounts = np.array([int(r["amount"]) for r in added], dtype=np.uint64)
        cat = np.concatenate
        eff2 = cat([eff, np.minimum(amounts - amounts % np.uint64(ETH), np.uint64(32 * ETH))])
        far = np.full(k, FAR, dtype=np.uint64)
        pk2 = cat([self.pubkeys, np.array([r["pubkey"] for r in added], dtype=np.uint8).reshape(k, 48)])
        wc2 = cat([wc, np.array([r["withdrawal_credentials"] for r in added], dtype=np.uint8).reshape(k, 32)])
        e.set_validators(eff2, cat([flags & 3, np.zeros(k, dtype=np.uint8)]))
        e.state_set_validators(eff2, cat([flags, np.zeros(k, dtype=np.uint8)]))
        e.registry_set_epochs(cat([act, far]), cat([ext, far]))
        e.state_set_balances(cat([bal, amounts]), cat([score, np.zeros(k, dtype=np.uint64)]), cat([wdr, far]))
        e.registry_set_static(pk2, wc2, cat([elig, far]))
        e.participation_set(0, cat([cur, np.zeros(k, dtype=np.uint8)]))
        e.participation_set(1, cat([prev, np.zeros(k, dtype=np.uint8)]))


def rows_of(pubkeys, sigs, amount=32 * ETH):
    rows = np.zeros(len(pubkeys), dtype=DEPOSIT_DTYPE)
    for i, (pk, sig) in enumerate(zip(pubkeys, sigs)):
        rows[i] = (np.frombuffer(pk, dtype=np.uint8), np.zeros(32, dtype=np.uint8), amount, np.frombuffer(sig, dtype=np.uint8))
    return rows


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    rng = np.random.default_rng(1)
    host = Host(n, rng)
    msg = np.frombuffer(g2.to_bytes192(g2.mul(MSG, g2.G2)), dtype=np.uint8)
    per_rep = 4096 + 2
    pks, sigs = real_keys(REPS * per_rep)
    zero_sig = bytes(96)
    print(f"# pe_process_deposits at {n} resident validators; ms per call, {REPS} alternated repetitions, min | median")
    results = {}
    for name in ("block16", "topups4096", "new4096"):
        e = pea.Engine(device=0)      # the engine route: grows in place
        host.load(e, n)
        t0 = time.perf_counter()
        e.process_deposits(rows_of([host.pubkeys[0].tobytes()], [zero_sig], 1), None)   # builds the index
        first = (time.perf_counter() - t0) * 1e3
        info = e.deposit_index_info()
        if name == "block16":
            print(f"index build: {info['build_ms']:.3f} ms on the device for {info['keys']} keys in {info['slots']} slots "
                  f"(first call {first:.2f} ms wall), once per handle")
        p = pea.Engine(device=0)      # the host route: always back at n validators before a repetition
        t_engine, t_trip, t_dict = [], [], []
        for rep in range(REPS):
            fresh = slice(rep * per_rep, (rep + 1) * per_rep)
            kp, ks = pks[fresh], sigs[fresh]
            if name == "block16":
                who = rng.integers(0, n, size=14)
                rows = rows_of([host.pubkeys[v].tobytes() for v in who] + kp[:2], [zero_sig] * 14 + ks[:2], ETH)
            elif name == "topups4096":
                who = rng.integers(0, n, size=4096)
                rows = rows_of([host.pubkeys[v].tobytes() for v in who], [zero_sig] * 4096, ETH)
            else:
                rows = rows_of(kp[2:], ks[2:])
            valid = [True] * rows.size
            mp = np.tile(msg, rows.size)
            host.load(p, n)
            t0 = time.perf_counter()
            host.round_trip(p, rows, valid)
            t_trip.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            res = e.process_deposits(rows, mp)
            t_engine.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            added, _ = host.dict_alone(rows, valid)
            t_dict.append((time.perf_counter() - t0) * 1e3)
            assert res["n_appended"] == len(added) == p.num_validators - n, (res["n_appended"], len(added))
        results[name] = (t_engine, t_trip, t_dict)
        fmt = lambda t: f"{min(t):9.3f} | {float(np.median(t)):9.3f}"  # noqa: E731
        print(f"{name:11s} engine {fmt(t_engine)}   download/dict/re-upload {fmt(t_trip)}   host dict alone {fmt(t_dict)}")
        e.close()
        p.close()
    eng, _, dic = results["block16"]
    verdict = "faster" if min(eng) < min(dic) else "NOT faster"
    print(f"# the 16-deposit block on the engine is {verdict} than the host dict alone ({min(eng):.3f} vs {min(dic):.3f} ms): the dict"
          f" holds no state on the device; the case the engine must win is the round trip ({min(results['block16'][1]):.1f} ms)")


if __name__ == "__main__":
    main()
