#!/usr/bin/env python
"""Times pe_verify_resident_data against the route it replaces, on one handle, alternated in one process.

One pe_aggregate_signed over device rows (compressed signatures, aggregate pubkeys requested) per shape, the shapes of
examples/verify_resident_timing.py:
    configs[3]'s step   8192 rows -> 2048 groups (four partial aggregates per committee)
    8192 groups         8192 rows -> 8192 groups (every committee attests to four different AttestationData)
Then, host to host, three alternated rounds after a warm-up of each:
    data       pe_verify_resident_data(domains): signing roots, hash_to_curve and pairings on the device, one call
    replaced   the rows read back from device memory, the first row of every group hashed with hashlib on the host
               (forkchoice.compute_signing_root: 9 SHA-256 per root, driven from Python -- a C caller pays less per root, the same
               read-back and upload), pe_hash_to_g2 from the host roots into device memory, pe_verify_resident over those points
The replaced route's parts are timed separately as well.  The signatures are multiples of G2 that are NOT over these messages,
so every group with a committee is decided by the full pairing product (verdict 0): both routes do the same device work, and
their verdicts, roots and counters are compared before anything is timed.  Every single time is printed, then the medians.

    python examples/verify_resident_data_timing.py [--rounds 3] [--out profiles/verify_resident_data_timing.txt]
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from pos_evolution_amd import forkchoice  # noqa: E402
from pos_evolution_amd.synth import ATT_DTYPE  # noqa: E402
from examples.verify_resident_timing import A, B, H_SCALAR, R, g2_multiples, world  # noqa: E402

GVR = bytes(range(32))
DOMAIN_PREVIOUS = forkchoice.compute_domain(forkchoice.DOMAIN_BEACON_ATTESTER, bytes([0, 0, 0, 1]), GVR)
DOMAIN_CURRENT = forkchoice.compute_domain(forkchoice.DOMAIN_BEACON_ATTESTER, bytes([0, 0, 0, 2]), GVR)


def host_root(row, fork_epoch):
    data = SimpleNamespace(slot=int(row["slot"]), index=int(row["index"]), beacon_block_root=row["beacon_block_root"].tobytes(),
                           source=SimpleNamespace(epoch=int(row["source_epoch"]), root=row["source_root"].tobytes()),
                           target=SimpleNamespace(epoch=int(row["target_epoch"]), root=row["target_root"].tobytes()))
    return forkchoice.compute_signing_root(data, DOMAIN_PREVIOUS if data.target.epoch < fork_epoch else DOMAIN_CURRENT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e, torch, comm, atts0, arena, bit_rows = world()
    say("device: %s" % torch.cuda.get_device_name(0))
    fork_epoch = int(atts0["target_epoch"][0])          # the rows' target epoch is the fork's first: the current domain
    sk = []
    for i, bits in enumerate(bit_rows):
        m = comm.members[comm.offsets[i // 4]:comm.offsets[i // 4 + 1]][bits]
        sk.append((len(m) * A + int(m.astype(np.int64).sum()) * B) % R)
    sigs = e.g2_compress(g2_multiples(e, [s * H_SCALAR % R for s in sk])).copy()
    for split in (False, True):
        atts = atts0.copy()
        if split:
            atts["source_root"][:, 31] ^= (np.arange(len(atts)) % 4).astype(np.uint8)
        t_rows = torch.from_numpy(np.ascontiguousarray(atts).view(np.uint8).reshape(-1).copy()).cuda()
        rows = pea.DeviceRows(t_rows.data_ptr(), len(atts), keep=t_rows)
        agg = e.aggregate_signed(sigs, packed=(rows, arena), compressed=True, want_aggregate_pubkeys=True)
        n_groups = agg["n_groups"]
        group_of = np.asarray(agg["group_of"][:len(atts)])
        first = np.full(n_groups, len(atts), dtype=np.int64)
        np.minimum.at(first, group_of, np.arange(len(atts)))
        d_points = torch.zeros(192 * n_groups, dtype=torch.uint8, device="cuda")
        points = pea.DeviceArena(d_points.data_ptr(), 192 * n_groups, keep=d_points)
        parts = {"read back": [], "hashlib": [], "hash_to_g2": [], "verify_resident": []}

        def data():
            return e.verify_resident_data(fork_epoch, DOMAIN_PREVIOUS, DOMAIN_CURRENT, apply=False)

        def replaced():
            t0 = time.perf_counter()
            back = t_rows.cpu().numpy().view(ATT_DTYPE)
            t1 = time.perf_counter()
            roots = np.frombuffer(b"".join(host_root(back[i], fork_epoch) for i in first), dtype=np.uint8).reshape(-1, 32)
            t2 = time.perf_counter()
            e.hash_to_g2(roots, out=points)
            t3 = time.perf_counter()
            v = e.verify_resident(points, apply=False)
            t4 = time.perf_counter()
            for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[name].append(1e3 * dt)
            return v, roots

        (v_data, r_data), st_data = data(), e._profile_verify_resident_stats()      # warm-up, and the comparison
        (v_repl, r_repl), st_repl = replaced(), e._profile_verify_resident_stats()
        assert np.array_equal(v_data, v_repl) and np.array_equal(r_data, r_repl) and st_data == st_repl
        for p in parts.values():
            p.clear()
        say("%d rows -> %d groups; both routes give the same verdicts (%d valid), roots and counters: %s"
            % (len(atts), n_groups, int((v_data == 1).sum()), st_data))
        times = {"data": [], "replaced": []}
        for r in range(max(1, args.rounds)):
            for name, fn in (("data", data), ("replaced", replaced)):
                t0 = time.perf_counter()
                fn()
                times[name].append(1e3 * (time.perf_counter() - t0))
                say("  round %d  %-8s %9.3f ms" % (r + 1, name, times[name][-1]))
        a, b = float(np.median(times["data"])), float(np.median(times["replaced"]))
        say("  median    data %9.3f ms   replaced %9.3f ms   difference %+.3f ms (%s)"
            % (a, b, a - b, "the one call is faster" if a < b else "the one call is NOT faster"))
        say("  replaced route, medians of its parts: " + "   ".join("%s %.3f ms" % (k, float(np.median(v))) for k, v in parts.items()))
        host = float(np.median(parts["read back"])) + float(np.median(parts["hashlib"]))
        say("  the host's share of the replaced route (read back + hashlib): %.3f ms; the one call against the device parts alone "
            "(hash_to_g2 + verify_resident): %+.3f ms" % (host, a - (b - host)))
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
