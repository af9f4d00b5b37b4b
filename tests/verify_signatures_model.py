"""The specification of pe_verify_signatures, in pure Python over oracle/g1.py and oracle/g2.py.

A member is (sk, s, status): its pubkey is sk * G1 (the registry's), its signature s * G2 (s None where the wire bytes do not
decode to a point of G2: status 1 malformed, 2 off the curve, 3 outside G2, 4 the identity).  A group's message point is
h * G2 (h = 0: the identity; h = None: a point off its curve).  With weights r_j the call decides, per group,

    e(sum_j r_j pk_j, H) * e(-g1, sum_j r_j sig_j) == 1     <=>     sum_j r_j (sk_j h - s_j) == 0  mod r

(the exponent of e(G1, G2), of prime order r; tests/test_verify_signatures_model.py holds this route to the pairing of
tests/pairing_model.py), over the members the settle pass left; a group that fails has each of those members decided alone.
"""
from math import comb

from oracle import g1, g2
from oracle.g1 import R_ORDER

STRIPE = 16                      # the handle's default k (pe_profile_verify_set_stripe)
STATUS_IDENTITY = 4
STAT_NAMES = ("settled", "failed_groups", "rechecked", "pairing_runs", "k")


def verify(members, offsets, msgs, r, k=STRIPE):
    """-> (member_verdict, sig_status, group_verdict, (sum_pk_dlog, sum_sig_dlog) per group, stats tuple of STAT_NAMES)."""
    n_groups = len(offsets) - 1
    verdict = [0] * len(members)
    status = [m[2] for m in members]
    group, sums = [], []
    settled = sum(1 for st in status if st != 0)
    failed = rechecked = 0
    for g in range(n_groups):
        js = range(offsets[g], offsets[g + 1])
        live = [j for j in js if status[j] == 0]
        sums.append((sum(r[j] * members[j][0] for j in live) % R_ORDER, sum(r[j] * members[j][1] for j in live) % R_ORDER))
        h = msgs[g]
        if h is None:                      # off its curve: decided where a pair of the group carries it
            group.append(2 if live else 1 if not len(js) else 0)
            continue
        if h == 0:
            group.append(0)
            continue
        if sum(r[j] * (members[j][0] * h - members[j][1]) for j in live) % R_ORDER == 0:
            for j in live:
                verdict[j] = 1
            group.append(1 if len(live) == len(js) else 0)
            continue
        failed += 1
        rechecked += len(live)
        for j in live:
            verdict[j] = 1 if (members[j][0] * h - members[j][1]) % R_ORDER == 0 else 0
        group.append(0)
    runs = 0 if n_groups == 0 else 2 if rechecked else 1
    return verdict, status, group, sums, (settled, failed, rechecked, runs, k)


def sum_bytes(sums):
    """The weighted sums as pe_profile_verify_sums returns them: canonical affine wire bytes."""
    return (b"".join(g1.to_bytes96(g1.mul(a, g1.G)) for a, _ in sums), b"".join(g2.to_bytes192(g2.mul(b, g2.G2)) for _, b in sums))


def aggregate_bytes(members, offsets, verdict):
    """Per group the compressed plain sum of the signatures of the members with verdict 1 (closed form)."""
    out = []
    for g in range(len(offsets) - 1):
        s = sum(members[j][1] for j in range(offsets[g], offsets[g + 1]) if verdict[j]) % R_ORDER
        out.append(g2.compress(g2.mul(s, g2.G2)))
    return b"".join(out)


# ---------------------------------------------------------------- what the weighted sums cost, counted from the code
def wave_max_adds(k, slots):
    """The additions a wave runs per bit plane: the expected maximum of `slots` independent Binomial(k, 1/2) counts (a slot's
    members whose random scalar has the bit set)."""
    cdf, acc = [], 0
    for c in range(k + 1):
        acc += comb(k, c)
        cdf.append(acc / 2 ** k)
    return sum(1 - cdf[c] ** slots for c in range(k))


G2_DBL, G2_ADD = 15, 18      # Fp products per lane of g2x_double (3 squarings, 6 products in Fp2) and g2x_add_affine (2, 8)
G1_DBL, G1_ADD = 9, 10       # g1x_double (3 S + 6 M) and g1x_add_affine (2 S + 8 M)


def fp_products_per_point(k=STRIPE):
    """Fp products per lane and point of the two Horner kernels on random scalars: (G2 per signature, G1 per key), each
    (executed, useful): 64 doublings per stripe of k, then per plane the wave's maximum count of additions (executed) against
    the 32 additions a point needs (useful)."""
    g2_exec = 64 * (G2_DBL + wave_max_adds(k, 32) * G2_ADD) / k
    g1_exec = 64 * (G1_DBL + wave_max_adds(k, 64) * G1_ADD) / k
    return (g2_exec, 64 * G2_DBL / k + 32 * G2_ADD), (g1_exec, 64 * G1_DBL / k + 32 * G1_ADD)
