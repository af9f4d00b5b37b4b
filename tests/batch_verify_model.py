"""Pure-Python model of pe_batch_verify (engine_batch.cpp, bls_batch_kernels.hip) -- TEST INFRASTRUCTURE ONLY, and the
specification of the call: settle, scale, chunk, multiply, exponentiate, fall back.

    prod_g e(r_g pk_g, H(m_g)) * e(-g1, sum_g r_g sig_g) == 1

Values are those of oracle/g1.py and oracle/g2.py (ints, Fp2 tuples, None = infinity); the pairing is tests/pairing_model.py's.

A group is (pk, msg, sig).  The steps:
  settle    a point off its curve gives 2; an identity key, message point or signature gives 0; a signature outside G2 gives 0.
            What is settled never enters the batch.
  chunk     the live groups in order, c to a chunk; a chunk is the pairs (r pk, msg) of its groups and the one pair
            (-g1, sum r sig): ONE Miller loop, whose value, exponentiated, is 1 iff the chunk is valid.
  multiply  the chunk values, by a tree of fan-in F (launches = levels of that tree).
  top       ONE final exponentiation of the product; 1: every live group is valid.
  fall back otherwise: the final exponentiation of every chunk value, then the groups of the failing chunks one by one, unscaled.

batch_verify returns (verdicts, stats, gt) with stats = (live, chunks, product launches, top-level exponentiations, chunk values
exponentiated in the fallback, groups rechecked, c, F): pe_profile_batch_stats' tuple; gt = the 576 bytes of pe_profile_batch_gt.

By construction.  With pk = a G1, msg = b G2, sig = s G2 every pairing value is e(G1, G2)^x and "is 1" reads "x == 0 (mod r)":
pass dlogs = [(a, b, s), ...] (None for a group the settle pass takes out) and batch_verify decides every product in the
exponent, computing no pairing; gt is then None.  tests/test_batch_verify_model.py holds the two routes to each other.
"""
from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from tests import pairing_model as pm

CHUNK = 2      # the engine's default c (the one that won at 8192 groups: DESIGN.md 3.9)
FAN = 8        # BLS_BATCH_FAN
NEG_G1 = g1.neg(g1.G)
VALID, INVALID, BAD_POINT = 1, 0, 2


def _g1_ok(pt):
    return pt is None or (0 <= pt[0] < P and 0 <= pt[1] < P and g1.is_on_curve(pt))


def _g2_ok(pt):
    return pt is None or (all(0 <= c < P for xy in pt for c in xy) and g2.is_on_curve(pt))


def in_g2(pt):
    return g2.mul(R_ORDER, pt) is None


def settle(group):
    """None for a live group, else its verdict."""
    pk, msg, sig = group
    if not (_g1_ok(pk) and _g2_ok(msg) and _g2_ok(sig)):
        return BAD_POINT
    if pk is None or msg is None or sig is None:
        return INVALID
    if not in_g2(sig):
        return INVALID
    return None


def product_launches(chunks, fan=FAN):
    n = 0
    while chunks > 1:
        chunks = -(-chunks // fan)
        n += 1
    return n


def _tree_product(values, fan):
    while len(values) > 1:
        nxt = []
        for i in range(0, len(values), fan):
            acc = values[i]
            for v in values[i + 1:i + fan]:
                acc = pm.f12_mul(acc, v)
            nxt.append(acc)
        values = nxt
    return values[0]


def batch_verify(groups, scalars, c=CHUNK, fan=FAN, dlogs=None):
    assert len(scalars) == len(groups) and all(0 < r < 1 << 64 for r in scalars)
    verdicts = [settle(g) for g in groups]
    live = [i for i, v in enumerate(verdicts) if v is None]
    for i in live:
        verdicts[i] = VALID
    chunks = [live[k:k + c] for k in range(0, len(live), c)]
    launches = product_launches(len(chunks), fan)
    if not live:
        return verdicts, (0, 0, 0, 0, 0, 0, c, fan), (None if dlogs is not None else pm.gt_bytes(pm.F12_ONE))

    if dlogs is not None:       # every product decided in the exponent of e(G1, G2)
        def excess(i):
            a, b, s = dlogs[i]
            return (a * b - s) % R_ORDER
        chunk_one = [sum(scalars[i] * excess(i) for i in ch) % R_ORDER == 0 for ch in chunks]
        top_one = sum(scalars[i] * excess(i) for i in live) % R_ORDER == 0
        group_one = lambda i: excess(i) == 0
        gt = None
    else:
        values = []
        for ch in chunks:
            pairs = [(g1.mul_unreduced(scalars[i], groups[i][0]), groups[i][1]) for i in ch]
            pairs.append((NEG_G1, g2.sum_points([g2.mul(scalars[i], groups[i][2]) for i in ch])))
            values.append(pm.miller_loop(pairs))
        top = pm.final_exp(_tree_product(values, fan))
        top_one = top == pm.F12_ONE
        gt = pm.gt_bytes(top)
        chunk_one = None
        group_one = lambda i: pm.pairing_product([(groups[i][0], groups[i][1]), (NEG_G1, groups[i][2])]) == pm.F12_ONE

    if top_one:
        return verdicts, (len(live), len(chunks), launches, 1, 0, 0, c, fan), gt
    if chunk_one is None:
        chunk_one = [pm.final_exp(v) == pm.F12_ONE for v in values]
    rechecked = 0
    for ch, ok in zip(chunks, chunk_one):
        if ok:
            continue
        for i in ch:
            rechecked += 1
            verdicts[i] = VALID if group_one(i) else INVALID
    return verdicts, (len(live), len(chunks), launches, 1, len(chunks), rechecked, c, fan), gt

