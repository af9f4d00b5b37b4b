"""Inputs that hold the sync-committee and proposer kernels (sync_kernels.hip, sample_walk.h, engine_sync.cpp) at their
bounds, as plain data built from fixed seeds; no GPU here.  tests/test_sync_bounds_cases.py checks from the models alone
(tests/sync_committee_model.py, tests/epoch_model.py) that the cases reach what they are meant to reach and that they tell
plausible wrong kernels from the right one; tests/test_gpu_sync_bounds.py holds the engine to the models on the same cases.

  A  acceptance_cases()  effective_balance * 255 >= max_effective_balance * byte where only 128-bit products decide
  B  rewards_cases()     k_sync_rewards at 4, 36, 37, 63 and 64 aggregates: the second trip of the bit staging, the proposer
                         lanes up to 63, first-appearance ownership over up to 63 earlier proposers
  C  verdict_batch() / wide_verdict_batch() / out_of_range_cases()   k_sync_members and the verdict composition at 64
                         aggregates: empty, valid, invalid and undecodable ones interleaved
  D  three_batch_cases() / exhaustion_case()   k_sync_append's running count across three candidate batches"""
import hashlib

import numpy as np

from tests import sync_committee_model as M

ETH = 10**9
MAX_EFF = 32 * ETH
BATCH = 16384                       # kernels.h: SYNC_SAMPLE_BATCH
MAX_AGGS = 64                       # PE_SYNC_MAX_BATCH
STAGE_STRIDE = 36                   # k_sync_rewards stages 576 words a trip = the bits of 36 aggregates
A_SK, B_SK = 0x1234567, 0x89ABCDE   # sk_v = A + v B: synth.registry_points' progression
WIDE_INCREMENT = 2**48              # effective_balance / increment fits the engine's 16 bits for every uint64


def seed(tag, k=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), k)).digest()


def bits_of(positions):
    b = bytearray(64)
    for p in positions:
        b[p // 8] |= 1 << (p % 8)
    return bytes(b)


# ================================================================ A: acceptance over the whole u64 range
K = 2**56
LADDER_MAX_EFF = 255 * K            # eb = j K: eb * 255 == max_eff * byte exactly at byte == j
TOP = 2**64 - 1
INV255 = 0xFEFEFEFEFEFEFEFF         # 255 * INV255 = 1 (mod 2^64)
REP01 = 0x0101010101010101          # 255 * REP01 = 2^64 - 1
LADDER_LEVELS = (1, 2, 3, 5, 128, 254, 255)


def true_rule(eb, max_eff, byte):
    return eb * 255 >= max_eff * byte


def acceptance_kind(eb, max_eff, byte):
    """Where the comparison of the two 128-bit products is decided."""
    left, right = eb * 255, max_eff * byte
    if left == right:
        return "equal"
    if left >> 64 != right >> 64:
        return "high_differs"
    return "high_equal_accepts" if left > right else "high_equal_rejects"


def random_byte(sd, i):
    return hashlib.sha256(bytes(sd) + (i // 32).to_bytes(8, "little")).digest()[i % 32]


def examined(indices, sd, rounds, tries):
    """(i, candidate, random byte) of the first `tries` candidates of the sampling loop."""
    walk = M.Walk(sd, len(indices), rounds)
    for i in range(tries):
        yield i, int(indices[walk(i % len(indices))]), random_byte(sd, i)


def sample(indices, bal, sd, rounds, max_eff, size, max_tries=1 << 20, rule=true_rule):
    """M.next_sync_committee_indices with the acceptance rule as an argument (the CPU test holds it to M with true_rule)."""
    members = []
    for i, candidate, byte in examined(indices, sd, rounds, max_tries):
        if rule(int(bal[candidate]), max_eff, byte):
            members.append(candidate)
            if len(members) == size:
                return members, i + 1
    return None, max_tries


def _ladder(n_val, levels):
    """j K, j K - 1 and j K + 1 over the levels.  With j K and j K - 1 alone the high words are equal only at byte == j (255 j K
    has high word j - 1, as 255 K byte has byte - 1), where j K is the exact equality and j K - 1 loses in the low word; j K + 1
    wins there in the low word."""
    return [levels[v % len(levels)] * K + (0, -1, 1)[(v // len(levels)) % 3] for v in range(n_val)]


def acceptance_cases():
    """-> [dict(name, max_eff, bal, n_val, active: int | sorted list, rounds, proposer_seeds, syncs: [(size, seed)])]"""
    rng = np.random.default_rng(255)
    subset = sorted(int(v) for v in rng.choice(300, size=257, replace=False))
    top = [TOP, 2**63, 2**63 - 1, 2**56, 1, 0]
    one = [TOP, 2**63, INV255, REP01, REP01 + 1, 2**56, 1, 0]
    cases = [
        dict(name="ladder-257", max_eff=LADDER_MAX_EFF, bal=_ladder(300, LADDER_LEVELS), active=subset,
             syncs=[(64, 0), (512, 1), (512, 2), (512, 3), (512, 4)]),
        dict(name="ladder-3", max_eff=LADDER_MAX_EFF, bal=[200 * K, 200 * K - 1, 200 * K + 1, 0, TOP], active=3,
             syncs=[(64, 0), (512, 1)]),
        dict(name="top-257", max_eff=TOP, bal=[top[v % 6] for v in range(270)], active=257, syncs=[(64, 0), (512, 1)]),
        dict(name="top-3", max_eff=TOP, bal=[2**63, 2**63 - 1, 2**56, TOP, 0], active=3, syncs=[(64, 0), (512, 1)]),
        dict(name="one-257", max_eff=1, bal=[one[v % 8] for v in range(270)], active=257, syncs=[(64, 0), (512, 1)]),
        dict(name="one-3", max_eff=1, bal=[INV255, 0, TOP, 1, 1], active=3, syncs=[(64, 0), (512, 1)]),
    ]
    for c in cases:
        c["n_val"] = len(c["bal"])
        c["rounds"] = 10
        c["indices"] = list(range(c["active"])) if isinstance(c["active"], int) else c["active"]
        c["proposer_seeds"] = [seed("bounds-p-" + c["name"], k) for k in range(8)]
        c["syncs"] = [(size, seed("bounds-s-" + c["name"], k)) for size, k in c["syncs"]]
    return cases


# ================================================================ B: rewards at the batch bounds
N_VAL_REWARDS = 700
WRAPPER = 77                        # starts at 2^64 - 1 - participant_reward / 2: its first credit wraps


def _few(size, rng, last_unique):
    """`size` positions over 40 validators (WRAPPER among them); with last_unique the last position lists a validator no
    other position lists."""
    pool = [int(v) for v in rng.choice(np.arange(100, 400), size=39, replace=False)] + [WRAPPER]
    members = [pool[int(k)] for k in rng.integers(0, 40, size=size)]
    members[1] = WRAPPER
    if last_unique:
        members[size - 1] = 450
    return members


def rewards_cases():
    """-> [dict(name, size, n, members, total, bal, aggs: [(bits, proposer)], last_unique)] over N_VAL_REWARDS validators.
    Proposer schemes: "mixed" -- the same outside validator at b = 0 and b = n - 1 only, the member first listed at the last
    position at b = 1 (where the committee has one), then outside validators (a new one every time), present members and
    absent members in turn; "one" -- one validator for all n."""
    cases = []
    plan = [(65, 4, "few", "mixed"), (65, 36, "few", "mixed"), (65, 37, "few", "one-outside"), (65, 63, "few", "mixed"),
            (65, 64, "few", "mixed"), (512, 4, "few", "mixed"), (512, 36, "solo", "mixed"), (512, 37, "few", "mixed"),
            (512, 63, "few", "one-member"), (512, 64, "few", "mixed"), (512, 64, "solo", "one-outside")]
    for size, n, committee, scheme in plan:
        rng = np.random.default_rng(1000 * size + 10 * n + len(committee) + len(scheme))
        last_unique = committee == "few" and size == 512
        members = [WRAPPER] * size if committee == "solo" else _few(size, rng, last_unique)
        total = int(rng.integers(20_000, 900_000)) * 32 * ETH
        pr, _ = M.reward_scalars(total, size)
        bal = [int(b) for b in rng.choice(np.array([0, 1, pr - 1, pr, pr + 1, 3 * pr, 32 * ETH], dtype=np.uint64), size=N_VAL_REWARDS)]
        bal[WRAPPER] = 2**64 - 1 - pr // 2
        inside = set(members)
        outside = iter(v for v in range(500, N_VAL_REWARDS) if v not in inside)
        ends = next(outside)
        fixed = next(outside)
        aggs = []
        for b in range(n):
            positions = [p for p in range(size) if rng.random() < 0.6]
            if size == 512 and b == min(n - 1, 40):       # only words 14 and 15
                positions = [p for p in range(448, 512) if rng.random() < 0.6]
            if committee == "solo" and b % 5 == 2:        # the one validator cut about 500 times: down to 0 from anywhere
                positions = [p for p in range(size) if rng.random() < 0.02]
            on, off = [p for p in positions], sorted(set(range(size)) - set(positions))
            if scheme == "one-outside":
                proposer = fixed
            elif scheme == "one-member":
                proposer = members[7]
            elif b in (0, n - 1):
                proposer = ends
            elif b == 1 and last_unique:
                proposer = members[size - 1]
            elif b % 3 == 0 or (b % 3 == 1 and not on) or (b % 3 == 2 and not off):
                proposer = next(outside)
            elif b % 3 == 1:
                proposer = members[on[int(rng.integers(0, len(on)))]]     # a present member
            else:
                proposer = members[off[int(rng.integers(0, len(off)))]]   # an absent member
            aggs.append((bits_of(positions), int(proposer)))
        cases.append(dict(name=f"{size}x{n}-{committee}-{scheme}", size=size, n=n, members=members, total=total, bal=bal, aggs=aggs,
                          last_unique=last_unique))
    return cases


def reward_trace(bal, members, aggs, pr, qr):
    """The reference's loop once more, keeping per validator the order of what happened to it:
    -> ({validator: [(b, "credit" | "wrap" | "cut" | "cut0" | "proposer")]}, the balances it leaves) -- "wrap": a credit that
    passed 2^64; "cut0": a decrease that met less than the reward."""
    bal = list(bal)
    events = {}
    for b, (bits, proposer) in enumerate(aggs):
        for p, v in enumerate(members):
            if M.bit(bits, p):
                if bal[v] + pr >= 2**64:
                    events.setdefault(v, []).append((b, "wrap"))
                bal[v] = (bal[v] + pr) % 2**64
                bal[proposer] = (bal[proposer] + qr) % 2**64
                events.setdefault(v, []).append((b, "credit"))
                events.setdefault(proposer, []).append((b, "proposer"))
            else:
                events.setdefault(v, []).append((b, "cut0" if bal[v] < pr else "cut"))
                bal[v] -= min(bal[v], pr)
    return events, bal


# ================================================================ C: participants and verdicts at 64 aggregates
N_VAL_VERDICTS = 600
ROOT, DOMAIN = hashlib.sha256(b"block").digest(), bytes([7, 0, 0, 0]) + hashlib.sha256(b"fork").digest()[:28]
OTHER_ROOT = hashlib.sha256(b"other").digest()
UNDECODABLE = bytes([0x9F]) + b"\xff" * 95   # compressed, x.c1 >= p


def committee(size, n_val=N_VAL_VERDICTS):
    """test_gpu_sync_committee._committee: `size` members with a duplicate pair at positions 0 and 2."""
    rng = np.random.default_rng(size)
    members = [int(v) for v in rng.integers(0, n_val, size=size)]
    if size >= 3:
        members[2] = members[0]
    return members


def secret_sum(members, positions):
    return sum(A_SK + int(members[p]) * B_SK for p in positions)


def _row(kind, members, positions, proposer, signed_positions=None, signed_root=ROOT, signature=None):
    """One aggregate as data.  signature: None = the secret sum of the members at signed_positions (default the
    participants) over (signed_root, DOMAIN); "infinity"; "undecodable"."""
    if signature is None and not positions and signed_positions is None:
        signature = "infinity"
    signed = positions if signed_positions is None else signed_positions
    return dict(kind=kind, positions=list(positions), bits=bits_of(positions), proposer=int(proposer), root=ROOT, domain=DOMAIN,
                signature=signature, sk=None if signature else secret_sum(members, signed), signed_root=signed_root)


def model_verdict(members, row, participants=M.participants):
    """eth_fast_aggregate_verify over keys sk_v G: -> (verdict, sig_status, number of participants)."""
    who = participants(members, row["bits"])
    if row["signature"] == "undecodable":
        return 0, 1, len(who)
    if not who:
        return int(row["signature"] == "infinity"), 0, 0
    if row["signature"] == "infinity":
        return 0, 0, len(who)
    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    key = sum(A_SK + v * B_SK for v in who) % r
    return int(key != 0 and row["sk"] % r == key and row["signed_root"] == row["root"]), 0, len(who)


def _sets65(members):
    rng = np.random.default_rng(65)
    return {"everyone": list(range(65)), "last": [64], "pair": [0, 2], "dense": [p for p in range(65) if rng.random() < 0.6]}


def verdict_batch(valid_only=False):
    """-> (members, rows): 64 aggregates over committee(65).  Four participant sets, the whole committee over another root and
    the duplicate member's key once: six signatures.  Invalid ones at b = 0, 37 and 63 with an empty one next to each;
    valid_only puts a valid one in the place of every invalid one."""
    members = committee(65)
    sets = _sets65(members)
    names = list(sets)

    def valid(b):
        return _row("valid-" + names[b % 4], members, sets[names[b % 4]], proposer=(37 * b) % N_VAL_VERDICTS)

    def nobody(b):
        return _row("nobody", members, [], proposer=b)

    makers = {
        "flipped": lambda b: _row("flipped", members, sets["everyone"][:-1], b, signed_positions=sets["everyone"]),
        "wrong-root": lambda b: _row("wrong-root", members, sets["everyone"], b, signed_root=OTHER_ROOT),
        "undecodable": lambda b: _row("undecodable", members, sets["dense"], b, signature="undecodable"),
        "nobody-signed": lambda b: _row("nobody-signed", members, [], b, signed_positions=sets["last"]),
        "once": lambda b: _row("once", members, sets["pair"], b, signed_positions=[0]),   # the duplicate's key counted once
        "infinity": lambda b: _row("infinity", members, sets["last"], b, signature="infinity"),
    }
    layout = {0: "flipped", 1: "nobody", 36: "nobody", 37: "wrong-root", 38: "nobody", 62: "nobody", 63: "undecodable",
              5: "nobody-signed", 6: "nobody", 11: "once", 12: "undecodable", 20: "nobody", 21: "nobody", 22: "flipped",
              33: "infinity", 34: "wrong-root", 45: "nobody-signed", 50: "nobody", 51: "flipped", 57: "nobody"}
    rows = []
    for b in range(MAX_AGGS):
        what = layout.get(b)
        if what == "nobody":
            rows.append(nobody(b))
        elif what is None:
            rows.append(valid(b))
        elif not valid_only:
            rows.append(makers[what](b))
        else:   # a valid one in its place (no new signature): nobody stays nobody, now with the infinity signature
            rows.append(nobody(b) if what == "nobody-signed" else valid(b))
    return members, rows


def wide_verdict_batch():
    """-> (members, rows): 64 aggregates over committee(512): everyone, a 0.6-dense set and the first and last lane of every
    wave (three signatures), flipped copies and empty ones among them."""
    members = committee(512)
    rng = np.random.default_rng(512)
    edges = sorted({0, 2} | {64 * w for w in range(8)} | {64 * w + 63 for w in range(8)})
    sets = [list(range(512)), [p for p in range(512) if rng.random() < 0.6], edges]
    rows = []
    for b in range(MAX_AGGS):
        s = sets[b % 3]
        if b % 7 == 3:
            rows.append(_row("nobody", members, [], b))
        elif b in (0, 37, 63) or b % 11 == 5:   # one participant's bit cleared under the whole set's signature
            drop = s[(5 * b) % len(s)]
            rows.append(_row("flipped", members, [p for p in s if p != drop], b, signed_positions=s))
        else:
            rows.append(_row("valid", members, s, b))
    return members, rows


def out_of_range_cases():
    """-> [(size, b, position)]: a set bit at position `size` exactly, and at 511, in aggregate b = 0 and b = 63 of a full batch."""
    out = []
    for size in (1, 63, 64, 65, 511):
        for position in sorted({size, 511}):
            out += [(size, 0, position), (size, MAX_AGGS - 1, position)]
    return out


def out_of_range_batch(size, b, position):
    """64 aggregates over range(size) as the committee, honest and unsigned (nobody, or participants under SYNC_APPLY), the one
    at b with the stray bit."""
    members = list(range(size))
    rows = [_row("plain", members, [p for p in range(size) if (p + k) % 3 == 0], k, signature="infinity") for k in range(MAX_AGGS)]
    rows[b] = _row("stray", members, rows[b]["positions"] + [position], b, signature="infinity")
    return members, rows


# ================================================================ D: sampling across three candidate batches
def three_batch_cases():
    """1 000 validators at 0.3 ETH against 32: bytes 0 .. 2 accept, 3 in 256 -- 512 members take about 43 700 candidates."""
    return [dict(n_val=1000, bal=[3 * ETH // 10] * 1000, seed=seed("third", k), rounds=10, size=512) for k in range(3)]


def exhaustion_case():
    """Nobody holds anything: only byte 0 accepts, and 2 * BATCH + 1 candidates yield about 128 members of the 512 asked for."""
    return dict(n_val=1000, bal=[0] * 1000, seed=seed("exhaust"), rounds=10, size=512, max_tries=2 * BATCH + 1)
