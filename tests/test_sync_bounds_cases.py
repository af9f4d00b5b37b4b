"""CPU: the cases of tests/sync_bounds_cases.py, judged from the models alone (tests/sync_committee_model.py,
tests/epoch_model.py).  Coverage: the candidates the sampling examines meet every way the 128-bit comparison can be decided;
the reward batches saturate, re-credit, wrap and own proposers beyond aggregate 36; the sampling cases need a third candidate
batch.  Bite: each of seven plausible wrong kernels, restated as a mutant of the model, differs from the model in an output
tests/test_gpu_sync_bounds.py asserts.  No kernel runs here and none is broken: the mutants are Python."""
import collections
import functools

import pytest

from tests import epoch_model
from tests import sync_bounds_cases as C
from tests import sync_committee_model as M

A_CASES = C.acceptance_cases()
B_CASES = C.rewards_cases()
U64 = 2**64


# ---------------------------------------------------------------- A
@functools.lru_cache(maxsize=None)
def _a_runs(rule=C.true_rule):
    """Every asserted output of family A under an acceptance rule: {(case, entry point, k): (members | proposer, tries)}."""
    out = {}
    for c in A_CASES:
        for k, sd in enumerate(c["proposer_seeds"]):
            members, tries = C.sample(c["indices"], c["bal"], sd, c["rounds"], c["max_eff"], 1, epoch_model.DEFAULT_MAX_TRIES, rule)
            out[c["name"], "proposer", k] = (None, tries) if members is None else (members[0], tries - 1)
        for k, (size, sd) in enumerate(c["syncs"]):
            out[c["name"], f"sync{size}", k] = C.sample(c["indices"], c["bal"], sd, c["rounds"], c["max_eff"], size, 1 << 17, rule)
    return out


def test_sample_is_the_models_sampling():
    for c in A_CASES:
        for k, sd in enumerate(c["proposer_seeds"]):
            assert _a_runs()[c["name"], "proposer", k] == epoch_model.proposer(c["indices"], c["bal"], sd, c["rounds"], c["max_eff"])
        for k, (size, sd) in enumerate(c["syncs"]):
            want = M.next_sync_committee_indices(c["indices"], c["bal"], sd, c["rounds"], c["max_eff"], size)
            assert want[0] is not None and _a_runs()[c["name"], f"sync{size}", k] == want


def test_acceptance_cases_reach_every_kind_of_decision():
    kinds = collections.Counter()
    per_case = collections.defaultdict(collections.Counter)
    n_examined = 0
    for c in A_CASES:
        runs = [(sd, _a_runs()[c["name"], "proposer", k][1] + 1) for k, sd in enumerate(c["proposer_seeds"])]
        runs += [(sd, _a_runs()[c["name"], f"sync{size}", k][1]) for k, (size, sd) in enumerate(c["syncs"])]
        for sd, tries in runs:
            for _, candidate, byte in C.examined(c["indices"], sd, c["rounds"], tries):
                kind = C.acceptance_kind(c["bal"][candidate], c["max_eff"], byte)
                kinds[kind] += 1
                per_case[c["name"]][kind] += 1
                n_examined += 1
    print("A: candidates examined", n_examined, dict(kinds), {k: dict(v) for k, v in per_case.items()})
    for kind in ("equal", "high_equal_accepts", "high_equal_rejects", "high_differs"):
        assert kinds[kind] >= 3, (kind, kinds)
    # the ladder alone sees them, on both sides of the equality, and products beyond 64 bits are the rule, not the exception
    ladder = per_case["ladder-257"]
    assert min(ladder["equal"], ladder["high_equal_accepts"], ladder["high_equal_rejects"]) >= 3, ladder
    assert {len(c["indices"]) for c in A_CASES} == {3, 257}
    assert all(len(c["proposer_seeds"]) >= 8 and {s for s, _ in c["syncs"]} == {64, 512} for c in A_CASES)
    assert any(b * 255 >= U64 for c in A_CASES for b in c["bal"]) and any(c["max_eff"] * 255 >= U64 for c in A_CASES)


def _mod64(eb, max_eff, byte):           # both products in 64 bits
    return (eb * 255) % U64 >= (max_eff * byte) % U64


def _low_unguarded(eb, max_eff, byte):   # l_hi > r_hi || l_lo >= r_lo: the low words compared whether the high ones are equal or not
    left, right = eb * 255, max_eff * byte
    return left >> 64 > right >> 64 or left % U64 >= right % U64


def _high_only(eb, max_eff, byte):       # (an eighth, for the low-word-rejects kind) the low words never compared
    return (eb * 255) >> 64 >= (max_eff * byte) >> 64


@pytest.mark.parametrize("rule", [_mod64, _low_unguarded, _high_only], ids=lambda r: r.__name__)
def test_acceptance_mutants_are_caught(rule):
    got = _a_runs(rule)
    caught = [key for key in got if got[key] != _a_runs()[key]]
    print("A mutant", rule.__name__, "first caught by", caught[0] if caught else None, "of", len(caught))
    assert caught
    assert {key[1] == "proposer" for key in caught} == {True, False}    # through both entry points


# ---------------------------------------------------------------- B
def _rewards_variant(c, blind_from=None, members_only=False, window=None):
    """M.process_sync_aggregates, or one of three wrong kernels:
    blind_from    aggregates b >= blind_from read as all-zero bits (the staging loop's second trip lost); the participants'
                  count is k_sync_members' and stays right
    members_only  a proposer outside the committee is never paid (no proposer lanes)
    window        a proposer lane looks for an earlier lane with its validator among the `window` aggregates before it only:
                  one seen longer ago gets a second owner; both owners replay the same events and store the same balance,
                  so the balances are right and the validator's credits are counted twice
    -> (balances, stats)"""
    pr, qr = M.reward_scalars(c["total"], c["size"])
    bal = list(c["bal"])
    inside = set(c["members"])
    stats = {"n_participants": 0, "credited": 0, "debited": 0, "n_saturated": 0}
    paid = collections.Counter()
    for b, (bits, proposer) in enumerate(c["aggs"]):
        stats["n_participants"] += len(M.participants(c["members"], bits))
        if blind_from is not None and b >= blind_from:
            bits = bytes(64)
        for p, v in enumerate(c["members"]):
            if M.bit(bits, p):
                bal[v] = (bal[v] + pr) % U64
                stats["credited"] += pr
                if not members_only or proposer in inside:
                    bal[proposer] = (bal[proposer] + qr) % U64
                    stats["credited"] += qr
                    paid[proposer] += qr
            else:
                cut = min(bal[v], pr)
                stats["n_saturated"] += bal[v] < pr
                bal[v] -= cut
                stats["debited"] += cut
    if window is not None:
        proposers = [p for _, p in c["aggs"]]
        for b, v in enumerate(proposers):
            if v not in inside and v in proposers[:b] and v not in proposers[max(0, b - window):b]:
                stats["credited"] += paid[v]
    return bal, stats


def _rewards_model(c):
    pr, qr = M.reward_scalars(c["total"], c["size"])
    bal = list(c["bal"])
    return bal, M.process_sync_aggregates(bal, c["members"], c["aggs"], pr, qr)


@functools.lru_cache(maxsize=None)
def _b_true(name):
    return _rewards_model(next(c for c in B_CASES if c["name"] == name))


def test_rewards_cases_cover_the_batch_bounds():
    assert {(c["size"], c["n"]) for c in B_CASES} == {(s, n) for s in (65, 512) for n in (4, 36, 37, 63, 64)}
    seen = collections.Counter()
    for c in B_CASES:
        pr, qr = M.reward_scalars(c["total"], c["size"])
        assert pr > 2 and len(c["bal"]) == C.N_VAL_REWARDS
        members, aggs, n = c["members"], c["aggs"], c["n"]
        assert _rewards_variant(c) == _b_true(c["name"])                         # the variant with nothing wrong is the model
        events, left = C.reward_trace(c["bal"], members, aggs, pr, qr)
        assert left == _b_true(c["name"])[0]
        assert len({bits for bits, _ in aggs}) == n                             # every aggregate different
        density = sum(len(M.participants(members, bits)) for bits, _ in aggs) / (n * c["size"])
        assert 0.45 < density < 0.65, density
        inside, proposers = set(members), [p for _, p in aggs]
        distinct = len(inside)
        seen["few"] += distinct <= 40 and c["size"] / distinct > 1.5
        seen["few-512"] += c["size"] == 512 and 2 < distinct <= 41 and c["size"] / distinct > 12
        seen["solo-512"] += c["size"] == 512 and distinct == 1
        seen["words 14 and 15 only"] += any(not any(bits[:56]) and any(bits[56:]) for bits, _ in aggs)
        seen["words 14 and 15 only, b >= 36"] += any(not any(bits[:56]) and any(bits[56:]) for bits, _ in aggs[C.STAGE_STRIDE:])
        seen["saturated"] += _b_true(c["name"])[1]["n_saturated"] > 0
        for v, ev in events.items():
            what = [w for _, w in ev]
            if "cut0" in what:
                seen["cut at 0, credited later"] += any(w in ("credit", "proposer") for w in what[what.index("cut0"):])
            if "credit" in what:
                seen["credited, cut later"] += any(w in ("cut", "cut0") for w in what[what.index("credit"):])
            seen["wrap"] += "wrap" in what and v == C.WRAPPER
            if v not in inside:
                seen["owner at b >= 36"] += ev[0][0] >= C.STAGE_STRIDE and proposers.index(v) >= C.STAGE_STRIDE
        for b, (bits, v) in enumerate(aggs):
            where = [p for p, m in enumerate(members) if m == v]
            seen["proposer outside"] += not where
            seen["proposer present"] += any(M.bit(bits, p) for p in where)
            seen["proposer absent"] += any(not M.bit(bits, p) for p in where)
            seen["proposer first listed at 511"] += where == [511]
        seen["one proposer for all, n >= 37"] += len(set(proposers)) == 1 and n > C.STAGE_STRIDE
        seen["ends only"] += n >= 3 and proposers[0] == proposers[-1] and proposers.count(proposers[0]) == 2
        seen["ends only, n = 64"] += n == 64 and proposers[0] == proposers[-1] and proposers.count(proposers[0]) == 2
    print("B:", len(B_CASES), "cases", dict(seen))
    for name in ("few", "few-512", "solo-512", "words 14 and 15 only", "words 14 and 15 only, b >= 36", "saturated",
                 "cut at 0, credited later", "credited, cut later", "wrap", "owner at b >= 36", "proposer outside", "proposer present",
                 "proposer absent", "proposer first listed at 511", "one proposer for all, n >= 37", "ends only", "ends only, n = 64"):
        assert seen[name] > 0, name


@pytest.mark.parametrize("name,mutant", [("blind from 36", dict(blind_from=C.STAGE_STRIDE)), ("members only", dict(members_only=True)),
                                         ("window 32", dict(window=32))])
def test_rewards_mutants_are_caught(name, mutant):
    caught = [c["name"] for c in B_CASES if _rewards_variant(c, **mutant) != _b_true(c["name"])]
    print("B mutant", name, "first caught by", caught[0] if caught else None, "of", len(caught))
    assert caught
    if "blind_from" in mutant:   # and by the balances alone, not only through the totals
        assert any(_rewards_variant(c, **mutant)[0] != _b_true(c["name"])[0] for c in B_CASES)


# ---------------------------------------------------------------- C
def _verdicts(members, rows, participants=M.participants, scatter=True):
    """-> (verdicts, statuses, n_participants); scatter False: what the pairing returns lands at its own index t, not at the
    position good[t] of the aggregate it belongs to."""
    triples = [C.model_verdict(members, r, participants) for r in rows]
    verdicts = [t[0] for t in triples]
    if not scatter:
        good = [b for b, (r, t) in enumerate(zip(rows, triples)) if t[2] and t[1] == 0 and r["signature"] is None]
        verdicts = [0 if b in good else v for b, v in enumerate(verdicts)]
        for t, b in enumerate(good):
            verdicts[t] = triples[b][0]
    return verdicts, [t[1] for t in triples], sum(t[2] for t in triples)


def _once(members, bits):
    return sorted(set(M.participants(members, bits)))


def test_verdict_batches_interleave_and_their_mutants_are_caught():
    members, rows = C.verdict_batch()
    assert len(rows) == C.MAX_AGGS and len(members) == 65 and members[0] == members[2]
    verdicts, statuses, _ = _verdicts(members, rows)
    kinds = collections.Counter(r["kind"].split("-")[0] if r["kind"].startswith("valid") else r["kind"] for r in rows)
    print("C:", dict(kinds), "verdicts", "".join(map(str, verdicts)))
    for kind in ("valid", "nobody", "nobody-signed", "flipped", "wrong-root", "undecodable", "once", "infinity"):
        assert kinds[kind] > 0, kind
    for b in (0, 37, 63):       # an invalid one with an empty one beside it
        assert verdicts[b] == 0 and any(rows[q]["kind"] == "nobody" and verdicts[q] == 1 for q in (b - 1, b + 1) if 0 <= q < 64)
    assert statuses[63] == 1 and rows[0]["kind"] == "flipped" and rows[37]["kind"] == "wrong-root"
    assert all(v == (r["kind"].startswith("valid") or r["kind"] == "nobody") for v, r in zip(verdicts, rows))
    signatures = {(r["sk"], r["signed_root"]) for r in rows if r["signature"] is None}
    assert len(signatures) <= 6, len(signatures)
    fixed_members, fixed = C.verdict_batch(valid_only=True)
    assert fixed_members == members and _verdicts(members, fixed)[0] == [1] * 64
    assert {(r["sk"], r["signed_root"]) for r in fixed if r["signature"] is None} <= signatures
    assert [r["positions"] == [] for r in fixed] == [r["positions"] == [] for r in rows]
    wide_members, wide = C.wide_verdict_batch()
    wide_verdicts = _verdicts(wide_members, wide)[0]
    assert len(wide) == 64 and len({(r["sk"], r["signed_root"]) for r in wide if r["signature"] is None}) == 3
    assert any(r["positions"] == list(range(512)) for r in wide) and 0 < sum(wide_verdicts) < 64
    assert [wide_verdicts[b] for b in (0, 37, 63)] == [0, 0, 0]
    for name, kw in (("participants without duplicates", dict(participants=_once)), ("group order", dict(scatter=False))):
        caught = [tag for tag, (m, r) in (("65", (members, rows)), ("65 repaired", (members, fixed)), ("512", (wide_members, wide)))
                  if _verdicts(m, r, **kw) != _verdicts(m, r)]
        print("C mutant", name, "first caught by", caught[0] if caught else None, "of", len(caught))
        assert caught


def test_out_of_range_bits_sit_at_the_size_and_at_the_end():
    cases = C.out_of_range_cases()
    assert {s for s, _, _ in cases} == {1, 63, 64, 65, 511} and {b for _, b, _ in cases} == {0, 63}
    for size, b, position in cases:
        members, rows = C.out_of_range_batch(size, b, position)
        assert position in (size, 511) and len(rows) == 64
        for k, r in enumerate(rows):
            stray = [p for p in range(512) if M.bit(r["bits"], p) and p >= size]
            assert stray == ([position] if k == b else [])
    assert {(s, p) for s, _, p in cases} >= {(s, s) for s in (1, 63, 64, 65, 511)} | {(s, 511) for s in (1, 63, 64, 65)}


# ---------------------------------------------------------------- D
def test_sampling_cases_need_a_third_batch():
    tries = []
    for c in C.three_batch_cases():
        members, t = M.next_sync_committee_indices(range(c["n_val"]), c["bal"], c["seed"], c["rounds"], C.MAX_EFF, c["size"])
        assert members is not None and t > 2 * C.BATCH
        tries.append(t)
    print("D: tries", tries)
    assert tries == [42949, 42234, 45272]
    assert any(t % C.BATCH not in (0, 1) for t in tries)     # max_tries = tries - 1 falls inside a batch
    c = C.exhaustion_case()
    assert c["max_tries"] == 2 * C.BATCH + 1
    got = M.next_sync_committee_indices(range(c["n_val"]), c["bal"], c["seed"], c["rounds"], C.MAX_EFF, c["size"], c["max_tries"])
    assert got == (None, c["max_tries"])
    reached = C.sample(list(range(c["n_val"])), c["bal"], c["seed"], c["rounds"], C.MAX_EFF, 1, c["max_tries"])
    assert reached[0] is not None                            # a zero balance is accepted at byte 0: some are, not 512
