"""-m gpu: the workgroup-count scans of the withdrawal sweep and of the block operations (k_withdrawals_scan, k_block_ops_scan)
past one wave of counts and past one tile, the call's last lane of k_block_ops_apply at every residue of n_slots, and the search
over the operations' slot offsets (block_ops_op_of_slot) over a long table.  The helpers, the models and the rule are those of
tests/test_gpu_withdrawals.py and tests/test_gpu_block_ops.py: every comparison is bit for bit against the sequential loops
(W.process_withdrawals_sequential, B.block_operations_sequential), there is no tolerance anywhere in this file, and no SSZ root
is asked for at these sizes (the roots are held at the small ones).

256 = the positions or slots of one workgroup AND the counts of one scan tile, 64 = a wave.  A scan walks n_wg counts:
  n_wg <= 64         one wave of counts; the other waves' totals are zero          (the two older files stay here)
  64 < n_wg <= 256   the cross-wave term `before += wave_total[w]`
  n_wg > 256         the tile loop: the carry, the second barrier, the ragged last tile
so the large shapes are the smallest that reach the code: 256 * 258 + 77 swept validators = 259 workgroups, and 33 000 validators
under two whole-registry attester slashings = 131 925 slots = 516 workgroups.  Every case first asserts, on the model's layout
alone, the workgroups (position // 256, slot // 256) its hits or events lie in: a change to a helper cannot move it back into the
first regime unseen.

Where a rank alone decides (the withdrawals), the same hits are also run as FEWER than k = 64 beside k = 16: behind a wrong offset
a hit of rank >= k would only race another for a record, a hit of rank < k leaves its own record unwritten.  Where the proposer is
slashed, its balance is its penalty minus the rewards the loop has paid before it: one reward less in the prefix saturates it."""
import numpy as np
import pytest

from tests import block_ops_cases as K
from tests import block_ops_model as B
from tests import registry_updates_model as M
from tests import test_gpu_block_ops as TB
from tests import test_gpu_withdrawals as TW
from tests import withdrawals_model as W
from tests.test_withdrawals_model import EPOCH

pytestmark = pytest.mark.gpu
CUR = K.CUR
WG = 256  # WD_WG = BLOCK_OPS_WG = the scan's tile


def wgs(places):
    return [int(x) // WG for x in places]


# ================================================================ withdrawals: 259 workgroups, the last tile ragged
N_WD = WG * 258 + 77


def lane_pos(w):
    """the one hit of workgroup w, in a lane that moves with w"""
    return w * WG + (w * 37) % WG


@pytest.fixture(scope="module")
def wd_big():
    """one blank registry of N_WD validators and its keys; never written: a case arms a copy"""
    return W.blank_registry(N_WD), TW.keys(N_WD)


def wd_load(e, a, keys):
    """test_gpu_withdrawals.load with the keys made once"""
    n = len(a["bal"])
    flags = np.ones(n, dtype=np.uint8)
    e.set_validators(a["eff"], flags)
    e.state_set_validators(a["eff"], (flags | 8).astype(np.uint8))
    e.registry_set_epochs(np.zeros(n, dtype=np.uint64), np.full(n, W.FAR, dtype=np.uint64))
    e.state_set_balances(a["bal"], None, a["wdr"])
    e.registry_set_static(keys, a["cred"], np.zeros(n, dtype=np.uint64))


def wd_arm(e, wd_big, positions, start):
    """hits at the given sweep POSITIONS of a sweep that starts at `start` -> (the registry, the validators in position order)"""
    blank, keys = wd_big
    assert all(0 <= j < N_WD for j in positions) and sorted(positions) == list(positions)
    validators = [(start + j) % N_WD for j in positions]
    a = W.set_hits(W.copy_registry(blank), validators)
    wd_load(e, a, keys)
    return a, validators


def wd_shape(bound):
    """(workgroups, scan tiles, counts in the last tile, positions in the last workgroup)"""
    n_wg = -(-bound // WG)
    return n_wg, -(-n_wg // WG), (n_wg - 1) % WG + 1, (bound - 1) % WG + 1


def wd_compute_then_apply(e, a, start, p, validators):
    """k = max_withdrawals_per_payload hits or more: the k-th is debited, the one behind it is not"""
    k = p.max_withdrawals_per_payload
    last, behind = validators[k - 1], validators[k]
    _, expected, _ = TW.check(e, a, EPOCH, 7, start, p)
    b, _, res = TW.check(e, a, EPOCH, 7, start, p, expected, True)
    assert res["applied"] == 1 and [w[1] for w in expected] == validators[:k]
    assert expected[-1][1] == last and res["next_withdrawal_validator_index"] == (last + 1) % N_WD
    assert b["bal"][behind] == a["bal"][behind] and b["bal"][last] != a["bal"][last]


P16 = W.Params(max_validators_per_sweep=N_WD)
P64 = W.Params(max_withdrawals_per_payload=64, max_validators_per_sweep=N_WD)


@pytest.mark.parametrize("start", [0, N_WD - 1, N_WD - 300, 64 * WG])
def test_withdrawal_hits_on_either_side_of_every_scan_edge(engine_factory, wd_big, start):
    """one hit per workgroup, the k-th (k = 16) in workgroup E and the next in E + 1, for E | E + 1 = a scan-wave edge of the first
    tile (63 | 64, 127 | 128), the tile edge (255 | 256) and inside the ragged second tile (256 | 257); the same 18 hits under
    k = 64, where each rank is its workgroup's offset alone.  The starts move the registry's wrap to positions 1 and 300 and
    put validator 0 at position N_WD - 64 * 256."""
    assert wd_shape(N_WD) == (259, 2, 3, 77)
    e = engine_factory()
    for edge in (63, 127, 255, 256):
        positions = [lane_pos(w) for w in range(edge - 15, edge + 3)]
        assert wgs(positions) == list(range(edge - 15, edge + 3)) and wgs(positions[15:17]) == [edge, edge + 1]
        a, validators = wd_arm(e, wd_big, positions, start)
        _, expected, res = TW.check(e, a, EPOCH, 7, start, P64)
        assert [w[1] for w in expected] == validators and res["n_withdrawals"] == 18
        assert res["next_withdrawal_validator_index"] == (start + N_WD) % N_WD
        wd_compute_then_apply(e, a, start, P16, validators)
    e.close()


@pytest.mark.parametrize("extra", [8, 9])
def test_every_selected_withdrawal_in_or_behind_the_second_tile(engine_factory, wd_big, extra):
    """no hit below position 250 * 256: one per workgroup 250 .. 258 and `extra` more inside 257, over all four waves of it.
    8: the 16th hit is 257's last, the 17th is 258's; 9: both lie inside 257"""
    lanes = [3, 40, 64, 70, 127, 128, 200, 254, 255][:extra]
    positions = sorted([lane_pos(w) for w in range(250, 259)] + [257 * WG + lane for lane in lanes])
    where = wgs(positions)
    assert len(set(positions)) == 9 + extra and min(positions) >= 250 * WG and max(positions) < N_WD
    assert sorted(set(where)) == list(range(250, 259)) and where.count(257) == 1 + extra
    assert where[15:17] == ([257, 258] if extra == 8 else [257, 257])
    e = engine_factory()
    a, validators = wd_arm(e, wd_big, positions, 0)
    _, expected, res = TW.check(e, a, EPOCH, 7, 0, P64)
    assert [w[1] for w in expected] == validators and res["n_withdrawals"] == 9 + extra
    wd_compute_then_apply(e, a, 0, P16, validators)
    e.close()


def test_fewer_withdrawals_than_k_carried_through_the_tile_edge(engine_factory, wd_big):
    """k = 64, one hit per workgroup from 200 upward: 59 hits, 56 in the first tile and 3 in the second, every rank its
    workgroup's offset; the next validator index is the parameter's"""
    start = 12345
    positions = [lane_pos(w) for w in range(200, 259)]
    assert wgs(positions) == list(range(200, 259)) and len(positions) == 59 < P64.max_withdrawals_per_payload
    e = engine_factory()
    a, validators = wd_arm(e, wd_big, positions, start)
    _, expected, res = TW.check(e, a, EPOCH, 2**40, start, P64)
    assert [w[1] for w in expected] == validators and res["n_withdrawals"] == 59
    assert res["next_withdrawal_validator_index"] == (start + N_WD) % N_WD == start
    _, _, res = TW.check(e, a, EPOCH, 2**40, start, P64, expected, True)
    assert res["applied"] == 1 and res["next_withdrawal_index"] == 2**40 + 59 and res["next_withdrawal_validator_index"] == start
    e.close()


def test_every_validator_withdrawable(engine_factory, wd_big):
    """every count is 256 (the last 77) and the total is N_WD; workgroup 0 alone selects, every other offset has reached k"""
    blank, keys = wd_big
    a = W.set_hits(W.copy_registry(blank), range(N_WD))
    e = engine_factory()
    wd_load(e, a, keys)
    for p in (P16, P64):
        k = p.max_withdrawals_per_payload
        assert k <= WG  # positions 0 .. k - 1
        for start in (0, N_WD - 5):  # the second: the selection itself wraps
            _, expected, res = TW.check(e, a, EPOCH, 3, start, p)
            assert [w[1] for w in expected] == [(start + j) % N_WD for j in range(k)]
            _, _, res = TW.check(e, a, EPOCH, 3, start, p, expected, True)
            assert res["applied"] == 1 and res["next_withdrawal_validator_index"] == (start + k) % N_WD
            e.state_set_balances(a["bal"], None, a["wdr"])
    e.close()


@pytest.mark.parametrize("sweep", [16384, 16385])
def test_the_mainnet_sweep_is_the_edge_of_one_wave_of_counts(engine_factory, wd_big, sweep):
    """MAX_VALIDATORS_PER_WITHDRAWALS_SWEEP = 16384 is exactly 64 workgroups, 16385 is 65: the k-th hit at position 16383, the
    next at the position 16385 adds, whose offset is the first scan wave's total"""
    assert W.Params().max_validators_per_sweep == 16384
    p16 = W.Params(max_validators_per_sweep=sweep)
    p64 = W.Params(max_withdrawals_per_payload=64, max_validators_per_sweep=sweep)
    assert wd_shape(min(N_WD, sweep))[0] == (64 if sweep == 16384 else 65)
    positions = [lane_pos(w) for w in range(48, 63)] + [16383, 16384]
    assert wgs(positions) == list(range(48, 65)) and len(positions) == 17
    e = engine_factory()
    a, validators = wd_arm(e, wd_big, positions, 0)
    swept = [v for v in validators if v < sweep]
    _, expected, res = TW.check(e, a, EPOCH, 7, 0, p64)
    assert [w[1] for w in expected] == swept and len(swept) == (16 if sweep == 16384 else 17)
    assert res["next_withdrawal_validator_index"] == sweep % N_WD
    wd_compute_then_apply(e, a, 0, p16, validators)  # the 17th is not swept or not selected: untouched either way
    e.close()


# ================================================================ block operations: 516 workgroups, three tiles
N_BO = 33000


@pytest.fixture(scope="module")
def bo_big():
    """The layout of the large block, from the model's candidate order alone (an attester slashing takes len(i1) + len(i2)
    slots; events occur only on first-list elements that the second list holds).  Never written."""
    n, p = N_BO, K.params()
    outside = list(range(n - 22, n))          # in neither list: the proposer that is not slashed, a proposer slashing's, the exits'
    free, late, exiting = outside[0], outside[1], outside[2:]
    whole = list(range(n - 22))
    # G: B alone can take them.  B's first list starts behind A's two lists, and `whole` is 0 .. len - 1: slot = start_b + v
    g_slots = [257 * WG + 200, 258 * WG + 5, 259 * WG + 100, 320 * WG - 1, 320 * WG, 320 * WG + 1, 320 * WG + 2, 320 * WG + 3]
    start_b = 2 * len(whole) - len(g_slots)
    G = [s - start_b for s in g_slots]
    assert start_b >= WG * WG and all(0 <= v < len(whole) for v in G) and whole == list(range(len(whole)))
    first = [v for v in whole if v not in set(G)]  # A's first list; A's slot of v = its place in it
    f_slots = [7, 16383, 16384, 16385, 16386, 16387, 32767, 32768, 32769, 32770, 32771]
    F = sorted({first[s] for s in f_slots} | {16383, 16384, 32767, 32768})
    assert not set(F) & set(G) and len(first) > 128 * WG + 3
    root = lambda x: bytes([x]) * 32  # noqa: E731
    ops = [B.attester_slashing(*TB.votes(0), first, whole), B.attester_slashing(*TB.votes(1), whole, whole)]
    ops += [B.voluntary_exit(v, CUR - i % 2) for i, v in enumerate(exiting[:10])]
    ops += [B.proposer_slashing(9, late, root(1), 9, late, root(2))]
    ops += [B.voluntary_exit(v, CUR) for v in exiting[10:]]
    off = np.concatenate([[0], np.cumsum([len(op["i1"]) + len(op["i2"]) if op["kind"] == B.ATTESTER_SLASHING else 1 for op in ops])])
    n_slots = int(off[-1])
    place = {v: j for j, v in enumerate(first)}
    slots = dict(A=[place[v] for v in F], B=[int(off[1]) + v for v in G], singles=[int(x) for x in off[2:-1]])
    a = M.blank_registry(n, p)
    a["bal"] += np.arange(n, dtype=np.uint64)
    a["slashed"][:] = 1                       # nobody else is slashable: the loop passes over them at no cost
    a["slashed"][F + G + outside] = 0
    return dict(a=a, p=p, ops=ops, F=F, G=G, free=free, late=late, exiting=exiting, slots=slots, n_slots=n_slots, first=first)


def test_the_large_block_reaches_every_regime(bo_big):
    """the model's layout alone (no engine): which workgroups hold events, and what the scan makes of 516 counts"""
    s, n_slots = bo_big["slots"], bo_big["n_slots"]
    n_wg = n_slots // WG + 1
    assert n_slots == 131925 and n_wg == 516 and -(-n_wg // WG) == 3 and n_wg % WG == 4           # three tiles, the last ragged
    in_a = wgs(s["A"])
    assert {0, 63, 64, 127, 128} <= set(in_a) and max(in_a) == 128                               # tile 0 and its scan-wave edges
    assert in_a.count(64) >= 4 and in_a.count(128) >= 4
    assert wgs(s["B"]) == [257, 258, 259, 319, 320, 320, 320, 320]                               # tile 1: its first waves' edge
    assert set(wgs(s["singles"])) == {515} and len(s["singles"]) == 21 and n_slots // WG == 515  # tile 2, the last lane's too
    assert len(bo_big["F"]) + len(bo_big["G"]) + 21 <= 100


@pytest.mark.parametrize("proposer_at", ["late", "middle", "early", "none"])
def test_block_operations_over_three_scan_tiles(engine_factory, bo_big, proposer_at):
    """A = (whole - G, whole) and B = (whole, whole) over 33 000 validators of whom F and G alone are slashable, then ten
    exits, a proposer slashing and ten exits in the last workgroup.  With churn limit 4 every fourth fresh exit moves the epoch:
    each event's exit epoch is its workgroup's `fresh` offset.  The proposer: `late` -- the proposer slashing's, in the third
    tile, behind every reward; `middle` -- the first of workgroup 320, behind A's rewards (the carry) and those of workgroups
    257 .. 319 (the scan's first wave); `early` -- the first event of all; `none` -- not slashed, paid by the last lane."""
    p, F, G = bo_big["p"], bo_big["F"], bo_big["G"]
    a = M.copy_registry(bo_big["a"])
    reward = lambda v: int(a["eff"][v]) // p.whistleblower_reward_quotient      # noqa: E731
    penalty = lambda v: int(a["eff"][v]) // p.min_slashing_penalty_quotient     # noqa: E731
    order = F + G + [bo_big["late"]]          # the slashed in the loop's order: A's in list order, B's, the proposer slashing's
    assert order == sorted(F) + sorted(G) + [bo_big["late"]]
    proposer = dict(late=bo_big["late"], middle=G[4], early=F[0], none=bo_big["free"])[proposer_at]
    if proposer_at in ("late", "middle"):
        a["eff"][proposer] = 2 * p.max_effective_balance                       # a penalty of 32 rewards: the prefix fits below it
        before = sum(reward(v) for v in order[:order.index(proposer)])
        assert 0 < before < penalty(proposer) and before == reward(F[0]) * order.index(proposer)
        a["bal"][proposer] = penalty(proposer) - before                         # one reward less in the prefix: cut at 0
        if proposer_at == "middle":
            assert bo_big["slots"]["B"][4] == 320 * WG and (320 % WG) // 64 == 1   # the second wave of the second tile's scan
    elif proposer_at == "early":
        assert bo_big["slots"]["A"][0] == 7
        a["bal"][proposer] = penalty(proposer) - 1                              # nothing before it: cut at 0
    e = engine_factory()
    TB.load(e, a)
    want, status, st = TB.check(e, a, proposer, bo_big["ops"], p)
    fresh = len(order) + len(bo_big["exiting"])
    assert status == [0] * len(bo_big["ops"]) and st["n_slashed"] == len(order) and st["n_exits_initiated"] == fresh
    assert st["churn_limit"] == 4 and st["last_exit_epoch"] - st["first_exit_epoch"] == (fresh - 1) // 4
    assert st["n_saturated"] == (1 if proposer_at == "early" else 0)
    assert st["proposer_rewards"] == sum(reward(v) for v in order)
    if proposer_at == "none":
        assert int(want["bal"][proposer]) - int(a["bal"][proposer]) == st["proposer_rewards"]
    else:
        cut = penalty(proposer) - (1 if proposer_at == "early" else 0)
        assert st["penalties"] == sum(penalty(v) for v in order if v != proposer) + cut
        assert int(want["bal"][proposer]) == int(a["bal"][proposer]) + st["proposer_rewards"] - cut
    e.close()


# ================================================================ the call's last lane; the search over the slot offsets
@pytest.mark.parametrize("n_slots", [255, 256, 257, 512])
def test_the_last_lane_pays_the_proposer(engine_factory, n_slots):
    """n_slots / 256 + 1 workgroups: at a multiple of 256 the lane s == n_slots is alone in the last one"""
    n, p, proposer = 600, K.params(), 599
    a = M.blank_registry(n, p)
    a["bal"] += np.arange(n, dtype=np.uint64)
    singles = [B.voluntary_exit(590, CUR), B.proposer_slashing(3, 591, b"a" * 32, 3, 591, b"b" * 32)]
    len1 = (n_slots - len(singles)) // 2
    len2 = n_slots - len(singles) - len1
    i1, i2 = list(range(len1)), list(range(5, 5 + len2))
    ops = [B.attester_slashing(*TB.votes(), i1, i2)] + singles
    assert len(i1) + len(i2) + len(singles) == n_slots and max(i2) < 590            # the model's layout
    assert (n_slots // WG + 1, n_slots % WG == 0) == {255: (1, False), 256: (2, True), 257: (2, False), 512: (3, True)}[n_slots]
    e = engine_factory()
    TB.load(e, a)
    want, status, st = TB.check(e, a, proposer, ops, p)
    assert status == [0, 0, 0] and st["n_slashed"] == len1 - 5 + 1 and st["proposer_rewards"] > 0 and st["n_saturated"] == 0
    assert int(want["bal"][proposer]) - int(a["bal"][proposer]) == st["proposer_rewards"]
    assert int(e.state_get_balances()[0][proposer]) == int(a["bal"][proposer]) + st["proposer_rewards"]
    e.close()


@pytest.mark.parametrize("invalid", [None, "no slot", "one slot"])
def test_three_hundred_operations(engine_factory, invalid):
    """100 exits and 198 proposer slashings of distinct validators with attester slashings of 65 and 257 validators among them:
    an offset table of 301 entries whose gaps are 1, 130 and 514.  invalid: operation 150 fails -- on the host (its headers; it
    then takes NO slot, and the search passes over it) or on the device (an exit of a validator slashed earlier) -- nothing
    moves and every status is the loop's"""
    n, p, proposer = 600, K.params(), 599
    a = M.blank_registry(n, p)
    a["bal"] += np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(300)
    ops = []
    for t, v in enumerate(int(x) for x in rng.permutation(298)):
        if t % 3 == 0:
            ops.append(B.voluntary_exit(v, CUR - t % 2))
        else:
            ops.append(B.proposer_slashing(t, v, bytes([1 + t % 250]) * 32, t, v, bytes([251]) * 32))
    ops.insert(100, B.attester_slashing(*TB.votes(0), range(530, 595), range(530, 595)))
    ops.insert(200, B.attester_slashing(*TB.votes(1), range(300, 557), range(300, 557)))
    if invalid == "no slot":
        ops[150] = B.proposer_slashing(5, 598, b"c" * 32, 5, 598, b"c" * 32)
    elif invalid == "one slot":
        ops[150] = B.voluntary_exit(ops[1]["prop1"], CUR)
    gaps = [0 if o == 150 and invalid == "no slot" else len(op["i1"]) + len(op["i2"]) if op["kind"] == B.ATTESTER_SLASHING else 1
            for o, op in enumerate(ops)]
    assert len(ops) == 300 and len(gaps) + 1 > WG and {1, 130, 514} <= set(gaps) and sum(gaps) in (941, 942)
    assert sum(op["kind"] == B.VOLUNTARY_EXIT for op in ops) in (100, 101)
    e = engine_factory()
    TB.load(e, a)
    _, status, st = TB.check(e, a, proposer, ops, p)
    if invalid is None:
        slashed = 198 + 65 + 257 - len(range(530, 557))
        assert status == [0] * 300 and st["n_slashed"] == slashed and st["n_exits_initiated"] == slashed + 100
    else:
        want = B.HEADER_MISMATCH if invalid == "no slot" else B.ALREADY_EXITING
        assert [o for o, s in enumerate(status) if s] == [150] and status[150] == want and st["n_invalid"] == 1
        assert st["n_slashed"] == 0 and st["n_exits_initiated"] == 0
    e.close()
