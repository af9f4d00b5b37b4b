"""The world and the batches that hold update_latest_messages (pe:1435-1441) and the flag loop of process_attestation
(pe:745-749) to the spec where the ORDER of rows inside one batch decides the outcome, as plain data: nothing of the engine
or of oracle/spec.py is imported.  tests/test_att_rules_model.py replays every batch here through oracle/spec.py and pins
tests/att_rules_model.py to it; tests/test_gpu_lmd_flag_routes.py holds every kernel route to the model.

32 slots per epoch, ONE committee per slot (committee id = slot % 32), three tables (epochs 1, 2, 3).  The clock and the
state stand at slot 70 (epoch 2; epoch 1 is the previous one), after the tick at slot 98 (epoch 3).

  g(0) - P32 - P33 - P34 - P35 - P36 - P37 - T64 - T65 - T66 - T67 - T68 - T69        the state's chain (tip T69)
                                           \\ U64 - U65 - U66 - U67                    a fork at the epoch boundary

A row of slot 69 (delay 1) earns flags 7 with vote T69, 3 with T64..T68 (head wrong), 1 with U64..U67 (target U64 wrong);
one of slot 68 (delay 2) earns 3 or 1; a row of epoch 1 (delay >= 7) earns 2.

Committees that the cases attest in (the rest are fillers whose rows only add bits to a batch):
  epoch 2   HOT  = 5 (slot 69)  size `hot`              holds the SPECIAL validators at the seam positions of its size
            HOT2 = 4 (slot 68)  the next size of SIZES   ordinary members -- or, `overlapping`, the specials AGAIN at other
                                                         positions: the table is then no partition
  epoch 1   HOTP = 31 (slot 63) the size after that     the specials again: a validator's committee of the previous epoch
            ONE = 30 size 1, P127 = 29 size 127, P128 = 28, 27, 26 size 128: bit totals of 511 and 512 exactly
  epoch 3   HOT3 = 1 (slot 97)  the fourth size          the specials once more
Specials: registry indices 255, 256, 257 (one lane per validator, 256 per workgroup) and n_val - 1 (with n_val = 4100 the
last, partial workgroup), then a few more.  Seams: bit positions 0, 31, 32, 62, 63, 64, 127, 128 and the last one."""
import hashlib

from tests import att_rules_model as M

SPE, CPS = 32, 1
SIZES = (1, 63, 64, 65, 129)
S0, S1 = 70, 98
HOT, HOT2, HOTP, ONE, P127, P128, HOT3 = 5, 4, 31, 30, 29, (28, 27, 26), 1
EPOCHS = (1, 2, 3)
VOTES_BY_MASK = {7: ["T69"], 3: ["T68", "T67", "T66", "T65", "T64"], 1: ["U67", "U66", "U65", "U64"]}
LMD_VOTES = ["T68", "U67", "T67", "U66", "T66"]     # all of slot <= 68: votable from HOT and from HOT2
PREV_VOTES = ["P35", "P34", "P36", "P33", "P37", "P32"]


def _h(label):
    return hashlib.sha256(b"lmd-flag:" + label.encode()).digest()


def seams(n):
    return sorted({0, 31, 32, 62, 63, 64, 127, 128, n - 1} & set(range(n)))


def specials(n_val):
    return [256, 255, 257, n_val - 1, 0, 511, 512, 1023, 1024]


def _table(n_val, sizes, placed, seed):
    """32 committees of `sizes`; placed = {committee: {position: validator}}, every other seat from a fixed permutation."""
    used = {v for seats in placed.values() for v in seats.values()}
    pool = [v for v in sorted(range(n_val), key=lambda v: _h(f"perm/{seed}/{v}")) if v not in used]
    assert sum(sizes) <= len(pool) + sum(len(s) for s in placed.values())
    return [[placed[c][i] if i in placed.get(c, {}) else pool.pop() for i in range(n)] for c, n in enumerate(sizes)]


def _seats(size, n_val, reverse=False):
    pos = seams(size)
    who = specials(n_val)[:len(pos)]
    return dict(zip(reversed(pos) if reverse else pos, who))


class World:
    def __init__(self, hot=64, n_val=4096, overlapping=False):
        i = SIZES.index(hot)
        self.hot, self.n_val, self.overlapping = hot, n_val, overlapping
        self.size = {k: SIZES[(i + j) % len(SIZES)] for j, k in enumerate(("hot", "hot2", "hotp", "hot3"))}
        chain = [("g", None, 0)]
        for names, first_parent in ((["P32", "P33", "P34", "P35", "P36", "P37", "T64", "T65", "T66", "T67", "T68", "T69"], "g"),
                                    (["U64", "U65", "U66", "U67"], "P37")):
            prev = first_parent
            for n in names:
                chain.append((n, prev, int(n[1:])))
                prev = n
        self.chain = chain
        self.R = {n: _h("block/" + n) for n, _, _ in chain}
        self.name_of = {r: n for n, r in self.R.items()}
        self.blocks = {self.R[n]: (self.R[p] if p else None, s) for n, p, s in chain}
        s2 = [160, 160, 160, 160, self.size["hot2"], hot] + [100] * 26
        s1 = [50] * 6 + [100] * 20 + [128, 128, 128, 127, 1, self.size["hotp"]]
        s3 = [600, self.size["hot3"]] + [100] * 30
        p2 = {HOT: _seats(hot, n_val)}
        if overlapping:
            p2[HOT2] = _seats(self.size["hot2"], n_val, reverse=True)
        self.committees = {1: _table(n_val, s1, {HOTP: _seats(self.size["hotp"], n_val, reverse=True)}, 1),
                           2: _table(n_val, s2, p2, 2),
                           3: _table(n_val, s3, {HOT3: _seats(self.size["hot3"], n_val)}, 3)}
        self.balances = [(17 + v % 16) * 10**9 for v in range(n_val)]
        self.increments = [b // 10**9 for b in self.balances]
        self.brpi = 1013
        self.sc = {S0: M.StateCtx(slot=S0, tip=self.R["T69"], current_justified=(1, self.R["P32"]),
                                  previous_justified=(0, self.R["g"])),
                   S1: M.StateCtx(slot=S1, tip=self.R["T69"], current_justified=(2, self.R["T64"]),
                                  previous_justified=(1, self.R["P32"]))}

    def members_of(self, epoch, flat):
        return self.committees[epoch][flat]

    def anc(self, name, slot):
        return self.name_of[M.get_ancestor(self.blocks, self.R[name], slot)]

    def committee_ctx(self, clock_slot, resident):
        """Host rows read every loaded table; rows resident on the device the tables of the clock's two epochs."""
        cur = clock_slot // SPE
        loaded = {cur, cur - 1} & set(EPOCHS) if resident else set(EPOCHS)
        return M.CommitteeCtx(cps=CPS, size=lambda ep, flat: len(self.committees[ep][flat]), loaded_epochs=frozenset(loaded))

    def scenario(self, clock_slot):
        """What tests/test_gpu_att_rules.py's helpers read of a scenario."""
        return dict(time=clock_slot * 12, state=self.sc[clock_slot])

    # ------------------------------------------------------------ rows
    def bits(self, epoch, cid, label, seam=1):
        """About half of the committee's bits, by hash of the label; the seam positions all set (seam = 1), all clear
        (0), or alternating (2)."""
        n = len(self.committees[epoch][cid])
        out = [1 if _h(f"bits/{label}/{i}")[0] < 128 else 0 for i in range(n)]
        for j, i in enumerate(seams(n)):
            out[i] = (1, 0)[j % 2] if seam == 2 else seam
        return out

    def row(self, clock_slot, tag, epoch, cid, vote, bits=None, seam=1):
        sc = self.sc[clock_slot]
        bits = self.bits(epoch, cid, f"{tag}/{vote}", seam) if bits is None else bits
        source = sc.current_justified if epoch == sc.slot // SPE else sc.previous_justified
        return dict(tag=tag, slot=epoch * SPE + cid, index=0, beacon_block_root=self.R[vote], source=tuple(source),
                    target=(epoch, self.R[self.anc(vote, epoch * SPE)]), from_block=False, n_bits=len(bits), sig_valid=True,
                    popcount=sum(bits), overlap=False, bits=bits)

    def fillers(self, clock_slot, epochs):
        """Full rows of filler committees: at least 512 bits for every table named."""
        out = []
        for ep in sorted(epochs):
            cids, vote = {1: (range(6, 12), "P33"), 2: (range(0, 4), "T64"), 3: ([0], "T69")}[ep]
            out += [self.row(clock_slot, "filler", ep, c, vote, bits=[1] * len(self.committees[ep][c])) for c in cids]
        return out

    def others(self, clock_slot=S0):
        """Rows of other committees to interleave with: three of HOT2 (the same table as HOT), four of HOTP (another)."""
        return [self.row(clock_slot, f"other {i}", 2, HOT2, v) for i, v in enumerate(("T68", "T67", "T65"))] + \
               [self.row(clock_slot, f"other {i + 3}", 1, HOTP, v) for i, v in enumerate(PREV_VOTES[:4])]


_WORLDS = {}


def world(hot=64, n_val=4096, overlapping=False):
    key = (hot, n_val, overlapping)
    if key not in _WORLDS:
        _WORLDS[key] = World(*key)
    return _WORLDS[key]


def rotations(rows):
    return [rows[i:] + rows[:i] for i in range(len(rows))]


# where k rows that compete sit among the rows of other committees: in neighbouring waves, across the border of a
# workgroup (four rows each), and workgroups apart -- 9, 5 and 9 rows in all
INTERLEAVE = {1: (2, 3), 2: (0, 7, 9), 3: (0, 3, 4, 5), 5: (0, 1, 4, 7, 8, 9)}


def interleave(rows, others):
    *at, total = INTERLEAVE[len(rows)]
    rows, others, out = list(rows), list(others), []
    for i in range(total):
        out.append(rows.pop(0) if i in at else others.pop(0))
    assert not rows
    return out


def batch(rows):
    keys = {(r["slot"], r["index"], r["beacon_block_root"], r["source"], r["target"]) for r in rows}
    assert len(keys) == len(rows), "rows with equal AttestationData would form one group"
    return ("batch", rows)


def _hot_of(w, j):
    """The committee of the j-th competing row: HOT, and on an overlapping table every other one HOT2."""
    return HOT2 if w.overlapping and j % 2 else HOT


# ------------------------------------------------------------ the cases: lists of steps
# ("batch", rows, clock slot) | ("mark", validators): store.equivocating_indices | ("tick",): the clock and the state
# move to slot 98 and the participation arrays rotate
def equal_epochs(w, k, rotation, interleaved):
    """Case 1: one validator in k rows of one target epoch that vote for different blocks."""
    rows = [w.row(S0, f"competes {j}", 2, _hot_of(w, j), LMD_VOTES[j]) for j in range(k)]
    rows = rotations(rows)[rotation]
    first = rows[0]
    if interleaved:
        rows = interleave(rows, w.others())
    return [batch(rows)], first


def stored_message(w, variant):
    """Case 2.  "sequence": epoch 2, epoch 2 again (kept), epoch 1 (kept), and after the tick epoch 3 (replaced, for the half
    of the seam validators its row names).  "later first" / "earlier first": on a stored message of epoch 1, one batch with
    a row of epoch 2 and another of epoch 1."""
    if variant == "sequence":
        return [batch([w.row(S0, "E", 2, HOT, "T68")]), batch([w.row(S0, "E again", 2, HOT, "T67")]),
                batch([w.row(S0, "E - 1", 1, HOTP, "P35")]), ("tick",),
                ("batch", [w.row(S1, "E + 1", 3, HOT3, "T69", seam=2)])]
    pair = [w.row(S0, "E + 1", 2, HOT, "T68"), w.row(S0, "E", 1, HOTP, "P36")]
    return [batch([w.row(S0, "stored", 1, HOTP, "P34")]), batch(pair if variant == "later first" else pair[::-1])]


def two_tables(w, later_first, interleaved=False):
    """Case 3: a validator attests in its committee of the previous epoch and in the one of the current epoch."""
    pair = [w.row(S0, "current", 2, HOT, "T69"), w.row(S0, "previous", 1, HOTP, "P37")]
    pair = pair if later_first else pair[::-1]
    return [batch(interleave(pair, w.others()) if interleaved else pair)]


def equivocating(w, between):
    """Case 4: marked before the batch (no message at all), or between two batches (the stored message stays)."""
    who = specials(w.n_val)[:2] + [w.committees[2][HOT][-1], w.committees[1][HOTP][0]]
    rows = [w.row(S0, f"competes {j}", 2, _hot_of(w, j), LMD_VOTES[j]) for j in range(3)]
    if between:
        return [batch([w.row(S0, "stored", 1, HOTP, "P34")]), ("mark", who), batch(rows)]
    return [("mark", who), batch(rows + [w.row(S0, "previous", 1, HOTP, "P35")])]


FLAG_ORDERS = {1: [[7]], 2: [[1, 7], [3, 7]], 3: [[1, 3, 7], [7, 3, 1]], 5: [[1, 1, 3, 3, 7], [7, 3, 3, 1, 1]]}


def flag_rounds(w, masks, rotation, interleaved):
    """Case 6: len(masks) rows on one committee with overlapping bit sets; each pays the flags fresh at its turn."""
    free = {m: list(v) for m, v in VOTES_BY_MASK.items()}
    rows = []
    for j, m in enumerate(masks):
        cid = HOT2 if (w.overlapping and j % 2 and m != 7) else HOT   # slot 68 has no row of flags 7
        vote = next(v for v in free[m] if int(v[1:]) <= 2 * SPE + cid)
        free[m].remove(vote)
        rows.append(w.row(S0, f"flags {m} #{j}", 2, cid, vote))
    rows = rotations(rows)[rotation]
    if interleaved:
        taken = {r["beacon_block_root"] for r in rows if r["slot"] == 2 * SPE + HOT2}
        rows = interleave(rows, [o for o in w.others() if o["beacon_block_root"] not in taken or o["slot"] != 2 * SPE + HOT2] +
                          [w.row(S0, "other 7", 2, HOT2, "T64"), w.row(S0, "other 8", 2, HOT2, "U64")])
    return [batch(rows)]


def straddle(w, at_threshold):
    """Rows of the epoch-1 table whose n_bits sum to 511 (8 x 511 = n_val - 8 at 4096 validators) or, with one more row of
    the one-member committee, to 512.  That row comes last and names a validator the first one of its committee named."""
    rows = [w.row(S0, "competes 0", 1, P127, "P35"), w.row(S0, "competes 1", 1, P127, "P34"),
            w.row(S0, "wide 0", 1, P128[0], "P33"), w.row(S0, "wide 1", 1, P128[1], "P36"),
            w.row(S0, "one 0", 1, ONE, "P35", bits=[1])]
    if at_threshold:
        rows.append(w.row(S0, "one 1", 1, ONE, "P37", bits=[1]))
    assert sum(r["n_bits"] for r in rows) == (512 if at_threshold else 511)
    return [batch(rows)]


def voided_group(w):
    """Case 5, rows resident on the device: two rows of equal data whose bits overlap form one group, which is voided.
    -> (the rows as handed over, the groups as the model sees them)."""
    a1 = w.row(S0, "voided", 2, HOT2, "T68")
    a2 = dict(a1, bits=w.bits(2, HOT2, "voided, second member"))
    assert any(x and y for x, y in zip(a1["bits"], a2["bits"])) or len(a1["bits"]) == 1
    if len(a1["bits"]) == 1:
        a2["bits"] = [1]
    a2["popcount"] = sum(a2["bits"])
    union = [x | y for x, y in zip(a1["bits"], a2["bits"])]
    group = dict(a1, bits=union, popcount=sum(union), overlap=True)
    b = w.row(S0, "same committee", 2, HOT2, "T67")
    c = w.row(S0, "neighbour", 2, HOT, "T69")
    d = w.row(S0, "previous", 1, HOTP, "P35")
    return [b, a1, c, a2, d], [b, group, c, d]


def replay(model, w, steps, resident):
    """The model over a case's steps -> per batch what Run.batch returns."""
    clock, out = S0, []
    for step in steps:
        if step[0] == "mark":
            model.equivocating.update(step[1])
        elif step[0] == "tick":
            clock = S1
            model.part = ([0] * w.n_val, model.part[0])   # process_participation_flag_updates
        else:
            out.append(model.batch(step[1], w.blocks, clock, w.sc[clock], w.committee_ctx(clock, resident), w.members_of))
    return out
