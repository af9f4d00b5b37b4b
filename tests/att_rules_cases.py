"""The world and the boundary matrix of the attestation rules, as plain data: one hand-built chain, the spec's own
committees for 2048 validators, and scenarios (store clock + state + a batch of rows) in which every inequality of
validate_on_attestation (A.4) and process_attestation (pe:724-730, A.9) has rows on both sides of its edge.
tests/test_att_rules_model.py pins the model's answer for every row to oracle/spec.py; tests/test_gpu_att_rules.py holds
the engine to the model on the same rows.

The chain (slots; 32 per epoch; A = the main chain, B = a fork):
  epoch 0   g(0) A1 A2 . . . A30 A31
  epoch 1   A32 A33 A34 A35 [36-44 empty] A45 .. A62, then the siblings A63 and B63 (both children of A62, last slot)
  epoch 2   [64, 65 empty on A] A66 .. A80 [81-93 empty] A94 A95;  B65 on B63   (first slot empty: checkpoint = A63 / B63)
  epoch 3   wholly empty
  epoch 4   A128 A129                                                               (first slot occupied)"""
import hashlib
from contextlib import contextmanager

from oracle import spec
from tests import att_rules_model as M
from tests.scenario import genesis

N_VAL, SPE, CPS, SIZE = 2048, 32, 2, 32
EPOCHS = (0, 1, 2, 3)  # epochs whose committees exist
_PRESET = dict(TARGET_COMMITTEE_SIZE=32, SHUFFLE_ROUND_COUNT=10, EPOCHS_PER_HISTORICAL_VECTOR=64)


@contextmanager
def preset():
    """oracle.spec bound to 32 slots per epoch and 2 committees of 32 per slot at 2048 validators; restored afterwards."""
    name = spec.PRESET_NAME
    old = {k: getattr(spec, k) for k in spec.PRESETS[name]}
    spec.use_preset("mainnet", **_PRESET)
    try:
        yield
    finally:
        spec.use_preset(name, **old)


def _root(label):
    return hashlib.sha256(b"att-rules:" + label.encode()).digest()


def _chain():
    out = [("g", None, 0)]
    prev = "g"

    def run(slots, prefix="A"):
        nonlocal prev
        for s in slots:
            out.append((f"{prefix}{s}", prev, s))
            prev = f"{prefix}{s}"

    run([1, 2, 30, 31, 32, 33, 34, 35] + list(range(45, 64)))
    out.append(("B63", "A62", 63))
    out.append(("B65", "B63", 65))
    run(list(range(66, 81)) + [94, 95, 128, 129])
    return out


def spec_genesis_state():
    """Call inside preset().  The registry every committee of the world is shuffled from."""
    state, _ = genesis(N_VAL)
    for i, v in enumerate(state.validators):
        v.effective_balance = (17 + i % 16) * 10**9
    return state


class World:
    def __init__(self):
        self.chain = _chain()
        self.R = {name: _root(name) for name, _, _ in self.chain}
        self.name_of = {r: n for n, r in self.R.items()}
        self.blocks = {self.R[n]: (self.R[p] if p else None, s) for n, p, s in self.chain}
        with preset():
            st = spec_genesis_state()
            self.balances = [v.effective_balance for v in st.validators]
            self.increments = [b // spec.EFFECTIVE_BALANCE_INCREMENT for b in self.balances]
            self.brpi = spec.get_base_reward_per_increment(st)
            self.committees = {}
            for ep in EPOCHS:
                assert spec.get_committee_count_per_slot(st, ep) == CPS
                self.committees[ep] = [spec.get_beacon_committee(st, ep * SPE + c // CPS, c % CPS) for c in range(SPE * CPS)]
                assert all(len(c) == SIZE for c in self.committees[ep])
        self.scenarios = _scenarios(self)

    def members_of(self, epoch, flat):
        return self.committees[epoch][flat]

    def anc(self, name, slot):
        return self.name_of[M.get_ancestor(self.blocks, self.R[name], slot)]

    def parent(self, name):
        return self.name_of[self.blocks[self.R[name]][0]]


_WORLD = None


def world():
    global _WORLD
    if _WORLD is None:
        _WORLD = World()
    return _WORLD


def _bits(label):
    h = hashlib.sha256(b"bits:" + label.encode()).digest()
    bits = [1 if h[i] < 180 else 0 for i in range(SIZE)]
    bits[h[0] % SIZE] = 1
    return bits


class _Batch:
    def __init__(self, w, sc):
        self.w, self.sc, self.rows = w, sc, []

    def source_for(self, epoch):
        return self.sc.current_justified if epoch == self.sc.slot // SPE else self.sc.previous_justified

    def add(self, tag, slot, index, vote, t_epoch, target, source=None, from_block=False, vote_root=None, target_root=None,
            bits=None, sig_valid=True):
        w = self.w
        bits = _bits(f"{tag}/{slot}/{index}/{len(self.rows)}") if bits is None else bits
        self.rows.append(dict(
            tag=tag, slot=slot, index=index, beacon_block_root=vote_root or w.R[vote],
            source=tuple(source if source is not None else self.source_for(t_epoch)),
            target=(t_epoch, target_root or w.R[target]), from_block=from_block, n_bits=len(bits), sig_valid=sig_valid,
            popcount=sum(bits), overlap=False, bits=bits))

    def done(self):
        keys = {(r["slot"], r["index"], r["beacon_block_root"], r["source"], r["target"]) for r in self.rows}
        assert len(keys) == len(self.rows), "rows with equal AttestationData would form one group"
        return self.rows


# the row whose position (slot % SPE) * CPS + index is 2^64 exactly: 0 in 64-bit arithmetic, committee 0 -- which exists
WRAP_SLOT_IN_EPOCH, WRAP_INDEX, WRAP_TAG = 3, 2**64 - 6, "index = 2^64 - 6: the position's 64-bit sum wraps to 0"
assert WRAP_SLOT_IN_EPOCH * CPS + WRAP_INDEX == 2**64

CJ_NAME, PJ_NAME = "A32", "g"  # current_justified = (1, A32), previous_justified = (0, g): they differ


def _state(w, slot, tip):
    return M.StateCtx(slot=slot, tip=w.R[tip], current_justified=(1, w.R[CJ_NAME]), previous_justified=(0, w.R[PJ_NAME]))


def _fork_choice_matrix(w):
    """Store clock in the middle of slot 70 (epoch 2); the state is the one of slot 70 on the A chain."""
    sc = _state(w, 70, "A69")
    b = _Batch(w, sc)
    a = b.add
    a("valid: current epoch, epoch-start slot empty", 66, 0, "A66", 2, "A63")
    a("valid: previous epoch, data.slot empty", 40, 0, "A35", 1, "A32")
    a("target epoch current + 1", 96, 0, "A69", 3, "A69")
    a("target epoch previous - 1", 5, 0, "A2", 0, "g")
    a("target epoch previous - 1, from a block", 5, 1, "A2", 0, "g", from_block=True)
    a("slot 32E - 1, E = 2", 63, 1, "A62", 2, "A62")
    a("slot 32E, E = 2", 64, 0, "A63", 2, "A63")
    a("slot 32E + 31, E = 2", 95, 0, "A69", 2, "A63")
    a("slot 32E + 32, E = 2", 96, 1, "A69", 2, "A63")
    a("slot 32E - 1, E = 1", 31, 0, "A31", 1, "A31")
    a("slot 32E, E = 1", 32, 0, "A32", 1, "A32")
    a("slot 32E + 31, E = 1", 63, 0, "A63", 1, "A32")
    a("slot 32E + 32, E = 1", 64, 1, "A63", 1, "A32")
    a("block.slot = data.slot - 1", 67, 0, "A66", 2, "A63")
    a("block.slot = data.slot", 67, 1, "A67", 2, "A63")
    a("block.slot = data.slot + 1", 67, 0, "A68", 2, "A63")
    a("ancestor: epoch-start slot occupied", 50, 0, "A50", 1, "A32")
    a("ancestor: epoch-start slot empty, clock = slot + 2", 68, 0, "A68", 2, "A63")
    a("ancestor: the vote is older than the epoch start", 66, 1, "A60", 2, "A60")
    a("ancestor: older vote, target = the checkpoint of the chain", 65, 0, "A60", 2, "A63")
    a("ancestor: the fork's own checkpoint", 65, 1, "B65", 2, "B63")
    a("wrong target: sibling of equal slot", 68, 1, "A68", 2, "B63")
    a("wrong target: the target's parent", 69, 0, "A68", 2, "A62")
    a("wrong target: the target's child", 69, 1, "A68", 2, "A66")
    a("wrong target: known block off the vote's chain", 62, 0, "A62", 1, "B65")
    a("clock = data.slot", 70, 0, "A70", 2, "A63")
    a("clock = data.slot + 1", 69, 0, "A69", 2, "A63")
    a("unknown target root", 61, 0, "A61", 1, None, target_root=_root("nowhere 1"))
    a("unknown block root", 61, 1, None, 1, "A32", vote_root=_root("nowhere 2"))
    a("unknown target and block root", 60, 0, None, 1, None, vote_root=_root("nowhere 3"), target_root=_root("nowhere 4"))
    a("valid", 59, 0, "A59", 1, "A32")
    a("valid", 59, 1, "A59", 1, "A32")
    a("valid", 58, 0, "A58", 1, "A32")
    # A.7 and pe:730, one defect per row (what a row with two of them answers is not modelled)
    a("no bit set", 57, 0, "A57", 1, "A32", bits=[0] * SIZE)
    a("signature verdict false", 57, 1, "A57", 1, "A32", sig_valid=False)
    a("fewer bits than the committee has members", 56, 0, "A56", 1, "A32", bits=_bits("short")[:SIZE - 8])
    return dict(name="fork choice, clock in slot 70", time=70 * 12 + 11, state=sc, rows=b.done(),
                want_status={0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12}, want_pstatus={0, 1, 2, 10, 11, 12, 13})


def _epoch_zero(w):
    """Store clock and state in epoch 0: the previous epoch IS the current one."""
    sc = M.StateCtx(slot=20, tip=w.R["A2"], current_justified=(0, w.R["g"]), previous_justified=(0, w.R["g"]))
    b = _Batch(w, sc)
    a = b.add
    a("valid", 2, 0, "A2", 0, "g")
    a("valid", 1, 0, "A1", 0, "g")
    a("valid", 1, 1, "A1", 0, "g")
    a("clock = data.slot + 1", 19, 0, "A2", 0, "g")
    a("clock = data.slot", 20, 0, "A2", 0, "g")
    a("slot 32E + 31, E = 0", 31, 0, "A2", 0, "g")
    a("target epoch current + 1", 32, 0, "A2", 1, "A2")
    a("slot 32E + 32, E = 0", 32, 1, "A2", 0, "g")
    a("source of another epoch", 3, 0, "A2", 0, "g", source=(1, w.R["g"]))
    return dict(name="epoch 0", time=20 * 12, state=sc, rows=b.done(), want_status={0, 1, 2, 7}, want_pstatus={0, 1, 2, 13, 14})


def _state_matrix(w, S):
    """state.slot = S with the store clock at the start of the same slot.  The tip is the A chain's last block before S."""
    tip = w.anc("A129", S - 1)
    sc = _state(w, S, tip)
    b = _Batch(w, sc)
    cur, prev = S // SPE, S // SPE - 1
    used = set()

    def head(slot):
        return w.anc(tip, slot)

    def plain(tag, slot, index, vote=None, target=None, **kw):
        ep = slot // SPE
        vote = vote or head(slot)
        b.add(tag, slot, index, vote, kw.pop("t_epoch", ep), target or w.anc(head(slot), ep * SPE), **kw)
        used.add((slot, index))

    for k in range(3):  # plain valid rows: delay 3 and 4
        plain("valid", S - 3 - k // 2, k % 2)
    for delay in (0, 1, 2, 5, 6, 31, 32, 33):
        if S - delay >= 0 and (S - delay, 0) not in used:
            plain(f"inclusion delay {delay}", S - delay, 0)
    # first wins: the second accepted row on a committee earns only the flags the first one left (pe:745-749)
    plain("first wins: second row, wrong head", S - 1, 0, vote=w.parent(head(S - 1)))
    plain("first wins: first row, wrong head", S - 1, 1, vote=w.parent(head(S - 1)))
    plain("first wins: second row, all three flags", S - 1, 1)
    plain("target right, head wrong", S - 2, 1, vote=w.parent(head(S - 2)))
    t = w.anc(head(S - 5), ((S - 5) // SPE) * SPE)
    plain("target wrong: the target's parent", S - 5, 1, target=w.parent(t) if t != "g" else "A1")
    # source
    free = [(s, 1) for s in range(S - 6, S - 31, -1) if (s, 1) not in used]
    cur_free = [x for x in free if x[0] // SPE == cur]
    prev_free = [x for x in free if x[0] // SPE == prev]

    def take(*lists):
        lst = next(x for x in lists if x)
        x = lst.pop(0)
        used.add(x)
        return x

    s, i = take(cur_free, prev_free)
    j = b.source_for(s // SPE)
    plain("source: right epoch, wrong root", s, i, source=(j[0], w.R["A33"]))
    s, i = take(prev_free, cur_free)
    j = b.source_for(s // SPE)
    plain("source: right root, wrong epoch", s, i, source=(j[0] + 1, j[1]))
    if cur_free:
        s, i = take(cur_free)
        plain("source: current-epoch row with the previous justified checkpoint", s, i, source=sc.previous_justified)
    if prev_free:
        s, i = take(prev_free)
        plain("source: previous-epoch row with the current justified checkpoint", s, i, source=sc.current_justified)
    # committee index
    plain("index = cps: the next slot's first committee for the fork choice, pe:727 for the state", S - 6, CPS)
    last = prev * SPE + SPE - 1
    if (last, CPS) not in used:
        plain("flat committee id = n_committees", last, CPS)
    # epoch against slot
    s, i = take(prev_free, cur_free)
    plain("target epoch neither previous nor current, slot of another epoch (pe:724 before pe:725)", s, i, t_epoch=cur + 2)
    plain("target epoch neither previous nor current, matching slot", (cur + 2) * SPE + 1, 0, vote=tip, target=tip)
    s, i = take(cur_free, prev_free)
    other = cur if s // SPE == prev else prev
    plain("target epoch of the other admitted epoch (pe:725)", s, i, t_epoch=other)
    # committee index again (last, so that the rows above keep their numbers): an index no 32-bit committee count reaches --
    # either side of 2^32 - 1, where the device keeps it out of the position's sum, and two that a 64-bit sum would wrap: at
    # slot % 32 = 3 with two committees per slot, 2^64 - 6 wraps onto committee 0
    wrap_slot = max(s for s in range(S - SPE, S) if s % SPE == WRAP_SLOT_IN_EPOCH)
    plain("index = 2^32 - 2", S - 6, 2**32 - 2)
    plain("index = 2^32 - 1", S - 6, 2**32 - 1)
    plain(WRAP_TAG, wrap_slot, WRAP_INDEX)
    plain("index = 2^64 - 1", S - 6, 2**64 - 1)
    return dict(name=f"state.slot {S}", time=S * 12, state=sc, rows=b.done(), want_status={0, 7, 9},
                want_pstatus={0, 1, 2, 9, 13, 14})


STATE_SLOTS = (64, 65, 69, 70, 95, 127)  # first, second, sixth, seventh and last slot of an epoch; last slot of an empty epoch


def _scenarios(w):
    return [_fork_choice_matrix(w), _epoch_zero(w)] + [_state_matrix(w, S) for S in STATE_SLOTS]


def committee_ctx(sc_time, resident):
    """Which epochs have a table for a route: the host-row path reads every loaded table; over rows resident in device
    memory "committees are resolved against the tables of the store's CURRENT and PREVIOUS epoch" and "a from-block row with
    an older target reads PE_ATT_NO_COMMITTEE_TABLE" (include/posevo.h, PE_ROWS_RESIDENT)."""
    loaded = set(EPOCHS)
    if resident:
        cur = sc_time // 12 // SPE
        loaded &= {cur, max(cur - 1, 0)}
    return M.CommitteeCtx(cps=CPS, size=SIZE, loaded_epochs=frozenset(loaded))
