"""The rules an attestation passes before it may touch the store or the state, as a plain table-driven model: integers,
dicts and the text of include/posevo.h -- nothing of the engine is imported.

  fork-choice side   validate_on_attestation (A.4), committee resolution of get_indexed_attestation (A.6),
                     is_valid_indexed_attestation (A.7)
  state side         the asserts of process_attestation (pe:724-730) and
                     get_attestation_participation_flag_indices (A.9)

Statuses are the pe_att_status of the FIRST assert that fails, in the order oracle/spec.py evaluates them;
tests/test_att_rules_model.py pins every case of the boundary matrix (tests/att_rules_cases.py) to oracle/spec.py itself.

An attestation is a dict: slot, index, beacon_block_root, source = (epoch, root), target = (epoch, root), from_block,
n_bits, sig_valid, popcount, overlap.  The store is `blocks`: root -> (parent_root, slot), and its current slot.  The state
is a StateCtx.  Committees are a CommitteeCtx: committees per slot, the committee size -- one int where every committee
has it, else a function (epoch, flat committee id) -> size -- and which epochs have a table loaded: the one notion here
that the spec does not have (a state always knows its committees; PE_ATT_NO_COMMITTEE_TABLE, include/posevo.h).
Nothing here asks a table to be a partition: members_of (Run.batch) may name a validator in several committees."""
import os
import re
from collections import namedtuple

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "posevo.h")


def _status_values():
    text = open(_HEADER).read()
    body = text[text.index("PE_ATT_OK"):text.index("} pe_att_status;")]
    return {name: int(val) for name, val in re.findall(r"(PE_ATT_\w+)\s*=\s*(\d+)", body)}


ST = _status_values()
OK = ST["PE_ATT_OK"]
EPOCH_TIME = ST["PE_ATT_TARGET_EPOCH_NOT_CURRENT_OR_PREVIOUS"]
EPOCH_SLOT = ST["PE_ATT_TARGET_EPOCH_SLOT_MISMATCH"]
UNKNOWN_TARGET = ST["PE_ATT_UNKNOWN_TARGET_ROOT"]
UNKNOWN_BLOCK = ST["PE_ATT_UNKNOWN_BEACON_BLOCK_ROOT"]
BLOCK_AFTER_SLOT = ST["PE_ATT_BLOCK_AFTER_ATTESTATION_SLOT"]
TARGET_NOT_ANCESTOR = ST["PE_ATT_TARGET_NOT_ANCESTOR"]
SLOT_NOT_PAST = ST["PE_ATT_SLOT_NOT_IN_PAST"]
NO_TABLE = ST["PE_ATT_NO_COMMITTEE_TABLE"]
INDEX_RANGE = ST["PE_ATT_COMMITTEE_INDEX_OUT_OF_RANGE"]
BITS_LENGTH = ST["PE_ATT_BITS_LENGTH_MISMATCH"]
EMPTY = ST["PE_ATT_EMPTY_OR_INVALID_INDICES"]
BAD_SIGNATURE = ST["PE_ATT_BAD_SIGNATURE"]
INCLUSION = ST["PE_ATT_INCLUSION_WINDOW"]
SOURCE = ST["PE_ATT_SOURCE_MISMATCH"]

TIMELY_SOURCE, TIMELY_TARGET, TIMELY_HEAD = 1, 2, 4
FLAG_WEIGHTS = (14, 26, 14)  # PARTICIPATION_FLAG_WEIGHTS (A.9)

StateCtx = namedtuple("StateCtx", "slot tip current_justified previous_justified")
CommitteeCtx = namedtuple("CommitteeCtx", "cps size loaded_epochs")
Consts = namedtuple("Consts", "spe min_delay")
MAINNET = Consts(spe=32, min_delay=1)


def isqrt(n):
    x, y = n, (n + 1) // 2
    while y < x:
        x, y = y, (y + n // y) // 2
    return x


def get_ancestor(blocks, root, slot):
    """A.2: the block of `root`'s chain at `slot`, or the latest one before it when that slot is empty."""
    parent, s = blocks[root]
    while s > slot:
        root = parent
        parent, s = blocks[root]
    return root


def flat_committee(att, cc, k=MAINNET):
    """get_beacon_committee's position (A.6): (slot % SLOTS_PER_EPOCH) * committees_per_slot + data.index.  The fork-choice
    side asserts nothing about data.index itself, only this position has to exist (include/posevo.h, pe_set_committees:
    "committee id = (slot % SLOTS_PER_EPOCH) * committees_per_slot + index"); pe:727 belongs to the state side."""
    return (att["slot"] % k.spe) * cc.cps + att["index"]


def _committee_status(att, cc, k, state_side):
    if att["target"][0] not in cc.loaded_epochs:
        return NO_TABLE
    if state_side and att["index"] >= cc.cps:  # pe:727
        return INDEX_RANGE
    if flat_committee(att, cc, k) >= cc.cps * k.spe:
        return INDEX_RANGE
    size = cc.size(att["target"][0], flat_committee(att, cc, k)) if callable(cc.size) else cc.size
    if att["n_bits"] < size:  # pe:730; for the fork choice bits[i] is read for every committee position (A.6)
        return BITS_LENGTH
    if att["n_bits"] > size:
        if state_side:  # pe:730
            return BITS_LENGTH
        # A.6 reads the committee's length of them and ignores the rest; the engine does so for bits in host memory and
        # refuses them where they are resident (include/posevo.h, PE_BITS_RESIDENT): no row of the matrix goes there
        raise NotImplementedError("more bits than committee members on the fork-choice side are not modelled")
    return OK


def _indexed_status(att):
    """A.7 is ONE assert of the spec; the engine reports it as two statuses.  A row has at most one of the defects here: what
    a row with no bit set AND a false signature verdict answers is not modelled (the spec does not say)."""
    empty, unverifiable = att["popcount"] == 0, not att["sig_valid"] or att["overlap"]
    if empty and unverifiable:
        raise NotImplementedError("two defects of is_valid_indexed_attestation in one row are not modelled")
    if empty:
        return EMPTY
    if unverifiable:  # an aggregate whose members share a bit never verifies (A.8)
        return BAD_SIGNATURE
    return OK


def fork_choice_status(att, blocks, cur_slot, cc, k=MAINNET):
    t_epoch, t_root = att["target"]
    if not att["from_block"]:
        cur_epoch = cur_slot // k.spe
        prev_epoch = cur_epoch - 1 if cur_epoch > 0 else 0
        if t_epoch not in (cur_epoch, prev_epoch):
            return EPOCH_TIME
    if t_epoch != att["slot"] // k.spe:
        return EPOCH_SLOT
    if t_root not in blocks:
        return UNKNOWN_TARGET
    if att["beacon_block_root"] not in blocks:
        return UNKNOWN_BLOCK
    if not blocks[att["beacon_block_root"]][1] <= att["slot"]:
        return BLOCK_AFTER_SLOT
    if t_root != get_ancestor(blocks, att["beacon_block_root"], t_epoch * k.spe):
        return TARGET_NOT_ANCESTOR
    if not cur_slot >= att["slot"] + 1:
        return SLOT_NOT_PAST
    return _committee_status(att, cc, k, state_side=False) or _indexed_status(att)


def state_status(att, blocks, sc, cc, k=MAINNET):
    """-> (status, flag mask, which): which = 0 current_epoch_participation, 1 previous (pe:739-742)."""
    t_epoch, t_root = att["target"]
    cur_epoch = sc.slot // k.spe
    prev_epoch = cur_epoch - 1 if cur_epoch > 0 else 0
    which = 0 if t_epoch == cur_epoch else 1
    if t_epoch not in (prev_epoch, cur_epoch):                                     # pe:724
        return EPOCH_TIME, 0, which
    if t_epoch != att["slot"] // k.spe:                                            # pe:725
        return EPOCH_SLOT, 0, which
    if not att["slot"] + k.min_delay <= sc.slot <= att["slot"] + k.spe:            # pe:726
        return INCLUSION, 0, which
    st = _committee_status(att, cc, k, state_side=True)                            # pe:727-730
    if st:
        return st, 0, which
    justified = sc.current_justified if t_epoch == cur_epoch else sc.previous_justified
    if tuple(att["source"]) != tuple(justified):                                   # assert is_matching_source (A.9)
        return SOURCE, 0, which
    # get_block_root(state, epoch) / get_block_root_at_slot(state, slot): both slots lie before state.slot by pe:726
    matching_target = t_root == get_ancestor(blocks, sc.tip, t_epoch * k.spe)
    matching_head = matching_target and att["beacon_block_root"] == get_ancestor(blocks, sc.tip, att["slot"])
    delay = sc.slot - att["slot"]
    mask = 0
    if delay <= isqrt(k.spe):
        mask |= TIMELY_SOURCE
    if matching_target and delay <= k.spe:
        mask |= TIMELY_TARGET
    if matching_head and delay == k.min_delay:
        mask |= TIMELY_HEAD
    st = _indexed_status(att)                                                      # pe:736
    return st, (mask if st == OK else 0), which


def update_latest_messages(latest, attesters, att, equivocating=(), slots=None):
    """pe:1435-1441 on `latest`: validator -> (epoch, root).  `slots` (vote-expiry variant, pe:1585-1596): validator ->
    data.slot of the attestation its latest message came from."""
    t_epoch = att["target"][0]
    for v in attesters:
        if v in equivocating:
            continue
        if v not in latest or t_epoch > latest[v][0]:
            latest[v] = (t_epoch, att["beacon_block_root"])
            if slots is not None:
                slots[v] = att["slot"]


def apply_flags(participation, attesters, mask, increments, base_reward_per_increment):
    """pe:744-749 on one participation array (a list): -> proposer_reward_numerator."""
    numerator = 0
    for v in attesters:
        for f, weight in enumerate(FLAG_WEIGHTS):
            if mask >> f & 1 and not participation[v] >> f & 1:
                participation[v] |= 1 << f
                numerator += increments[v] * base_reward_per_increment * weight
    return numerator


class Run:
    """What a sequence of batches leaves behind: latest messages (with the slot each came from) and both participation
    arrays.  `equivocating` is store.equivocating_indices: add to it between batches."""

    def __init__(self, n_validators, increments, base_reward_per_increment, k=MAINNET):
        self.latest = {}
        self.slots = {}
        self.equivocating = set()
        self.part = ([0] * n_validators, [0] * n_validators)  # [0] current, [1] previous
        self.increments = increments
        self.brpi = base_reward_per_increment
        self.k = k

    def batch(self, atts, blocks, cur_slot, sc, cc, members_of):
        """members_of(epoch, flat committee id) -> the committee's validators; every att also carries `bits` (a list of
        0 / 1).  on_attestation over the whole batch, then process_attestation over the whole batch, each in batch order.
        -> dict of per-row lists: status, count, pstatus, mask, which, numerator."""
        out = dict(status=[], count=[], pstatus=[], mask=[], which=[], numerator=[])
        for a in atts:
            st = fork_choice_status(a, blocks, cur_slot, cc, self.k)
            out["status"].append(st)
            out["count"].append(a["popcount"] if st == OK else 0)
            if st == OK:
                com = members_of(a["target"][0], flat_committee(a, cc, self.k))
                update_latest_messages(self.latest, [v for v, b in zip(com, a["bits"]) if b], a, self.equivocating, self.slots)
        for a in atts:
            st, mask, which = state_status(a, blocks, sc, cc, self.k)
            num = 0
            if st == OK:
                com = members_of(a["target"][0], flat_committee(a, cc, self.k))
                num = apply_flags(self.part[which], [v for v, b in zip(com, a["bits"]) if b], mask, self.increments, self.brpi)
            out["pstatus"].append(st)
            out["mask"].append(mask)
            out["which"].append(which)
            out["numerator"].append(num)
        return out
