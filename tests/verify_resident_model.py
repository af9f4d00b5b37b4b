"""The rule table of pe_verify_resident (include/posevo.h), restated on the host with the pairing replaced by its exponent.

A group is described by what the resident aggregate and the call know about it; every point is a known multiple of its
generator: the aggregate key is ``key`` * G1 (the sum of the secret keys of the union's members), the message point ``h`` * G2,
the aggregate signature ``sig`` * G2.  Then

    e(key G1, h G2) e(-G1, sig G2) = e(G1, G2)^(key h - sig)

is 1 exactly when key * h - sig == 0 (mod r): e(G1, G2) has order r.  tests/test_verify_resident_model.py holds one group to
the real pairing of tests/pairing_model.py.

The table, first matching row wins (ROWS is its order; the kernels' counters and the stats hook use the same one):

    no_committee        the group has no committee                       -> UNDECIDED (3); the verdict is not applied
    bad_message         message point not canonical / not on its curve   -> BAD_POINT (2)
    overlap             the members' bits overlap                        -> 0
    bad_member          a member's signature did not decode / failed the leg's subgroup check -> 0
    empty_key           the union is empty: the aggregate key is the identity -> 0
    identity_signature  the aggregate signature is the identity         -> 0
    identity_message    the message point is the identity               -> 0
    not_g2              the aggregate signature lies outside G2          -> 0
    pairing             key * h - sig == 0 (mod r) -> 1, else 0
"""
from dataclasses import dataclass
from typing import Optional

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
INVALID, VALID, BAD_POINT, UNDECIDED = 0, 1, 2, 3
ROWS = ("no_committee", "bad_message", "overlap", "bad_member", "empty_key", "identity_signature", "identity_message", "not_g2",
        "pairing")


@dataclass
class Group:
    key: int = 1                 # the aggregate key's scalar; 0 = the identity (an empty union)
    h: int = 1                   # the message point's scalar; 0 = the identity
    sig: int = 1                 # the aggregate signature's scalar; 0 = the identity
    no_committee: bool = False   # status_agg != 0
    bad_message: bool = False    # the message point's bytes are not a canonical curve point
    overlap: bool = False
    bad_member: bool = False
    sig_in_g2: bool = True       # False: the aggregate is a curve point outside G2 (a non-zero scalar then means nothing)


def decide(g: Group):
    """-> (verdict, deciding row)."""
    if g.no_committee:
        return UNDECIDED, "no_committee"
    if g.bad_message:
        return BAD_POINT, "bad_message"
    for row, hit in (("overlap", g.overlap), ("bad_member", g.bad_member), ("empty_key", g.key % R_ORDER == 0),
                     ("identity_signature", g.sig % R_ORDER == 0), ("identity_message", g.h % R_ORDER == 0),
                     ("not_g2", not g.sig_in_g2)):
        if hit:
            return INVALID, row
    return (VALID if (g.key * g.h - g.sig) % R_ORDER == 0 else INVALID), "pairing"


def applied_sig_valid(before: int, g: Group) -> int:
    """AttGroup::sig_valid after the call under PE_VERIFY_APPLY: sig_valid &= (verdict == 1), rows 2 to 4 only."""
    v, row = decide(g)
    return before if row == "no_committee" else (before if v == VALID else 0)


def stats(groups, subgroup_pass: Optional[bool] = None) -> dict:
    """What pe_profile_verify_resident_stats reports for these groups."""
    out = {r: 0 for r in ROWS}
    for g in groups:
        out[decide(g)[1]] += 1
    out["groups"] = len(groups)
    if subgroup_pass is not None:
        out["subgroup_pass"] = int(subgroup_pass)
    return out
