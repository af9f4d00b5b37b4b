"""CPU: the rule table of pe_verify_resident as tests/verify_resident_model.py restates it -- every row, the precedence of the
rows, what PE_VERIFY_APPLY does with a verdict, one group held to the real pairing of tests/pairing_model.py -- and the surface
the call has on every layer (header, binding, engine, forkchoice)."""
import dataclasses
import os
import re

import pytest

from oracle import g1, g2
from tests import pairing_model as pm
from tests import verify_resident_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
R = vm.R_ORDER
KEY, H = 0x1F2E3D4C5B6A7988ABCDEF % R, 0x5A3C19E0F1D2B4A697887766 % R
HONEST = vm.Group(key=KEY, h=H, sig=KEY * H % R)
# one field changed per row of the table, in the table's order
TRIGGER = dict(no_committee=dict(no_committee=True), bad_message=dict(bad_message=True), overlap=dict(overlap=True),
               bad_member=dict(bad_member=True), empty_key=dict(key=0), identity_signature=dict(sig=0),
               identity_message=dict(h=0), not_g2=dict(sig_in_g2=False))


def test_the_honest_group_and_its_forgeries():
    assert vm.decide(HONEST) == (vm.VALID, "pairing")
    assert vm.decide(dataclasses.replace(HONEST, sig=(HONEST.sig + 1) % R)) == (vm.INVALID, "pairing")
    assert vm.decide(dataclasses.replace(HONEST, sig=KEY * (H + 1) % R)) == (vm.INVALID, "pairing")     # signed another message
    assert vm.decide(dataclasses.replace(HONEST, key=(KEY + 1) % R)) == (vm.INVALID, "pairing")         # another signer set
    assert vm.decide(dataclasses.replace(HONEST, sig=HONEST.sig + R)) == (vm.VALID, "pairing")           # scalars are mod r
    # the cancelling pair: sig_a + D and sig_b - D are both invalid although their sum is the honest sum
    other = vm.Group(key=KEY + 5, h=H, sig=(KEY + 5) * H % R)
    d = 0xD00D
    a, b = dataclasses.replace(HONEST, sig=(HONEST.sig + d) % R), dataclasses.replace(other, sig=(other.sig - d) % R)
    assert vm.decide(a)[0] == vm.decide(b)[0] == vm.INVALID
    assert (a.sig + b.sig - a.key * a.h - b.key * b.h) % R == 0


@pytest.mark.parametrize("row", list(TRIGGER))
def test_every_row_decides_an_otherwise_honest_group(row):
    want = {"no_committee": vm.UNDECIDED, "bad_message": vm.BAD_POINT}.get(row, vm.INVALID)
    assert vm.decide(dataclasses.replace(HONEST, **TRIGGER[row])) == (want, row)


def test_precedence_is_the_order_of_the_table():
    rows = list(TRIGGER)
    assert tuple(rows) + ("pairing",) == vm.ROWS
    for i, first in enumerate(rows):
        for later in rows[i + 1:]:
            both = dataclasses.replace(HONEST, **{**TRIGGER[later], **TRIGGER[first]})
            assert vm.decide(both)[1] == first, (first, later)
    everything = dataclasses.replace(HONEST, **{k: v for t in TRIGGER.values() for k, v in t.items()})
    assert vm.decide(everything) == (vm.UNDECIDED, "no_committee")
    # rows 3 give 0 whatever the pairing value would be: an empty key with an identity signature has exponent 0
    assert vm.decide(vm.Group(key=0, h=H, sig=0)) == (vm.INVALID, "empty_key")
    assert vm.decide(vm.Group(key=KEY, h=0, sig=0)) == (vm.INVALID, "identity_signature")


def test_apply_ands_the_verdict_into_sig_valid():
    for before in (0, 1):
        assert vm.applied_sig_valid(before, HONEST) == before                                     # 1 leaves the flag alone
        assert vm.applied_sig_valid(before, dataclasses.replace(HONEST, sig=1)) == 0
        assert vm.applied_sig_valid(before, dataclasses.replace(HONEST, bad_message=True)) == 0   # verdict 2 is not 1
        assert vm.applied_sig_valid(before, dataclasses.replace(HONEST, no_committee=True)) == before   # untouched
    g = dataclasses.replace(HONEST, overlap=True)
    assert vm.applied_sig_valid(vm.applied_sig_valid(1, g), g) == 0                                # twice is harmless


def test_stats_count_groups_by_deciding_row():
    groups = [HONEST, dataclasses.replace(HONEST, sig=3), dataclasses.replace(HONEST, key=0), dataclasses.replace(HONEST, h=0)]
    s = vm.stats(groups, subgroup_pass=True)
    assert s["pairing"] == 2 and s["empty_key"] == 1 and s["identity_message"] == 1 and s["groups"] == 4
    assert sum(s[r] for r in vm.ROWS) == 4 and s["subgroup_pass"] == 1


def test_the_exponent_route_is_a_real_pairing():
    """e(key G1, h G2) e(-G1, sig G2) == 1 exactly where key h - sig == 0 (mod r), with small scalars so that it stays quick."""
    key, h = 5, 7
    pk, msg = g1.mul(key, g1.G), g2.mul(h, g2.G2)
    for sig, want in ((35, vm.VALID), (36, vm.INVALID)):
        f = pm.pairing_product([(pk, msg), (g1.neg(g1.G), g2.mul(sig, g2.G2))])
        assert (f == pm.F12_ONE) == (want == vm.VALID)
        assert vm.decide(vm.Group(key=key, h=h, sig=sig))[0] == want


def test_the_kernels_count_in_the_models_order():
    text = open(os.path.join(CSRC, "kernels.h")).read()
    names = re.search(r"enum \{ (BLS_RES_NO_COMMITTEE[^}]*)\}", text).group(1).replace("\n", " ")
    got = [n.strip()[len("BLS_RES_"):].lower().replace(" = 0", "") for n in names.split(",") if n.strip()]
    want = [r.replace("identity_signature", "identity_sig").replace("identity_message", "identity_msg") for r in vm.ROWS]
    assert got == want + ["reasons"]
    assert int(re.search(r"BLS_UNDECIDED\s*=\s*(\d+)", text).group(1)) == vm.UNDECIDED


def test_surface_on_every_layer():
    from pos_evolution_amd import _abi, engine, forkchoice
    boundary = open(os.path.join(ROOT, "include", "posevo.h")).read()
    profile = open(os.path.join(ROOT, "include", "posevo_profile.h")).read()
    for name, text in (("pe_verify_resident", boundary), ("pe_profile_verify_resident_stats", profile)):
        args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name     # handle included
    assert "pe_profile_verify_resident_stats" not in boundary                   # measurement is not boundary
    assert int(re.search(r"#define\s+PE_BLS_UNDECIDED\s+(\d+)", boundary).group(1)) == _abi.PE_BLS_UNDECIDED == vm.UNDECIDED
    assert int(re.search(r"#define\s+PE_VERIFY_APPLY\s+0x(\w+?)u", boundary).group(1), 16) == _abi.PE_VERIFY_APPLY
    assert int(re.search(r"#define\s+PE_VERIFY_RESIDENT_STATS\s+(\d+)", profile).group(1)) == _abi.PE_VERIFY_RESIDENT_STATS \
        == len(vm.ROWS) + 2
    assert callable(engine.Engine.verify_resident) and callable(forkchoice.verify_resident_attestations)
