"""CPU: tests/att_signing_model.py -- the signing root of an attestation -- against what follows from SSZ alone, against
pos_evolution_amd.forkchoice's scalar functions, and against its own recorded vectors; and the layout of pe_attester_domains in
C and in the binding."""
import ctypes as C
import json
import os
import subprocess
from types import SimpleNamespace

import pytest

from tests import att_signing_model as am
from tests import ssz_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(row):
    """a row as the duck-typed AttestationData forkchoice takes"""
    return SimpleNamespace(slot=row["slot"], index=row["index"], beacon_block_root=row["beacon_block_root"],
                           source=SimpleNamespace(epoch=row["source_epoch"], root=row["source_root"]),
                           target=SimpleNamespace(epoch=row["target_epoch"], root=row["target_root"]))


def _all_rows():
    return [am.base_row()] + am.one_field_changed() + am.outside_data_changed() + am.edge_rows() + am.random_rows(16, 3)


def test_the_zero_objects_follow_from_the_zero_hashes():
    """From SSZ alone: the all-zero Checkpoint is two zero chunks, so its root is Z[1].  The all-zero AttestationData is NOT
    eight zero chunks -- chunks 3 and 4 are the Checkpoints' roots, Z[1] each -- so its root is not Z[3] but the tree over
    (0, 0, 0, Z[1], Z[1], 0, 0, 0), written out here in zero hashes and one-hash steps."""
    z, H = sm.zero_hashes(), sm.H
    zero = dict(slot=0, index=0, beacon_block_root=bytes(32), source_epoch=0, source_root=bytes(32), target_epoch=0,
                target_root=bytes(32))
    assert am.checkpoint_root(0, bytes(32)) == z[1]
    assert am.attestation_data_chunks(zero) == [z[0], z[0], z[0], z[1], z[1]]
    want = H(H(z[1] + H(z[0] + z[1])) + H(H(z[1] + z[0]) + z[1]))
    assert am.attestation_data_root(zero) == want != z[3]
    # a tree whose five chunks ARE zero is Z[3]: the merkleization itself pads with zero chunks
    assert sm.merkleize([z[0]] * 5, 3) == z[3]


def test_five_chunks_merkleize_as_eight():
    for row in _all_rows():
        chunks = am.attestation_data_chunks(row)
        assert len(chunks) == 5
        assert am.attestation_data_root(row) == sm.merkleize_literal(chunks + [bytes(32)] * 3, 3)
        assert am.checkpoint_root(row["source_epoch"], row["source_root"]) == \
            sm.H(int(row["source_epoch"]).to_bytes(8, "little") + bytes(24) + row["source_root"])


def test_one_field_moves_the_root_and_nothing_outside_the_data_does():
    args = (5, am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT)
    base = am.signing_root(am.base_row(), *args)
    changed = [am.signing_root(r, *args) for r in am.one_field_changed()]
    assert len({base, *changed}) == 8
    assert all(am.signing_root(r, *args) == base for r in am.outside_data_changed())


def test_forkchoice_computes_what_the_model_computes():
    from pos_evolution_amd import forkchoice as fc

    assert fc.DOMAIN_BEACON_ATTESTER == am.DOMAIN_BEACON_ATTESTER
    gvr = bytes(range(7, 39))
    for version in (bytes(4), bytes([1, 2, 3, 4]), bytes([255] * 4)):
        assert fc.compute_fork_data_root(version, gvr) == am.compute_fork_data_root(version, gvr)
        for dtype in (am.DOMAIN_BEACON_ATTESTER, bytes([7, 0, 0, 0])):
            d = fc.compute_domain(dtype, version, gvr)
            assert d == am.compute_domain(dtype, version, gvr) and d[:4] == dtype and len(d) == 32
    assert fc.compute_domain(am.DOMAIN_BEACON_ATTESTER) == am.compute_domain(am.DOMAIN_BEACON_ATTESTER, bytes(4), bytes(32))
    for fork_epoch in (0, 1, 2**32, 2**64 - 1):
        state = SimpleNamespace(fork=SimpleNamespace(previous_version=bytes([0, 0, 0, 1]), current_version=bytes([0, 0, 0, 2]),
                                                     epoch=fork_epoch), genesis_validators_root=gvr)
        prev, cur = (am.compute_domain(am.DOMAIN_BEACON_ATTESTER, v, gvr) for v in (bytes([0, 0, 0, 1]), bytes([0, 0, 0, 2])))
        assert prev != cur
        for epoch in {0, max(fork_epoch - 1, 0), fork_epoch, 2**64 - 1}:
            got = fc.get_domain(state, am.DOMAIN_BEACON_ATTESTER, epoch)
            assert got == am.get_domain(fork_epoch, bytes([0, 0, 0, 1]), bytes([0, 0, 0, 2]), gvr, am.DOMAIN_BEACON_ATTESTER, epoch)
            assert got == am.pick_domain(epoch, fork_epoch, prev, cur) == (prev if epoch < fork_epoch else cur)
    for row in _all_rows():
        for domain in (am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT):
            assert fc.compute_signing_root(_data(row), domain) == am.signing_root(row, 0, domain, domain)
    for row, fork_epoch in am.fork_edge_cases():
        want = am.DOMAIN_PREVIOUS if row["target_epoch"] < fork_epoch else am.DOMAIN_CURRENT
        assert am.signing_root(row, fork_epoch, am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT) == fc.compute_signing_root(_data(row), want)


def test_recorded_vectors():
    want = json.load(open(am.GOLDEN_PATH))
    assert want == json.loads(json.dumps(am.golden_vectors()))
    assert os.path.getsize(am.GOLDEN_PATH) < 16384
    assert len({r["signing_root"] for r in want["rows"]}) == len(want["rows"])
    # the base row at the fork takes the current domain, the same data one epoch below it the previous one
    base, below = want["rows"][0], want["rows"][-1]
    assert base["target_epoch"] == want["fork_epoch"] == below["target_epoch"] + 1
    assert base["signing_root"] == sm.H(bytes.fromhex(base["data_root"]) + bytes.fromhex(want["domain_current"])).hex()
    assert below["signing_root"] == sm.H(bytes.fromhex(below["data_root"]) + bytes.fromhex(want["domain_previous"])).hex()


def test_struct_layout_in_c_and_in_the_binding(tmp_path):
    from pos_evolution_amd import _abi

    assert C.sizeof(_abi.pe_attester_domains) == 72
    assert [(_abi.pe_attester_domains.fork_epoch.offset), _abi.pe_attester_domains.domain_previous.offset,
            _abi.pe_attester_domains.domain_current.offset] == [0, 8, 40]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "posevo.h"\n'
                   'typedef char size_is_72[sizeof(pe_attester_domains) == 72 ? 1 : -1];\n'
                   'typedef char prev_at_8[offsetof(pe_attester_domains, domain_previous) == 8 ? 1 : -1];\n'
                   'typedef char cur_at_40[offsetof(pe_attester_domains, domain_current) == 40 ? 1 : -1];\n'
                   'typedef char tag_is_43[sizeof(PE_ETH2_DST) == 44 ? 1 : -1];\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])
    header = open(os.path.join(ROOT, "include", "posevo.h")).read()
    assert ('"%s"' % _abi.ETH2_DST.decode()) in header
    for name in ("pe_attestation_signing_roots", "pe_verify_resident_data"):
        assert name in _abi.SIGNATURES


def test_python_surface():
    from pos_evolution_amd import engine, forkchoice

    for name in ("attestation_signing_roots", "verify_resident_data"):
        assert callable(getattr(engine.Engine, name))
    for name in ("compute_fork_data_root", "compute_domain", "get_domain", "compute_signing_root", "verify_resident_attestation_data",
                 "verify_resident_attestations"):
        assert callable(getattr(forkchoice, name))
