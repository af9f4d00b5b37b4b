"""CPU: pos_evolution_amd/csrc/att_signing_row.h -- the text k_att_signing_roots runs per lane -- compiled by the host compiler
alone into a program of its own (tests/native/att_signing_row_host.cpp) and held to tests/att_signing_model.py: random rows,
the 64-bit edges of every integer field, the fork boundary at both ends of the epoch range, one field changed at a time, and
the fields outside AttestationData.  And the build side: the kernel's resource report shows no scratch."""
import os
import re
import struct
import subprocess

import pytest

from tests import att_signing_model as am
from tests import ssz_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("att_signing") / "att_signing_row_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "att_signing_row_host.cpp"),
                           "-o", str(exe)])

    def run(rows, fork_epoch, domain_previous=am.DOMAIN_PREVIOUS, domain_current=am.DOMAIN_CURRENT):
        """-> [(data root, signing root)] per row"""
        data = struct.pack("<Q", fork_epoch) + domain_previous + domain_current + am.to_records(rows).tobytes()
        out = subprocess.run([str(exe)], input=data, capture_output=True)
        assert out.returncode == 0, out.stderr.decode()
        assert len(out.stdout) == 64 * len(rows) + 32
        assert out.stdout[-32:] == sm.zero_hashes()[1]                 # the constant of the header
        return [(out.stdout[64 * i:64 * i + 32], out.stdout[64 * i + 32:64 * i + 64]) for i in range(len(rows))]
    return run


def _want(rows, fork_epoch, prev=am.DOMAIN_PREVIOUS, cur=am.DOMAIN_CURRENT):
    return [(am.attestation_data_root(r), am.signing_root(r, fork_epoch, prev, cur)) for r in rows]


def test_random_rows(program):
    rows = am.random_rows(200, 5)
    for fork_epoch in (0, 2**63, 2**64 - 1):                           # uniform target epochs fall on both sides of 2^63
        assert program(rows, fork_epoch) == _want(rows, fork_epoch)
    assert program([], 7) == []


def test_integer_fields_at_their_edges(program):
    rows = am.edge_rows()
    assert {r[f] for r in rows for f in ("slot", "index", "source_epoch", "target_epoch")} >= set(am.U64_EDGES)
    for fork_epoch in (0, 2**32, 2**32 + 1, 2**64 - 1):
        assert program(rows, fork_epoch) == _want(rows, fork_epoch)


def test_the_fork_boundary(program):
    cases = am.fork_edge_cases()
    assert {(r["target_epoch"], f) for r, f in cases} >= {(0, 0), (0, 1), (1, 1), (2**64 - 2, 2**64 - 1), (2**64 - 1, 2**64 - 1),
                                                          (2**32 - 1, 2**32), (2**32, 2**32)}
    for row, fork_epoch in cases:
        (data_root, root), = program([row], fork_epoch)
        domain = am.DOMAIN_PREVIOUS if row["target_epoch"] < fork_epoch else am.DOMAIN_CURRENT
        assert data_root == am.attestation_data_root(row)
        assert root == sm.H(data_root + domain) == am.signing_root(row, fork_epoch, am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT)
        swapped, = program([row], fork_epoch, am.DOMAIN_CURRENT, am.DOMAIN_PREVIOUS)
        assert swapped[0] == data_root and swapped[1] != root


def test_exactly_the_seven_fields_enter(program):
    rows = [am.base_row()] + am.one_field_changed() + am.outside_data_changed()
    got = program(rows, 5)
    assert got == _want(rows, 5)
    assert len({g[1] for g in got[:8]}) == 8 and len({g[0] for g in got[:8]}) == 8
    assert all(g == got[0] for g in got[8:]) and len(got) == 12


def test_the_kernel_uses_no_scratch():
    log = open(os.path.join(CSRC, "att_signing_kernels.resource.log")).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", log)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", log)]
    assert len(names) == len(scratch) == len(spills) == len(lds) == 1 and "k_att_signing_roots" in names[0]
    assert scratch == [0] and spills == [0] and lds == [0]
    # the register count DESIGN.md 3.12 quotes is the log's
    vgprs = int(re.search(r" VGPRs: (\d+)", log).group(1))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"k_att_signing_roots[^\n]*\b%d VGPRs" % vgprs, design), vgprs
    # ... and the kernel lives outside g1_kernels.hip, whose resource signatures are pinned
    assert "k_att_signing_roots" not in open(os.path.join(CSRC, "g1_kernels.hip")).read()
