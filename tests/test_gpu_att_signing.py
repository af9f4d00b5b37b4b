"""-m gpu: pe_attestation_signing_roots -- the signing roots of attestation rows from k_att_signing_roots, byte for byte
against tests/att_signing_model.py: the lane, wave and workgroup edges of the launch, rows and roots in host and in device
memory (16-byte aligned: in place; one byte off: the copy route), the integer and fork edges of the host test, and the error
returns, each of which writes nothing and is followed by a valid call."""
import ctypes as C

import numpy as np
import pytest

import pos_evolution_amd as pea
from pos_evolution_amd import _abi
from tests import att_signing_model as am

pytestmark = pytest.mark.gpu
WG = 256                                                     # lanes of one workgroup of k_att_signing_roots
FORK = 2**63                                                 # uniform random target epochs fall on both sides
DOMAINS = (am.DOMAIN_PREVIOUS, am.DOMAIN_CURRENT)


@pytest.fixture(scope="module")
def engine(engine_factory):
    return engine_factory(device=0)


@pytest.fixture(scope="module")
def many():
    """WG + 1 random rows and their model roots, computed once"""
    rows = am.random_rows(WG + 1, 21)
    want = np.frombuffer(b"".join(am.signing_root(r, FORK, *DOMAINS) for r in rows), dtype=np.uint8).reshape(-1, 32)
    assert {r["target_epoch"] < FORK for r in rows} == {True, False}
    return am.to_records(rows), want


def _want(rows, fork_epoch):
    return np.frombuffer(b"".join(am.signing_root(r, fork_epoch, *DOMAINS) for r in rows), dtype=np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, WG + 1])
def test_lane_wave_and_workgroup_edges(engine, many, n):
    recs, want = many
    got = engine.attestation_signing_roots(recs[:n], FORK, *DOMAINS)
    assert got.shape == (n, 32) and np.array_equal(got, want[:n])


def test_rows_and_roots_in_host_and_device_memory(engine, many):
    import torch

    recs, want = many
    n = 65
    flat = recs[:n].view(np.uint8).reshape(-1)
    rows16 = torch.from_numpy(flat.copy()).cuda()
    rows1 = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), flat])).cuda()
    assert rows16.data_ptr() % 16 == 0 and (rows1.data_ptr() + 1) % 16 == 1
    sources = {"host": recs[:n], "device": pea.DeviceRows(rows16.data_ptr(), n, keep=rows16),
               "device + 1": pea.DeviceRows(rows1.data_ptr() + 1, n, keep=rows1)}
    for name, src in sources.items():
        assert np.array_equal(engine.attestation_signing_roots(src, FORK, *DOMAINS), want[:n]), name
        out16 = torch.full((32 * n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
        res = engine.attestation_signing_roots(src, FORK, *DOMAINS, out=pea.DeviceArena(out16.data_ptr(), 32 * n, keep=out16))
        assert res.__class__ is pea.DeviceArena
        back = out16.cpu().numpy()
        assert np.array_equal(back[:32 * n].reshape(n, 32), want[:n]) and (back[32 * n:] == 0xAB).all(), name
        out1 = torch.full((32 * n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
        engine.attestation_signing_roots(src, FORK, *DOMAINS, out=pea.DeviceArena(out1.data_ptr() + 1, 32 * n, keep=out1))
        back = out1.cpu().numpy()
        assert back[0] == 0xAB and np.array_equal(back[1:1 + 32 * n].reshape(n, 32), want[:n]) and (back[1 + 32 * n:] == 0xAB).all(), name
    # the roots lie as pe_hash_to_g2 takes its messages: device roots -> points, against host roots -> points
    out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    arena = engine.attestation_signing_roots(sources["device"], FORK, *DOMAINS, out=pea.DeviceArena(out.data_ptr(), 32 * n, keep=out))
    assert np.array_equal(engine.hash_to_g2((arena, 32))[:3], engine.hash_to_g2(want[:3]))
    # a list of AttRow is packed as every other call packs it
    r = am.base_row()
    att = pea.AttRow(r["slot"] % 2**63, r["index"], r["beacon_block_root"], r["source_epoch"], r["source_root"], r["target_epoch"],
                     r["target_root"], bits=np.ones(3, dtype=bool))
    assert engine.attestation_signing_roots([att], FORK, *DOMAINS)[0].tobytes() == \
        am.signing_root(dict(r, slot=r["slot"] % 2**63), FORK, *DOMAINS)


def test_field_and_fork_edges(engine):
    rows = am.edge_rows()
    for fork_epoch in (0, 2**32, 2**32 + 1, 2**64 - 1):
        assert np.array_equal(engine.attestation_signing_roots(am.to_records(rows), fork_epoch, *DOMAINS), _want(rows, fork_epoch))
    for row, fork_epoch in am.fork_edge_cases():
        got = engine.attestation_signing_roots(am.to_records([row]), fork_epoch, *DOMAINS)[0].tobytes()
        assert got == am.signing_root(row, fork_epoch, *DOMAINS)
        swapped = engine.attestation_signing_roots(am.to_records([row]), fork_epoch, DOMAINS[1], DOMAINS[0])[0].tobytes()
        assert swapped == am.signing_root(row, fork_epoch, DOMAINS[1], DOMAINS[0]) != got
    rows = [am.base_row()] + am.one_field_changed() + am.outside_data_changed()
    got = engine.attestation_signing_roots(am.to_records(rows), 5, *DOMAINS)
    assert np.array_equal(got, _want(rows, 5))
    assert len({g.tobytes() for g in got[:8]}) == 8 and all(g.tobytes() == got[0].tobytes() for g in got[8:])


def test_error_returns_write_nothing_and_a_valid_call_follows(engine, engine_factory, many):
    recs, want = many
    n = 5
    lib, h = engine._lib, engine._h
    dom = engine._attester_domains(FORK, *DOMAINS)
    sentinel = np.full(32 * n, 0x77, dtype=np.uint8)
    rows_ptr = recs.ctypes.data

    def valid_call_follows(e=engine):
        assert np.array_equal(e.attestation_signing_roots(recs[:n], FORK, *DOMAINS), want[:n])

    def call(n_rows, dom_arg, e=engine):
        return e._lib.pe_attestation_signing_roots(e._h, rows_ptr, n_rows, dom_arg, sentinel.ctypes.data)

    assert call(n, None) == _abi.PE_ERR_INVALID_ARG and (sentinel == 0x77).all()      # NULL dom
    valid_call_follows()
    assert lib.pe_attestation_signing_roots(h, None, n, C.byref(dom), sentinel.ctypes.data) == _abi.PE_ERR_INVALID_ARG
    assert lib.pe_attestation_signing_roots(h, rows_ptr, n, C.byref(dom), None) == _abi.PE_ERR_INVALID_ARG
    assert (sentinel == 0x77).all()
    valid_call_follows()
    with engine.pipeline():                                                           # inside a pipeline
        assert call(n, C.byref(dom)) == _abi.PE_ERR_STATE and (sentinel == 0x77).all()
    valid_call_follows()
    assert call(2**24 + 1, C.byref(dom)) == _abi.PE_ERR_CAPACITY and (sentinel == 0x77).all()   # a size only: no such buffer
    valid_call_follows()
    assert call(0, C.byref(dom)) == _abi.PE_OK and (sentinel == 0x77).all()           # n == 0
    assert lib.pe_attestation_signing_roots(h, None, 0, C.byref(dom), None) == _abi.PE_OK
    d = engine_factory(device=0)                                                      # under pe_dist_init*
    valid_call_follows(d)
    d.dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    assert call(n, C.byref(dom), d) == _abi.PE_ERR_STATE and (sentinel == 0x77).all()
    d.dist_destroy()
    valid_call_follows(d)
    with pytest.raises(ValueError):
        engine.attestation_signing_roots(recs[:n], FORK, bytes(31), DOMAINS[1])
