"""The message of an attestation's signature, as the consensus specification computes it -- the specification of
pos_evolution_amd/csrc/att_signing_row.h, k_att_signing_roots and pe_verify_resident_data.

Built from tests/ssz_model.py's ``merkleize`` and ``u64_chunk`` (which the SSZ golden vectors pin) and hashlib:

    hash_tree_root(Checkpoint)        merkleize([u64_chunk(epoch), root], 1)
    hash_tree_root(AttestationData)   merkleize([slot, index, beacon_block_root, root(source), root(target)], 3)
    compute_signing_root(data, d)     hash_tree_root(SigningData(root(data), d)) = merkleize([root(data), d], 1)
    compute_fork_data_root(v, gvr)    merkleize([v padded to a chunk, gvr], 1)
    compute_domain(type, v, gvr)      type + compute_fork_data_root(v, gvr)[:28]
    get_domain(fork, type, epoch, gvr)  compute_domain over fork.previous_version if epoch < fork.epoch else current_version

A row is a dict (or a record of synth.ATT_DTYPE) with the seven fields of AttestationData as pe_attestation names them.
"""
import json
import os

import numpy as np

from tests import ssz_model as sm

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "att_signing_vectors.json")
DOMAIN_BEACON_ATTESTER = bytes([1, 0, 0, 0])
U64_EDGES = (0, 2**32, 2**64 - 1)
FIELDS = ("slot", "index", "beacon_block_root", "source_epoch", "source_root", "target_epoch", "target_root")


def _b(v) -> bytes:
    return v.tobytes() if isinstance(v, np.ndarray) else bytes(v)


def checkpoint_root(epoch: int, root: bytes) -> bytes:
    assert len(root) == 32
    return sm.merkleize([sm.u64_chunk(int(epoch)), bytes(root)], 1)


def attestation_data_chunks(row) -> list:
    return [sm.u64_chunk(int(row["slot"])), sm.u64_chunk(int(row["index"])), _b(row["beacon_block_root"]),
            checkpoint_root(int(row["source_epoch"]), _b(row["source_root"])),
            checkpoint_root(int(row["target_epoch"]), _b(row["target_root"]))]


def attestation_data_root(row) -> bytes:
    return sm.merkleize(attestation_data_chunks(row), 3)


def compute_fork_data_root(current_version: bytes, genesis_validators_root: bytes) -> bytes:
    assert len(current_version) == 4 and len(genesis_validators_root) == 32
    return sm.merkleize([bytes(current_version) + bytes(28), bytes(genesis_validators_root)], 1)


def compute_domain(domain_type: bytes, fork_version: bytes = bytes(4), genesis_validators_root: bytes = bytes(32)) -> bytes:
    assert len(domain_type) == 4
    return bytes(domain_type) + compute_fork_data_root(fork_version, genesis_validators_root)[:28]


def get_domain(fork_epoch: int, previous_version: bytes, current_version: bytes, genesis_validators_root: bytes,
               domain_type: bytes, epoch: int) -> bytes:
    version = previous_version if int(epoch) < int(fork_epoch) else current_version
    return compute_domain(domain_type, version, genesis_validators_root)


def pick_domain(target_epoch: int, fork_epoch: int, domain_previous: bytes, domain_current: bytes) -> bytes:
    """get_domain's choice between the two domains a fork leaves (pe_attester_domains)"""
    return domain_previous if int(target_epoch) < int(fork_epoch) else domain_current


def signing_root(row, fork_epoch: int, domain_previous: bytes, domain_current: bytes) -> bytes:
    domain = pick_domain(int(row["target_epoch"]), fork_epoch, domain_previous, domain_current)
    assert len(domain) == 32
    return sm.merkleize([attestation_data_root(row), bytes(domain)], 1)


# ---------------------------------------------------------------------------------------------------------------- rows
def base_row() -> dict:
    return dict(slot=0x0102030405060708, index=0x1112131415161718, beacon_block_root=bytes(range(32, 64)),
                source_epoch=0x2122232425262728, source_root=bytes(range(64, 96)),
                target_epoch=0x3132333435363738, target_root=bytes(range(96, 128)), bits_offset=0, n_bits=0, flags=0, reserved0=0)


def one_field_changed() -> list:
    """seven rows, each differing from base_row() in exactly one field of AttestationData"""
    out = []
    for name in FIELDS:
        r = base_row()
        r[name] = (r[name] ^ 1) if isinstance(r[name], int) else bytes([r[name][0] ^ 1]) + r[name][1:]
        out.append(r)
    return out


def outside_data_changed() -> list:
    """rows that differ from base_row() only outside AttestationData: the same root"""
    out = []
    for name, v in (("flags", 0xFFFFFFFF), ("n_bits", 12345), ("bits_offset", 0x80000001), ("reserved0", 7)):
        r = base_row()
        r[name] = v
        out.append(r)
    return out


def edge_rows() -> list:
    """slot, index and both epochs at 0, 2^32 and 2^64 - 1: every combination of one value per field is too many; each
    field walks the edges while the others stay at the base row's, then all four together at each edge."""
    out = []
    for name in ("slot", "index", "source_epoch", "target_epoch"):
        for v in U64_EDGES:
            r = base_row()
            r[name] = v
            out.append(r)
    for v in U64_EDGES:
        r = base_row()
        r.update(slot=v, index=v, source_epoch=v, target_epoch=v)
        out.append(r)
    return out


def fork_edge_cases() -> list:
    """[(row, fork_epoch)]: target_epoch at fork_epoch - 1 and at fork_epoch, with fork_epoch at 0 and at 2^64 - 1 (and in
    between); fork_epoch 0 has nothing before it, so every epoch takes the current domain."""
    out = []
    for fork_epoch in (0, 1, 2**32, 2**64 - 1):
        for target in sorted({max(fork_epoch - 1, 0), fork_epoch, 0, 2**64 - 1}):
            r = base_row()
            r["target_epoch"] = target
            out.append((r, fork_epoch))
    return out


def random_rows(n: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        u = [int(x) for x in rng.integers(0, 2**64, size=4, dtype=np.uint64)]
        out.append(dict(slot=u[0], index=u[1], beacon_block_root=rng.bytes(32), source_epoch=u[2], source_root=rng.bytes(32),
                        target_epoch=u[3], target_root=rng.bytes(32), bits_offset=int(rng.integers(0, 2**32)),
                        n_bits=int(rng.integers(0, 2**32)), flags=int(rng.integers(0, 2**32)), reserved0=0))
    return out


def to_records(rows):
    """rows -> a structured array of pe_attestation (synth.ATT_DTYPE)"""
    from pos_evolution_amd import synth

    out = np.zeros(len(rows), dtype=synth.ATT_DTYPE)
    for i, r in enumerate(rows):
        for name in synth.ATT_DTYPE.names:
            v = r[name]
            out[name][i] = np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray)) else v
    return out


DOMAIN_PREVIOUS = compute_domain(DOMAIN_BEACON_ATTESTER, bytes([0, 0, 0, 1]), bytes(range(200, 232)))
DOMAIN_CURRENT = compute_domain(DOMAIN_BEACON_ATTESTER, bytes([0, 0, 0, 2]), bytes(range(200, 232)))


# ------------------------------------------------------------------------------------------------------------- vectors
def golden_vectors() -> dict:
    """A small recorded set, written by this model: the test regenerates and compares it."""
    rows = [base_row()] + one_field_changed() + edge_rows()[:3] + random_rows(4, 11)
    fork_epoch = 0x3132333435363738      # the base row's target epoch: it takes the current domain, one below the previous
    below = base_row()
    below["target_epoch"] = fork_epoch - 1
    rows.append(below)
    return {
        "domain_type": DOMAIN_BEACON_ATTESTER.hex(),
        "fork_epoch": fork_epoch,
        "domain_previous": DOMAIN_PREVIOUS.hex(),
        "domain_current": DOMAIN_CURRENT.hex(),
        "fork_data_root": compute_fork_data_root(bytes([0, 0, 0, 2]), bytes(range(200, 232))).hex(),
        "rows": [{**{k: (v.hex() if isinstance(v, bytes) else v) for k, v in r.items() if k in FIELDS},
                  "data_root": attestation_data_root(r).hex(),
                  "signing_root": signing_root(r, fork_epoch, DOMAIN_PREVIOUS, DOMAIN_CURRENT).hex()} for r in rows],
    }


if __name__ == "__main__":
    with open(GOLDEN_PATH, "w") as f:
        json.dump(golden_vectors(), f, indent=1)
        f.write("\n")
