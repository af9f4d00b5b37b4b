"""SSZ merkleisation of the per-validator fields of BeaconState (pe:354-369) with hashlib and nothing else: the model the
engine's pe_state_roots / pe_ssz_merkleize (pos_evolution_amd/csrc/engine_ssz.cpp, ssz_kernels.hip) are held to.

The reference names hash_tree_root (pe:142, 423, 1016) and holds no text of it; the rules are the SSZ specification's
[UPSTREAM-MEMORY]:
  * a chunk is 32 bytes; basic values pack little-endian, 4 uint64 or 32 uint8 to a chunk, the last chunk zero-padded
  * Z[0] = 32 zero bytes, Z[k + 1] = H(Z[k] || Z[k])
  * merkleize(chunks, depth) = the root of the binary tree of 2^depth leaves whose absent leaves are Z[0]
  * mix_in_length(root, n) = H(root || uint256_le(n))
  * hash_tree_root(List[basic, N]) = mix_in_length(merkleize(pack(values), log2(N * size / 32)), len(values))
  * hash_tree_root(List[Container, N]) = mix_in_length(merkleize([hash_tree_root(c) for c], log2 N), len)
  * hash_tree_root(Container) = merkleize of its fields' roots; Bytes48 is two chunks, the second zero-padded
`merkleize` is written twice -- the literal form and the zero-hash form -- and tests/test_ssz_model.py holds them to each other."""
import hashlib
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssz_vectors.json")
FAR_FUTURE_EPOCH = 2**64 - 1
ZERO_CHUNK = bytes(32)


def H(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def zero_hashes(n: int = 65) -> List[bytes]:
    z = [ZERO_CHUNK]
    for _ in range(n - 1):
        z.append(H(z[-1] + z[-1]))
    return z


Z = zero_hashes()


def chunks_of(data: bytes) -> List[bytes]:
    """Little-endian packed bytes -> 32-byte chunks, the last one zero-padded."""
    data = bytes(data)
    if len(data) % 32:
        data += bytes(32 - len(data) % 32)
    return [data[i:i + 32] for i in range(0, len(data), 32)]


def pack_u64(values) -> List[bytes]:
    return chunks_of(np.asarray(values, dtype="<u8").tobytes())


def pack_u8(values) -> List[bytes]:
    return chunks_of(np.asarray(values, dtype=np.uint8).tobytes())


def merkleize_literal(chunks: List[bytes], depth: int) -> bytes:
    """Pad to 2^depth chunks, hash every level in full."""
    assert len(chunks) <= 2**depth
    level = list(chunks) + [ZERO_CHUNK] * (2**depth - len(chunks))
    for _ in range(depth):
        level = [H(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


def merkleize(chunks: List[bytes], depth: int) -> bytes:
    """The zero-hash form: only nodes with a present child are computed; a missing right sibling of height k is Z[k]."""
    assert len(chunks) <= 2**depth
    if not chunks:
        return Z[depth]
    level = list(chunks)
    for k in range(depth):
        if len(level) % 2:
            level.append(Z[k])
        level = [H(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


def mix_in_length(root: bytes, n: int) -> bytes:
    return H(root + int(n).to_bytes(32, "little"))


def u64_chunk(v: int) -> bytes:
    return int(v).to_bytes(8, "little") + bytes(24)


def pubkey_leaf(pubkey48: bytes) -> bytes:
    assert len(pubkey48) == 48
    return H(pubkey48 + bytes(16))


def validator_root(pubkey48: bytes, withdrawal_credentials: bytes, effective_balance: int, slashed: int,
                   activation_eligibility_epoch: int, activation_epoch: int, exit_epoch: int, withdrawable_epoch: int) -> bytes:
    """hash_tree_root(Validator), fields in the order of pe:36-45."""
    assert len(withdrawal_credentials) == 32
    leaves = [pubkey_leaf(pubkey48), bytes(withdrawal_credentials), u64_chunk(effective_balance),
              bytes([1 if slashed else 0]) + bytes(31), u64_chunk(activation_eligibility_epoch), u64_chunk(activation_epoch),
              u64_chunk(exit_epoch), u64_chunk(withdrawable_epoch)]
    return merkleize(leaves, 3)


def u64_list_root(values, limit_log2: int = 40) -> bytes:
    return mix_in_length(merkleize(pack_u64(values), limit_log2 - 2), len(values))


def u8_list_root(values, limit_log2: int = 40) -> bytes:
    return mix_in_length(merkleize(pack_u8(values), limit_log2 - 5), len(values))


@dataclass
class Registry:
    """The per-validator part of a BeaconState, one entry per validator in every list."""
    pubkeys: List[bytes] = field(default_factory=list)
    withdrawal_credentials: List[bytes] = field(default_factory=list)
    effective_balance: List[int] = field(default_factory=list)
    slashed: List[int] = field(default_factory=list)
    activation_eligibility_epoch: List[int] = field(default_factory=list)
    activation_epoch: List[int] = field(default_factory=list)
    exit_epoch: List[int] = field(default_factory=list)
    withdrawable_epoch: List[int] = field(default_factory=list)
    balances: List[int] = field(default_factory=list)
    inactivity_scores: List[int] = field(default_factory=list)
    previous_epoch_participation: List[int] = field(default_factory=list)
    current_epoch_participation: List[int] = field(default_factory=list)

    def __len__(self):
        return len(self.balances)

    def validator_leaves(self) -> List[bytes]:
        return [validator_root(self.pubkeys[v], self.withdrawal_credentials[v], self.effective_balance[v], self.slashed[v],
                               self.activation_eligibility_epoch[v], self.activation_epoch[v], self.exit_epoch[v],
                               self.withdrawable_epoch[v]) for v in range(len(self))]


def validators_root(leaves: List[bytes], limit_log2: int = 40) -> bytes:
    return mix_in_length(merkleize(leaves, limit_log2), len(leaves))


def state_roots(reg: Registry, limit_log2: int = 40) -> dict:
    """The five list roots, named as pe_state_root_set names them."""
    return {"balances": u64_list_root(reg.balances, limit_log2),
            "inactivity_scores": u64_list_root(reg.inactivity_scores, limit_log2),
            "previous_epoch_participation": u8_list_root(reg.previous_epoch_participation, limit_log2),
            "current_epoch_participation": u8_list_root(reg.current_epoch_participation, limit_log2),
            "validators": validators_root(reg.validator_leaves(), limit_log2)}


ENGINE_MAX_EFFECTIVE_BALANCE = 65535 * 10**9 + 10**9 - 1  # the engine keeps effective_balance / increment in 16 bits


def random_registry(n: int, seed: int, max_effective_balance: int = 2**64 - 1) -> Registry:
    """All 64 bits of every uint64 in use (top bytes non-zero: a wrong byte order cannot pass), all 256 participation byte
    values once n allows, epochs that include 2^64 - 1, both `slashed` values.  effective_balance alone is uniform in
    0 .. max_effective_balance (ENGINE_MAX_EFFECTIVE_BALANCE for a registry an engine with the default increment takes)."""
    rng = np.random.default_rng(seed)

    def u64s():
        return [int(x) for x in (rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2)
                                 + rng.integers(0, 2, size=n, dtype=np.uint64)) | np.uint64(1 << 63)]

    def epochs():
        e = u64s()
        for v in range(0, n, 3):
            e[v] = FAR_FUTURE_EPOCH
        return e

    def part():
        p = rng.integers(0, 256, size=n, dtype=np.uint8)
        p[:min(n, 256)] = (np.arange(min(n, 256)) + seed) % 256
        return [int(x) for x in p]

    return Registry(pubkeys=[rng.bytes(48) for _ in range(n)], withdrawal_credentials=[rng.bytes(32) for _ in range(n)],
                    effective_balance=[x % (max_effective_balance + 1) for x in u64s()], slashed=[int(x) for x in (np.arange(n) + seed) % 2],
                    activation_eligibility_epoch=epochs(), activation_epoch=epochs(), exit_epoch=epochs(),
                    withdrawable_epoch=epochs(), balances=u64s(), inactivity_scores=u64s(),
                    previous_epoch_participation=part(), current_epoch_participation=part())
