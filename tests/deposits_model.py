"""process_deposit (pos-evolution.md lines 139-175) restated line by line with hashlib: the specification
pe_process_deposits / pe_deposit_signing_roots (pos_evolution_amd/csrc/engine_deposit.cpp, deposit_kernels.hip, deposit_row.h)
are held to -- TEST INFRASTRUCTURE ONLY.

The signature verdict is a parameter (`sig_ok[i]`: what bls.Verify(pubkey, signing_root, signature) returns for deposit i): the
pairing itself is tests/pairing_model.py's subject.  What the reference names without holding its text is the consensus
specification's [UPSTREAM-MEMORY]:
  * is_valid_merkle_branch(leaf, branch, depth, index, root): value = leaf; for i < depth: value = H(branch[i] || value) if
    index // 2^i % 2 else H(value || branch[i]); value == root
  * get_validator_from_deposit: effective_balance = min(amount - amount % EFFECTIVE_BALANCE_INCREMENT, MAX_EFFECTIVE_BALANCE),
    the four epochs FAR_FUTURE_EPOCH, slashed False, pubkey and withdrawal_credentials copied
  * compute_signing_root(obj, domain) = hash_tree_root(SigningData(hash_tree_root(obj), domain))
  * increase_balance: balances[index] += delta
oracle/_ref holds the reference's fork-choice and attestation functions (oracle/ref_extract.py's list); process_deposit is not
among them, so this model is not held to the reference's own text by execution -- it is held to it by reading."""
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

from tests import ssz_model as S

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deposit_vectors.json")
DEPOSIT_CONTRACT_TREE_DEPTH = 32
FAR_FUTURE_EPOCH = 2**64 - 1
EFFECTIVE_BALANCE_INCREMENT = 10**9
MAX_EFFECTIVE_BALANCE = 32 * 10**9
APPENDED, TOPUP, IGNORED_BAD_SIGNATURE, BAD_PROOF = 0, 1, 2, 3
NONE = 0xFFFFFFFF
H = S.H


@dataclass
class DepositData:
    pubkey: bytes
    withdrawal_credentials: bytes
    amount: int
    signature: bytes

    def wire(self) -> bytes:
        """struct pe_deposit_data: 184 bytes."""
        return self.pubkey + self.withdrawal_credentials + int(self.amount).to_bytes(8, "little") + self.signature


def deposit_message_root(d: DepositData) -> bytes:
    return S.merkleize([S.pubkey_leaf(d.pubkey), d.withdrawal_credentials, S.u64_chunk(d.amount)], 2)


def deposit_data_root(d: DepositData) -> bytes:
    assert len(d.signature) == 96
    sig_root = S.merkleize(S.chunks_of(d.signature), 2)  # three chunks padded to four
    return S.merkleize([S.pubkey_leaf(d.pubkey), d.withdrawal_credentials, S.u64_chunk(d.amount), sig_root], 2)


def signing_root(d: DepositData, domain: bytes) -> bytes:
    return H(deposit_message_root(d) + domain)


def is_valid_merkle_branch(leaf: bytes, branch: Sequence[bytes], depth: int, index: int, root: bytes) -> bool:
    value = leaf
    for i in range(depth):
        if index // (2**i) % 2:
            value = H(branch[i] + value)
        else:
            value = H(value + branch[i])
    return value == root


def branch_root(leaf: bytes, branch: Sequence[bytes], index: int) -> bytes:
    """The root a branch proves its leaf against (how the tests make valid proofs: any 33 siblings give one)."""
    value = leaf
    for i in range(DEPOSIT_CONTRACT_TREE_DEPTH + 1):
        value = H(branch[i] + value) if index // (2**i) % 2 else H(value + branch[i])
    return value


def deposit_tree_proofs(leaves: List[bytes], first_index: int = 0):
    """A real deposit tree over `leaves` at indices first_index ..: (deposit_root, one 33-node proof per leaf).  The leaves
    before first_index are zero chunks.  Depth 32, then the length mix-in as node 32."""
    count = first_index + len(leaves)
    level = {first_index + i: leaf for i, leaf in enumerate(leaves)}
    proofs = [[] for _ in leaves]
    idx = [first_index + i for i in range(len(leaves))]
    for k in range(DEPOSIT_CONTRACT_TREE_DEPTH):
        for j in range(len(leaves)):
            proofs[j].append(level.get(idx[j] ^ 1, S.Z[k]))
        nxt = {}
        for p in {i >> 1 for i in level}:
            nxt[p] = H(level.get(2 * p, S.Z[k]) + level.get(2 * p + 1, S.Z[k]))
        level = nxt
        idx = [i >> 1 for i in idx]
    length = int(count).to_bytes(32, "little")
    for j in range(len(leaves)):
        proofs[j].append(length)
    return H(level[0] + length), proofs


def process_deposits(reg: S.Registry, deposits: List[DepositData], sig_ok: Sequence[bool], proofs: Optional[List[List[bytes]]] = None,
                     eth1_deposit_index: int = 0, deposit_root: bytes = b"", increment: int = EFFECTIVE_BALANCE_INCREMENT,
                     max_effective_balance: int = MAX_EFFECTIVE_BALANCE, far_future_epoch: int = FAR_FUTURE_EPOCH):
    """process_deposit for every deposit in order, on `reg` in place.  Returns (status, index credited or NONE).  A failing
    proof is the reference's assert: the function then returns the statuses with NOTHING applied (reg untouched), the failing
    deposits BAD_PROOF, every index NONE."""
    if proofs is not None:
        bad = [not is_valid_merkle_branch(deposit_data_root(d), proofs[i], DEPOSIT_CONTRACT_TREE_DEPTH + 1,
                                          eth1_deposit_index + i, deposit_root) for i, d in enumerate(deposits)]
    else:
        bad = [False] * len(deposits)
    work = reg
    if any(bad):
        import copy
        work = copy.deepcopy(reg)
    status, index = [], []
    for i, d in enumerate(deposits):
        pubkey, amount = d.pubkey, d.amount
        validator_pubkeys = work.pubkeys
        if pubkey not in validator_pubkeys:
            if sig_ok[i]:                                         # bls.Verify(pubkey, signing_root, deposit.data.signature)
                work.pubkeys.append(pubkey)                       # get_validator_from_deposit
                work.withdrawal_credentials.append(d.withdrawal_credentials)
                work.effective_balance.append(min(amount - amount % increment, max_effective_balance))
                work.slashed.append(0)
                work.activation_eligibility_epoch.append(far_future_epoch)
                work.activation_epoch.append(far_future_epoch)
                work.exit_epoch.append(far_future_epoch)
                work.withdrawable_epoch.append(far_future_epoch)
                work.balances.append(amount)
                work.previous_epoch_participation.append(0)
                work.current_epoch_participation.append(0)
                work.inactivity_scores.append(0)
                status.append(APPENDED)
                index.append(len(work.balances) - 1)
            else:
                status.append(IGNORED_BAD_SIGNATURE)
                index.append(NONE)
        else:
            v = validator_pubkeys.index(pubkey)
            work.balances[v] += amount                            # increase_balance
            status.append(TOPUP)
            index.append(v)
    if any(bad):
        return [BAD_PROOF if b else s for b, s in zip(bad, status)], [NONE] * len(deposits)
    return status, index


def index_slots(n_keys: int) -> int:
    """deposit_row.h, deposit_index_slots: the pubkey index's size for n_keys keys."""
    t = 64
    while t < 2 * n_keys:
        t *= 2
    return t


def index_slot(pubkey48: bytes, slots: int) -> int:
    """... and the slot a pubkey's probe sequence starts at."""
    return int.from_bytes(S.pubkey_leaf(pubkey48)[:4], "little") & (slots - 1)
