"""The specification of pe_process_withdrawals, pe_process_bls_to_execution_changes and pe_bls_change_signing_roots
(pos_evolution_amd/csrc/engine_withdrawals.cpp, withdrawal_kernels.hip, withdrawals_row.h): Capella's functions as the consensus
specification writes them -- the reference holds the Validator fields (pe:36-45) and `balances` (pe:112), not these functions'
text, so each is quoted in the docstring of its restatement -- as SEQUENTIAL loops over plain Python integers, and beside them
the CLOSED FORM the kernels compute (independent predicates per sweep position, the first k hits in position order, the first
potent change per validator).  tests/test_withdrawals_model.py holds the two forms to each other.

A registry here is a dict of numpy arrays: cred uint8[n, 32], wdr / eff / bal uint64[n].  A withdrawal is the tuple (index,
validator_index, address: 20 bytes, amount); a change the tuple (validator_index, from_bls_pubkey: 48 bytes,
to_execution_address: 20 bytes, signature_valid)."""
import hashlib
import json
import os
from dataclasses import asdict, dataclass

import numpy as np

from tests import ssz_model as SSZ

FAR = 2**64 - 1
U64 = 2**64
ETH = 10**9
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "withdrawals_vectors.json")
BLS_PREFIX, ETH1_PREFIX = 0x00, 0x01
MAX_PER_PAYLOAD_LIMIT = 64
# pe_wd_status / pe_cred_status (include/posevo.h)
WD_OK, WD_COUNT, WD_INDEX, WD_VALIDATOR, WD_ADDRESS, WD_AMOUNT = 0, 80, 81, 82, 83, 84
CRED_OK, CRED_BAD_INDEX, CRED_NOT_BLS, CRED_PUBKEY_MISMATCH, CRED_BAD_SIGNATURE = 0, 96, 97, 98, 99
RESULT = ("next_withdrawal_index", "next_withdrawal_validator_index", "n_full", "n_partial", "total_gwei", "n_withdrawals",
          "status", "first_mismatch", "applied")
FIELDS = ("cred", "wdr", "eff", "bal")


@dataclass
class Params:
    """pe_withdrawals_params, mainnet values (minimal preset: 4 withdrawals, a sweep of 16)."""
    max_effective_balance: int = 32 * ETH
    max_withdrawals_per_payload: int = 16
    max_validators_per_sweep: int = 16384
    eth1_prefix: int = ETH1_PREFIX

    def abi(self) -> dict:
        return asdict(self)


def copy_registry(a: dict) -> dict:
    return {k: np.array(a[k], dtype=np.uint8 if k == "cred" else np.uint64) for k in FIELDS}


# ------------------------------------------------------------------ the predicates
def has_eth1_withdrawal_credential(cred: bytes, p: Params = Params()) -> bool:
    """def has_eth1_withdrawal_credential(validator: Validator) -> bool:
        return validator.withdrawal_credentials[:1] == ETH1_ADDRESS_WITHDRAWAL_PREFIX"""
    return cred[0] == p.eth1_prefix


def is_fully_withdrawable_validator(cred: bytes, withdrawable_epoch: int, balance: int, epoch: int, p: Params = Params()) -> bool:
    """def is_fully_withdrawable_validator(validator: Validator, balance: Gwei, epoch: Epoch) -> bool:
        return (
            has_eth1_withdrawal_credential(validator)
            and validator.withdrawable_epoch <= epoch
            and balance > 0
        )"""
    return has_eth1_withdrawal_credential(cred, p) and withdrawable_epoch <= epoch and balance > 0


def is_partially_withdrawable_validator(cred: bytes, effective_balance: int, balance: int, p: Params = Params()) -> bool:
    """def is_partially_withdrawable_validator(validator: Validator, balance: Gwei) -> bool:
        has_max_effective_balance = validator.effective_balance == MAX_EFFECTIVE_BALANCE
        has_excess_balance = balance > MAX_EFFECTIVE_BALANCE
        return has_eth1_withdrawal_credential(validator) and has_max_effective_balance and has_excess_balance"""
    return (has_eth1_withdrawal_credential(cred, p) and effective_balance == p.max_effective_balance
            and balance > p.max_effective_balance)


def check_params(n: int, start: int, next_index: int, p: Params, n_payload=None):
    """Every refusal of pe_process_withdrawals that reads no resident array (PE_ERR_INVALID_ARG)."""
    if n == 0:
        raise ValueError("the registry is empty")
    if start >= n:
        raise ValueError("next_withdrawal_validator_index lies outside the registry")
    if 0 in (p.max_effective_balance, p.max_withdrawals_per_payload, p.max_validators_per_sweep, p.eth1_prefix):
        raise ValueError("a parameter is 0")
    if p.eth1_prefix > 0xFF:
        raise ValueError("eth1_prefix is not one byte")
    if p.max_withdrawals_per_payload > MAX_PER_PAYLOAD_LIMIT:
        raise ValueError("max_withdrawals_per_payload above 64")
    if n_payload is not None and n_payload > p.max_withdrawals_per_payload:
        raise ValueError("the payload holds more than max_withdrawals_per_payload withdrawals")
    if next_index + p.max_withdrawals_per_payload >= U64:
        raise ValueError("next_withdrawal_index + max_withdrawals_per_payload exceeds 64 bits")


# ------------------------------------------------------------------ the sequential loops
def get_expected_withdrawals(a: dict, epoch: int, next_index: int, start: int, p: Params = Params()):
    """def get_expected_withdrawals(state: BeaconState) -> Sequence[Withdrawal]:
        epoch = get_current_epoch(state)
        withdrawal_index = state.next_withdrawal_index
        validator_index = state.next_withdrawal_validator_index
        withdrawals: List[Withdrawal] = []
        bound = min(len(state.validators), MAX_VALIDATORS_PER_WITHDRAWALS_SWEEP)
        for _ in range(bound):
            validator = state.validators[validator_index]
            balance = state.balances[validator_index]
            if is_fully_withdrawable_validator(validator, balance, epoch):
                withdrawals.append(Withdrawal(
                    index=withdrawal_index,
                    validator_index=validator_index,
                    address=ExecutionAddress(validator.withdrawal_credentials[12:]),
                    amount=balance,
                ))
                withdrawal_index += WithdrawalIndex(1)
            elif is_partially_withdrawable_validator(validator, balance):
                withdrawals.append(Withdrawal(
                    index=withdrawal_index,
                    validator_index=validator_index,
                    address=ExecutionAddress(validator.withdrawal_credentials[12:]),
                    amount=balance - MAX_EFFECTIVE_BALANCE,
                ))
                withdrawal_index += WithdrawalIndex(1)
            if len(withdrawals) == MAX_WITHDRAWALS_PER_PAYLOAD:
                break
            validator_index = ValidatorIndex((validator_index + 1) % len(state.validators))
        return withdrawals

    -> (withdrawals, their kinds: 1 full, 2 partial)"""
    n = len(a["bal"])
    withdrawal_index, validator_index = next_index, start
    withdrawals, kinds = [], []
    bound = min(n, p.max_validators_per_sweep)
    for _ in range(bound):
        cred = bytes(a["cred"][validator_index])
        balance = int(a["bal"][validator_index])
        if is_fully_withdrawable_validator(cred, int(a["wdr"][validator_index]), balance, epoch, p):
            withdrawals.append((withdrawal_index, validator_index, cred[12:], balance))
            kinds.append(1)
            withdrawal_index += 1
        elif is_partially_withdrawable_validator(cred, int(a["eff"][validator_index]), balance, p):
            withdrawals.append((withdrawal_index, validator_index, cred[12:], balance - p.max_effective_balance))
            kinds.append(2)
            withdrawal_index += 1
        if len(withdrawals) == p.max_withdrawals_per_payload:
            break
        validator_index = (validator_index + 1) % n
    return withdrawals, kinds


def compare_payload(expected, payload):
    """process_withdrawals' asserts over the payload in their order -> (status, first differing entry)."""
    if len(payload) != len(expected):
        return WD_COUNT, min(len(payload), len(expected))
    for i, (e, w) in enumerate(zip(expected, payload)):
        for field, status in ((0, WD_INDEX), (1, WD_VALIDATOR), (2, WD_ADDRESS), (3, WD_AMOUNT)):
            if (bytes(e[field]) if field == 2 else int(e[field])) != (bytes(w[field]) if field == 2 else int(w[field])):
                return status, i
    return WD_OK, 0


def _result(a, expected, kinds, next_index, start, p, payload, apply):
    n = len(a["bal"])
    status, first = (WD_OK, 0) if payload is None else compare_payload(expected, payload)
    new_index = expected[-1][0] + 1 if expected else next_index
    if len(expected) == p.max_withdrawals_per_payload:
        new_validator = (expected[-1][1] + 1) % n
    else:
        new_validator = (start + p.max_validators_per_sweep) % n
    applied = int(bool(apply) and status == WD_OK)
    return dict(next_withdrawal_index=new_index, next_withdrawal_validator_index=new_validator, n_full=kinds.count(1),
                n_partial=kinds.count(2), total_gwei=min(sum(w[3] for w in expected), FAR), n_withdrawals=len(expected),
                status=status, first_mismatch=first, applied=applied,
                withdrawals_root=withdrawals_list_root(expected, p.max_withdrawals_per_payload))


def process_withdrawals_sequential(a: dict, epoch: int, next_index: int, start: int, p: Params = Params(), payload=None,
                                   apply: bool = False):
    """def process_withdrawals(state: BeaconState, payload: ExecutionPayload) -> None:
        expected_withdrawals = get_expected_withdrawals(state)
        assert len(payload.withdrawals) == len(expected_withdrawals)

        for expected_withdrawal, withdrawal in zip(expected_withdrawals, payload.withdrawals):
            assert withdrawal == expected_withdrawal
            decrease_balance(state, withdrawal.validator_index, withdrawal.amount)

        # Update the next withdrawal index if this block contained withdrawals
        if len(expected_withdrawals) != 0:
            latest_withdrawal = expected_withdrawals[-1]
            state.next_withdrawal_index = WithdrawalIndex(latest_withdrawal.index + 1)

        # Update the next validator index to start the next withdrawal sweep
        if len(expected_withdrawals) == MAX_WITHDRAWALS_PER_PAYLOAD:
            # Next sweep starts after the latest withdrawal's validator index
            next_validator_index = ValidatorIndex((expected_withdrawals[-1].validator_index + 1) % len(state.validators))
            state.next_withdrawal_validator_index = next_validator_index
        else:
            # Advance sweep by the max length of the sweep if there was not a full set of withdrawals
            next_index = state.next_withdrawal_validator_index + MAX_VALIDATORS_PER_WITHDRAWALS_SWEEP
            next_validator_index = ValidatorIndex(next_index % len(state.validators))
            state.next_withdrawal_validator_index = next_validator_index

    -> (the registry after the call, the expected withdrawals, pe_withdrawals_result as a dict).  payload None: compute only.
    A failing assert is a status: the registry is returned unchanged.  apply needs a payload (the engine's refusal)."""
    check_params(len(a["bal"]), start, next_index, p, None if payload is None else len(payload))
    if apply and payload is None:
        raise ValueError("apply without a payload")
    expected, kinds = get_expected_withdrawals(a, epoch, next_index, start, p)
    res = _result(a, expected, kinds, next_index, start, p, payload, apply)
    b = copy_registry(a)
    if res["applied"]:
        for _, v, _, amount in expected:
            b["bal"][v] = max(0, int(b["bal"][v]) - amount)  # decrease_balance
    return b, expected, res


def process_withdrawals_closed(a: dict, epoch: int, next_index: int, start: int, p: Params = Params(), payload=None,
                               apply: bool = False):
    """The form the kernels compute: bound <= n, so every position reads the registry as it was before the call; the hits are the
    positions whose predicate holds, the withdrawals the first k of them in position order, rank = the count of hits before."""
    n = len(a["bal"])
    check_params(n, start, next_index, p, None if payload is None else len(payload))
    if apply and payload is None:
        raise ValueError("apply without a payload")
    bound = min(n, p.max_validators_per_sweep)
    v = (np.uint64(start) + np.arange(bound, dtype=np.uint64)) % np.uint64(n)
    v = v.astype(np.int64)
    prefix = a["cred"][v, 0] == p.eth1_prefix
    bal, maxeb = a["bal"][v], np.uint64(p.max_effective_balance)
    full = prefix & (a["wdr"][v] <= np.uint64(epoch)) & (bal > 0)
    partial = ~full & prefix & (a["eff"][v] == maxeb) & (bal > maxeb)
    kind = full.astype(np.uint8) + 2 * partial.astype(np.uint8)
    hit = kind != 0
    rank = np.cumsum(hit) - hit  # exclusive
    take = np.flatnonzero(hit & (rank < p.max_withdrawals_per_payload))
    expected = [(next_index + int(rank[j]), int(v[j]), bytes(a["cred"][v[j], 12:]),
                 int(bal[j]) - (0 if kind[j] == 1 else p.max_effective_balance)) for j in take]
    kinds = [int(kind[j]) for j in take]
    res = _result(a, expected, kinds, next_index, start, p, payload, apply)
    b = copy_registry(a)
    if res["applied"] and expected:
        idx = np.array([w[1] for w in expected], dtype=np.int64)
        b["bal"][idx] -= np.array([w[3] for w in expected], dtype=np.uint64)  # one writer per balance
    return b, expected, res


# ------------------------------------------------------------------ address changes
def bls_credentials(pubkey48: bytes) -> bytes:
    """BLS_WITHDRAWAL_PREFIX + hash(pubkey)[1:]"""
    return bytes([BLS_PREFIX]) + hashlib.sha256(bytes(pubkey48)).digest()[1:]


def process_bls_changes_sequential(cred: np.ndarray, changes):
    """def process_bls_to_execution_change(state: BeaconState, signed_address_change: SignedBLSToExecutionChange) -> None:
        address_change = signed_address_change.message

        assert address_change.validator_index < len(state.validators)

        validator = state.validators[address_change.validator_index]

        assert validator.withdrawal_credentials[:1] == BLS_WITHDRAWAL_PREFIX
        assert validator.withdrawal_credentials[1:] == hash(address_change.from_bls_pubkey)[1:]

        # Fork-agnostic domain since address changes are valid across forks
        domain = compute_domain(DOMAIN_BLS_TO_EXECUTION_CHANGE, genesis_validators_root=state.genesis_validators_root)
        signing_root = compute_signing_root(address_change, domain)
        assert bls.Verify(address_change.from_bls_pubkey, signing_root, signed_address_change.signature)

        validator.withdrawal_credentials = (
            ETH1_ADDRESS_WITHDRAWAL_PREFIX
            + b'\\x00' * 11
            + address_change.to_execution_address
        )

    for every change in order, bls.Verify being the injected verdict.  -> (credentials after the call, statuses, stats).  A
    failing assert is the change's status; it leaves nothing, the loop goes on over what the valid changes left, and a block
    with any invalid change returns the credentials unchanged."""
    work = np.array(cred, dtype=np.uint8)
    status = []
    for index, pubkey, address, valid in changes:
        if not index < len(work):
            status.append(CRED_BAD_INDEX)
            continue
        c = bytes(work[index])
        if c[:1] != bytes([BLS_PREFIX]):
            status.append(CRED_NOT_BLS)
        elif c[1:] != hashlib.sha256(bytes(pubkey)).digest()[1:]:
            status.append(CRED_PUBKEY_MISMATCH)
        elif not valid:
            status.append(CRED_BAD_SIGNATURE)
        else:
            work[index] = np.frombuffer(bytes([ETH1_PREFIX]) + bytes(11) + bytes(address), dtype=np.uint8)
            status.append(CRED_OK)
    n_invalid = sum(s != CRED_OK for s in status)
    stats = dict(n_applied=0 if n_invalid else len(status), n_invalid=n_invalid)
    return (np.array(cred, dtype=np.uint8) if n_invalid else work), status, stats


def process_bls_changes_closed(cred: np.ndarray, changes):
    """The form the kernels compute: a change is POTENT if every assert holds on the credentials before the call; first[v] =
    the least position of a potent change naming v; a change behind first[v] fails the prefix check."""
    cred = np.array(cred, dtype=np.uint8)
    n = len(cred)
    checks = []
    for index, pubkey, _, valid in changes:
        ok_index = index < n
        c = bytes(cred[index]) if ok_index else bytes(32)
        checks.append((ok_index, ok_index and c[0] == BLS_PREFIX, ok_index and c[1:] == hashlib.sha256(bytes(pubkey)).digest()[1:],
                       bool(valid)))
    first = {}
    for pos, (change, ok) in enumerate(zip(changes, checks)):
        if all(ok):
            first[change[0]] = min(first.get(change[0], pos), pos)
    status = []
    for pos, (change, (ok_index, ok_prefix, ok_hash, ok_sig)) in enumerate(zip(changes, checks)):
        if not ok_index:
            status.append(CRED_BAD_INDEX)
        elif not ok_prefix or first.get(change[0], pos) < pos:
            status.append(CRED_NOT_BLS)
        elif not ok_hash:
            status.append(CRED_PUBKEY_MISMATCH)
        elif not ok_sig:
            status.append(CRED_BAD_SIGNATURE)
        else:
            status.append(CRED_OK)
    n_invalid = sum(s != CRED_OK for s in status)
    out = cred.copy()
    if not n_invalid:
        for index, _, address, _ in changes:
            out[index] = np.frombuffer(bytes([ETH1_PREFIX]) + bytes(11) + bytes(address), dtype=np.uint8)
    return out, status, dict(n_applied=0 if n_invalid else len(status), n_invalid=n_invalid)


# ------------------------------------------------------------------ SSZ roots (tests/ssz_model.py's rules)
def withdrawal_root(w) -> bytes:
    """hash_tree_root(Withdrawal): index, validator_index, address (Bytes20: one chunk), amount."""
    index, validator, address, amount = w
    return SSZ.merkleize([SSZ.u64_chunk(index), SSZ.u64_chunk(validator), bytes(address) + bytes(12), SSZ.u64_chunk(amount)], 2)


def withdrawals_list_root(withdrawals, limit: int) -> bytes:
    """hash_tree_root(List[Withdrawal, limit])"""
    depth = (limit - 1).bit_length()
    return SSZ.mix_in_length(SSZ.merkleize([withdrawal_root(w) for w in withdrawals], depth), len(withdrawals))


def bls_change_root(change) -> bytes:
    """hash_tree_root(BLSToExecutionChange): validator_index, from_bls_pubkey (Bytes48: two chunks), to_execution_address."""
    index, pubkey, address = change[0], change[1], change[2]
    return SSZ.merkleize([SSZ.u64_chunk(index), SSZ.pubkey_leaf(bytes(pubkey)), bytes(address) + bytes(12)], 2)


def bls_change_signing_root(change, domain: bytes) -> bytes:
    """compute_signing_root: hash_tree_root(SigningData(object_root, domain))"""
    assert len(domain) == 32
    return SSZ.H(bls_change_root(change) + bytes(domain))


# ------------------------------------------------------------------ registries
def address_of(v: int) -> bytes:
    return hashlib.sha256(b"address" + int(v).to_bytes(8, "little")).digest()[:20]


def pubkey_of(v: int) -> bytes:
    return hashlib.sha256(b"key" + int(v).to_bytes(8, "little")).digest() + hashlib.sha256(b"key2" + int(v).to_bytes(8, "little")).digest()[:16]


def eth1_credentials(v: int, prefix: int = ETH1_PREFIX) -> bytes:
    """prefix || eleven bytes that are NOT zero (nothing may read them) || the address"""
    return bytes([prefix]) + bytes([0xA0 + k for k in range(11)]) + address_of(v)


def blank_registry(n: int, p: Params = Params()) -> dict:
    """n validators the sweep passes over: BLS credentials of pubkey_of(v), not withdrawable, balance = effective = the maximum."""
    cred = np.array([np.frombuffer(bls_credentials(pubkey_of(v)), dtype=np.uint8) for v in range(n)], dtype=np.uint8).reshape(n, 32)
    u = lambda x: np.full(n, x, dtype=np.uint64)  # noqa: E731
    return dict(cred=cred, wdr=u(FAR), eff=u(p.max_effective_balance), bal=u(p.max_effective_balance))


def set_hits(a: dict, validators, p: Params = Params(), kind="mixed"):
    """make the given validators withdrawable: even ones partially (an excess of 1 + v Gwei), odd ones fully"""
    for v in validators:
        a["cred"][v] = np.frombuffer(eth1_credentials(v, p.eth1_prefix), dtype=np.uint8)
        if kind == "partial" or (kind == "mixed" and v % 2 == 0):
            a["bal"][v] = p.max_effective_balance + 1 + v
        else:
            a["wdr"][v] = 0
            a["bal"][v] = 7 + v
    return a


def random_registry(n: int, seed: int, epoch: int, p: Params = Params(), density: float = 0.1) -> dict:
    """every class of validator at random: the three prefixes, withdrawable epochs around `epoch`, balances around 0 and the
    maximum, effective balances at and one increment below the maximum; `density` scales how many have the eth1 prefix"""
    rng = np.random.default_rng(seed)
    a = blank_registry(n, p)
    prefix = rng.choice([0, p.eth1_prefix, 2], size=n, p=[(1 - density) * 0.8, density, (1 - density) * 0.2])
    for v in range(n):
        if prefix[v] != 0:
            a["cred"][v] = np.frombuffer(eth1_credentials(v, int(prefix[v])), dtype=np.uint8)
    a["wdr"] = rng.choice(np.array([max(epoch, 1) - 1, epoch, epoch + 1, FAR], dtype=np.uint64), size=n)
    a["eff"] = rng.choice(np.array([p.max_effective_balance, p.max_effective_balance - ETH], dtype=np.uint64), size=n, p=[0.8, 0.2])
    m = p.max_effective_balance
    a["bal"] = rng.choice(np.array([0, 1, m - 1, m, m + 1, m + 3 * ETH, 2**63 + 5], dtype=np.uint64), size=n)
    return a


# seeds of the random states, fixed so that the model alone yields 0, fewer than k and exactly k withdrawals
# (tests/test_withdrawals_model.py checks that): (n, seed, density, start)
RANDOM_CASES = ((300, 1, 0.0, 7), (300, 2, 0.02, 299), (300, 3, 0.5, 150), (65, 4, 0.1, 64), (600, 5, 0.2, 0), (1, 6, 1.0, 0))


def change_for(v: int, valid: bool = True, pubkey=None, address=None):
    return (v, pubkey_of(v) if pubkey is None else pubkey, address_of(v) if address is None else address, valid)


# ------------------------------------------------------------------ recorded vectors
def golden_cases():
    """small cases whose outputs tests/golden/withdrawals_vectors.json records"""
    p = Params(max_withdrawals_per_payload=4, max_validators_per_sweep=16)
    out = []
    for n, hits, start, epoch in ((5, [0, 4], 4, 10), (20, [1, 3, 5, 17, 18, 19], 17, 3), (16, [], 2, 0)):
        a = set_hits(blank_registry(n, p), hits, p)
        _, expected, res = process_withdrawals_sequential(a, epoch, 1000, start, p)
        out.append(dict(n=n, hits=hits, start=start, epoch=epoch,
                        withdrawals=[[w[0], w[1], w[2].hex(), w[3]] for w in expected],
                        result={k: res[k] for k in RESULT}, root=res["withdrawals_root"].hex(),
                        entry_roots=[withdrawal_root(w).hex() for w in expected]))
    domain = bytes(range(32))
    changes = [change_for(v) for v in (0, 7, 2**40 + 3)]
    return dict(params=p.abi(), withdrawals=out, domain=domain.hex(),
                changes=[[c[0], c[1].hex(), c[2].hex()] for c in changes],
                signing_roots=[bls_change_signing_root(c, domain).hex() for c in changes],
                credentials=[bls_credentials(c[1]).hex() for c in changes])


if __name__ == "__main__":  # python -m tests.withdrawals_model: rewrite the recorded vectors
    with open(GOLDEN_PATH, "w") as f:
        json.dump(golden_cases(), f, indent=1)
        f.write("\n")
