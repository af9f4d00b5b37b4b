"""The sequential model of pe_slasher_ingest (include/posevo.h): the specification the engine's slasher is held to.

Pure Python, one row and one validator at a time.  Every comparison of two AttestationData goes through the
reference's ``is_slashable_attestation_data`` (oracle.spec, pe:1134-1143): the model decides nothing about what is
slashable, only which pairs meet.

State: per validator and target epoch of the window (W - H, W] the FIRST structurally valid AttestationData the
validator attested, in hand-over order; per epoch the list of distinct AttestationData recorded for it (at most D).
A piece of evidence is ``(validator, kind, d1_bytes, d2_bytes)`` with the 128 bytes of each AttestationData as
struct pe_attestation lays them out, so that the engine's evidence compares with it after its ids are resolved.

Two votes of one target epoch satisfy the function in both argument orders (its double-vote clause is symmetric); the
model states such a pair once, ``d1`` the recorded vote and ``d2`` the new one.  Votes of different target epochs can
satisfy only the surround clause, in one order: ``d1`` is then the surrounding vote.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from oracle import spec

DOUBLE, SURROUND = 1, 2
FUTURE_TARGET, TOO_OLD, TABLE_FULL = 32, 33, 34
NO_COMMITTEE_TABLE, COMMITTEE_INDEX_OUT_OF_RANGE, BITS_LENGTH_MISMATCH = 8, 9, 10


def data_of(row) -> spec.AttestationData:
    """One ATT_DTYPE row -> the reference's AttestationData (pe:689-697)."""
    return spec.AttestationData(
        slot=int(row["slot"]), index=int(row["index"]), beacon_block_root=spec.Root(row["beacon_block_root"].tobytes()),
        source=spec.Checkpoint(int(row["source_epoch"]), spec.Root(row["source_root"].tobytes())),
        target=spec.Checkpoint(int(row["target_epoch"]), spec.Root(row["target_root"].tobytes())))


def data_bytes(row) -> bytes:
    return row.tobytes()[:128]


class SlasherModel:
    def __init__(self, n_val: int, history: int, max_data: int, slots_per_epoch: int, only=None):
        """only: model just these validators (a sample of a large registry); statuses and tables are unaffected."""
        self.n_val, self.H, self.D, self.spe = n_val, history, max_data, slots_per_epoch
        self.only = None if only is None else np.asarray(sorted(only), dtype=np.int64)
        self.W = None
        self.committees = {}                      # epoch -> (offsets, members): a partition of the registry
        self.records = defaultdict(dict)           # validator -> {target epoch: (AttestationData, bytes)}
        self.tables = {}                          # epoch -> [bytes, ...] in order of first appearance

    def set_committees(self, epoch: int, offsets, members):
        self.committees[epoch] = (np.asarray(offsets), np.asarray(members))

    def in_window(self, epoch: int) -> bool:
        return self.W is not None and epoch <= self.W and epoch + self.H > self.W

    def ingest(self, atts, arena, current_epoch: int):
        """-> (status list, evidence list) or None when current_epoch decreased (nothing changes)."""
        if self.W is not None and current_epoch < self.W:
            return None
        self.W = current_epoch
        for e in [e for e in self.tables if not self.in_window(e)]:
            del self.tables[e]
        for rec in self.records.values():
            for e in [e for e in rec if not self.in_window(e)]:
                del rec[e]
        status, accepted = [], []
        for row in atts:
            e = int(row["target_epoch"])
            st, members = 0, None
            if e > self.W:
                st = FUTURE_TARGET
            elif e + self.H <= self.W:
                st = TOO_OLD
            elif e not in self.committees:
                st = NO_COMMITTEE_TABLE
            else:
                offsets, mem = self.committees[e]
                n_comm = len(offsets) - 1
                pos = (int(row["slot"]) % self.spe) * (n_comm // self.spe) + int(row["index"])
                if pos >= n_comm:
                    st = COMMITTEE_INDEX_OUT_OF_RANGE
                else:
                    members = mem[int(offsets[pos]):int(offsets[pos + 1])]
                    if int(row["n_bits"]) < len(members):
                        st = BITS_LENGTH_MISMATCH
            if st == 0:
                table = self.tables.setdefault(e, [])
                b = data_bytes(row)
                if b not in table:
                    if len(table) >= self.D:
                        st = TABLE_FULL
                    else:
                        table.append(b)
            status.append(st)
            if st == 0:
                off, nb = int(row["bits_offset"]), len(members)
                bits = np.unpackbits(arena[off:off + (nb + 7) // 8], bitorder="little")[:nb].astype(bool)
                voters = members[bits]
                if self.only is not None:
                    voters = voters[np.isin(voters, self.only)]
                accepted.append((data_of(row), data_bytes(row), [int(v) for v in voters]))
        evidence = []
        for alpha, alpha_b, voters in accepted:         # batch order; the validators of one row are independent
            e = alpha.target.epoch
            for v in voters:
                rec = self.records[v]
                if e in rec and rec[e][0] == alpha:
                    continue                            # the row was already processed
                for beta, beta_b in rec.values():
                    same_epoch = beta.target.epoch == e
                    for d1, b1, d2, b2 in ((beta, beta_b, alpha, alpha_b), (alpha, alpha_b, beta, beta_b)):
                        if spec.is_slashable_attestation_data(d1, d2):
                            if same_epoch and d1 is alpha:
                                continue                # the symmetric double vote, stated once as (recorded, new)
                            evidence.append((v, DOUBLE if same_epoch else SURROUND, b1, b2))
                if e not in rec:
                    rec[e] = (alpha, alpha_b)
        return status, evidence

    def records_of(self, epoch: int):
        """-> (source epoch, data bytes or None) per validator for one target epoch."""
        recs = (self.records.get(v, {}) for v in range(self.n_val))
        return [((rec[epoch][0].source.epoch, rec[epoch][1]) if epoch in rec else (None, None)) for rec in recs]

    def slashed(self, evidence) -> set:
        return {ev[0] for ev in evidence}
