#!/usr/bin/env python
"""Regenerates tests/golden/ssz_vectors.json from tests/ssz_model.py (hashlib only): a dozen small registries -- the
per-validator part of a BeaconState -- with their five list roots and the hash_tree_root of every Validator.  The file
holds data only; it regenerates byte for byte (tests/test_ssz_model.py).

    python tests/golden/generate_ssz.py          # rewrites ssz_vectors.json
"""
import json
import os
import sys
from dataclasses import asdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import ssz_model as M  # noqa: E402

OUT = M.GOLDEN_PATH
# (validators, limit_log2): the packing remainders of both widths (4 uint64, 32 uint8 to a chunk), the smallest limit the
# engine takes, the mainnet limit and the widest
CASES = [(0, 40), (1, 40), (1, 5), (3, 40), (4, 40), (5, 6), (31, 40), (32, 5), (33, 40), (33, 64), (64, 6), (65, 40)]


def to_json(reg: M.Registry) -> dict:
    d = asdict(reg)
    d["pubkeys"] = [b.hex() for b in reg.pubkeys]
    d["withdrawal_credentials"] = [b.hex() for b in reg.withdrawal_credentials]
    return d


def from_json(d: dict) -> M.Registry:
    d = dict(d)
    d["pubkeys"] = [bytes.fromhex(x) for x in d["pubkeys"]]
    d["withdrawal_credentials"] = [bytes.fromhex(x) for x in d["withdrawal_credentials"]]
    return M.Registry(**d)


def cases():
    out = []
    for i, (n, limit_log2) in enumerate(CASES):
        reg = M.random_registry(n, 354 + i)
        out.append({"name": f"n{n}_limit{limit_log2}", "limit_log2": limit_log2, "registry": to_json(reg),
                    "validator_leaves": [x.hex() for x in reg.validator_leaves()],
                    "roots": {k: v.hex() for k, v in M.state_roots(reg, limit_log2).items()}})
    return out


def render() -> str:
    """One JSON object per line, so that a diff shows the case that changed."""
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=True) for c in cases()) + "\n]\n"


if __name__ == "__main__":
    open(OUT, "w").write(render())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
