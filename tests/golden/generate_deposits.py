"""Regenerates tests/golden/deposit_vectors.json from tests/deposits_model.py: python -m tests.golden.generate_deposits"""
import json

from tests import deposits_model as M
from tests import ssz_model as S
from tests.test_deposits_model import random_case

SHAPES = [(1, 1), (5, 16), (63, 20), (64, 65), (65, 40), (100, 130)]


def main():
    cases = []
    for k, (n_reg, n) in enumerate(SHAPES):
        reg, deposits, sig_ok = random_case(100 + k, n_reg, n)
        status, index = M.process_deposits(reg, deposits, sig_ok)
        roots = S.state_roots(reg)
        cases.append(dict(seed=100 + k, n_reg=n_reg, n=n, status=status, index=index, n_after=len(reg),
                          validators_root=roots["validators"].hex(), balances_root=roots["balances"].hex(),
                          signing_root_0=M.signing_root(deposits[0], bytes(range(32))).hex(),
                          data_root_0=M.deposit_data_root(deposits[0]).hex()))
    comment = "tests/deposits_model.py over tests/test_deposits_model.py's random_case(seed, n_reg, n): recorded results"
    json.dump({"comment": comment, "cases": cases}, open(M.GOLDEN_PATH, "w"), indent=1)


if __name__ == "__main__":
    main()
