"""CPU: the build side of the sync committee calls -- the library exports them, and no kernel of sync_kernels.hip uses
scratch memory (a resource log of its own).  Skipped where the library is not built; a built library without the log fails."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
LOG = os.path.join(CSRC, "sync_kernels.resource.log")

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "pos_evolution_amd", "libposevo.so")),
                                reason="libposevo.so is not built")


def test_no_kernel_uses_scratch():
    assert os.path.exists(LOG), "the build of sync_kernels.o left no resource log"
    log = open(LOG).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) == 4
    for want in ("k_sync_sample", "k_sync_append", "k_sync_members", "k_sync_rewards"):
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))


def test_the_library_exports_the_calls():
    from pos_evolution_amd import _abi
    lib = _abi.load()
    for name in ("pe_sync_committee_compute", "pe_sync_committee_set", "pe_sync_committee_get", "pe_sync_committee_rotate",
                 "pe_sync_params_default", "pe_process_sync_aggregate"):
        assert hasattr(lib, name), name
    assert lib.pe_abi_version() == 15
    p = _abi.pe_sync_params()
    lib.pe_sync_params_default(p)
    assert (p.total_active_balance, p.base_reward_factor) == (0, 64)
