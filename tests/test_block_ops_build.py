"""CPU: the build side of pe_process_block_operations -- no kernel of block_ops_kernels.hip uses scratch memory (a resource
log of its own), the ABI version stays 15 (additions only), and the header's entry points are _abi.SIGNATURES'.  The log and
library checks are skipped where the library is not built; a built library without the log fails."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
LOG = os.path.join(CSRC, "block_ops_kernels.resource.log")
KERNELS = ("k_block_ops_lists", "k_block_ops_claim", "k_block_ops_resolve", "k_block_ops_scan", "k_block_ops_apply")

built = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "pos_evolution_amd", "libposevo.so")),
                           reason="libposevo.so is not built")


@built
def test_no_kernel_uses_scratch():
    assert os.path.exists(LOG), "the build of block_ops_kernels.o left no resource log"
    log = open(LOG).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) == len(KERNELS)
    for want in KERNELS:
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "posevo.h")).read(), flags=re.S)


def test_the_abi_version_stays_15_and_the_header_is_the_binding():
    from pos_evolution_amd import _abi
    text = header_text()
    assert int(re.search(r"#define\s+PE_ABI_VERSION\s+(\d+)", text).group(1)) == 15
    symbols = set(re.findall(r"\b(pe_[a-z0-9_]+)\s*\(", text))
    profile = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "posevo_profile.h")).read(), flags=re.S)
    symbols |= set(re.findall(r"\b(pe_[a-z0-9_]+)\s*\(", profile))
    assert sorted(symbols) == sorted(_abi.SIGNATURES)
    for name in ("pe_process_block_operations", "pe_block_ops_params_default"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name
    # the structs field for field, the constants value for value
    for struct in (_abi.pe_block_op, _abi.pe_block_ops_params, _abi.pe_block_ops_stats):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), text, flags=re.S).group(1)
        fields = re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)
        assert fields == [name for name, _ in struct._fields_], struct.__name__
    assert C.sizeof(_abi.pe_block_op) == 408
    for name, value in re.findall(r"(PE_OP_[A-Z_]+)\s*=?\s*(0x[0-9a-f]+|\d+)u?\b", text):
        if hasattr(_abi, name):
            assert getattr(_abi, name) == int(value, 0), name
    codes = {int(v) for _, v in re.findall(r"(PE_OP_[A-Z_]+) = (\d+)", text)}
    assert codes == set(_abi.OP_STATUS_NAMES)


@built
def test_the_library_exports_the_calls():
    from pos_evolution_amd import _abi
    lib = _abi.load()
    assert lib.pe_abi_version() == 15
    p = _abi.pe_block_ops_params()
    lib.pe_block_ops_params_default(p)
    assert [getattr(p, name) for name, _ in _abi.pe_block_ops_params._fields_] == [32, 512, 8192, 256, 256, 4, 4, 65536]
    r = _abi.pe_registry_params()
    lib.pe_registry_params_default(r)
    for name in ("min_validator_withdrawability_delay", "max_seed_lookahead", "min_per_epoch_churn_limit", "churn_limit_quotient"):
        assert getattr(p, name) == getattr(r, name), name
    lib.pe_strerror.restype = C.c_char_p
    for code, text in _abi.OP_STATUS_NAMES.items():
        assert code == 0 or lib.pe_strerror(code).decode().startswith("block operation"), code
