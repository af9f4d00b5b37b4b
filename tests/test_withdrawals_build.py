"""CPU: the build side of pe_process_withdrawals / pe_process_bls_to_execution_changes -- no kernel of withdrawal_kernels.hip
uses scratch memory (a resource log of its own), the ABI version stays 15 (additions only), the header's structs, constants
and entry points are _abi's, and pe_withdrawal is 44 bytes.  The log and library checks are skipped where the library is not
built; a built library without the log fails."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
LOG = os.path.join(CSRC, "withdrawal_kernels.resource.log")
KERNELS = ("k_withdrawals_flag", "k_withdrawals_scan", "k_withdrawals_select", "k_withdrawals_apply", "k_bls_changes_claim",
           "k_bls_changes_resolve", "k_bls_changes_apply", "k_bls_change_signing_roots")

built = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "pos_evolution_amd", "libposevo.so")),
                           reason="libposevo.so is not built")


@built
def test_no_kernel_uses_scratch():
    assert os.path.exists(LOG), "the build of withdrawal_kernels.o left no resource log"
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
    for name in ("pe_process_withdrawals", "pe_withdrawals_params_default", "pe_process_bls_to_execution_changes",
                 "pe_bls_change_signing_roots"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name
    # the structs field for field, the constants value for value
    for struct in (_abi.pe_withdrawal, _abi.pe_withdrawals_params, _abi.pe_withdrawals_result, _abi.pe_bls_change,
                   _abi.pe_bls_changes_stats):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), text, flags=re.S).group(1)
        fields = re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)
        assert fields == [name for name, _ in struct._fields_], struct.__name__
    assert C.sizeof(_abi.pe_withdrawal) == 44 and C.sizeof(_abi.pe_bls_change) == 80
    assert re.search(r"#pragma pack\(push, 1\)\s*typedef struct pe_withdrawal \{", text)
    assert (_abi.pe_withdrawal.validator_index.offset, _abi.pe_withdrawal.address.offset, _abi.pe_withdrawal.amount.offset) == (8, 16, 36)
    found = 0
    for name, value in re.findall(r"(PE_(?:WD|CRED)_[A-Z_]+)\s*=?\s*(0x[0-9a-f]+|\d+)u?\b", text):
        assert getattr(_abi, name) == int(value, 0), name
        found += 1
    assert found == 6 + 5 + 3
    assert {int(v) for _, v in re.findall(r"(PE_WD_[A-Z_]+) = (\d+)", text)} == set(_abi.WD_STATUS_NAMES) == {0, 80, 81, 82, 83, 84}
    assert {int(v) for _, v in re.findall(r"(PE_CRED_[A-Z_]+) = (\d+)", text)} == set(_abi.CRED_STATUS_NAMES) == {0, 96, 97, 98, 99}
    # the block operations' prefix keeps its own codes
    assert not [n for n in re.findall(r"(PE_OP_[A-Z_]+) = (\d+)", text) if int(n[1]) >= 80]


def test_the_numpy_rows_are_the_structs():
    from pos_evolution_amd import _abi, engine
    for dtype, struct in ((engine.WITHDRAWAL_DTYPE, _abi.pe_withdrawal), (engine.BLS_CHANGE_DTYPE, _abi.pe_bls_change)):
        assert dtype.itemsize == C.sizeof(struct)
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name


@built
def test_the_library_exports_the_calls():
    from pos_evolution_amd import _abi
    lib = _abi.load()
    assert lib.pe_abi_version() == 15
    p = _abi.pe_withdrawals_params()
    lib.pe_withdrawals_params_default(p)
    assert [getattr(p, name) for name, _ in _abi.pe_withdrawals_params._fields_] == [32 * 10**9, 16, 16384, 1]
    lib.pe_strerror.restype = C.c_char_p
    for code in _abi.WD_STATUS_NAMES:
        assert code == 0 or lib.pe_strerror(code).decode().startswith("withdrawals:"), code
    for code in _abi.CRED_STATUS_NAMES:
        assert code == 0 or lib.pe_strerror(code).decode().startswith("address change:"), code
