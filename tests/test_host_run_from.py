"""Host-side checks of the resumable closed loops that need no GPU: the entry points are
exported by the library, declared in the header and prototyped in the ctypes binding with
the header's argument counts, and they came without an ABI bump.
"""
import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "ntm_mpc.h"
NAMES = ("ntm_mpc_run_from", "ntm_mpc_run_from_device", "ntm_mpc_run_est_from", "ntm_mpc_run_est_from_device")


def test_run_from_symbols_are_exported_and_prototyped():
    import ntm_mpc
    from ntm_mpc import _lib as L
    lib = ntm_mpc.load()
    assert ntm_mpc.has_run_from()
    text = HEADER.read_text()
    assert re.search(r"#define\s+NTM_MPC_HAS_RUN_FROM\s+1\b", text)
    for name in NAMES:
        assert hasattr(lib, name), name
        res, args = L.EXPORTS[name]
        assert res is C.c_int
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in the header"
        assert len(args) == len(m.group(1).split(",")), name
        assert getattr(lib, name).argtypes == args
    # the device forms end with the stream, the state comes right after k_sim, active_ws is int32 on the host
    assert L.EXPORTS["ntm_mpc_run_from"][1][5:9] == [L._DP, L._DP, L._DP, L._IP]
    assert L.EXPORTS["ntm_mpc_run_est_from"][1][6:12] == [L._DP, L._DP, L._DP, L._IP, L._DP, L._DP]


def test_abi_version_is_still_7():
    import ntm_mpc
    from ntm_mpc._lib import ABI_VERSION
    assert ABI_VERSION == 7 and ntm_mpc.load().ntm_abi_version() == 7
    assert re.search(r"#define\s+NTM_MPC_ABI_VERSION\s+7\b", HEADER.read_text())


def test_null_context_is_refused_without_a_gpu():
    import ntm_mpc
    lib = ntm_mpc.load()
    assert lib.ntm_mpc_run_from(None, None, None, 1, 1, *([None] * 10)) == -1
    assert lib.ntm_mpc_run_est_from(None, None, None, None, 1, 1, *([None] * 15)) == -1
