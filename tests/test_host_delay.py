"""Host-side checks of the actuator dead time's additions (NTM_MPC_HAS_INPUT_DELAY, still
ABI v7) that need no GPU: the ctypes mirror of ntm_delay, the header's macros and the six
exported entry points.
"""
import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "ntm_mpc.h"
SYMBOLS = ("ntm_mpc_step_dly", "ntm_mpc_step_dly_device", "ntm_mpc_run_dly", "ntm_mpc_run_dly_device",
           "ntm_mpc_run_dly_from", "ntm_mpc_run_dly_from_device")


def test_delay_struct_layout_and_abi():
    """ctypes mirror of ntm_delay: two int32 (8 bytes); Delay.to_c; the ABI version stays 7
    and sizeof(ntm_estimator) stays 56."""
    import ntm_mpc
    from ntm_mpc._lib import ABI_VERSION, MAX_DELAY, NtmDelay, NtmEstimator
    assert C.sizeof(NtmDelay) == 8
    assert [getattr(NtmDelay, f).offset for f in ("steps", "predict")] == [0, 4]
    d = ntm_mpc.Delay(steps=3).to_c()
    assert (d.steps, d.predict) == (3, 1)
    d = ntm_mpc.Delay(steps=8, predict=False).to_c()
    assert (d.steps, d.predict) == (8, 0)
    assert ntm_mpc.Delay().steps == 0 and ntm_mpc.Delay().predict is True
    assert MAX_DELAY == 8 and ntm_mpc.MAX_DELAY == 8
    assert ABI_VERSION == 7 and ntm_mpc.load().ntm_abi_version() == 7
    assert C.sizeof(NtmEstimator) == 56


def test_header_defines_the_delay_macros_and_struct():
    text = HEADER.read_text()
    assert re.search(r"^#define\s+NTM_MPC_HAS_INPUT_DELAY\s+1\b", text, re.M)
    assert re.search(r"^#define\s+NTM_MAX_DELAY\s+8\b", text, re.M)
    assert re.search(r"^#define\s+NTM_MPC_ABI_VERSION\s+7\b", text, re.M)
    assert re.search(r"^#define\s+NTM_MPC_HAS_RUN_FROM\s+1\b", text, re.M)
    m = re.search(r"typedef struct \{([^}]*)\} ntm_delay;", text)
    assert m, "ntm_delay not declared"
    fields = re.findall(r"int32_t\s+(\w+);", m.group(1))
    assert fields == ["steps", "predict"]
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", text, re.M), name


def test_library_exports_the_six_entry_points():
    """The built library exports them, the binding lists them in an optional set of its
    own, and has_run_from() keeps its meaning."""
    import ntm_mpc
    from ntm_mpc import _lib as L
    lib = ntm_mpc.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTS and name in L.OPTIONAL_DELAY and name not in L.OPTIONAL
        assert getattr(lib, name).argtypes == L.EXPORTS[name][1]
    assert set(L.OPTIONAL_DELAY) == set(SYMBOLS)
    assert set(L.OPTIONAL) == {"ntm_mpc_run_from", "ntm_mpc_run_from_device", "ntm_mpc_run_est_from",
                               "ntm_mpc_run_est_from_device"}
    assert ntm_mpc.has_input_delay() and ntm_mpc.has_run_from()

    class Old:                                         # a library from before this feature
        pass
    old = Old()
    for name in L.OPTIONAL:
        setattr(old, name, object())
    assert L.has_run_from(old) and not L.has_input_delay(old)
