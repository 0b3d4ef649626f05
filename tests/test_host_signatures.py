"""Every ctypes signature in ntm_mpc._lib.EXPORTS against its prototype in include/ntm_mpc.h:
the result type, the argument count and each argument's kind.  A miscount in the table fails
no other test; it hands a kernel launch garbage.  No GPU and no built library needed.
"""
import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "ntm_mpc.h"

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double,
           "unsigned long long": C.c_ulonglong}


def prototypes():
    """name -> (result type, [argument types]) as C spells them, const dropped."""
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    txt = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", txt, flags=re.M)          # preprocessor lines, continued ones too
    txt = re.sub(r"\{[^{}]*\}", "", txt.replace('extern "C" {', ""))      # struct and enum bodies
    out = {}
    for stmt in txt.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(ntm_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m or m.group(1).split()[0] == "typedef":
            continue
        norm = lambda t: re.sub(r"\s*\*", "*", " ".join(w for w in t.split() if w != "const"))     # noqa: E731
        args = [] if m.group(3).strip() == "void" else [a.strip() for a in m.group(3).split(",")]
        # an argument is "type name": the name is the last identifier
        out[m.group(2)] = (norm(m.group(1)), [norm(re.sub(r"\w+$", "", a)) for a in args])
    return out


def matches(ctype, c):
    """The kind rules: a scalar its exact ctypes type; T* a POINTER to T's ctypes type or
    Structure; ntm_ctx** POINTER(c_void_p); a c_void_p entry accepts any pointer."""
    from ntm_mpc import _lib as L
    structs = {"ntm_physics": L.NtmPhysics, "ntm_config": L.NtmConfig, "ntm_scenario_gen": L.NtmScenarioGen,
               "ntm_observer": L.NtmObserver, "ntm_estimator": L.NtmEstimator, "ntm_delay": L.NtmDelay}
    if c == "void":
        return ctype is None
    if c == "char*":
        return ctype is C.c_char_p
    if c == "ntm_ctx**":
        return ctype is C.POINTER(C.c_void_p)
    if c.endswith("*"):
        base = c[:-1]
        if ctype is C.c_void_p:
            return "*" not in base
        target = SCALARS.get(base) or structs.get(base)
        return target is not None and ctype is C.POINTER(target)
    return ctype is SCALARS[c]


def test_exports_match_the_header_prototypes():
    from ntm_mpc._lib import EXPORTS
    protos = prototypes()
    assert len(EXPORTS) == 56 and set(protos) == set(EXPORTS)
    for name, (res, args) in EXPORTS.items():
        c_res, c_args = protos[name]
        assert matches(res, c_res), f"{name}: result {res} against {c_res}"
        assert len(args) == len(c_args), f"{name}: {len(args)} arguments against {len(c_args)} in the header"
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert matches(a, c), f"{name}: argument {i} {a} against {c}"


def test_the_check_sees_a_miscount_and_a_wrong_kind():
    """The checker itself: one pointer too many, and int32_t* where the header has double*."""
    from ntm_mpc._lib import _DP, _IP
    c_res, c_args = prototypes()["ntm_mpc_run_dly_from"]
    assert c_res == "int" and len(c_args) == 7 + 18
    assert c_args[7:11] == ["double*", "double*", "double*", "int32_t*"]
    assert matches(_DP, "double*") and not matches(_IP, "double*") and not matches(C.c_int32, "int64_t")
    assert matches(C.c_void_p, "double*") and not matches(C.c_void_p, "ntm_ctx**")
