"""The assigned replay's entry points at the ABI boundary.  CPU only: nothing here needs a device."""
import ctypes as C
import os
import re

import fognetsimpp_amd._abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fognet_replay_assigned_dev", "fognet_run_assigned_dev")


def header():
    return open(os.path.join(ROOT, "include", "fognet_hip.h")).read()


def test_library_exports_both_symbols():
    lib = abi.load()
    for n in NAMES:
        assert hasattr(lib, n), n


def test_mirror_and_header_agree():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, n
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == ["fognet_ctx *ctx", "const fognet_batch_in *in", "const int32_t *assign",
                          "fognet_batch_out *out", "void *hip_stream"], params
        res, args = abi.SIGNATURES[n]
        assert res is C.c_int
        assert args == [C.c_void_p, C.POINTER(abi.BatchIn), C.c_void_p, C.POINTER(abi.BatchOut), C.c_void_p]
    defs = dict(re.findall(r"^#define\s+(FOGNET_ASSIGNED_\w+)\s+(\d+)\s*$", header(), re.M))
    assert int(defs["FOGNET_ASSIGNED_TILE"]) == abi.ASSIGNED_TILE == 64
    assert int(defs["FOGNET_ASSIGNED_LDS_NODES"]) == abi.ASSIGNED_LDS_NODES
    assert re.search(r"#define FOGNET_ABI_VERSION 10\b", header()) and abi.ABI_VERSION == 10  # additive


def test_null_arguments_are_refused_without_a_device():
    lib = abi.load()
    bi, bo = abi.BatchIn(), abi.BatchOut()
    for n in NAMES:
        fn = getattr(lib, n)
        assert fn(None, None, None, None, None) == abi.FOGNET_ERR_ARG
        assert fn(None, C.byref(bi), None, C.byref(bo), None) == abi.FOGNET_ERR_ARG


def test_package_exports_the_mirror():
    import fognetsimpp_amd as fa
    for n in ("run_assigned", "assign_round_robin", "assign_random"):
        assert callable(getattr(fa, n)) and n in fa.__all__
