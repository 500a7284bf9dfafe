"""The visual bundle adjustment's C ABI: its exports are in the built library, declared in include/omv.h and bound in
_lib.py, and its three structs have the layout of their ctypes mirrors (a failed static_assert otherwise), as C++17 and
as C11."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from openmavis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["omv_vba_create", "omv_vba_destroy", "omv_vba_set_problem", "omv_vba_set_levels", "omv_vba_optimize",
         "omv_vba_evaluate", "omv_vba_reset", "omv_vba_debug_solve", "omv_vba_enable_timing", "omv_vba_stage_ms"]
MIRRORS = {"omv_vba_problem": _lib.VbaProblem, "omv_vba_opts": _lib.VbaOpts, "omv_vba_result": _lib.VbaResult}


def test_exported_symbols_and_python_surface():
    assert all(n in _lib.SIGNATURES for n in NAMES)
    header = open(os.path.join(ROOT, "include", "omv.h")).read()
    assert all(f"omv_status {n}(" in header for n in NAMES)
    assert os.path.exists(_lib.LIB_PATH), "libomv_hip.so not built"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in NAMES)
    from openmavis_amd.optimizer import LocalBundleAdjustment
    for m in ("set_problem", "set_levels", "optimize", "evaluate", "reset", "debug_solve"):
        assert callable(getattr(LocalBundleAdjustment, m))
    assert list(inspect.signature(LocalBundleAdjustment.optimize).parameters)[1:6] == [
        "iterations", "lambda_init", "max_trials", "huber_mono", "huber_stereo"]


@pytest.mark.parametrize("compiler,flags", [("g++", ["-x", "c++", "-std=c++17"]), ("gcc", ["-x", "c", "-std=c11"])])
def test_struct_layouts_match_the_ctypes_mirrors(compiler, flags, tmp_path):
    if shutil.which(compiler) is None:
        pytest.skip(f"{compiler} absent")
    lines = ["#include <stddef.h>", '#include "omv.h"', "#ifdef __cplusplus", "#define A(c, m) static_assert(c, m)",
             "#else", "#define A(c, m) _Static_assert(c, m)", "#endif"]
    for cname, cls in MIRRORS.items():
        lines.append(f'A(sizeof({cname}) == {ctypes.sizeof(cls)}, "sizeof({cname})");')
        for fname, _ in cls._fields_:
            member = "lambda" if fname == "lambda_" else fname
            lines.append(f'A(offsetof({cname}, {member}) == {getattr(cls, fname).offset}, "{cname}.{member}");')
    src = tmp_path / "vba_abi.c"
    src.write_text("\n".join(lines) + "\nint vba_abi_anchor(void) { return 0; }\n")
    r = subprocess.run([compiler, *flags, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "vba_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_adapter_and_consumer_compile():
    """omv_adapt::LocalBundleAdjustment and tests/cpp/vba_consumer.cpp compile with g++ -Wall -Werror against omv.h and
    the HIP runtime headers alone (run on the GPU by tests/test_vba_consumer_gpu.py)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("g++ or HIP headers absent")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                        os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "vba_consumer.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
