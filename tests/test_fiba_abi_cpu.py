"""The full inertial bundle adjustment's C ABI: its exports are in the built library, declared in include/omv.h and bound
in _lib.py, its three structs have the layout of their ctypes mirrors (a failed static_assert otherwise), as C++17 and as
C11, and the adapter with its consumer compiles warning-free."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from openmavis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["omv_fiba_create", "omv_fiba_destroy", "omv_fiba_set_problem", "omv_fiba_optimize", "omv_fiba_evaluate",
         "omv_fiba_reset", "omv_fiba_debug_solve", "omv_fiba_enable_timing", "omv_fiba_stage_ms"]


def _mirrors():
    return {"omv_fiba_problem": _lib.FibaProblem, "omv_fiba_opts": _lib.FibaOpts, "omv_fiba_result": _lib.FibaResult}


def test_exported_symbols_and_python_surface():
    assert all(n in _lib.SIGNATURES for n in NAMES)
    header = open(os.path.join(ROOT, "include", "omv.h")).read()
    assert all(f"omv_status {n}(" in header for n in NAMES)
    assert "omv_fiba_set_comm" not in header   # one rank only
    assert os.path.exists(_lib.LIB_PATH), "libomv_hip.so not built"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in NAMES)
    from openmavis_amd.optimizer import FullInertialBA
    for m in ("set_problem", "optimize", "evaluate", "reset", "debug_solve", "enable_timing", "stage_ms"):
        assert callable(getattr(FullInertialBA, m))
    sig = inspect.signature(FullInertialBA.optimize).parameters
    assert list(sig)[1:4] == ["iterations", "lambda_init", "max_trials"]
    assert (sig["iterations"].default, sig["lambda_init"].default, sig["max_trials"].default) == (100, 1e-5, 10)


@pytest.mark.parametrize("compiler,flags", [("g++", ["-x", "c++", "-std=c++17"]), ("gcc", ["-x", "c", "-std=c11"])])
def test_struct_layouts_match_the_ctypes_mirrors(compiler, flags, tmp_path):
    if shutil.which(compiler) is None:
        pytest.skip(f"{compiler} absent")
    lines = ["#include <stddef.h>", '#include "omv.h"', "#ifdef __cplusplus", "#define A(c, m) static_assert(c, m)",
             "#else", "#define A(c, m) _Static_assert(c, m)", "#endif"]
    for cname, cls in _mirrors().items():
        lines.append(f'A(sizeof({cname}) == {ctypes.sizeof(cls)}, "sizeof({cname})");')
        for fname, _ in cls._fields_:
            member = "lambda" if fname == "lambda_" else fname
            lines.append(f'A(offsetof({cname}, {member}) == {getattr(cls, fname).offset}, "{cname}.{member}");')
    # the embedded problem is omv_lba_problem itself, whose layout tests/abi_check.cpp pins
    lines.append(f'A(sizeof(((omv_fiba_problem *)0)->base) == {ctypes.sizeof(_lib.LbaProblem)}, "omv_fiba_problem.base");')
    src = tmp_path / "fiba_abi.c"
    src.write_text("\n".join(lines) + "\nint fiba_abi_anchor(void) { return 0; }\n")
    r = subprocess.run([compiler, *flags, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "fiba_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_adapter_and_consumer_compile():
    """omv_adapt::FullInertialBA and tests/cpp/fiba_consumer.cpp compile with g++ -Wall -Werror against omv.h and the HIP
    runtime headers alone (run on the GPU by tests/test_fiba_consumer_gpu.py)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("g++ or HIP headers absent")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                        os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "fiba_consumer.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
