"""The replay workspace layouts (fognetsimpp_amd/csrc/workspace.h) are host-only C++: a stand-alone
program (tests/c/workspace_check.cpp) walks each layout at fixed shapes and checks alignment, order,
part sizes and totals, and the literal offsets the library has always used.  The program is built with
AddressSanitizer and UBSan (host code only).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fognetsimpp_amd", "csrc")


def test_workspace_header_is_host_only():
    """workspace.h compiles on its own with the host compiler: no HIP header, nothing from internal.h."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-include", os.path.join(CSRC, "workspace.h"), "-x", "c++", os.devnull], check=True)


def test_workspace_layouts(tmp_path):
    exe = str(tmp_path / "workspace_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "c", "workspace_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "workspace: all checks passed" in p.stdout
