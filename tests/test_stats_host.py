"""The host side of the statistics records (csrc/stats_host.cpp) as a stand-alone program under
AddressSanitizer + UBSan.  CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stats_check_under_sanitizers(tmp_path):
    """tests/c/stats_check.cpp: for each of the seven records the empty record as the identity, the
    merge commutative, associative and equal to a restatement of the header's rule, carries and
    wraps, null arguments; one replication added to a job and to a group."""
    exe = str(tmp_path / "stats_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "stats_check.cpp"),
                    os.path.join(ROOT, "fognetsimpp_amd", "csrc", "stats_host.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "stats_check: all checks passed" in p.stdout
