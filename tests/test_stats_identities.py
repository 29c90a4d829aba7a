"""The packed statistics pass bins a queueTime from the double it already holds and converts the
queueStartTime round trip without a range test (replay_common.h hist_bin_raw(double),
simtime_to_int64_inrange).  A stand-alone host program (tests/c/stats_identities_check.cpp) restates
both helpers in plain C++ and sets them against the formulas the other passes keep, over every power
of two and its neighbours, the 2^53 edge, both ends of the tick range and 10^8 seeded random values
each.  Built with AddressSanitizer and UBSan (host code only: a conversion out of range would be
reported).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stats_identities(tmp_path):
    exe = str(tmp_path / "stats_identities_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c", "stats_identities_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "stats identities: all checks passed" in p.stdout
