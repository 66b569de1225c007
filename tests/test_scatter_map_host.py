"""The packed scatter's load map on the host (no GPU): tools/scatter_map_check.cpp
replays stage_packed_body's steps lane by lane over csrc/scatter_map.h for
every length 2..64, group sizes 1, 2, 63 and 64 and both start parities, and
checks that every block event is loaded once and stored at [event][history].
"""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quickcheck-state-machine-distributed_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("scatter_map") / "scatter_map_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tools", "scatter_map_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    return out.stdout


def test_every_event_once_and_in_place(report):
    assert "FAIL" not in report
    # 63 lengths x 4 group sizes x 2 start parities
    assert re.search(r"^504 cases, 0 failed$", report, re.M), report[-200:]


def test_conflict_degrees(report):
    """Per store instruction of a full group: a power-of-two length of 16 or
    more is 4-way (a quad of lanes writes 8 rows of one column: the least the
    64-byte quads allow) where block order is N0 / 2 -way; shorter ones and
    the other lengths are as in block order."""
    deg = {int(m[1]): (int(m[2]), int(m[3])) for m in re.finditer(r"^\s*(\d+)\s+(\d+) \(\s*(\d+)\)", report, re.M)}
    assert sorted(deg) == list(range(2, 65))
    for n0, (new, old) in deg.items():
        if n0 & (n0 - 1):
            assert new == old, n0
        else:
            assert old == max(1, n0 // 2) and new == min(old, 4), (n0, new, old)
