"""The index arithmetic of the motion chain's list prefetch (h264-fer_amd/csrc/fer_chain_idx.h) through
tools/chain_idx_host_check.cpp, a stand-alone program without the HIP runtime: for every even row length 2 .. 480, every
step, the distances 0, 1 and 2 and every lane, the step asked for lies in the row, equals the unclamped one wherever that is
inside, and every offset reads an entry of that step's own partition in arrays that end with the row.  Built plainly here
(its place under AddressSanitizer + UBSan is a developer's run, see the file).  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("chain_idx_host") / "chain_idx_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "chain_idx_host_check.cpp"), "-o", str(out)], check=True, timeout=120)
    return out


def test_chain_idx_host_check_program(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # rows 2, 4, .. 480: sum of gw = 57 840 steps, three distances, 64 lanes
    assert r.stdout.strip() == "ok %d" % (57840 * 3 * 64), r.stdout


def test_the_kernel_addresses_the_lists_through_the_header_only():
    """k_me_resolve's request goes through chain_idx / chain_ahead_step; no second statement of the layout next to it"""
    src = (ROOT / "h264-fer_amd" / "csrc" / "fer_me.hip").read_text()
    body = src[src.index("auto request = [&]"):src.index("ResStage ahead[RES_AHEAD]")]
    assert "chain_idx(" in body and "chain_rel_part(" in body
    assert "* 17" not in body and "* 33" not in body
    assert src.count("chain_ahead_step(") >= 3  # the start of a row, the step's request, the request again after a wrong guess
