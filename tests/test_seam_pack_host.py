"""The host packer of the per-macroblock seam (h264-fer_amd/csrc/fer_seam_pack_host.h: the table of the FerDev arrays that
ferhip_residual_mbs, ferhip_intra_mbs and ferhip_mv_mbs build by hand, the level record, the neighbour copy, the job packing
and the job order) through tools/seam_pack_host_check.cpp, a stand-alone program without the HIP runtime.  Built plainly
here (its place under AddressSanitizer + UBSan is a developer's run, see the file), it must pass its own checks: every
stride against the literal the device code uses, every stream range inside its array, the level round trip, the packed
arrays of every job kind entry by entry, the order function.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_seam_pack_host_check_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "seam_pack_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "seam_pack_host_check.cpp"), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "seam_pack_host_check ok"
