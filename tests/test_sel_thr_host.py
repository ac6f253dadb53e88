"""The coarse threshold of the motion search's selections (h264-fer_amd/csrc/fer_sel_thr.h) through
tools/sel_thr_host_check.cpp, a stand-alone program without the HIP runtime: over every value below 2^21 the code is
monotone, the threshold of a value's code is monotone, at least the value, within the granule bound the header states
and below 2^21; over random and adversarial sets of 64 lane minima and every need 1 .. 33 the coarse bound, searched as
the kernel searches it, is at least the exact need-th smallest, admits at least `need` lanes and is the threshold of
the exact one's code, and the 21-step search gives the exact one.  Built plainly and, as a stand-alone program, under
AddressSanitizer + UBSan.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tools" / "sel_thr_host_check.cpp"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no C++ compiler")
    return c


def _run(cxx, out, flags):
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(SRC), "-o", str(out)], check=True, timeout=300)
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 1 << 21 and int(words[2]) > 500000, r.stdout


def test_sel_thr_host_check_program(cxx, tmp_path):
    _run(cxx, tmp_path / "sel_thr_host_check", [])


def test_sel_thr_host_check_program_under_sanitizers(cxx, tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime to link")
    _run(cxx, tmp_path / "sel_thr_host_check_san", SAN)

