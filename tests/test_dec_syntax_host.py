"""The decoder's host readers of untrusted bytes (h264-fer_amd/csrc/fer_dec_syntax_host.h: bit reader, SPS / PPS / slice header
parsers, split_stream, split_avcc, the configuration record walk) through tools/dec_syntax_host_check.cpp, a stand-alone
program without the HIP runtime.  Built plainly here (its place under AddressSanitizer + UBSan is a developer's run, see the
file), it must pass its own checks, and its listing of the units of the committed streams must be the one of
tests/nal_split_model.py / tests/avcc_model.py, which test_nal_split_model_host.py and test_avcc_model_host.py pin to the
oracle.  The header values themselves stay pinned by the bit-exact GPU decode tests.  No GPU."""
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import avcc_model as am
import nal_split_model as sm
from conftest import golden_bytes

ROOT = Path(__file__).resolve().parent.parent
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]
DRUGI_PREFIX = 200000  # bytes of drugi.264: some forty pictures, cut inside a slice


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("dec_syntax") / "dec_syntax_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "dec_syntax_host_check.cpp"), "-o", str(out)], check=True, timeout=120)
    return out


def _streams():
    return [(g, golden_bytes(g)) for g in GOLDENS] + [("drugi.264 prefix", golden_bytes("drugi.264")[:DRUGI_PREFIX])]


def _listing(units):
    return ["%d %d %d %d" % (t, r, len(p), zlib.adler32(p)) for t, r, p in units]


def _run(exe, path, data, *args):
    path.write_bytes(data)
    r = subprocess.run([str(exe), str(path), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_dec_syntax_host_check_program(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_split_stream_lists_the_models_units(exe, tmp_path):
    for name, data in _streams():
        want = _listing(sm.split(data))
        assert len(want) >= 4, name
        assert _run(exe, tmp_path / "s.264", data) == want, name


def test_split_avcc_lists_the_models_units(exe, tmp_path):
    for name, data in _streams():
        for L in (2, 4) if len(data) < DRUGI_PREFIX else (4,):
            framed = am.annexb_to_avcc(data, L)
            units, fault = am.avcc_split(framed, L)
            assert fault == 0 and len(units) >= 4, name
            want = _listing([(t, r, p) for _, _, t, r, p in units]) + ["overrun 0"]
            assert _run(exe, tmp_path / "s.avcc", framed, str(L)) == want, (name, L)
            cut = framed[:-3]  # the last unit overruns: the units in front of it, and the fault
            assert _run(exe, tmp_path / "s.avcc", cut, str(L)) == want[:-2] + ["overrun 1"], (name, L)
