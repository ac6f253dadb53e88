"""The live decoder's host demultiplexer (split_ts, h264-fer_amd/csrc/fer_dec_syntax_host.h) through tools/ts_host_check.cpp, a
stand-alone program without the HIP runtime.  Built plainly here (its place under AddressSanitizer + UBSan is a developer's
run, see the file), it must pass its own checks, and its listing of the units, the fault and the expectation must be the one
of tests/ts_model.py, on the committed streams, on the dressed input and on the fault catalogue.  No GPU."""
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import ts_model as tm
from conftest import golden_bytes

ROOT = Path(__file__).resolve().parent.parent
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("ts_host") / "ts_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "ts_host_check.cpp"), "-o", str(out)], check=True, timeout=120)
    return out


def _want(data, pid, expect):
    es, fault, nxt = tm.demux(data, pid, expect)
    return ["%d %d %d %d" % (t, r, len(p), zlib.adler32(p)) for t, r, p in tm.units_of(es)] + [f"fault {fault}", f"cc {nxt}"]


def _run(exe, path, data, pid, expect):
    path.write_bytes(data)
    r = subprocess.run([str(exe), str(path), str(pid), str(expect)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_ts_host_check_program(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_split_ts_lists_the_models_units_of_the_golden_streams(exe, tmp_path):
    for name in GOLDENS:
        stream = golden_bytes(name)
        for with_psi in (False, True):
            data = b"".join(tm.mux_stream(stream, tm.HDR, with_psi))
            want = _want(data, tm.HDR["pid"], tm.HDR["cc"])
            assert len(want) == len(tm.stream_units(stream)) + 2 and want[-2] == "fault 0"
            assert _run(exe, tmp_path / "s.ts", data, tm.HDR["pid"], tm.HDR["cc"]) == want, name
            assert _run(exe, tmp_path / "s.ts", data, tm.HDR["pid"], -1) == want, name
            # a packet lost in the middle, and the last one lost
            k = (len(data) // 188 // 2) * 188
            lost = data[:k] + data[k + 188:]
            assert _run(exe, tmp_path / "s.ts", lost, tm.HDR["pid"], tm.HDR["cc"]) == _want(lost, tm.HDR["pid"], tm.HDR["cc"]), name
            assert _run(exe, tmp_path / "s.ts", data[:-188], tm.HDR["pid"], -1) == _want(data[:-188], tm.HDR["pid"], -1), name
        dressed, k = tm.dress(tm.access_units_of(stream), 0x100, 5)
        assert _run(exe, tmp_path / "d.ts", dressed, 0x100, 5) == _want(dressed, 0x100, 5) == _want(data, 0x100, -1)[:-1] + [f"cc {(5 + k) & 15}"]


def test_split_ts_on_the_fault_catalogue(exe, tmp_path):
    for name, data, pid, expect, fault, stands in tm.catalogue():
        got = _run(exe, tmp_path / "c.ts", data, pid, expect)
        assert got == _want(data, pid, expect), name
        assert got[-2] == f"fault {fault}" and len(got) == len(tm.units_of(stands)) + 2, name
