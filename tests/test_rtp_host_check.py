"""The live decoder's host depacketiser (split_rtp, h264-fer_amd/csrc/fer_dec_syntax_host.h) through tools/rtp_host_check.cpp, a
stand-alone program without the HIP runtime.  Built plainly here (its place under AddressSanitizer + UBSan is a developer's
run, see the file), it must pass its own checks, and its listing of the units, the fault and the expectation must be the one
of tests/rtp_model.py followed by the unit rules of tests/avcc_model.py, on the committed streams and on the fault catalogue.
No GPU."""
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import avcc_model as am
import rtp_model as rm
from conftest import golden_bytes

ROOT = Path(__file__).resolve().parent.parent
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("rtp_host") / "rtp_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "rtp_host_check.cpp"), "-o", str(out)], check=True, timeout=120)
    return out


def _want(packets, expect):
    units, fault, nxt = rm.depacketise(packets, expect)
    rows = ["%d %d %d %d" % (t, r, len(p), zlib.adler32(p)) for t, r, p in am.split(rm.to_avcc(units), 4)]
    return rows + [f"fault {fault}", f"seq {nxt}"]


def _run(exe, path, packets, expect):
    path.write_bytes(b"".join(len(p).to_bytes(4, "little") + bytes(p) for p in packets))
    r = subprocess.run([str(exe), str(path), str(expect)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_rtp_host_check_program(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_split_rtp_lists_the_models_units_of_the_golden_streams(exe, tmp_path):
    for name in GOLDENS:
        for P in (80, 95, 1400, 65535):
            packets, units = rm.packetise_stream(golden_bytes(name), P)
            want = _want(packets, 65530)
            assert len(want) == len(units) + 2 and want[-2] == "fault 0"
            assert _run(exe, tmp_path / "s.rtp", packets, 65530) == want, (name, P)
            assert _run(exe, tmp_path / "s.rtp", packets, -1) == want, (name, P)
            # a packet lost in the middle, and the last one lost
            k = len(packets) // 2
            lost = packets[:k] + packets[k + 1:]
            assert _run(exe, tmp_path / "s.rtp", lost, 65530) == _want(lost, 65530), (name, P)
            assert _run(exe, tmp_path / "s.rtp", packets[:-1], 65530) == _want(packets[:-1], 65530), (name, P)


def test_split_rtp_on_the_fault_catalogue(exe, tmp_path):
    for name, packets, expect, fault, front in rm.catalogue():
        got = _run(exe, tmp_path / "c.rtp", packets, expect)
        assert got == _want(packets, expect), name
        assert got[-2] == f"fault {fault}" and len(got) == len(front) + 2, name


def test_a_unit_without_payload_ends_the_list_not_the_walk(exe, tmp_path):
    packets = [rm.raw_packet(bytes([0x41, 1, 2]), 5), rm.raw_packet(bytes([0x68]), 6), rm.raw_packet(bytes([0x67, 1]), 7)]
    assert _run(exe, tmp_path / "h.rtp", packets, 5) == _want(packets, 5) == ["1 2 2 %d" % zlib.adler32(b"\x01\x02"), "fault 0", "seq 8"]
