"""The fragmented MP4 code that runs on the host (h264-fer_amd/csrc/fer_mp4_host.h: the box walk the device kernel shares, the
initialisation segment, the words of a segment's front; split_mp4 of fer_dec_syntax_host.h) through tools/mp4_host_check.cpp, a
stand-alone program without the HIP runtime.  Built plainly here (its place under AddressSanitizer + UBSan is a developer's
run, see the file), it must pass its own checks, and its listings must be those of tests/mp4_model.py on the committed
streams, on the dressed input, on the fault catalogue and on every truncation.  No GPU."""
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import avcc_model
import mp4_model as mm
import ts_model as tm
from conftest import golden_bytes

ROOT = Path(__file__).resolve().parent.parent
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]
HDR = dict(decode_time=(1 << 32) + 90000, sequence=0x01020304, duration=3000)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("mp4_host") / "mp4_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "mp4_host_check.cpp"), "-o", str(out)], check=True, timeout=180)
    return out


def _want(run, L=4):
    samples, fault = mm.demux(run, L)
    return ["%d %d %d %d" % (t, r, len(p), zlib.adler32(p)) for t, r, p in mm.units(run, L)] + [f"samples {len(samples)}", f"fault {fault}"]


def _run(exe, *args):
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def _list(exe, path, run, L=4):
    path.write_bytes(run)
    return _run(exe, path, L)


def _fragments(name):
    aus = tm.access_units_of(golden_bytes(name))
    samples, types = [avcc_model.annexb_to_avcc(e) for e, _ in aus], [t for _, t in aus]
    return samples, types


def test_mp4_host_check_program(exe):
    _run(exe)


def test_split_mp4_lists_the_models_units_of_the_golden_streams(exe, tmp_path):
    for name in GOLDENS:
        samples, types = _fragments(name)
        run = b"".join(mm.segment(samples[g: g + 2], [t == 5 for t in types[g: g + 2]], dict(HDR, sequence=g), 3) for g in range(0, len(samples), 2))
        want = _want(run)
        assert want[-2:] == [f"samples {len(samples)}", "fault 0"] and len(want) > len(samples) + 2
        assert _list(exe, tmp_path / "s.mp4", run) == want, name
        for vname, dressed, stand in mm.dress([samples[:2], samples[2:]]):
            got = _list(exe, tmp_path / "d.mp4", dressed)
            assert got == _want(dressed) and got[-2:] == [f"samples {len(stand)}", "fault 0"], (name, vname)


def test_split_mp4_on_the_fault_catalogue(exe, tmp_path):
    for L in (4, 2, 1):
        for name, run, stand, fault in mm.catalogue(L):
            got = _list(exe, tmp_path / "c.mp4", run, L)
            assert got == _want(run, L), (L, name)
            assert got[-2:] == [f"samples {len(stand)}", f"fault {fault}"], (L, name)


def test_split_mp4_on_every_truncation(exe, tmp_path):
    cases = mm.catalogue()
    runs = [cases[0][1], mm.dress([cases[0][2][:2], cases[0][2][2:]])[-1][1], next(r for n, r, _, _ in cases if "overrun inside" in n)]
    samples, types = _fragments(GOLDENS[2])
    runs.append(mm.segment(samples[:1], [True], HDR, 1) + mm.segment(samples[1:], [False] * (len(samples) - 1), HDR, 6))
    for run in runs:
        (tmp_path / "t.mp4").write_bytes(run)
        got = _run(exe, tmp_path / "t.mp4", 4, "trunc")
        assert len(got) == len(run) + 1
        # every length of the three short runs; the long run (two fragments of a committed stream, the model being slow on
        # it) is compared at every 7th length and at every length around its fragments' ends -- the program takes them all
        step = 1 if len(run) < 4000 else 7
        near = [k for e in (len(mm.cut_runs(run)[0]), len(run)) for k in range(max(e - 40, 0), min(e + 40, len(run)) + 1)]
        for k in sorted(set(range(0, len(run) + 1, step)) | set(near)):
            s, f = mm.demux(run[:k])
            assert got[k] == f"{k} {len(s)} {f}", k


def test_builders_equal_the_model(exe, tmp_path):
    for name in GOLDENS[:2]:
        sps, pps = avcc_model.parameter_sets_of(golden_bytes(name))
        for dw, dh, ts in ((176, 144, 90000), (50, 38, 25), (65535, 1, 0xFFFFFFFF)):
            got = _run(exe, "init", sps.hex(), pps.hex(), dw, dh, ts)
            ini = mm.init_segment(sps, pps, dw, dh, ts)
            off, n = mm.find_avcc(ini)
            assert got == [ini.hex(), f"avcc {off} {n}"]
            (tmp_path / "i.mp4").write_bytes(ini)
            assert _run(exe, "avcc", tmp_path / "i.mp4") == [f"avcc {off} {n}"]
            (tmp_path / "i.mp4").write_bytes(ini.replace(b"avc1", b"mp4v"))
            assert _run(exe, "avcc", tmp_path / "i.mp4") == ["none"]
        assert _run(exe, "init", sps.hex(), pps.hex(), 176, 144, 0) == ["", "none"]
    for K, n in ((1, 1), (2, 1), (3, 3), (6, 4), (4096, 4096), (4096, 1)):
        samples = [bytes([k & 255]) * (k % 7) for k in range(n)]
        seg = bytearray(mm.segment(samples, [False] * n, HDR, K))
        seg[88: 88 + 12 * n] = bytes(12 * n)  # the trun entries are append's
        D = mm.data_offset(K)
        assert _run(exe, "front", n, K, sum(map(len, samples)), HDR["decode_time"], HDR["sequence"]) == [bytes(seg[:D]).hex()], (K, n)
