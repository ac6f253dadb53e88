"""The host half of SRTP (h264-fer_amd/csrc/fer_srtp_host.h: AES-128 key schedule and block, key derivation, HMAC midstates,
header rule, index estimate, argument checks) through tools/srtp_host_check.cpp, a stand-alone program without the HIP
runtime.  Built plainly here (its place under AddressSanitizer + UBSan is a developer's run, see the file), it must pass its
own checks, and agree with tests/golden/srtp_kat.json and with a listing tests/srtp_model.py writes.  No GPU."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import srtp_model as sm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("srtp_host") / "srtp_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "srtp_host_check.cpp"), "-o", str(out)], check=True, timeout=120)
    return out


def _list(exe, path, lines):
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), "list", str(path)], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout


def test_srtp_host_check_program(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_host_half_equals_the_openssl_record(exe, tmp_path):
    rec = json.loads((ROOT / "tests" / "golden" / "srtp_kat.json").read_text())
    lines = ["ecb %s %s %s" % (r["key"], r["in"], r["out"]) for r in rec["ecb"]]
    lines += ["ctr %s %s %s" % (r["key"], r["iv"], r["out"]) for r in rec["ctr"]]
    lines += ["hmac %s %s %s" % (r["key"], r["msg"] or "-", r["out"]) for r in rec["hmac"]]
    rc, out = _list(exe, tmp_path / "kat.txt", lines)
    assert rc == 0 and out == "%d records\n" % len(lines), out
    # the program does compare: one changed digit is found
    bad = lines[:]
    bad[3] = bad[3][:-1] + ("0" if bad[3][-1] != "0" else "1")
    rc, out = _list(exe, tmp_path / "bad.txt", bad)
    assert rc == 1 and "record 4 (ecb) differs" in out


def test_host_half_equals_the_models_listing(exe, tmp_path):
    rng = np.random.default_rng(20261021)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    lines = []
    masters = [(rb(16), rb(14)) for _ in range(6)]
    for mk, ms in masters:
        k_e, k_a, k_s = sm.derive(mk, ms)
        lines.append("derive %s %s %s %s %s" % (mk.hex(), ms.hex(), k_e.hex(), k_a.hex(), k_s.hex()))
        mi, mo = sm.hmac_midstates(k_a)
        lines.append("row %s %s %s %s %s" % (mk.hex(), ms.hex(), sm.expand_key(k_e).tobytes().hex(), b"".join(x.to_bytes(4, "big") for x in mi).hex(),
                                           b"".join(x.to_bytes(4, "big") for x in mo).hex()))
    # the header rule on every truncation of dressed headers
    for cc in range(16):
        for ext in (None, 0, 3):
            for b0 in (0, 0x40):  # version 2 and version 3
                p = bytearray(sm.rtp_packet(rb(6), 7, cc=cc, ext=ext))
                p[0] ^= b0
                for n in range(len(p) + 1):
                    lines.append("hdr %s %d" % (bytes(p[:n]).hex() or "-", sm.header_len(bytes(p[:n]))))
    assert {int(x.split()[-1]) for x in lines if x.startswith("hdr")} >= {0, 12, 16, 72, 76, 88}
    for roc in (0, 1, 5, 0xFFFFFFFF):
        for s_l in (0, 1, 2, 32767, 32768, 32769, 65534, 65535, 12345, 54321):
            for seq in (0, 1, 32767, 32768, 32769, 65534, 65535, (s_l + 32768) & 0xFFFF, (s_l + 32769) & 0xFFFF, (s_l - 32769) & 0xFFFF):
                lines.append("est %d %d %d %d" % (roc, s_l, seq, sm.estimate(roc, s_l, seq)))
    # whole packets: the host route of tools/srtp_rate.py
    for k, n in enumerate((0, 1, 15, 16, 17, 40, 41, 42, 43, 44, 45, 100, 1388)):
        mk, ms = masters[k % len(masters)]
        roc, s_l = (0, 65530) if k & 1 else (9, 100)
        p = sm.rtp_packet(rb(n), 65533 + k, ssrc=0x01020304 * (k + 1) & 0xFFFFFFFF, cc=k % 3, ext=(None, 0, 2)[k % 3])
        out, _ = sm.protect([(0, p)], [sm.derive(mk, ms)], [(roc, s_l, 1)])
        lines.append("protect %s %s %d %d %s %s" % (mk.hex(), ms.hex(), roc, s_l, p.hex(), out[0].hex()))
    rc, out = _list(exe, tmp_path / "model.txt", lines)
    assert rc == 0 and out == "%d records\n" % len(lines), out
