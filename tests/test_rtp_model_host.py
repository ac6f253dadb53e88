"""tests/rtp_model.py pinned to what exists: the round trip over the committed golden streams, the fragment arithmetic, two
hand-written packets, the byte-serial restatements, the fault catalogue, a hand-written SDP line; and the library's
exports and binding of the RTP calls.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import nal_model
import rtp_model as rm

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]
PS = (80, 81, 95, 128, 1400, 1472, 16384, 65535)
# counted with a prototype of the definition before the model was written
COUNTS = {("qcif_ippp_4f_qp12_w16.264", 80): 573, ("qcif_ippp_4f_qp12_w16.264", 128): 333, ("qcif_ippp_4f_qp12_w16.264", 1400): 30,
          ("qcif_skip_5f_qp12.264", 80): 441, ("qcif_skip_5f_qp12.264", 128): 258, ("qcif_skip_5f_qp12.264", 1400): 26}


def _kind(p):
    return p[12] & 31


@pytest.mark.parametrize("name", GOLDENS)
def test_round_trip_on_the_golden_streams(name):
    x = (GOLD / name).read_bytes()
    for P in PS:
        packets, units = rm.packetise_stream(x, P)
        assert len(units) >= 4 and b"".join(b"\x00\x00\x00\x01" + u for u in units) == x
        assert max(len(p) for p in packets) <= P
        assert int.from_bytes(packets[0][2:4], "big") == 65530
        got, fault, nxt = rm.depacketise(packets, 65530)
        assert got == units and fault == 0 and nxt == (65530 + len(packets)) & 0xFFFF, f"{name} P = {P}"
        assert rm.depacketise(packets) == (units, 0, nxt), "no expectation"
        if (name, P) in COUNTS:
            assert len(packets) == COUNTS[name, P]
        kinds = {_kind(p) for p in packets}
        if name == "qcif_skip_5f_qp12.264" and P <= 1472:
            assert kinds == {1, 24, 28}, "its 6-byte P slices are single-NAL packets"
        if P >= 16384:
            assert kinds <= {1, 5, 24}, "every slice is a single-NAL packet"
        # M ends every access unit and nothing else
        assert sum(p[1] >> 7 for p in packets) == sum(1 for u in units if u[0] & 31 in (1, 5))
        if P in (80, 1400):
            assert rm.depacketise_serial(packets, 65530) == (units, 0, nxt)
            h = dict(rm.HDR)
            for au in rm.access_units_of(x)[:2]:
                assert rm.packetise_serial(au, P, h) == rm.packetise(au, P, h)
                h["seq"] = (h["seq"] + 1000) & 0xFFFF


@pytest.mark.parametrize("P", (80, 81, 95, 1400, 65535))
def test_fragment_count_and_last_fragment(P):
    B, F = P - 12, P - 14
    rng = np.random.default_rng(P)
    for N in (1, 2, B - 1, B, B + 1, F + 1, F + 2, 2 * F + 1, 2 * F + 2):
        u = bytes([0x65]) + rng.integers(4, 256, N - 1).astype(np.uint8).tobytes()
        pk = rm.packetise([u], P, rm.HDR)
        assert [len(p) for p in pk] == rm.fragments(N, P)
        if N <= B:
            assert len(pk) == 1 and pk[0][12:] == u and pk[0][1] == 0x80 | 96
            continue
        n = -(-(N - 1) // F)
        assert len(pk) == n >= 2
        last = N - 1 - (n - 1) * F
        assert 1 <= last <= F and len(pk[-1]) == 14 + last and all(len(p) == P for p in pk[:-1])
        assert [p[13] >> 6 for p in pk] == [2] + [0] * (n - 2) + [1]
        assert all(p[12] == 0x7C and p[13] & 31 == 5 for p in pk)
        assert b"".join(p[14:] for p in pk) == u[1:]
        assert rm.packetise_serial([u], P, rm.HDR) == pk
    # by hand: B = F + 2, so the shortest unit that is cut (N = B + 1) leaves F + 2 bytes behind its header byte
    assert rm.fragments(B, P) == [P] and rm.fragments(B + 1, P) == [P, 14 + 2]
    assert rm.fragments(2 * F + 1, P) == [P, P] and rm.fragments(2 * F + 2, P) == [P, P, 15]


def test_hand_written_fu_a_and_stap_a_packets():
    hdr = dict(ssrc=0xA1B2C3D4, timestamp=0x01020304, seq=65535, payload_type=96)
    P = 80
    u = bytes([0x65]) + bytes(range(100, 170))  # N = 71 > B = 68: fragments of 66 and 4 bytes
    pk = rm.packetise([u], P, hdr)
    assert pk[0] == bytes.fromhex("8060ffff01020304a1b2c3d4" "7c85") + bytes(range(100, 166))
    assert pk[1] == bytes.fromhex("80e0000001020304a1b2c3d4" "7c45") + bytes(range(166, 170))
    sps, pps, idr = bytes.fromhex("2742c0299a746b20"), bytes.fromhex("28ce7880"), bytes.fromhex("2588840a")
    pk = rm.packetise([sps, pps, idr], P, hdr)
    assert pk[0] == bytes.fromhex("8060ffff01020304a1b2c3d4" "38" "0008" "2742c0299a746b20" "0004" "28ce7880")
    assert pk[1] == bytes.fromhex("80e0000001020304a1b2c3d4" "2588840a")
    assert rm.packetise_serial([sps, pps, idr], P, hdr) == pk
    assert rm.depacketise(pk, 65535) == ([sps, pps, idr], 0, 1)
    assert rm.sdp_fmtp(sps, pps) == "profile-level-id=42c029;packetization-mode=1;sprop-parameter-sets=J0LAKZp0ayA=,KM54gA=="
    # the profile bytes are RBSP bytes: an SPS whose first bytes are escaped
    assert rm.sdp_fmtp(bytes.fromhex("67000003aa"), b"\x68\x01").startswith("profile-level-id=0000aa;")


def test_vectorised_forms_equal_the_byte_serial_ones_on_drawn_units():
    rng = np.random.default_rng(5)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 255], np.uint8)
    for k in range(120):
        P = int(rng.choice([80, 81, 95, 128, 300]))
        units = []
        if k & 1:
            units += [nal_model.frame_nal(7, alphabet[rng.integers(0, 7, 9)])[4:], nal_model.frame_nal(8, alphabet[rng.integers(0, 7, 4)])[4:]]
        units.append(nal_model.frame_nal((1, 5)[k & 1], alphabet[rng.integers(0, 7, int(rng.integers(0, 900)))], nal_ref_idc=k % 4)[4:])
        hdr = dict(ssrc=int(rng.integers(0, 1 << 32)), timestamp=int(rng.integers(0, 1 << 32)), seq=int(rng.integers(65000, 65536)),
                   payload_type=int(rng.integers(0, 128)))
        pk = rm.packetise(units, P, hdr)
        assert rm.packetise_serial(units, P, hdr) == pk, f"draw {k}"
        want = (units, 0, (hdr["seq"] + len(pk)) & 0xFFFF)
        assert rm.depacketise(pk, hdr["seq"]) == want and rm.depacketise_serial(pk, hdr["seq"]) == want, f"draw {k}"


def test_fault_catalogue():
    names = set()
    for name, packets, expect, fault, front in rm.catalogue():
        got = rm.depacketise(packets, expect)
        assert got == rm.depacketise_serial(packets, expect), name
        assert got[1] == fault and got[0] == front, f"{name}: {got[1]}, {len(got[0])} units"
        assert (got[2] == -1) == (fault != 0), f"{name}: a fault clears the expectation"
        names.add(name)
    assert {"short_header", "version_1", "csrc_overruns", "extension_overruns", "padding_overruns", "pad_byte_0", "stap_size_0",
            "stap_size_overruns", "fu_s_and_e", "fu_continuation_without_start", "fu_start_while_open", "single_inside_open_fu",
            "type_0", "type_25", "type_29", "gap", "open_unit_at_the_end"} <= names
    faults = {f for _, _, _, f, _ in rm.catalogue()}
    assert faults == {0, rm.MALFORMED, rm.GAP, rm.TRUNCATED} and 1 not in faults


def test_csrc_extension_and_padding_decode_like_plain_packets():
    x = (GOLD / GOLDENS[3]).read_bytes()
    packets, units = rm.packetise_stream(x, 95)
    dressed = []
    for k, p in enumerate(packets):
        cc, ext, pad = k % 4, (None, 0, 2)[k % 3], (0, 1, 4, 255)[k % 4]
        q = rm.raw_packet(p[12:], int.from_bytes(p[2:4], "big"), cc=cc, ext=ext, pad=pad, marker=p[1] >> 7)
        assert len(q) == len(p) + 4 * cc + (0 if ext is None else 4 + 4 * ext) + pad
        dressed.append(q)
    nxt = (65530 + len(packets)) & 0xFFFF
    assert rm.depacketise(dressed, 65530) == (units, 0, nxt) and rm.depacketise_serial(dressed, 65530) == (units, 0, nxt)


def test_layout_rounds_every_packet_to_16():
    a, b = [b"x" * 13, b"y" * 80, b"z" * 17], [b"w" * 16]
    placed, rows, index = rm.layout([a, [], b], [5, 0, 1])
    assert rows == [(0, 13, 0), (16, 80, 0), (96, 17, 0), (128, 16, 2)]
    assert index == [(0, 128, 5, 0, 3), (0, 0, 0, 0, 0), (128, 16, 1, 3, 1), (144, 2, 0, 4, 0)]
    assert [o for o, _ in placed] == [0, 16, 96, 128]


def test_library_exports_and_binds_the_new_symbols(pkg):
    lib = pkg.load_library()
    hdr = (ROOT / "include" / "ferhip.h").read_text()
    for n in ["ferhip_pack_rtp", "ferhip_fetch_rtp", "ferhip_rtp_blocks", "ferhip_write_sdp_fmtp", "ferhip_decs_decode_rtp", "ferhip_unrtp_blocks"]:
        assert re.search(r"\b" + n + r"\s*\(", hdr), f"{n} is not declared in include/ferhip.h"
        assert hasattr(lib, n), f"{n} declared in include/ferhip.h but not exported"
        assert getattr(lib, n).argtypes is not None, f"{n} is not bound"
    for t, dt, size in (("ferhip_rtp_hdr", pkg.RTP_HDR, 12), ("ferhip_rtp_pkt", pkg.RTP_PKT, 16), ("ferhip_rtp_au", pkg.RTP_AU, 24)):
        m = re.search(r"typedef struct \{([^}]*)\} " + t + ";", hdr)
        assert m and dt.itemsize == size
        fields = [f.strip() for part in m.group(1).split(";") if part.strip() for f in part.split(None, 1)[1].split(",")]
        assert fields == list(dt.names), t
    for name in ("pack_rtp_device", "fetch_rtp", "sdp_fmtp"):
        assert hasattr(pkg.FerHip, name)
    assert hasattr(pkg, "rtp_blocks_raw") and hasattr(pkg, "unrtp_blocks_raw") and hasattr(pkg.LiveDecoder, "decode_rtp")
    # argument checks that need no device
    h = pkg.rtp_hdr(1)
    idx = np.zeros(2, pkg.RTP_AU)
    lens, types = np.array([4], np.uint32), np.array([1], np.int32)
    src = np.zeros(16, np.uint8)
    args = lambda P=1400, hd=h, n=1, ix=idx: (src.ctypes.data, 16, lens.ctypes.data, types.ctypes.data, n, P, hd.ctypes.data if hd is not None else None,
                                               None, 0, None, 0, ix.ctypes.data if ix is not None else None)
    for kw in (dict(P=79), dict(P=65536), dict(hd=None), dict(n=0), dict(n=65536), dict(ix=None)):
        assert lib.ferhip_rtp_blocks(*args(**kw)) == -1, kw
    bad = pkg.rtp_hdr(1, payload_type=128)
    assert lib.ferhip_rtp_blocks(*args(hd=bad)) == -1
    bad = pkg.rtp_hdr(1)
    bad["reserved"] = 3
    assert lib.ferhip_rtp_blocks(*args(hd=bad)) == -1
    assert lib.ferhip_pack_rtp(None, 0, 1400, h.ctypes.data, None, 0, None, 0, idx.ctypes.data) == -1
    assert lib.ferhip_fetch_rtp(None, 0, 1400, h.ctypes.data, None, 0, None, 0, idx.ctypes.data) == -1
    assert lib.ferhip_write_sdp_fmtp(None, 0, None, 0) == 0
    assert lib.ferhip_decs_decode_rtp(None, None, 0, None, 0, None, 0, None, None) == -1
    rows = np.zeros(1, pkg.RTP_PKT)
    rows["bytes"] = 20
    assert pkg.unrtp_blocks_raw(b"\x80" * 16, rows, 1)[0] == -1, "a row that leaves the base"
    assert pkg.unrtp_blocks_raw(b"\x80" * 32, rows, 0)[0] == -1 and pkg.unrtp_blocks_raw(b"\x80" * 32, rows, 1, misalign=16)[0] == -1
    rows["stream"] = 1
    assert pkg.unrtp_blocks_raw(b"\x80" * 32, rows, 1)[0] == -1
