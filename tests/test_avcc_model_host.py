"""tests/avcc_model.py pinned to what exists: to tests/nal_split_model.py on the committed golden streams and on drawn unit
sets, to a byte-serial loop of the definition in include/ferhip.h on the adversarial ranges, and to a hand-written
AVCDecoderConfigurationRecord; and the library's exports and binding of the length-prefixed calls.  No GPU."""
import re
from pathlib import Path

import numpy as np

import avcc_model as am
import nal_model
import nal_split_model as sm

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]


def serial_split(s, L):
    """the definition, byte by byte -> (list of (type, ref_idc, rbsp), fault)"""
    n = len(s)
    out = []
    pos = 0
    while pos + L <= n:
        ln = 0
        for k in range(L):
            ln = ln * 256 + s[pos + k]
        st = pos + L
        en = st + ln
        if ln == 0:
            return out, 0
        if en > n:
            return out, 1
        rbsp = bytearray()
        for p in range(st + 1, en):
            if s[p] == 3 and p - 2 >= st + 1 and s[p - 2] == 0 and s[p - 1] == 0:
                continue
            rbsp.append(s[p])
        if not rbsp:
            return out, 0
        out.append((s[st] & 0x1F, (s[st] & 0x7F) >> 5, bytes(rbsp)))
        pos = en
    return out, int(pos < n)


def test_converted_golden_streams_split_into_the_same_units():
    for name in GOLDENS:
        x = (GOLD / name).read_bytes()
        want = sm.split(x)
        assert len(want) >= 4
        y = am.annexb_to_avcc(x, 4)
        assert len(y) == len(x), "a start code and a length are both four bytes"
        assert am.split(y, 4) == want and am.avcc_split(y, 4)[1] == 0, name
        assert serial_split(y, 4) == (want, 0), name


def test_converted_drawn_unit_sets_split_into_the_same_units():
    rng = np.random.default_rng(11)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 4, 0xFF], np.uint8)
    for k in range(200):
        # framed payloads back to back; a payload's trailing zeros would join the next start code: those end on a non-zero byte
        parts = []
        for _ in range(int(rng.integers(1, 6))):
            p = alphabet[rng.integers(0, alphabet.size, int(rng.integers(1, 300)))].copy()
            p[-1] = 0x80
            parts.append(nal_model.frame_nal(int(rng.integers(1, 32)), p, nal_ref_idc=int(rng.integers(0, 4))))
        x = b"".join(parts)
        want = sm.split(x)
        assert len(want) == len(parts)
        for L in (2, 4):
            y = am.annexb_to_avcc(x, L)
            assert am.split(y, L) == want and am.avcc_split(y, L)[1] == 0, f"draw {k}"
    # a header-only unit ends the range in both framings
    x = nal_model.frame_nal(7, b"\x01\x02") + nal_model.frame_nal(8, b"") + nal_model.frame_nal(5, b"\x04")
    assert am.split(am.annexb_to_avcc(x, 4), 4) == sm.split(x) == [(7, 1, b"\x01\x02")]


def test_model_equals_the_byte_serial_definition_on_the_adversarial_set():
    for L in (1, 2, 4):
        names = set()
        for name, r in am.corpus(L):
            units, fault = am.avcc_split(r, L)
            assert ([(t, ref, p) for _, _, t, ref, p in units], fault) == serial_split(r.tobytes(), L), f"L = {L}: {name}"
            names.add(name)
        assert {"overrun_by_one", "zero_length_in_the_middle", "length_one_in_the_middle", "header_00_then_00_03"} <= names
    # spot checks of the set itself, by hand
    c = dict(am.corpus(4))
    assert am.avcc_split(c["header_00_then_00_03"], 4) == ([(4, 9, 0, 0, b"\x00\x03\x05\x05")], 0)
    assert am.split(c["drop_twice_in_a_row"], 4) == [(5, 3, b"\x09\x00\x00\x00\x00\x07")]
    assert am.split(c["00_00_03_03"], 4) == [(5, 3, b"\x09\x00\x00\x03\x07")]
    assert am.avcc_split(c["overrun_by_one"], 4)[1] == 1 and len(am.split(c["overrun_by_one"], 4)) == 1
    assert am.avcc_split(c["stray_3"], 4) == ([(4, 8, 5, 3, b"\x01\x02\x03")], 1)
    assert am.avcc_split(c["zero_length_in_the_middle"], 4)[1] == 0 and len(am.split(c["zero_length_in_the_middle"], 4)) == 1
    assert len(am.split(c["start_codes_inside"], 4)) == 2
    assert max(len(p) for _, _, p in am.split(c["long_unit_65536"], 4)) > 60000


def test_layout_rounds_every_unit_to_16_and_stops_at_the_cut():
    u = am.unit
    a = u([1, 2], 4, 0x67) + u([], 4, 0x68) + u([4, 4, 4], 4)         # a header-only unit in the middle
    b = u(np.arange(1, 18), 4, 0x41) + bytes([0, 0, 0, 9, 0x65, 1])   # 17 bytes, then an overrun
    units, total, faults = am.layout([a, b"", b], 4)
    assert units == [(0, 7, 3, 2, 0), (2, 1, 2, 17, 16)] and total == 48 and faults == [0, 0, 1]


def test_config_record_by_hand(fo):
    """the oracle's SPS and PPS of a 48x32 stream at QP 12: 27 42 c0 29 9a 74 6b 20 and 28 ce 78 80"""
    W, H = 48, 32
    o = fo.Oracle(W, H, qp=12, window=16, maxdiff=3, intra_every=30)
    stream, _ = o.encode_stream(np.stack([fo.gen_frame(W, H, 0, 1234, 2)]))
    o.close()
    sps, pps = am.parameter_sets_of(stream)
    assert sps == bytes.fromhex("2742c0299a746b20") and pps == bytes.fromhex("28ce7880")
    want = bytes.fromhex("01" "42c029" "ff" "e1" "0008" "2742c0299a746b20" "01" "0004" "28ce7880")
    assert am.config_record(sps, pps) == want
    # the profile bytes are RBSP bytes: an SPS whose first bytes are escaped
    assert am.config_record(bytes.fromhex("67000003aa"), b"\x68\x01")[:4] == bytes.fromhex("010000aa")


def test_library_exports_and_binds_the_new_symbols(pkg):
    lib = pkg.load_library()
    hdr = (ROOT / "include" / "ferhip.h").read_text()
    new = ["ferhip_frame_nal_blocks_fmt", "ferhip_write_avcc_config", "ferhip_decs_set_input", "ferhip_decs_set_config",
           "ferhip_split_avcc_blocks"]
    for n in new:
        assert re.search(r"\b" + n + r"\s*\(", hdr), f"{n} is not declared in include/ferhip.h"
        assert hasattr(lib, n), f"{n} declared in include/ferhip.h but not exported"
        assert getattr(lib, n).argtypes is not None, f"{n} is not bound"
    assert int(re.search(r"#define FERHIP_AU_AVCC (\d+)", hdr).group(1)) == pkg.AU_AVCC
    assert int(re.search(r"#define FERHIP_AU_PARAM_SETS (\d+)", hdr).group(1)) == pkg.AU_PARAM_SETS
    assert pkg.AU_AVCC & pkg.AU_PARAM_SETS == 0
    assert int(re.search(r"#define FERHIP_IN_ANNEXB (\d+)", hdr).group(1)) == pkg.IN_ANNEXB
    assert int(re.search(r"#define FERHIP_IN_AVCC (\d+)", hdr).group(1)) == pkg.IN_AVCC
    for name in ("avcc_config",):
        assert hasattr(pkg.FerHip, name)
    for name in ("set_input", "set_config"):
        assert hasattr(pkg.LiveDecoder, name)
    # argument checks that need no device
    assert lib.ferhip_split_avcc_blocks(None, 0, None, 0, 0, 3, None, 0, None, 0, None, None) == -1
    assert lib.ferhip_decs_set_input(None, 0, 4) == -1 and lib.ferhip_decs_set_config(None, 0, None, 0) == -1
    assert lib.ferhip_write_avcc_config(None, 0, None, 0) == 0
