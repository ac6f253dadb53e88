"""tests/srtp_model.py, the reference of the SRTP tests, against what is published and against the openssl command line:
FIPS-197 appendix C.1, the keystream of RFC 3711 B.2, the key derivation of RFC 3711 B.3, HMAC-SHA1 of RFC 2202 case 1, the
whole record tests/golden/srtp_kat.json (regenerated where openssl is found), the index estimate against a transcription of
the RFC's pseudo-code, and protect / unprotect against each other.  No GPU."""
import hashlib
import hmac
import importlib.util
import json
import shutil
from pathlib import Path

import numpy as np
import pytest

import srtp_model as sm

GOLDEN = Path(__file__).resolve().parent / "golden"
H = bytes.fromhex


def _record():
    return json.loads((GOLDEN / "srtp_kat.json").read_text())


def test_fips_197_appendix_c1():
    assert sm.aes_ecb(H("000102030405060708090a0b0c0d0e0f"), H("00112233445566778899aabbccddeeff")) == H("69c4e0d86a7b0430d8cdb78070b4c55a")


def test_rfc_3711_b2_keystream():
    k_e, k_s = H("2B7E151628AED2A6ABF7158809CF4F3C"), H("F0F1F2F3F4F5F6F7F8F9FAFBFCFD")
    want = H("E03EAD0935C95E80E166B16DD92B4EB4" "D23513162B02D0F72A43A2FE4A5F97AB" "41E95B3BB0A2E8DD477901E4FCA894C0")
    assert sm.keystream(k_e, k_s, 0, 0, 48) == want
    # ... and its last three blocks, 0xfeff..0xff01: the counter is 16 bits wide
    iv = k_s + b"\xfe\xff"
    tail = sm.aes_cm(k_e, iv, 48)
    assert tail == H("EC8CDF7398607CB0F2D21675EA9EA1E4" "362B7C3C6773516318A077D7FC5073AE" "6A2CC3787889374FBEB4C81B17BA6C44")


def test_rfc_3711_b3_key_derivation():
    k_e, k_a, k_s = sm.derive(H("E1F97A0D3E018BE0D64FA32C06DE4139"), H("0EC675AD498AFEEBB6960B3AABE6"))
    assert k_e == H("C61E7A93744F39EE10734AFE3FF7A087")
    assert k_s == H("30CBBC08863D8C85D49DB34A9AE1")
    assert k_a == H("CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4")


def test_rfc_2202_case_1():
    assert hmac.new(b"\x0b" * 20, b"Hi There", hashlib.sha1).digest() == H("b617318655057264e28bc0b6fb378c8ef146be00")


def test_the_model_equals_the_openssl_record():
    rec = _record()
    assert len(rec["ecb"]) >= 16 and len(rec["ctr"]) >= 24 and [len(r["msg"]) // 2 for r in rec["hmac"]] == list(range(201))
    for r in rec["ecb"]:
        assert sm.aes_ecb(H(r["key"]), H(r["in"])) == H(r["out"])
    carries = 0
    for r in rec["ctr"]:
        iv, n = H(r["iv"]), r["n"]
        assert sm.aes_cm(H(r["key"]), iv, n) == H(r["out"]) and len(H(r["out"])) == n
        carries += iv[15] + (n + 15) // 16 > 256
    assert carries >= 4, "counters that carry from byte 15 into byte 14"
    for r in rec["hmac"]:
        assert hmac.new(H(r["key"]), H(r["msg"]), hashlib.sha1).digest() == H(r["out"])
        # ... and continued from the two midstates, the form a session keeps the key in
        assert sm.hmac_from_midstates(*sm.hmac_midstates(H(r["key"])), H(r["msg"])) == H(r["out"])


def test_the_record_is_what_openssl_writes_today():
    if shutil.which("openssl") is None:
        pytest.skip("no openssl command line")
    spec = importlib.util.spec_from_file_location("make_srtp_kat", GOLDEN / "make_srtp_kat.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.dumps(mod.make()) == (GOLDEN / "srtp_kat.json").read_text()


def _rfc_estimate(roc, s_l, seq):
    """RFC 3711 appendix A, transcribed"""
    if s_l < 32768:
        if seq - s_l > 32768:
            v = (roc - 1) % (1 << 32)
        else:
            v = roc
    else:
        if s_l - 32768 > seq:
            v = (roc + 1) % (1 << 32)
        else:
            v = roc
    return v


HAND = (((0, 65535, 0), 1), ((1, 2, 65534), 0), ((0, 0, 32768), 0), ((0, 0, 32769), 0xFFFFFFFF), ((5, 32768, 0), 5), ((5, 32769, 0), 6))


def test_index_estimate():
    for args, v in HAND:
        assert sm.estimate(*args) == v, args
    rng = np.random.default_rng(3711)
    edges = [0, 1, 2, 32766, 32767, 32768, 32769, 65534, 65535]
    for roc in (0, 1, 5, 0xFFFFFFFF):
        for s_l in edges + [int(x) for x in rng.integers(0, 65536, 12)]:
            for seq in edges + [(s_l + d) & 0xFFFF for d in (-32769, -32768, -32767, -1, 0, 1, 32767, 32768, 32769)]:
                assert sm.estimate(roc, s_l, seq) == _rfc_estimate(roc, s_l, seq), (roc, s_l, seq)


KEYS = [sm.derive(bytes(range(16 * s, 16 * s + 16)), bytes(range(100 + s, 114 + s))) for s in range(3)]


def _rows():
    rng = np.random.default_rng(5)
    rows = []
    for k, (cc, ext, n) in enumerate(((0, None, 0), (0, None, 1), (1, None, 15), (15, 3, 16), (0, 0, 17), (2, None, 1388), (0, None, 33))):
        rows.append((k % 3, sm.rtp_packet(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 65533 + k, ssrc=0xA0B0C0D0 + k, cc=cc, ext=ext)))
    return rows


def test_protect_then_unprotect_is_the_identity():
    rows = _rows()
    st0 = [(0, 0, 0), (7, 65530, 1), (0, 0, 0)]
    out, st1 = sm.protect(rows, KEYS, st0)
    assert all(len(o) == len(p) + sm.TAG and o[: sm.header_len(p)] == p[: sm.header_len(p)] for o, (_, p) in zip(out, rows))
    assert any(o[sm.header_len(p): len(p)] != p[sm.header_len(p):] for o, (_, p) in zip(out, rows))
    back, status, st2 = sm.unprotect([(s, o) for (s, _), o in zip(rows, out)], KEYS, st0)
    assert status == [0] * len(rows) and back == [p for _, p in rows] and st2 == st1
    # stream 0 took 65533, 0 (wrapped), 3: its index is roc 1, seq 3; stream 1 (roc 7 at 65530) took 65534 and 1; stream 2
    # took 65535 and 2
    assert st1[0] == (1, 3, 1) and st1[1] == (8, 1, 1) and st1[2] == (1, 2, 1)
    # malformed rows: None out, status 2, and they do not touch the state
    bad = [(0, b"\x80" * 11), (1, b"\x40" + bytes(40)), (2, sm.rtp_packet(b"", 1, ext=4)[:-1])]
    assert sm.protect(bad, KEYS, st0) == ([None] * 3, st0)
    assert sm.unprotect([(s, p + bytes(10)) for s, p in bad], KEYS, st0) == ([None] * 3, [2] * 3, st0)
    assert sm.unprotect([(0, sm.rtp_packet(b"", 1) + bytes(9))], KEYS, st0)[1] == [2]


def test_one_flipped_bit_anywhere_fails_the_tag():
    rows = _rows()[3:5]
    st0 = [(0, 100, 1)] * 3
    out, _ = sm.protect(rows, KEYS, st0)
    for k, ((s, _), o) in enumerate(zip(rows, out)):
        shape = 12 + 4 * (o[0] & 15) + (4 if o[0] & 16 else 0)  # up to here a bit may change the header's length
        for bit in range(8 * len(o)):
            d = bytearray(o)
            d[bit // 8] ^= 1 << (bit % 8)
            got, status, st = sm.unprotect([(s, bytes(d))], KEYS, st0)
            # never authentic; a tag that differs wherever the bit leaves the header's shape alone (byte 0 holds CC and X,
            # the extension's length its size: another shape may be malformed instead)
            assert got == [None] and status[0] in (1, 2) and st == st0, (k, bit)
            if 1 <= bit // 8 < 12 or bit // 8 >= shape:
                assert status == [1], (k, bit)
