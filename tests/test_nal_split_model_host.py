"""tests/nal_split_model.py against a byte loop that restates split_stream (csrc/fer_dec_syntax_host.h) line by line, on the
model's whole corpus, and against the framing model: a framed payload splits into exactly that payload."""
import nal_model
import nal_split_model as sm
import numpy as np


def _find_zz(s, frm, n, t0, t1):
    """next i in [frm, n - 2) with s[i] == s[i+1] == 0 and s[i+2] in (t0, t1), or -1"""
    i = frm
    while i + 2 < n:
        if s[i] == 0 and s[i + 1] == 0 and (s[i + 2] == t0 or s[i + 2] == t1):
            return i
        i += 1
    return -1


def split_stream(s):
    """split_stream, statement by statement -> list of (type, ref_idc, rbsp)"""
    n = len(s)
    out = []
    pos = 0
    while True:
        st = -1
        i = pos
        while i + 3 < n:  # 00 00 00 01
            z = _find_zz(s, i, n - 1, 0, 0)
            if z == -1:
                break
            if s[z + 3] == 1:
                st = z + 4
                break
            i = z + 1
        if st == -1:
            break
        en = _find_zz(s, st, n, 0, 1)
        if en == -1:
            en = n
        pos = en
        if en <= st:
            continue
        ref_idc = (s[st] & 0x7F) >> 5
        typ = s[st] & 0x1F
        w = bytearray()
        frm = st + 1
        while True:  # drop the emulation prevention byte of every 00 00 03
            z = _find_zz(s, frm, en, 3, 3)
            if z == -1:
                break
            w += s[frm: z + 2]
            frm = z + 3
        if frm < en:
            w += s[frm:en]
        if not w:
            break
        out.append((typ, ref_idc, bytes(w)))
    return out


def test_model_equals_the_byte_loop_on_the_corpus():
    for k, r in enumerate(sm.corpus()):
        assert sm.split(r) == split_stream(r.tobytes()), f"range {k} ({r.size} bytes)"


def test_model_equals_the_byte_loop_on_drawn_bytes():
    rng = np.random.default_rng(7)
    for k in range(300):
        r = sm.draw(rng, int(rng.integers(0, 400)))
        assert sm.split(r) == split_stream(r.tobytes()), f"draw {k}"


def test_framed_payloads_split_into_themselves():
    for k, (p, t) in enumerate(nal_model.corpus()):
        want = [(t, 1, p.tobytes())] if p.size else []  # a header byte alone is the empty payload that ends a range
        assert sm.split(nal_model.frame_nal(t, p)) == want, f"payload {k} ({p.size} bytes)"
    # ... and back to back (a payload's trailing zeros would join the next start code: those are left out)
    some = [(p, t) for p, t in nal_model.corpus() if 0 < p.size <= 20000 and p[-1] != 0][:64]
    assert len(some) >= 16
    joined = b"".join(nal_model.frame_nal(t, p) for p, t in some)
    assert sm.split(joined) == [(t, 1, p.tobytes()) for p, t in some]


def test_layout_rounds_every_unit_to_16_and_keeps_cut_units_in_the_buffer():
    r = np.array([0, 0, 0, 1, 0x67, 1, 2, 0, 0, 0, 1, 0x68, 0, 0, 0, 1, 0x65, 4, 4, 4], np.uint8)
    units, spans, total = sm.layout([r, r[:7]])
    assert units == [(0, 7, 3, 2, 0), (1, 7, 3, 2, 32)]
    assert spans == [(0, b"\x01\x02"), (16, b""), (16, b"\x04\x04\x04"), (32, b"\x01\x02")] and total == 48


def test_binding_exports_the_headers_prefix_length(pkg):
    import re
    from pathlib import Path
    h = (Path(__file__).resolve().parent.parent / "include" / "ferhip.h").read_text()
    assert int(re.search(r"#define FERHIP_SPLIT_PREFIX (\d+)", h).group(1)) == pkg.SPLIT_PREFIX
    assert pkg.NAL_UNIT.itemsize == 24
