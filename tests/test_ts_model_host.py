"""tests/ts_model.py pinned on the host: the array forms of the multiplexer and the demultiplexer against their byte-by-byte
restatements, known answers written by hand, the fault catalogue's stated outcomes, dressed input and the packet counts at
the edges of the definition (include/ferhip.h).  No GPU."""
import numpy as np

import nal_split_model as sm
import ts_model as tm
from conftest import golden_bytes

GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]


def _drawn_entries(rng, n):
    out = []
    for k in range(n):
        body = sm.draw(rng, int(rng.integers(1, 900)))
        out.append((tm.SC + bytes([0x65 if k % 3 == 0 else 0x41, 0x88]) + body.tobytes().replace(b"\x00\x00", b"\x00\x07"), 5 if k % 3 == 0 else 1))
    return out


def test_mux_equals_its_serial_form_and_demux_gives_the_units_back():
    for name in GOLDENS:
        stream = golden_bytes(name)
        aus = tm.access_units_of(stream)
        assert len(aus) >= 2 and aus[0][1] == 5
        for with_psi in (False, True):
            h = dict(tm.HDR)
            packets = tm.mux_stream(stream, h, with_psi)
            for (entry, t), pk in zip(aus, packets):
                assert pk == tm.mux_serial(entry, t, h, with_psi), name
                n = len(pk) // 188 - (2 if with_psi and t == 5 else 0)
                assert n == tm.npackets(20 + len(entry))
                assert (pk[:376] == tm.psi(h["pid"], h["pmt_pid"], h["psi_cc"])) == (with_psi and t == 5)
                if with_psi and t == 5:
                    h["psi_cc"] = (h["psi_cc"] + 1) & 15
                h.update(cc=(h["cc"] + n) & 15, pts=(h["pts"] + 3000) & 0x1FFFFFFFF, pcr=(h["pcr"] + 3000) & 0x1FFFFFFFF)
            data = b"".join(packets)
            got = tm.demux(data, tm.HDR["pid"], tm.HDR["cc"])
            assert got == tm.demux_serial(data, tm.HDR["pid"], tm.HDR["cc"]), name
            assert got[1] == 0 and got[2] == h["cc"]
            assert got[0] == b"".join(tm.delimiter(t) + e for e, t in aus)
            units = tm.units_of(got[0])
            assert units == tm.stream_units(stream)
            assert [u for u in units if u[0] != 9] == sm.split(stream), "the delimiters are the only units that were added"
            # a PID that nobody sends: nothing is taken and the expectation stays
            assert tm.demux(data, 0x44, 3) == (b"", 0, 3)


def test_drawn_units():
    rng = np.random.default_rng(7)
    h = dict(tm.HDR)
    data, es = b"", b""
    for entry, t in _drawn_entries(rng, 40):
        pk = tm.mux(entry, t, h, with_psi=True)
        assert pk == tm.mux_serial(entry, t, h, with_psi=True)
        data += pk
        es += tm.delimiter(t) + entry
        h["cc"] = (h["cc"] + tm.npackets(20 + len(entry))) & 15
    got = tm.demux(data, h["pid"], tm.HDR["cc"])
    assert got == tm.demux_serial(data, h["pid"], tm.HDR["cc"]) == (es, 0, h["cc"])


def test_known_answers_by_hand():
    p = tm.psi(0x100, 0x1000, 5)
    pat = bytes.fromhex("47400015" "00" "00B00D0001C100000001F000" "2AB104B2")
    pmt = bytes.fromhex("47500015" "00" "02B0120001C10000E100F0001BE100F000" "15BD4D56")
    assert p == pat + b"\xFF" * (188 - len(pat)) + pmt + b"\xFF" * (188 - len(pmt))
    assert tm.crc32_mpeg(b"123456789") == 0x0376E6E7, "the check value of CRC-32/MPEG-2"
    # packet 0 of a P picture with a payload of 3 bytes: L = 14 + 6 + 5 + 3 = 28, a0 = 155
    entry = tm.SC + bytes([0x21, 0xAA, 0xBB, 0xCC])
    hdr = dict(pts=0x1FFFFFFFF, pcr=0x155555555, pid=0x1ABC, pmt_pid=0x20, cc=9, psi_cc=0)
    want = (bytes.fromhex("475ABC39" "9B" "10" "AAAAAAAAFE00") + b"\xFF" * 148
            + bytes.fromhex("000001E0" "0000" "84" "80" "05" "2FFFFFFFFF") + bytes.fromhex("000000010930") + entry)
    assert len(want) == 188 and tm.mux(entry, 1, hdr) == want == tm.mux_serial(entry, 1, hdr)
    idr = tm.mux(tm.SC + bytes([0x25, 0xAA, 0xBB, 0xCC]), 5, hdr)
    assert idr[5] == 0x50 and idr[-10:-8] == bytes([0x09, 0x10])


def test_packet_counts_at_the_edges():
    want = {25: (1, [158]), 175: (1, [8]), 176: (1, [7]), 177: (2, [7, 182]), 359: (2, [7, 0]), 360: (2, [7, None]), 361: (3, [7, None, 182])}
    for L, (n, fields) in want.items():
        entry = tm.SC + bytes([0x21]) + bytes([0xAB] * (L - 25))
        pk = tm.mux(entry, 1, tm.HDR)
        assert pk == tm.mux_serial(entry, 1, tm.HDR)
        assert len(pk) == 188 * n == 188 * tm.npackets(L), L
        for k, a in enumerate(fields):
            p = pk[188 * k: 188 * (k + 1)]
            assert p[3] == (0x10 if a is None else 0x30) | ((tm.HDR["cc"] + k) & 15), (L, k)
            if a is not None:
                assert p[4] == a and (a == 0 or k == 0 or p[5] == 0) and p[6 if k else 12: 5 + a] == b"\xFF" * (5 + a - (6 if k else 12)), (L, k)
        assert tm.demux(pk, tm.HDR["pid"]) == (tm.delimiter(1) + entry, 0, (tm.HDR["cc"] + n) & 15)


def test_the_catalogue_states_its_faults():
    cat = tm.catalogue()
    names = [c[0] for c in cat]
    assert len(set(names)) == len(names)
    for rule in ("sync_byte", "transport_error", "scrambled", "afc_0", "adaptation_field_leaves_the_packet", "pes_start_code", "stream_id_below",
                 "stream_id_above", "marker_bits", "pes_header_leaves_the_packet", "continuation_with_none_open", "gap", "duplicate"):
        assert rule in names
    for name, data, pid, expect, fault, stands in cat:
        got = tm.demux(data, pid, expect)
        assert got == tm.demux_serial(data, pid, expect), name
        assert got[:2] == (stands, fault) and (got[2] == -1) == (fault != 0), name
    assert {c[4] for c in cat} == {0, tm.MALFORMED, tm.GAP}


def test_dressed_input_decodes_to_the_same_units():
    for name in GOLDENS[::3]:
        stream = golden_bytes(name)
        data, k = tm.dress(tm.access_units_of(stream), 0x100, 5)
        p = np.frombuffer(data, np.uint8).reshape(-1, 188)
        pids = (p[:, 1].astype(int) & 0x1F) << 8 | p[:, 2]
        afc = (p[:, 3] >> 4) & 3
        assert {0x33, 0x1FFF, 0x100} == set(pids.tolist()) and np.any((pids == 0x100) & (afc == 2))
        assert np.any((pids == 0x100) & (afc == 3) & (p[:, 4] == 183)), "a payload-less afc-3 packet"
        assert np.any((pids == 0x100) & (afc == 3) & (p[:, 4] == 9)), "stuffing in a middle packet"
        got = tm.demux(data, 0x100, 5)
        assert got == tm.demux_serial(data, 0x100, 5) and got[1:] == (0, (5 + k) & 15)
        assert tm.units_of(got[0]) == tm.stream_units(stream)
        assert tm.demux(data, 0x100, 6)[1] == tm.GAP
