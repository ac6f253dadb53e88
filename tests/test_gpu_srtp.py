"""SRTP on the device (ferhip_srtp_*, csrc/fer_srtp.hip) against tests/srtp_model.py, which test_srtp_model_host.py pins to
the published vectors and to the openssl command line.  Every comparison is byte-exact and takes the whole output buffer:
what the model does not place must still hold the fill value.  The known-answer surface (ferhip_srtp_blocks) covers the
lengths, alignments, index cases and faults; the context path and the loop back run an encoder, ferhip_pack_rtp, the
session calls and the live decoder."""
import ctypes as C

import numpy as np
import pytest

import srtp_model as sm

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3
FILL = 0xA5
PROTECT, UNPROTECT = 0, 1

MASTERS = [(bytes((7 * s + k) & 255 for k in range(16)), bytes((201 + 3 * s + k) & 255 for k in range(14))) for s in range(17)]
KEYS = [sm.derive(*m) for m in MASTERS]


def _payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _lay(packets, gap=3, lead=1):
    """the packets one behind the other at any alignment -> (base, [(offset, bytes)])"""
    base, at, where = bytearray(b"\x3C" * lead), lead, []
    for p in packets:
        where.append((at, len(p)))
        base += bytes(p) + b"\x3C" * gap
        at += len(p) + gap
    return bytes(base), where


def _table(pkg, rows, where):
    t = np.zeros(len(rows), pkg.RTP_PKT)
    for k, ((s, _), (off, n)) in enumerate(zip(rows, where)):
        t[k] = (off, n, s)
    return t


def _blocks(pkg, op, rows, states, misalign=0, short=0, n=None, what=""):
    """ferhip_srtp_blocks over rows = [(stream, packet)] against the model: buffer, table, status and state.  short: cap is
    that many bytes less than the total.  -> (the model's packets, status, states)"""
    n = n or len(states)
    if op == PROTECT:
        outs, st = sm.protect(rows, KEYS, states)
        status = [0 if o is not None else 2 for o in outs]
    else:
        outs, status, st = sm.unprotect(rows, KEYS, states)
    total = sm.layout(rows, outs)[0][-1][0]
    cap = total - short if short else total + 48
    table, placed = sm.layout(rows, outs, cap)
    base, where = _lay([p for _, p in rows])
    rc, out, tab, stat, st_out = pkg.srtp_blocks_raw(op, MASTERS[:n], states, base, _table(pkg, rows, where), misalign=misalign, cap=cap, fill=FILL)
    assert rc == 0, what
    want = np.full(max(cap, 1), FILL, np.uint8)
    for off, o in placed:
        want[off: off + len(o)] = np.frombuffer(o, np.uint8)
    assert [tuple(int(v) for v in r) for r in tab] == table, f"{what}: the table"
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])}"
    if op == UNPROTECT:
        assert list(stat) == status, f"{what}: status"
    assert st_out == st, f"{what}: state {st_out}, expected {st}"
    return outs, status, st


def _both(pkg, rows, states, what="", **kw):
    """protect, then unprotect what the model protected; the second gives the first's input back"""
    outs, _, st = _blocks(pkg, PROTECT, rows, states, what=what + " protect", **kw)
    back, status, st2 = _blocks(pkg, UNPROTECT, [(s, o) for (s, _), o in zip(rows, outs) if o is not None], states, what=what + " unprotect", **kw)
    assert back == [p for (_, p), o in zip(rows, outs) if o is not None] and st2 == st
    return outs, st


ST3 = [(0, 1000, 1), (2, 65000, 1), (0xFFFFFFFF, 7, 1)]


def test_every_length_12_to_160(pkg):
    rows = [(L % 3, sm.rtp_packet(_payload(L - 12, L), 1001 + L, ssrc=0xC0DE0000 + L)) for L in range(12, 161)]
    assert [len(p) for _, p in rows] == list(range(12, 161))
    _both(pkg, rows, ST3, "lengths 12..160")


def test_dressed_headers_and_an_empty_payload(pkg):
    rows = []
    for k, (cc, ext) in enumerate(((0, None), (1, None), (15, None), (0, 0), (0, 3), (1, 0), (15, 3))):
        for n in (0, 1, 16, 37):
            rows.append((k % 3, sm.rtp_packet(_payload(n, 100 * k + n), 2000 + len(rows), cc=cc, ext=ext, padding=bool(n & 1))))
    assert {sm.header_len(p) for _, p in rows} == {12, 16, 72, 28, 20, 88} and any(len(p) == sm.header_len(p) for _, p in rows)
    _both(pkg, rows, ST3, "dressed")


@pytest.mark.parametrize("L", (1400, 65525))
def test_long_packets(pkg, L):
    """1400: a datagram of the bench workload, 23 compressions; 65525: the longest SRTP datagram of 65535 bytes, 4095
    keystream blocks for one wavefront and 1025 compressions for one lane"""
    rows = [(1, sm.rtp_packet(_payload(L - 16, L), 65535, cc=1)), (0, sm.rtp_packet(_payload(50, 3), 1001))]
    assert len(rows[0][1]) == L and (L + 4 + 9 + 63) // 64 == {1400: 23, 65525: 1025}[L]
    _both(pkg, rows, ST3, f"L = {L}")


@pytest.mark.parametrize("misalign", range(16))
def test_every_misalignment(pkg, misalign):
    rows = [(k % 3, sm.rtp_packet(_payload(n, n), 999 + k, cc=k % 2, ext=(None, 1)[k % 3 == 0])) for k, n in enumerate((0, 1, 17, 32, 63, 148, 1388))]
    _both(pkg, rows, ST3, f"misalign {misalign}", misalign=misalign)


def test_untouched_bytes_and_caps(pkg):
    rows = [(k % 3, sm.rtp_packet(_payload(n, 7 * n), 999 + k)) for k, n in enumerate((5, 0, 33, 100, 21))]
    for op in (PROTECT, UNPROTECT):
        src = rows if op == PROTECT else [(s, o) for (s, _), o in zip(rows, sm.protect(rows, KEYS, ST3)[0])]
        total = sm.layout(src, (sm.protect if op == PROTECT else sm.unprotect)(src, KEYS, ST3)[0])[0][-1][0]
        last = len(src[-1][1]) + (10 if op == PROTECT else -10)
        tail = ((last + 15) & ~15) - last  # bytes between the last packet's end and the total
        assert tail == (5 if op == PROTECT else 15)
        # a cap that ends in the bytes behind the last packet still holds it; one byte short of its end does not
        _blocks(pkg, op, src, ST3, short=1, what=f"op {op}: the cap within the last slot's tail")
        _blocks(pkg, op, src, ST3, short=tail, what=f"op {op}: the cap at the last packet's end")
        _blocks(pkg, op, src, ST3, short=tail + 1, what=f"op {op}: one byte short of the last packet")
        _blocks(pkg, op, src, ST3, short=total - 1, what=f"op {op}: a cap of one byte")
    # a last packet that fills its slot: a cap one byte short of the total leaves it unwritten, and the table is true
    full = rows[:4] + [(1, sm.rtp_packet(_payload(26, 1), 1003))]
    assert len(full[-1][1]) + 10 == 48
    _blocks(pkg, PROTECT, full, ST3, short=1, what="one byte short of the total")
    # no buffer at all: the table, the status and the state still come
    base, where = _lay([p for _, p in rows])
    lib = pkg.load_library()
    keys, st = pkg.srtp_keys(MASTERS[:3]), np.zeros(3, pkg.SRTP_INDEX)
    tab, st_out = np.zeros(len(rows) + 1, pkg.RTP_PKT), np.zeros(3, pkg.SRTP_INDEX)
    b, t = np.frombuffer(base, np.uint8), _table(pkg, rows, where)
    assert lib.ferhip_srtp_blocks(PROTECT, keys.ctypes.data, st.ctypes.data, 3, b.ctypes.data, b.size, t.ctypes.data, t.size, 0, None, 0,
                                  tab.ctypes.data, None, st_out.ctypes.data) == 0
    want, _ = sm.layout(rows, sm.protect(rows, KEYS, [(0, 0, 0)] * 3)[0], 0)
    assert [tuple(int(v) for v in r) for r in tab] == want and int(tab[-1]["bytes"]) == 0


HAND = (((0, 65535, 0), 1), ((1, 2, 65534), 0), ((0, 0, 32768), 0), ((0, 0, 32769), 0xFFFFFFFF), ((5, 32768, 0), 5), ((5, 32769, 0), 6))


def test_index_estimate_hand_cases_per_stream(pkg):
    states = [(roc, s_l, 1) for (roc, s_l, _), _ in HAND]
    rows = [(s, sm.rtp_packet(_payload(20, s), seq, ssrc=s)) for s, ((_, _, seq), _) in enumerate(HAND)]
    for s, ((roc, s_l, seq), v) in enumerate(HAND):
        assert sm.estimate(roc, s_l, seq) == v
    outs, st = _both(pkg, rows, states, "hand cases")
    # the tag takes v: the packet of stream 0 under roc 1 is not the one under roc 0
    assert outs[0] != sm.protect(rows[:1], KEYS, [(1, 65535, 1)])[0][0]
    # v = roc + 1 lies in front of the state, v = roc - 1 behind it -- except below roc 0, where v is 2^32 - 1
    assert st[0] == (1, 0, 1) and st[1] == (1, 2, 1) and st[3] == (0xFFFFFFFF, 32769, 1) and st[5] == (6, 0, 1)


def test_a_stream_crosses_65535_in_one_call(pkg):
    rows = [(1, sm.rtp_packet(_payload(30 + k, k), 65516 + k)) for k in range(40)]
    assert [int.from_bytes(p[2:4], "big") for _, p in rows][19:21] == [65535, 0]
    outs, st = _both(pkg, rows, [(0, 0, 0), (3, 65515, 1), (9, 9, 1)], "wrap")
    assert st == [(0, 0, 0), (4, 19, 1), (9, 9, 1)], "roc + 1; the streams absent from the table keep their state"
    # the same from a state without an index: s_l is the first seq, 65516
    outs0, st0 = _both(pkg, rows, [(0, 0, 0), (3, 0, 0), (9, 9, 1)], "wrap, set == 0")
    assert st0[1] == (4, 19, 1) and outs0 == outs


def test_set_0_takes_the_first_seq(pkg):
    rows = [(0, b"\x80" * 11), (0, sm.rtp_packet(_payload(9, 1), 40000)), (0, sm.rtp_packet(_payload(9, 2), 100)), (0, sm.rtp_packet(_payload(9, 3), 39999))]
    outs, st = _both(pkg, rows, [(6, 1, 0)], "set == 0", n=1)
    # against s_l = 40000: seq 100 lies in the next period, 39999 in this one; against the state's own s_l = 1 neither would
    assert outs[0] is None and st == [(7, 100, 1)]
    assert sm.estimate(6, 40000, 100) == 7 and sm.estimate(6, 1, 100) == 6


def test_17_streams_interleaved(pkg):
    rng = np.random.default_rng(17)
    seq = [int(x) for x in rng.integers(0, 65536, 17)]
    states = [(s, seq[s], s & 1) for s in range(17)]
    rows = []
    for k in range(17 * 5):
        s = int(rng.integers(0, 17)) if k % 3 else k % 17
        if s == 11:
            continue  # stream 11 is absent
        seq[s] = (seq[s] + 1) & 0xFFFF
        rows.append((s, sm.rtp_packet(_payload(int(rng.integers(0, 200)), k), seq[s], ssrc=0xABCD0000 + s, cc=s % 4)))
    outs, st = _both(pkg, rows, states, "17 streams")
    assert st[11] == states[11] and len({o[-10:] for o in outs}) == len(outs)


def test_unprotect_faults(pkg):
    states = [(0, 500, 1), (0, 500, 1), (0, 500, 1)]
    plain = [(k % 3, sm.rtp_packet(_payload(40 + k, k), 501 + k, cc=1, ext=1)) for k in range(9)]
    good = [(s, o) for (s, _), o in zip(plain, sm.protect(plain, KEYS, states)[0])]
    hl = sm.header_len(plain[0][1])
    assert hl == 24

    def flipped(k, byte, bit=0):
        d = bytearray(good[k][1])
        d[byte] ^= 1 << bit
        return (good[k][0], bytes(d))

    # one bit in the header (the marker bit, a timestamp bit, a CSRC bit), in the payload and in the tag, one after another
    for byte, bit in ((1, 7), (5, 0), (13, 3), (hl, 0), (hl + 17, 6), (len(good[4][1]) - 10, 0), (len(good[4][1]) - 1, 7)):
        rows = good[:4] + [flipped(4, byte, bit)] + good[5:]
        _, status, st = _blocks(pkg, UNPROTECT, rows, states, what=f"bit {bit} of byte {byte}")
        assert status == [0] * 4 + [1] + [0] * 4 and st[1] == (0, 508, 1)
    # the last packet of stream 2 damaged: the state is taken from the authentic rows only
    _, status, st = _blocks(pkg, UNPROTECT, good[:8] + [flipped(8, 30)], states, what="the largest index damaged")
    assert status[8] == 1 and st[2] == (0, 506, 1)
    # under another stream's key; hl + 9 bytes; malformed rows between good ones
    short = sm.rtp_packet(b"", 7, cc=1, ext=1) + bytes(9)
    rows = [good[0], (1, good[0][1]), good[1], (0, short), (2, b"\x80" * 21), good[2], (1, b"\x00" * 60), (2, b"")] + good[3:]
    _, status, st = _blocks(pkg, UNPROTECT, rows, states, what="mixed faults")
    assert status == [0, 1, 0, 2, 2, 0, 2, 2] + [0] * 6 and st == [(0, 507, 1), (0, 508, 1), (0, 509, 1)]
    # a replayed older packet is authentic (there is no replay list) and does not move the state backwards
    _, status, st2 = _blocks(pkg, UNPROTECT, [good[0], good[3]], st, what="replay")
    assert status == [0, 0] and st2 == st


def test_blocks_refusals(pkg):
    lib = pkg.load_library()
    rows = [(0, sm.rtp_packet(b"abc", 1)), (2, sm.rtp_packet(b"defg", 2))]
    base, where = _lay([p for _, p in rows])
    t = _table(pkg, rows, where)
    st = [(0, 0, 0)] * 3
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:3], st, base, t)[0] == 0
    assert pkg.srtp_blocks_raw(2, MASTERS[:3], st, base, t)[0] == E_ARG and pkg.srtp_blocks_raw(-1, MASTERS[:3], st, base, t)[0] == E_ARG
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:2], st[:2], base, t)[0] == E_ARG, "stream >= S"
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:2] + [None], st, base, t)[0] == E_STATE, "a stream without a key"
    assert pkg.srtp_blocks_raw(PROTECT, [None] + MASTERS[1:3], st, base[:-4], t)[0] == E_ARG, "a row that leaves base comes first"
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:2] + [None], st, base, t[:1])[0] == 0, "a stream without a key that no row uses"
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:3], st, base[: where[1][0] + where[1][1] - 1], t)[0] == E_ARG
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:3], st, base, t, misalign=16)[0] == E_ARG
    assert pkg.srtp_blocks_raw(PROTECT, MASTERS[:3], st, base, t, misalign=-1)[0] == E_ARG


# ---- an encoder context, ferhip_pack_rtp and a session
W, H, S = 176, 144, 3
QP = 12
_cache = {}


def _frames(pkg):
    if "frames" not in _cache:
        a = np.stack([np.stack([pkg.gen_frame(W, H, t, 700 + 13 * s, 2) for t in range(3)]) for s in range(S)])
        a.setflags(write=False)
        _cache["frames"] = a
    return _cache["frames"]


def _session(pkg):
    sr = pkg.Srtp(S)
    for s in range(S):
        sr.set_key(s, *MASTERS[s])
    return sr


@pytest.mark.parametrize("P", (96, 1400))
def test_context_path_equals_the_model(pkg, P):
    """ferhip_pack_rtp -> ferhip_srtp_protect_dev on the table where it lies -> ferhip_sync -> copy: the model on
    ferhip_fetch_rtp's packets.  Two pictures, IDR and P: the sequence numbers run through 65535 and the state continues on
    the device without a host write in between."""
    feeds = _frames(pkg)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    sr = _session(pkg)
    assert [sr.get_index(s) for s in range(S)] == [(0, 0, 0)] * S
    cap, pcap = 1 << 19, 1 << 11
    dst, dpk, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
    sdst, sdst2, spk = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (pcap + 1))
    seq = np.array([65533, 65534, 7], np.int64)
    states = [(0, 0, 0)] * S
    for t in range(2):
        g.encode_live([feeds[s][t] for s in range(S)])
        hdr = pkg.rtp_hdr(S, ssrc=0xFACE0000 + np.arange(S), timestamp=3000 * t, seq=seq & 0xFFFF)
        per_stream, idx = g.fetch_rtp(hdr, P, pkg.AU_PARAM_SETS)
        rows = [(s, p) for s in range(S) for p in per_stream[s]]
        g.pack_rtp_device(hdr, P, dst.ptr, cap, dpk.ptr, pcap, dix.ptr, pkg.AU_PARAM_SETS)
        g.sync()
        npk = int(dix.download(dtype=pkg.RTP_AU)["first_pkt"][S])
        assert npk == len(rows) and npk >= (20 if P == 96 else 4)
        outs, want_st = sm.protect(rows, KEYS, states)
        table, placed = sm.layout(rows, outs, cap)
        want = np.full(cap, FILL, np.uint8)
        for off, o in placed:
            want[off: off + len(o)] = np.frombuffer(o, np.uint8)
        # the same call twice from the same state: once with the table on the device, once with it in host memory
        sdst.upload(want * 0 + FILL)
        sr.protect(g, dst.ptr, dpk.ptr, npk, sdst.ptr, cap, spk.ptr)
        g.sync()
        assert np.array_equal(sdst.download(), want), f"picture {t}: device table"
        assert [tuple(int(v) for v in r) for r in spk.download(16 * (npk + 1), dtype=pkg.RTP_PKT)] == table
        assert [sr.get_index(s) for s in range(S)] == want_st
        for s in range(S):
            sr.set_index(s, *states[s])
        sdst2.upload(want * 0 + FILL)
        sr.protect(g, dst.ptr, dpk.download(16 * npk, dtype=pkg.RTP_PKT), npk, sdst2.ptr, cap, spk.ptr)
        g.sync()
        assert np.array_equal(sdst2.download(), want), f"picture {t}: host table"
        assert [sr.get_index(s) for s in range(S)] == want_st
        states = want_st
        seq += idx["npkts"][:S]
    assert states[0][0] == 1 and states[1][0] == 1 and states[2][0] == 0, "streams 0 and 1 wrapped"
    # refusals of the session calls
    lib = pkg.load_library()
    vp = C.c_void_p
    rows_h = dpk.download(16 * npk, dtype=pkg.RTP_PKT)

    def prot(h=sr.h, c=g.ctx, src=dst.ptr, tab=rows_h.ctypes.data, n=npk, d=sdst.ptr, cp=cap, out=spk.ptr, dev=False):
        return (lib.ferhip_srtp_protect_dev if dev else lib.ferhip_srtp_protect)(h, c, vp(src), vp(tab), n, vp(d), cp, vp(out))

    assert prot() == 0 and prot(dev=True, tab=dpk.ptr) == 0
    for kw in (dict(h=None), dict(c=None), dict(src=None), dict(tab=None), dict(d=None), dict(out=None), dict(d=sdst.ptr + 8), dict(out=spk.ptr + 4),
               dict(dev=True, tab=dpk.ptr + 4)):
        assert prot(**kw) == E_ARG, kw
    assert prot(d=None, cp=0) == 0 and prot(n=0, src=None, tab=None) == 0
    bad = rows_h.copy()
    bad["stream"][1] = S
    assert prot(tab=bad.ctypes.data) == E_ARG
    two = pkg.Srtp(S)
    two.set_key(0, *MASTERS[0])
    assert prot(h=two.h) == E_STATE and prot(h=two.h, n=len(per_stream[0])) == 0
    assert lib.ferhip_srtp_set_key(sr.h, S, None, None) == E_ARG and lib.ferhip_srtp_set_index(sr.h, 0, 0, 65536, 1) == E_ARG
    assert lib.ferhip_srtp_set_index(sr.h, 0, 0, 0, 2) == E_ARG and lib.ferhip_srtp_get_index(sr.h, -1, None, None, None) == E_ARG
    g.sync()
    for x in (two, sr, g):
        x.close()


def test_loopback_without_the_bus(pkg):
    """encode -> pack -> protect -> unprotect into a second session with the same master keys -> ferhip_decs_decode_rtp, all
    where the encoder left the bytes; then the same with one packet's tag damaged on the device copy"""
    feeds = _frames(pkg)
    P = 96
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    tx, rx, rx_bad = _session(pkg), _session(pkg), _session(pkg)
    cap, pcap = 1 << 19, 1 << 11
    dst, dpk, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
    sdst, spk, plain = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (pcap + 1)), pkg.DeviceBuffer(cap)
    dec, dec_bad, ref = pkg.LiveDecoder(S, W, H, 1), pkg.LiveDecoder(S, W, H, 1), pkg.LiveDecoder(S, W, H, 1)
    seq = np.full(S, 65500, np.int64)
    for t in range(3):
        g.encode_live([feeds[s][t] for s in range(S)], nal_types=[pkg.NAL_IDR if t != 1 else pkg.NAL_SLICE] * S)
        entries, _ = g.fetch_nal(pkg.AU_PARAM_SETS)
        hdr = pkg.rtp_hdr(S, ssrc=np.arange(S) + 5, timestamp=3000 * t, seq=seq & 0xFFFF)
        g.pack_rtp_device(hdr, P, dst.ptr, cap, dpk.ptr, pcap, dix.ptr, pkg.AU_PARAM_SETS)
        g.sync()
        idx = dix.download(dtype=pkg.RTP_AU)
        npk = int(idx["first_pkt"][S])
        tx.protect(g, dst.ptr, dpk.ptr, npk, sdst.ptr, cap, spk.ptr)
        g.sync()
        srows = spk.download(16 * npk, dtype=pkg.RTP_PKT)
        assert np.array_equal(srows["bytes"], dpk.download(16 * npk, dtype=pkg.RTP_PKT)["bytes"] + 10)
        want, wpics, wst = ref.decode(entries)

        table, status = rx.unprotect(dec, sdst.ptr, srows, plain.ptr, cap, base_on_device=True)
        assert list(status) == [0] * npk and int(table[npk]["bytes"]) == npk
        # the plain packets are the ones ferhip_pack_rtp wrote
        a, b = plain.download(int(table[npk]["offset"])), dst.download(int(idx["offset"][S]))
        for r, q in zip(table[:npk], dpk.download(16 * npk, dtype=pkg.RTP_PKT)):
            assert int(r["bytes"]) == int(q["bytes"]) and np.array_equal(a[int(r["offset"]):][: int(r["bytes"])], b[int(q["offset"]):][: int(q["bytes"])])
        got, pics, st = dec.decode_rtp(plain.ptr, table[:npk], base_on_device=True)
        assert pics == wpics == [1] * S and st == wst == [0] * S and np.array_equal(got, want), f"picture {t}"

        # picture 1: the second packet of stream 1 loses a tag bit on the device
        hit = -1
        if t == 1:
            assert int(idx["npkts"][1]) >= 3
            hit = int(idx["first_pkt"][1]) + 1
            at = int(srows[hit]["offset"]) + int(srows[hit]["bytes"]) - 3
            sdst.upload(sdst.download(1, offset=at) ^ 0x10, offset=at)
        table, status = rx_bad.unprotect(dec_bad, sdst.ptr, srows, plain.ptr, cap, base_on_device=True)
        assert list(status) == [int(k == hit) for k in range(npk)]
        keep = table[:npk][table[:npk]["bytes"] > 0]
        assert keep.size == npk - (t == 1)
        got, pics, st = dec_bad.decode_rtp(plain.ptr, keep, base_on_device=True)
        if t == 1:
            assert st == [0, E_ARG, 0], "the gap is stream 1's"
            assert pics[0] == pics[2] == 1 and np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 2], want[:, 2])
        else:
            assert pics == [1] * S and st == [0] * S and np.array_equal(got, want), f"picture {t}: stream 1 restarts at its IDR"
        seq += idx["npkts"][:S]
    assert int(seq.max()) > 65536 and tx.get_index(0) == rx.get_index(0) and tx.get_index(0)[0] == 1
    # from host memory: one staging copy, the same table, status and bytes
    host = sdst.download(int(spk.download(16 * (npk + 1), dtype=pkg.RTP_PKT)[npk]["offset"]))
    rx2 = _session(pkg)
    for s in range(S):
        rx2.set_index(s, *rx_bad.get_index(s))
    before = plain.download()
    t1, s1 = rx_bad.unprotect(dec_bad, sdst.ptr, srows, plain.ptr, cap, base_on_device=True)
    dev_bytes = plain.download()
    plain.upload(before)
    t2, s2 = rx2.unprotect(dec_bad, host, srows, plain.ptr, cap)
    assert np.array_equal(t1, t2) and np.array_equal(s1, s2) and np.array_equal(plain.download(), dev_bytes)
    # refusals
    lib = pkg.load_library()
    vp = C.c_void_p
    tab, stat = np.zeros(npk + 1, pkg.RTP_PKT), np.zeros(npk, np.int32)

    def unp(h=rx.h, d=dec.h, base=sdst.ptr, on=1, rows=srows.ctypes.data, n=npk, out=plain.ptr, cp=cap, t=tab.ctypes.data, s=stat.ctypes.data):
        return lib.ferhip_srtp_unprotect(h, d, vp(base), on, vp(rows), n, vp(out), cp, vp(t), vp(s))

    assert unp() == 0
    for kw in (dict(h=None), dict(d=None), dict(base=None), dict(rows=None), dict(out=None), dict(t=None), dict(s=None), dict(on=2), dict(out=plain.ptr + 4)):
        assert unp(**kw) == E_ARG, kw
    assert unp(out=None, cp=0) == 0 and unp(n=0, base=None, rows=None, s=None) == 0
    bad = srows.copy()
    bad["stream"][0] = S
    assert unp(rows=bad.ctypes.data) == E_ARG
    nokey = pkg.Srtp(S)
    assert unp(h=nokey.h) == E_STATE
    for x in (nokey, rx2, tx, rx, rx_bad, dec, dec_bad, ref, g):
        x.close()
