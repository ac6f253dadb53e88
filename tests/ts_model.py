"""Model of the MPEG-2 transport stream (ISO/IEC 13818-1) as the library writes it (ferhip_pack_ts, ferhip_fetch_ts,
ferhip_ts_blocks, ferhip_write_ts_psi) and as the live decoder takes it apart (ferhip_decs_decode_ts, ferhip_unts_blocks), the
layout the device packer gives its output, and the fault catalogue that pins the way in.  The definitions stand in
include/ferhip.h.

Out.  E = the delimiter 00 00 00 01 09 a (a = 0x10 in front of an IDR slice, else 0x30) + the Annex-B entry.  PES packet =
00 00 01 E0 00 00 84 80 05 + five PTS bytes + E, L bytes.  n = 1 if L <= 176 else 1 + ceil((L - 176) / 184) packets of 188
bytes; packet 0 carries the PCR in an adaptation field of a0 = 7 (L >= 176) or 183 - L bytes behind its length byte and PES
bytes [0, min(L, 176)); packet k >= 1 carries c = min(184, L - 176 - 184 (k - 1)) bytes, right-aligned behind an
adaptation field of 183 - c bytes where c < 184.  With PSI a PAT and a PMT packet stand in front of an I picture.

In, per stream.  State: the expected continuity counter (-1 = none).  Per packet: sync byte and TEI, the PID (another one
is skipped), scrambling, afc (0 malformed, 2 skipped), the counter (a mismatch is a gap), and with PUSI the PES header.  The
first fault ends the walk, the PES packets completed in front of it stand, the open one is dropped, the expectation is
cleared.  fault: 0 none, 2 malformed, 3 gap.  What stands is one Annex-B range (nal_split_model).

mux / demux work on arrays; mux_serial / demux_serial restate them byte by byte.
"""
import numpy as np

import nal_split_model as sm

MALFORMED, GAP = 2, 3
HDR = dict(pts=0x1FFFFFFFF, pcr=0x155555555, pid=0x100, pmt_pid=0x1000, cc=14, psi_cc=15)
SC = b"\x00\x00\x00\x01"


def _arr(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)


# ---- PSI

def crc32_mpeg(data):
    """CRC-32/MPEG-2, bit by bit: polynomial 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final xor"""
    c = 0xFFFFFFFF
    for byte in bytes(data):
        for bit in range(7, -1, -1):
            top = (c >> 31) ^ ((byte >> bit) & 1)
            c = (c << 1) & 0xFFFFFFFF
            if top:
                c ^= 0x04C11DB7
    return c


def _psi_packet(pid, cc, section):
    p = bytes([0x47, 0x40 | pid >> 8, pid & 0xFF, 0x10 | cc, 0x00]) + section + crc32_mpeg(section).to_bytes(4, "big")
    return p + b"\xFF" * (188 - len(p))


def psi(pid, pmt_pid, cc):
    """the PAT and the PMT packet of a single-program stream whose video has PID pid: 376 bytes"""
    pat = bytes([0x00, 0xB0, 0x0D, 0x00, 0x01, 0xC1, 0x00, 0x00, 0x00, 0x01, 0xE0 | pmt_pid >> 8, pmt_pid & 0xFF])
    es = bytes([0xE0 | pid >> 8, pid & 0xFF])
    pmt = bytes([0x02, 0xB0, 0x12, 0x00, 0x01, 0xC1, 0x00, 0x00]) + es + bytes([0xF0, 0x00, 0x1B]) + es + bytes([0xF0, 0x00])
    return _psi_packet(0, cc, pat) + _psi_packet(pmt_pid, cc, pmt)


# ---- out

def pts_bytes(pts, marker=0x21):
    return bytes([marker | ((pts >> 29) & 0x0E), (pts >> 22) & 0xFF, 0x01 | ((pts >> 14) & 0xFE), (pts >> 7) & 0xFF, 0x01 | ((pts << 1) & 0xFE)])


def pcr_bytes(pcr):
    return bytes([(pcr >> 25) & 0xFF, (pcr >> 17) & 0xFF, (pcr >> 9) & 0xFF, (pcr >> 1) & 0xFF, ((pcr & 1) << 7) | 0x7E, 0x00])


def delimiter(nal_type):
    return SC + bytes([0x09, 0x10 if nal_type == 5 else 0x30])


def pes_packet(entry, nal_type, pts):
    """entry: the Annex-B bytes ferhip_pack_nal writes for the stream (parameter sets included where asked for)"""
    return bytes([0, 0, 1, 0xE0, 0, 0, 0x84, 0x80, 0x05]) + pts_bytes(pts) + delimiter(nal_type) + bytes(entry)


def npackets(L):
    return 1 if L <= 176 else 1 + -(-(L - 176) // 184)


def mux(entry, nal_type, hdr, with_psi=False):
    """one access unit -> its packets as one bytes: every PES byte scattered to its place at once"""
    pes = _arr(pes_packet(entry, nal_type, hdr["pts"]))
    L = pes.size
    n = npackets(L)
    out = np.full((n, 188), 0xFF, np.uint8)
    k = np.arange(n)
    c = np.minimum(184, L - 176 - 184 * (k - 1))  # PES bytes of packet k >= 1
    c[0] = min(L, 176)
    start = 188 - c
    start[0] = 12 if L >= 176 else 188 - L
    out[:, 0] = 0x47
    out[:, 1] = hdr["pid"] >> 8
    out[0, 1] |= 0x40
    out[:, 2] = hdr["pid"] & 0xFF
    out[:, 3] = np.where(start > 4, 0x30, 0x10) | ((hdr["cc"] + k) & 15)
    af = start > 4
    out[af, 4] = (start - 5)[af]
    out[af & (start > 5), 5] = 0x00
    out[0, 5] = 0x10 | (0x40 if nal_type == 5 else 0)
    out[0, 6:12] = _arr(pcr_bytes(hdr["pcr"]))
    x = np.arange(L)
    pk = np.where(x < 176, 0, 1 + (x - 176) // 184) if n > 1 else np.zeros(L, np.int64)
    first = np.where(pk == 0, 0, 176 + 184 * (pk - 1))
    out.reshape(-1)[188 * pk + start[pk] + (x - first)] = pes
    body = out.tobytes()
    return (psi(hdr["pid"], hdr["pmt_pid"], hdr["psi_cc"]) if with_psi and nal_type == 5 else b"") + body


def mux_serial(entry, nal_type, hdr, with_psi=False):
    """mux, one byte at a time"""
    pes = pes_packet(entry, nal_type, hdr["pts"])
    L = len(pes)
    out = bytearray()
    if with_psi and nal_type == 5:
        out += psi(hdr["pid"], hdr["pmt_pid"], hdr["psi_cc"])
    x, k = 0, 0
    while x < L:
        left = L - x
        out += bytes([0x47, (0x40 if k == 0 else 0) | hdr["pid"] >> 8, hdr["pid"] & 0xFF])
        cc = (hdr["cc"] + k) % 16
        if k == 0:
            room = 176
            stuffing = room - left if left < room else 0
            out.append(0x30 | cc)
            out.append(7 + stuffing)
            out.append(0x50 if nal_type == 5 else 0x10)
            out += pcr_bytes(hdr["pcr"])
            for _ in range(stuffing):
                out.append(0xFF)
        elif left >= 184:
            room = 184
            out.append(0x10 | cc)
        else:
            room = left
            out.append(0x30 | cc)
            out.append(183 - left)
            if 183 - left >= 1:
                out.append(0x00)
                for _ in range(182 - left):
                    out.append(0xFF)
        for _ in range(min(room, left)):
            out.append(pes[x])
            x += 1
        assert len(out) % 188 == 0
        k += 1
    return bytes(out)


# ---- in

def demux(data, pid, expect=-1):
    """the packets of one stream's runs, concatenated -> (the elementary-stream bytes that stand, fault, the expectation it
    leaves).  Every packet is classified at once; the counter, the open PES packet and the first fault follow from the
    arrays."""
    a = _arr(data)
    assert a.size % 188 == 0
    p = a.reshape(-1, 188).astype(np.int64)
    n = p.shape[0]
    if n == 0:
        return b"", 0, expect
    bad = (p[:, 0] != 0x47) | ((p[:, 1] & 0x80) != 0)
    mine = ((p[:, 1] & 0x1F) << 8 | p[:, 2]) == pid
    afc = (p[:, 3] >> 4) & 3
    bad |= mine & (((p[:, 3] >> 6) != 0) | (afc == 0) | ((afc == 3) & (p[:, 4] > 183)))
    pay = mine & ~bad & (afc != 2)
    at = np.where(afc == 3, 5 + p[:, 4], 4)  # where the payload begins
    pusi = pay & ((p[:, 1] & 0x40) != 0)
    room = 188 - at
    rows = np.arange(n)

    def byte(i):
        return p[rows, np.minimum(at + i, 187)]

    pes_ok = (room >= 9) & (byte(0) == 0) & (byte(1) == 0) & (byte(2) == 1) & ((byte(3) & 0xF0) == 0xE0) & ((byte(6) & 0xC0) == 0x80)
    pes_ok &= room >= 9 + byte(8)
    es_at = np.where(pusi, at + 9 + byte(8), at)
    # the counter: every payload packet against the one in front of it, the first against the expectation
    cc = p[:, 3] & 15
    idx = np.flatnonzero(pay)
    gap = np.zeros(n, bool)
    if idx.size:
        want = np.concatenate(([expect], (cc[idx[:-1]] + 1) & 15))
        gap[idx] = (want >= 0) & (cc[idx] != want)
    opened = np.cumsum(pusi) > 0  # a PES packet has begun at or in front of this packet
    fault = np.where(bad, MALFORMED, np.where(gap, GAP, np.where(pay & ((pusi & ~pes_ok) | (~pusi & ~opened)), MALFORMED, 0)))
    hit = np.flatnonzero(fault)
    end = int(hit[0]) if hit.size else n
    keep = pay.copy()
    keep[end:] = False
    if hit.size:
        starts = np.flatnonzero(pusi[:end])
        if starts.size:
            keep[starts[-1]:] = False  # the open PES packet is dropped
    es = b"".join(a[188 * k + es_at[k]: 188 * (k + 1)].tobytes() for k in np.flatnonzero(keep))
    if hit.size:
        return es, int(fault[end]), -1
    return es, 0, int((cc[idx[-1]] + 1) & 15) if idx.size else expect


def demux_serial(data, pid, expect=-1):
    """demux, packet by packet and byte by byte"""
    data = bytes(data)
    done, cur = bytearray(), None
    for o in range(0, len(data), 188):
        p = data[o: o + 188]
        if p[0] != 0x47 or p[1] & 0x80:
            return bytes(done), MALFORMED, -1
        if ((p[1] & 0x1F) << 8 | p[2]) != pid:
            continue
        if p[3] >> 6:
            return bytes(done), MALFORMED, -1
        afc = (p[3] >> 4) & 3
        if afc == 0:
            return bytes(done), MALFORMED, -1
        if afc == 2:
            continue
        at = 4
        if afc == 3:
            if p[4] > 183:
                return bytes(done), MALFORMED, -1
            at = 5 + p[4]
        if expect >= 0 and (p[3] & 15) != expect:
            return bytes(done), GAP, -1
        expect = ((p[3] & 15) + 1) % 16
        q = p[at:]
        if p[1] & 0x40:
            if len(q) < 9 or q[0:3] != b"\x00\x00\x01" or not 0xE0 <= q[3] <= 0xEF or q[6] & 0xC0 != 0x80 or len(q) < 9 + q[8]:
                return bytes(done), MALFORMED, -1
            if cur is not None:
                done += cur
            cur = bytearray()
            for b in q[9 + q[8]:]:
                cur.append(b)
        else:
            if cur is None:
                return bytes(done), MALFORMED, -1
            for b in q:
                cur.append(b)
    if cur is not None:
        done += cur
    return bytes(done), 0, expect


def units_of(es):
    """the elementary-stream bytes that stand -> list of (nal_unit_type, nal_ref_idc, RBSP): the Annex-B splitter's"""
    return sm.split(es)


# ---- streams and layout

def access_units_of(stream):
    """an Annex-B stream -> list of (entry, nal_type): the parameter sets in front of a slice belong to its entry"""
    s = _arr(stream)
    aus, begin = [], None
    for st, en, t, _, _ in sm.split_raw(s):
        if begin is None:
            begin = st - 4
        if t in (1, 5):
            aus.append((s[begin:en].tobytes(), t))
            begin = None
    assert begin is None
    return aus


def mux_stream(stream, hdr=HDR, with_psi=False, pts_step=3000):
    """every access unit of an Annex-B stream -> the packets of each as one bytes, in a list; cc, psi_cc, pts and pcr run on"""
    h = dict(hdr)
    out = []
    for entry, t in access_units_of(stream):
        out.append(mux(entry, t, h, with_psi))
        n = len(out[-1]) // 188
        if with_psi and t == 5:
            n -= 2
            h["psi_cc"] = (h["psi_cc"] + 1) & 15
        h["cc"] = (h["cc"] + n) & 15
        h["pts"] = (h["pts"] + pts_step) & 0x1FFFFFFFF
        h["pcr"] = (h["pcr"] + pts_step) & 0x1FFFFFFFF
    return out


def stream_units(stream):
    """what the decoder sees of an Annex-B stream behind the multiplexer: a delimiter in front of every access unit"""
    return units_of(b"".join(delimiter(t) + e for e, t in access_units_of(stream)))


def r16(n):
    return (int(n) + 15) & ~15


def layout(per_stream, types):
    """per_stream[s] = the packets of stream s as one bytes (b"" = no picture), types[s] = the slice's NAL unit type ->
    index rows (offset, bytes, nal_type, npkts, 0) with the last one = (total, streams that are there, 0, packets, 0)"""
    index, off, npk = [], 0, 0
    for s, pk in enumerate(per_stream):
        if not pk:
            index.append((0, 0, 0, 0, 0))
            continue
        index.append((off, len(pk), types[s], len(pk) // 188, 0))
        off += r16(len(pk))
        npk += len(pk) // 188
    index.append((off, sum(1 for pk in per_stream if pk), 0, npk, 0))
    return index


# ---- packets by hand, dressed input, the fault catalogue

def ts_packet(pid, cc, payload=b"", pusi=0, adapt=None, afc=None, sync=0x47, tei=0, scramble=0, fill=0xFF):
    """a packet by hand.  adapt None: the adaptation field is whatever right-aligns the payload (none for 184 bytes);
    adapt = n: a field of n bytes behind its length byte, the payload then fills the rest (and must).  afc overrides the
    two bits."""
    payload = bytes(payload)
    if adapt is None:
        adapt = 183 - len(payload) if len(payload) < 184 else None
    body = b""
    if adapt is not None:
        body = bytes([adapt]) + (bytes([0x00]) + bytes([fill]) * (adapt - 1) if adapt else b"")
    bits = afc if afc is not None else (3 if adapt is not None else 1)
    p = bytes([sync, tei << 7 | pusi << 6 | pid >> 8, pid & 0xFF, scramble << 6 | bits << 4 | (cc & 15)]) + body + payload
    assert len(p) <= 188
    return p + bytes([fill]) * (188 - len(p))


def pes_header(pts=0, dts=None, stream_id=0xE0):
    """9 + 5 bytes, or the 19-byte form with a DTS"""
    if dts is None:
        return bytes([0, 0, 1, stream_id, 0, 0, 0x84, 0x80, 5]) + pts_bytes(pts)
    return bytes([0, 0, 1, stream_id, 0, 0, 0x84, 0xC0, 10]) + pts_bytes(pts, 0x31) + pts_bytes(dts, 0x11)


def packets_of(pes, pid, cc, mid_stuffing=0):
    """a PES packet cut into packets another way than mux does: 184 bytes each from the front, or with mid_stuffing bytes
    of adaptation field in every packet; the last one right-aligned -> list of packets"""
    out, x, k = [], 0, 0
    room = 184 - (1 + mid_stuffing if mid_stuffing else 0)
    while x < len(pes):
        c = min(room, len(pes) - x)
        full = c == room
        out.append(ts_packet(pid, cc + k, pes[x: x + c], pusi=int(k == 0), adapt=(mid_stuffing or None) if full else None))
        x += c
        k += 1
    return out


def dress(access_units, pid, cc, other_pid=0x33):
    """access units [(entry, nal_type)] -> (packets as one bytes, payload packets): foreign PIDs, null packets and afc-2
    packets in between, a 19-byte PES header with a DTS, adaptation-field stuffing in middle packets, and a payload-less
    afc-3 packet (which counts) in every access unit"""
    out, k = [], 0
    for i, (entry, t) in enumerate(access_units):
        pes = pes_header(90000 + 3000 * i, 87000 + 3000 * i) + delimiter(t) + entry
        pk = packets_of(pes, pid, 0, mid_stuffing=(9, 0, 40)[i % 3])
        pk.insert(1 + (len(pk) > 2), ts_packet(pid, 0, b"", adapt=183))  # no payload, but afc 3: the counter counts it
        for p in pk:
            q = bytearray(p)
            q[3] = (q[3] & 0xF0) | ((cc + k) & 15)
            k += 1
            out.append(bytes(q))
            out.append(ts_packet(other_pid, 7 * k, b"\x11" * 184))                     # another PID, any counter
            if k % 3 == 0:
                out.append(ts_packet(0x1FFF, 0, b"\xFF" * 184))                        # a null packet
            if k % 4 == 0:
                out.append(ts_packet(pid, 9, b"", adapt=183, afc=2))                   # adaptation field only: not counted
            if k % 5 == 0:
                out.append(ts_packet(other_pid, 0, b"\x22" * 184, scramble=2, sync=0x47))  # not looked at beyond its PID
    return b"".join(out), k


def catalogue():
    """-> list of (name, packets as one bytes, pid, expect, fault, the elementary-stream bytes that stand).  Every entry but
    two begins with a good access unit in two packets (counters 15 and 0) and the first packet of a second one (counter 1),
    so that one PES packet stands in front of the fault and one is open at it."""
    pid = 0x100
    u1 = SC + bytes([0x09, 0x30]) + SC + bytes([0x41, 9, 8, 7] * 60)
    u2 = SC + bytes([0x09, 0x30]) + SC + bytes([0x41, 1, 2, 3])
    u3 = SC + bytes([0x09, 0x30]) + SC + bytes([0x41, 4, 5, 6, 7])
    begin = lambda cc, es=u2, **kw: ts_packet(pid, cc, pes_header(2) + es, pusi=1, **kw)
    cont = lambda cc, **kw: ts_packet(pid, cc, bytes([0x55] * 100), **kw)
    good = packets_of(pes_header(1) + u1, pid, 15) + [begin(1)]
    assert len(good) == 3
    h = pes_header(2)
    out = []

    def add(name, tail, fault, stands=u1, expect=15, front=True):
        out.append((name, b"".join((good if front else []) + list(tail)), pid, expect, fault, stands))

    add("sync_byte", [cont(2, sync=0x48)], MALFORMED)
    add("sync_byte_of_another_pid", [ts_packet(0x33, 0, b"\x00" * 184, sync=0x46)], MALFORMED)
    add("transport_error", [cont(2, tei=1)], MALFORMED)
    add("scrambled", [cont(2, scramble=1)], MALFORMED)
    add("afc_0", [cont(2, afc=0)], MALFORMED)
    add("adaptation_field_leaves_the_packet", [bytes([0x47, pid >> 8, pid & 0xFF, 0x32, 184]) + b"\xFF" * 183], MALFORMED)
    add("pes_start_code", [ts_packet(pid, 2, bytes([0, 0, 2]) + h[3:] + u3, pusi=1)], MALFORMED)
    add("stream_id_below", [ts_packet(pid, 2, pes_header(2, stream_id=0xDF) + u3, pusi=1)], MALFORMED)
    add("stream_id_above", [ts_packet(pid, 2, pes_header(2, stream_id=0xF0) + u3, pusi=1)], MALFORMED)
    add("marker_bits", [ts_packet(pid, 2, h[:6] + bytes([0x44]) + h[7:] + u3, pusi=1)], MALFORMED)
    add("pes_header_leaves_the_packet", [ts_packet(pid, 2, h[:8] + bytes([6]) + h[9:], pusi=1)], MALFORMED)
    add("pes_header_cut", [ts_packet(pid, 2, h[:8], pusi=1)], MALFORMED)
    add("continuation_with_none_open", [cont(15)], MALFORMED, stands=b"", expect=-1, front=False)
    add("gap", [cont(3)], GAP)
    add("gap_at_the_first_packet", [], GAP, stands=b"", expect=14)
    add("gap_at_a_pusi_packet", [begin(3, es=u3)], GAP)
    add("duplicate", [begin(1)], GAP)
    add("duplicate_continuation", [cont(2), cont(2)], GAP)
    add("malformed_beats_gap", [cont(7, tei=1)], MALFORMED)
    add("gap_beats_a_bad_pes_header", [ts_packet(pid, 7, pes_header(2, stream_id=0xBD) + u3, pusi=1)], GAP)
    add("fault_in_a_later_access_unit", [begin(2, es=u3), cont(3), cont(5)], GAP, stands=u1 + u2)
    # good ones: fault 0
    add("good_two_access_units", [], 0, stands=u1 + u2)
    add("good_no_expectation", [ts_packet(pid, 2, b"", adapt=183)], 0, stands=u1 + u2, expect=-1)
    add("good_wrap", [cont(c) for c in range(2, 20)], 0, stands=u1 + u2 + bytes([0x55] * 1800))
    return out
