"""Model of the RTP payload format of RFC 6184, packetization-mode 1, as the library writes it (ferhip_pack_rtp,
ferhip_fetch_rtp, ferhip_rtp_blocks, ferhip_write_sdp_fmtp) and as a receiver takes it apart, the layout the device packer
gives its output, and the fault catalogue that pins the way in.

Out (include/ferhip.h).  P = the whole datagram with its 12-byte RTP header, B = P - 12, F = B - 2.  A unit is its header
byte h and the payload with its emulation prevention bytes, N bytes.  The parameter sets in front of an access unit go into
one STAP-A packet (0x20 | 24, then a big-endian u16 size and the unit for each); a unit with N <= B is a single-NAL packet;
a longer one becomes n = ceil((N - 1) / F) FU-A packets, packet k = indicator (h & 0xE0) | 28, FU header
S << 7 | E << 6 | (h & 0x1F), unit bytes [1 + k F, 1 + min((k + 1) F, N - 1)).  Every packet starts with 0x80,
M << 7 | payload_type, seq + its index in the access unit, timestamp, ssrc; M only on the last packet.

In, per stream.  State: the expected sequence number (-1 = none) and an open FU-A unit.  Per packet: header (version 2, CSRC
list, extension, padding; what does not fit is malformed), sequence (a mismatch is a gap), payload by type (1..23 one unit, 24
STAP-A, 28 FU-A, else malformed).  A unit still open at the end is truncated.  The first fault ends the walk, the units
completed in front of it stand, the expectation is cleared.  fault: 0 none, 2 malformed, 3 gap, 4 truncated.

packetise / depacketise work on slices of arrays; packetise_serial / depacketise_serial restate them byte by byte.
"""
import base64

import numpy as np

import nal_split_model as sm

MALFORMED, GAP, TRUNCATED = 2, 3, 4
HDR = dict(ssrc=0x11223344, timestamp=0x55667788, seq=65530, payload_type=96)


def _arr(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)


def fragments(N, P):
    """-> the sizes of the packets of a unit of N bytes, RTP header included"""
    B, F = P - 12, P - 14
    if N <= B:
        return [12 + N]
    n = -(-(N - 1) // F)
    return [14 + min(F, N - 1 - k * F) for k in range(n)]


def rtp_header(hdr, k, marker):
    return (bytes([0x80, (0x80 if marker else 0) | hdr["payload_type"]]) + ((hdr["seq"] + k) & 0xFFFF).to_bytes(2, "big")
            + (hdr["timestamp"] & 0xFFFFFFFF).to_bytes(4, "big") + (hdr["ssrc"] & 0xFFFFFFFF).to_bytes(4, "big"))


def packetise(units, P, hdr):
    """the packets of one access unit: units = list of NAL units (header byte + escaped payload); the run of parameter sets
    (types 7 and 8) in front goes into one STAP-A packet, every other unit is a single-NAL packet or FU-A fragments"""
    assert 80 <= P <= 65535
    B, F = P - 12, P - 14
    units = [bytes(u) for u in units]
    nps = 0
    while nps < len(units) and units[nps][0] & 31 in (7, 8):
        nps += 1
    bodies = []
    if nps:
        bodies.append(bytes([0x20 | 24]) + b"".join(len(u).to_bytes(2, "big") + u for u in units[:nps]))
        assert len(bodies[0]) <= B
    for u in units[nps:]:
        N, h = len(u), u[0]
        if N <= B:
            bodies.append(u)
            continue
        a = np.frombuffer(u, np.uint8)
        n = -(-(N - 1) // F)
        for k in range(n):
            fu = (0x80 if k == 0 else 0) | (0x40 if k == n - 1 else 0) | (h & 0x1F)
            bodies.append(bytes([(h & 0xE0) | 28, fu]) + a[1 + k * F: 1 + min((k + 1) * F, N - 1)].tobytes())
    return [rtp_header(hdr, k, k == len(bodies) - 1) + b for k, b in enumerate(bodies)]


def packetise_serial(units, P, hdr):
    """packetise, one byte at a time"""
    B = P - 12
    F = B - 2
    out, cur = [], None

    def begin():
        nonlocal cur
        cur = bytearray([0x80, hdr["payload_type"]])
        seq = (hdr["seq"] + len(out)) % 65536
        cur += bytes([seq >> 8, seq & 255])
        for v in (hdr["timestamp"], hdr["ssrc"]):
            for sh in (24, 16, 8, 0):
                cur.append((v >> sh) & 255)

    def end():
        out.append(cur)

    i = 0
    if units and units[0][0] & 31 in (7, 8):
        begin()
        cur.append(0x38)
        while i < len(units) and units[i][0] & 31 in (7, 8):
            cur += bytes([len(units[i]) >> 8, len(units[i]) & 255])
            for b in units[i]:
                cur.append(b)
            i += 1
        end()
    for u in units[i:]:
        N = len(u)
        begin()
        if N <= B:
            for b in u:
                cur.append(b)
            end()
            continue
        cur += bytes([(u[0] & 0xE0) | 28, 0x80 | (u[0] & 0x1F)])
        room = F
        for e in range(1, N):
            if room == 0:
                end()
                begin()
                cur += bytes([(u[0] & 0xE0) | 28, u[0] & 0x1F])
                room = F
            cur.append(u[e])
            room -= 1
        cur[13] |= 0x40
        end()
    if out:
        out[-1][1] |= 0x80
    return [bytes(p) for p in out]


def _header(p):
    """-> (payload start, payload end, seq) or None for a malformed header"""
    L = len(p)
    if L < 12 or p[0] >> 6 != 2:
        return None
    hl = 12 + 4 * (p[0] & 15)
    if p[0] & 0x10:
        if hl + 4 > L:
            return None
        hl += 4 + 4 * int.from_bytes(p[hl + 2: hl + 4], "big")
        if hl > L:
            return None
    pad = 0
    if p[0] & 0x20:
        pad = p[L - 1]
        if pad < 1:
            return None
    if hl + pad >= L:
        return None
    return hl, L - pad, int.from_bytes(p[2:4], "big")


def depacketise(packets, expect=-1):
    """the packets of one stream in order -> (units, fault, expectation behind the last packet or -1 after a fault)"""
    units, open_unit = [], None
    for p in packets:
        p = bytes(p)
        h = _header(p)
        if h is None:
            return units, MALFORMED, -1
        st, en, seq = h
        if expect >= 0 and seq != expect:
            return units, GAP, -1
        expect = (seq + 1) & 0xFFFF
        pay = p[st:en]
        t = pay[0] & 31
        if open_unit is not None and t != 28:
            return units, MALFORMED, -1
        if 1 <= t <= 23:
            units.append(pay)
        elif t == 24:
            pos = 1
            if pos >= len(pay):
                return units, MALFORMED, -1
            while pos < len(pay):
                if pos + 2 > len(pay):
                    return units, MALFORMED, -1
                size = int.from_bytes(pay[pos: pos + 2], "big")
                if size == 0 or pos + 2 + size > len(pay):
                    return units, MALFORMED, -1
                units.append(pay[pos + 2: pos + 2 + size])
                pos += 2 + size
        elif t == 28:
            if len(pay) < 2:
                return units, MALFORMED, -1
            S, E = pay[1] >> 7, (pay[1] >> 6) & 1
            if (S and E) or (S and open_unit is not None) or (not S and open_unit is None):
                return units, MALFORMED, -1
            if S:
                open_unit = [bytes([(pay[0] & 0xE0) | (pay[1] & 0x1F)])]
            open_unit.append(pay[2:])
            if E:
                units.append(b"".join(open_unit))
                open_unit = None
        else:
            return units, MALFORMED, -1
    if open_unit is not None:
        return units, TRUNCATED, -1
    return units, 0, expect


def depacketise_serial(packets, expect=-1):
    """depacketise, one byte at a time"""
    units, cur = [], None  # cur: the open FU-A unit
    for p in packets:
        L = len(p)
        if L < 12 or (p[0] & 0xC0) != 0x80:
            return units, MALFORMED, -1
        hl = 12
        for _ in range(p[0] & 15):
            hl += 4
        if p[0] & 0x10:
            if hl + 4 > L:
                return units, MALFORMED, -1
            words = p[hl + 2] * 256 + p[hl + 3]
            hl += 4
            for _ in range(words):
                hl += 4
                if hl > L:
                    return units, MALFORMED, -1
        pad = 0
        if p[0] & 0x20:
            pad = p[L - 1]
            if pad == 0:
                return units, MALFORMED, -1
        if hl + pad >= L:
            return units, MALFORMED, -1
        seq = p[2] * 256 + p[3]
        if expect != -1 and seq != expect:
            return units, GAP, -1
        expect = 0 if seq == 65535 else seq + 1
        end = L - pad
        t = p[hl] & 31
        if cur is not None and t != 28:
            return units, MALFORMED, -1
        if t == 0 or (t > 24 and t != 28):
            return units, MALFORMED, -1
        if t < 24:
            u = bytearray()
            for i in range(hl, end):
                u.append(p[i])
            units.append(bytes(u))
        elif t == 24:
            i = hl + 1
            if i == end:
                return units, MALFORMED, -1
            while i < end:
                if end - i < 2:
                    return units, MALFORMED, -1
                size = p[i] * 256 + p[i + 1]
                i += 2
                if size == 0 or size > end - i:
                    return units, MALFORMED, -1
                u = bytearray()
                for _ in range(size):
                    u.append(p[i])
                    i += 1
                units.append(bytes(u))
        else:
            if end - hl < 2:
                return units, MALFORMED, -1
            S, E = p[hl + 1] & 0x80, p[hl + 1] & 0x40
            if S and E:
                return units, MALFORMED, -1
            if S:
                if cur is not None:
                    return units, MALFORMED, -1
                cur = bytearray([(p[hl] & 0xE0) | (p[hl + 1] & 0x1F)])
            elif cur is None:
                return units, MALFORMED, -1
            for i in range(hl + 2, end):
                cur.append(p[i])
            if E:
                units.append(bytes(cur))
                cur = None
    if cur is not None:
        return units, TRUNCATED, -1
    return units, 0, expect


# ---- streams and layout

def access_units_of(stream):
    """an Annex-B stream -> list of access units, each a list of NAL units (header byte + escaped payload, as they stand in
    the stream): the parameter sets in front of a slice belong to its access unit"""
    s = _arr(stream)
    aus, cur = [], []
    for st, en, t, _, _ in sm.split_raw(s):
        cur.append(s[st:en].tobytes())
        if t in (1, 5):
            aus.append(cur)
            cur = []
    assert not cur
    return aus


def packetise_stream(stream, P, hdr=HDR, ts_step=3000):
    """every access unit of an Annex-B stream -> (packets, units); seq runs on, the timestamp steps per access unit"""
    packets, units = [], []
    h = dict(hdr)
    for au in access_units_of(stream):
        pk = packetise(au, P, h)
        packets += pk
        units += au
        h["seq"] = (h["seq"] + len(pk)) & 0xFFFF
        h["timestamp"] = (h["timestamp"] + ts_step) & 0xFFFFFFFF
    return packets, units


def to_avcc(units):
    """the units behind 4-byte lengths: what steps 5 and 6 of the length-prefixed definition take (avcc_model.split)"""
    return b"".join(len(u).to_bytes(4, "big") + bytes(u) for u in units)


def r16(n):
    return (int(n) + 15) & ~15


def layout(per_stream, types):
    """per_stream[s] = the packets of stream s ([] = no picture), types[s] = the slice's NAL unit type -> (buffer as a list
    of (offset, packet), table rows (offset, bytes, stream), index rows (offset, bytes, nal_type, first_pkt, npkts) with the
    last one's `bytes` = the number of streams that are there).  Every packet starts at the next multiple of 16."""
    placed, rows, index, off = [], [], [], 0
    for s, pk in enumerate(per_stream):
        if not pk:
            index.append((0, 0, 0, 0, 0))
            continue
        first, begin = len(rows), off
        for p in pk:
            placed.append((off, p))
            rows.append((off, len(p), s))
            off += r16(len(p))
        index.append((begin, off - begin, types[s], first, len(pk)))
    index.append((off, sum(1 for pk in per_stream if pk), 0, len(rows), 0))
    return placed, rows, index


def sdp_fmtp(sps_unit, pps_unit):
    sps_unit, pps_unit = bytes(sps_unit), bytes(pps_unit)
    a = _arr(sps_unit)
    seg = a[1:]
    drop = np.zeros(seg.size, bool)
    if seg.size >= 3:
        drop[2:] = (seg[2:] == 3) & (seg[1:-1] == 0) & (seg[:-2] == 0)
    rbsp = seg[~drop].tobytes()
    return ("profile-level-id=%02x%02x%02x;packetization-mode=1;sprop-parameter-sets=%s,%s"
            % (rbsp[0], rbsp[1], rbsp[2], base64.b64encode(sps_unit).decode(), base64.b64encode(pps_unit).decode()))


# ---- the fault catalogue

def raw_packet(payload, seq, cc=0, ext=None, pad=0, version=2, marker=0, pt=96, pad_byte=None):
    """a packet by hand: cc CSRC entries, ext = number of extension words (None = no extension), pad padding bytes"""
    b0 = version << 6 | (0x20 if pad or pad_byte is not None else 0) | (0x10 if ext is not None else 0) | cc
    p = bytes([b0, marker << 7 | pt]) + (seq & 0xFFFF).to_bytes(2, "big") + bytes([1, 2, 3, 4, 5, 6, 7, 8])
    p += bytes([0xC5] * (4 * cc))
    if ext is not None:
        p += bytes([0xBE, 0xDE]) + ext.to_bytes(2, "big") + bytes([0xE7] * (4 * ext))
    p += bytes(payload)
    if pad:
        p += bytes([0] * (pad - 1)) + bytes([pad])
    elif pad_byte is not None:
        p += bytes([pad_byte])
    return p


def catalogue():
    """-> list of (name, packets, expect, fault, units in front of the fault).  Every entry begins with two good packets (a
    single-NAL unit, and a STAP-A of two) so that `units in front` is not empty, seq from 65534."""
    u1, u2, u3 = bytes([0x41, 9, 8, 7]), bytes([0x67, 1, 2]), bytes([0x68, 3])
    stap = bytes([0x38]) + len(u2).to_bytes(2, "big") + u2 + len(u3).to_bytes(2, "big") + u3
    good = [raw_packet(u1, 65534), raw_packet(stap, 65535)]
    front = [u1, u2, u3]
    fu = lambda s, e, body, nri=0x60, t=5: bytes([nri | 28, s << 7 | e << 6 | t]) + bytes(body)
    out = []

    def add(name, tail, fault, more=(), expect=65534, keep=3):
        out.append((name, good + list(tail), expect, fault, front[:keep] + list(more)))

    add("short_header", [raw_packet(u1, 0)[:11]], MALFORMED)
    add("version_1", [raw_packet(u1, 0, version=1)], MALFORMED)
    add("csrc_overruns", [raw_packet(b"", 0, cc=3)[:20]], MALFORMED)
    add("csrc_leaves_no_payload", [raw_packet(b"", 0, cc=2)], MALFORMED)
    add("extension_header_overruns", [bytes([0x90]) + raw_packet(b"", 0)[1:12] + bytes([0xBE, 0xDE, 0])], MALFORMED)
    add("extension_overruns", [raw_packet(u1, 0, ext=5)[:24]], MALFORMED)
    add("extension_leaves_no_payload", [raw_packet(b"", 0, ext=1)], MALFORMED)
    add("padding_overruns", [raw_packet(b"", 0, pad_byte=9)], MALFORMED)
    add("padding_leaves_no_payload", [raw_packet(b"", 0, pad=3)], MALFORMED)
    add("pad_byte_0", [raw_packet(u1, 0, pad_byte=0)], MALFORMED)
    add("stap_size_0", [raw_packet(bytes([0x38, 0, 2, 0x67, 1, 0, 0]), 0)], MALFORMED, [bytes([0x67, 1])])
    add("stap_size_overruns", [raw_packet(bytes([0x38, 0, 2, 0x67, 1, 0, 3, 0x68, 1]), 0)], MALFORMED, [bytes([0x67, 1])])
    add("stap_half_a_size", [raw_packet(bytes([0x38, 0, 2, 0x67, 1, 0]), 0)], MALFORMED, [bytes([0x67, 1])])
    add("stap_empty", [raw_packet(bytes([0x38]), 0)], MALFORMED)
    add("fu_s_and_e", [raw_packet(fu(1, 1, [1, 2]), 0)], MALFORMED)
    add("fu_one_byte", [raw_packet(bytes([0x7C]), 0)], MALFORMED)
    add("fu_continuation_without_start", [raw_packet(fu(0, 0, [1, 2]), 0)], MALFORMED)
    add("fu_end_without_start", [raw_packet(fu(0, 1, [1, 2]), 0)], MALFORMED)
    add("fu_start_while_open", [raw_packet(fu(1, 0, [1, 2]), 0), raw_packet(fu(1, 0, [3]), 1)], MALFORMED)
    add("single_inside_open_fu", [raw_packet(fu(1, 0, [1, 2]), 0), raw_packet(u1, 1)], MALFORMED)
    add("stap_inside_open_fu", [raw_packet(fu(1, 0, [1, 2]), 0), raw_packet(stap, 1)], MALFORMED)
    for t in (0, 25, 29):
        add(f"type_{t}", [raw_packet(bytes([0x60 | t, 1, 2]), 0)], MALFORMED)
    add("gap", [raw_packet(u1, 0), raw_packet(u2, 2)], GAP, [u1])
    add("gap_at_the_first_packet", [], GAP, expect=65533, keep=0)
    add("gap_inside_a_fu", [raw_packet(fu(1, 0, [1, 2]), 0), raw_packet(fu(0, 1, [3]), 2)], GAP)
    add("repeated_packet", [raw_packet(u1, 0), raw_packet(u1, 0)], GAP, [u1])
    add("open_unit_at_the_end", [raw_packet(fu(1, 0, [1, 2]), 0), raw_packet(fu(0, 0, [3]), 1)], TRUNCATED)
    add("malformed_header_beats_gap", [raw_packet(u1, 7, version=3)], MALFORMED)
    # good ones: fault 0
    add("good_fu_with_empty_fragments", [raw_packet(fu(1, 0, []), 0), raw_packet(fu(0, 0, [1, 2]), 1), raw_packet(fu(0, 1, []), 2)], 0,
        [bytes([0x65, 1, 2])])
    add("good_no_expectation", [], 0, expect=-1)
    return out
