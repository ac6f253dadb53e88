"""Model of the length-prefixed NAL framing of ISO/IEC 14496-15 ("AVCC": MP4, FLV, Matroska samples) as the library writes it
(FERHIP_AU_AVCC, ferhip_write_avcc_config) and reads it (ferhip_decs_set_input, ferhip_split_avcc_blocks), the layout the
device splitter gives its output, and the adversarial ranges that pin both.

The definition (include/ferhip.h).  For a range s[0..n) and a length size L in {1, 2, 4}, start with pos = 0 and repeat while
pos + L <= n: len = the big-endian integer at s[pos..pos+L), st = pos + L, en = st + len; len == 0: the unit is empty;
en > n: it overruns; else the unit is [st, en) with header byte s[st] and the RBSP s[st+1..en) without every s[p] = 03 that
has p - 2 >= st + 1 and s[p-2] = s[p-1] = 0; pos = en.  An empty unit, one with an empty RBSP (len == 1) or an overrunning one
ends the range; an overrun, and fewer than L bytes left over at the end, fault it.
The chain of lengths is walked unit by unit (it is serial by nature); the dropped bytes of a unit are a mask.
"""
import numpy as np

import nal_split_model as sm

CHUNK = 4096  # payload bytes of a unit's 16-byte-aligned image that one workgroup takes (csrc/fer_nalsplit.hip)


def _arr(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)


def annexb_to_avcc(stream, L=4):
    """every unit nal_split_model finds in an Annex-B range (the units behind a header-only one included), each behind its
    length of L bytes; the bytes of a unit -- header byte and escaped payload -- are copied as they are"""
    s = _arr(stream)
    out = bytearray()
    for st, en, _, _, _ in sm.split_raw(s):
        assert en - st < 1 << (8 * L)
        out += int(en - st).to_bytes(L, "big") + s[st:en].tobytes()
    return bytes(out)


def _rbsp(s, st, en):
    """s[st+1..en) without the dropped 03 bytes"""
    seg = s[st + 1: en]
    drop = np.zeros(seg.size, bool)
    if seg.size >= 3:
        drop[2:] = (seg[2:] == 3) & (seg[1:-1] == 0) & (seg[:-2] == 0)
    return seg[~drop].tobytes()


def avcc_split(data, L):
    """-> (units, fault): units = list of (st, en, nal_unit_type, nal_ref_idc, rbsp bytes) in front of the unit that ends the
    range; fault = 1 if the range overran"""
    s = _arr(data)
    n = s.size
    units, pos = [], 0
    while pos + L <= n:
        ln = int.from_bytes(s[pos: pos + L].tobytes(), "big")
        st = pos + L
        en = st + ln
        if ln == 0:
            return units, 0
        if en > n:
            return units, 1
        if ln == 1:
            return units, 0
        units.append((st, en, int(s[st]) & 0x1F, (int(s[st]) & 0x7F) >> 5, _rbsp(s, st, en)))
        pos = en
    return units, int(pos < n)


def split(data, L):
    """-> list of (nal_unit_type, nal_ref_idc, rbsp bytes), as nal_split_model.split gives it for Annex-B"""
    return [(t, r, p) for _, _, t, r, p in avcc_split(data, L)[0]]


def layout(ranges, L):
    """The device splitter's output for a list of ranges -> (units, total, faults): units = the table, a list of (range, type,
    ref_idc, bytes, offset); every unit starts at the next multiple of 16 and total = the buffer's size; faults[r] = 1 where
    range r overran.  The walk stops at the unit that ends a range: nothing behind it is in the table or in the buffer."""
    units, faults, off = [], [], 0
    for r, data in enumerate(ranges):
        us, f = avcc_split(data, L)
        faults.append(f)
        for _, _, t, ref, p in us:
            units.append((r, t, ref, len(p), off))
            off += (len(p) + 15) & ~15
    return units, off, faults


def config_record(sps_nal, pps_nal):
    """AVCDecoderConfigurationRecord for one SPS and one PPS NAL unit (header byte + escaped payload, no start code), 4-byte
    NAL lengths"""
    sps_nal, pps_nal = bytes(sps_nal), bytes(pps_nal)
    rbsp = _rbsp(_arr(sps_nal), 0, len(sps_nal))
    return (bytes([1, rbsp[0], rbsp[1], rbsp[2], 0xFC | 3, 0xE0 | 1]) + len(sps_nal).to_bytes(2, "big") + sps_nal
            + bytes([1]) + len(pps_nal).to_bytes(2, "big") + pps_nal)


def parameter_sets_of(stream):
    """the first SPS and the first PPS unit (header byte + escaped payload) of an Annex-B stream"""
    s = _arr(stream)
    raw = sm.split_raw(s)
    sps = next(s[a:b].tobytes() for a, b, t, _, _ in raw if t == 7)
    pps = next(s[a:b].tobytes() for a, b, t, _, _ in raw if t == 8)
    return sps, pps


def unit(payload, L, hdr=0x65):
    """one length-prefixed unit: the length of L bytes, the header byte, the payload as it is (no escaping)"""
    p = _arr(payload) if isinstance(payload, (bytes, bytearray)) else np.asarray(payload, np.uint8).reshape(-1)
    return (p.size + 1).to_bytes(L, "big") + bytes([hdr]) + p.tobytes()


def _fill(rng, n):
    """n bytes that take part in no pattern"""
    return rng.integers(4, 256, n).astype(np.uint8)


_corpus = {}


def corpus(L):
    """-> list of (name, range as a uint8 array) for length size L; built once per L, never modified by its users.
    L = 1 holds units of up to 255 bytes, L = 2 of up to 65535; only L = 4 holds longer ones."""
    if L in _corpus:
        return _corpus[L]
    rng = np.random.default_rng(20250101 + L)
    big = L >= 2  # units that reach a chunk edge
    out = []

    def add(name, *parts):
        out.append((name, np.frombuffer(b"".join(bytes(p) for p in parts), np.uint8)))

    u = lambda payload, hdr=0x65: unit(np.asarray(payload, np.uint8), L, hdr)
    add("empty_range")
    add("three_units", u([1, 2, 3], 0x67), u([9], 0x68), u(_fill(rng, 40)))
    # the dropped-03 predicate
    add("header_00_then_00_03", u([0, 3, 5, 5], 0x00))                 # p - 2 = st: this 03 stays
    add("header_00_then_00_03_00_00_03", u([0, 3, 0, 0, 3, 1], 0x00))  # ... and the second one goes
    add("drop_twice_in_a_row", u([9, 0, 0, 3, 0, 0, 3, 7]))
    add("00_00_03_03", u([9, 0, 0, 3, 3, 7]))
    add("drop_at_the_unit_end", u([9, 0, 0, 3]), u([7, 7]))
    add("payload_is_00_00_03", u([0, 0, 3]), u([7]))
    add("payload_is_03", u([3]), u([0, 3]), u([0, 0]))
    add("zeros_of_the_next_length_do_not_count", u([5, 0, 0]), u([3, 3, 3], 0x03))
    # start code patterns inside a unit mean nothing
    add("start_codes_inside", u([1, 0, 0, 0, 1, 0x65, 2, 0, 0, 1, 3, 0, 0, 0, 4]), u([8, 0, 0, 1]))
    # what ends a range
    add("zero_length_in_the_middle", u([1, 2]), (0).to_bytes(L, "big"), u([3, 4]))
    add("length_one_in_the_middle", u([1, 2]), (1).to_bytes(L, "big"), bytes([0x68]), u([3, 4]))
    add("length_one_first", (1).to_bytes(L, "big"), bytes([0x68]))
    add("overrun_by_one", u([1, 2], 0x67), (6).to_bytes(L, "big"), bytes([0x65, 1, 2, 3, 4]))
    add("overrun_first_unit", (200).to_bytes(L, "big"), bytes([0x65, 1]))
    if L == 4:
        add("overrun_huge_length", u([1]), bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x65, 1, 2]))
    for k in range(1, L):
        add(f"stray_{k}", u([1, 2, 3]), bytes([0] * k))
        add(f"stray_{k}_alone", bytes([0] * k))
    add("exact_end", u(_fill(rng, 17)), u(_fill(rng, 31)))
    add("all_zero_payload", u(np.zeros(50, np.uint8)))
    # drawn payloads over an alphabet that makes 00 00 03 frequent
    alphabet = np.array([0, 0, 0, 1, 2, 3, 3, 0xFF], np.uint8)
    for k in range(6):
        n = [int(rng.integers(1, 255 if L == 1 else 700)) for _ in range(int(rng.integers(1, 6)))]
        add(f"drawn_{k}", *[u(alphabet[rng.integers(0, alphabet.size, m)], int(rng.integers(0, 256))) for m in n])
    if big:
        # 00 00 03 across a chunk edge of the unit's image at each of its three phases, for every misalignment the test moves
        # the range to: the pattern is laid over a whole window around the payload offsets 4096 - 16 - L - 1 .. 4096 + 2
        for phase in range(3):
            p = _fill(rng, CHUNK + 64)
            for at in range(CHUNK - 24 - L + phase, CHUNK + 3, 3):
                p[at: at + 3] = (0, 0, 3)
            add(f"drops_around_the_first_chunk_edge_{phase}", u([1, 2], 0x67), u(p))
        lens = [CHUNK + 77, 2 * CHUNK + 9] if L == 2 else [CHUNK + 77, 2 * CHUNK + 9, 65535 + 1, 16 * CHUNK + 5]
        for m in lens:  # units that cross one and two (and more) chunk edges, drawn bytes
            add(f"long_unit_{m}", u(_fill(rng, 5), 0x68), u(alphabet[rng.integers(0, alphabet.size, m - 1)]), u([1, 2, 3], 0x41))
        add("long_all_zero", u(np.zeros(CHUNK + 100, np.uint8)))
    for _, r in out:
        r.setflags(write=False)
    _corpus[L] = out
    return out
