"""Model of the fragmented MP4 framing (ISO/IEC 14496-12 movie fragments around ISO/IEC 14496-15 samples) as the library
writes it (ferhip_mp4_open / _append / _close / _fetch, ferhip_mp4_blocks, ferhip_write_mp4_init) and as a receiver walks it,
a byte-serial restatement of both directions, dressed input and the fault catalogue.

The definition stands in include/ferhip.h.  Out: a stream's segment is moof (mfhd, traf (tfhd, tfdt, trun)), a free box that
pads the front to D = 104 + 12 K rounded up to 16, and the mdat with the samples back to back.  In: demux() walks a run of
top-level boxes by the rules stated at box_walk() and gives the samples of the fragments that are whole, and a fault:
2 malformed, 3 unsupported, 4 truncated, 1 an overrun of the length walk inside a sample.
"""
import struct

import numpy as np

import avcc_model

IDR_FLAGS, P_FLAGS = 0x02000000, 0x01010000
MATRIX = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)


def u32(x):
    return struct.pack(">I", x & 0xFFFFFFFF)


def box(kind, content=b""):
    kind = kind.encode() if isinstance(kind, str) else kind
    return u32(8 + len(content)) + kind + content


def full(kind, version, flags, content=b""):
    return box(kind, bytes([version]) + flags.to_bytes(3, "big") + content)


def box64(kind, content=b""):
    """the same box with a 64-bit size"""
    kind = kind.encode() if isinstance(kind, str) else kind
    return u32(1) + kind + struct.pack(">Q", 16 + len(content)) + content


def data_offset(K):
    return (104 + 12 * K + 15) & ~15


# ---- out

def segment(samples, is_idr, hdr, K):
    """one stream's closed segment: samples = list of bytes (n >= 1 of them), is_idr[n], hdr = dict(decode_time, sequence,
    duration)"""
    n = len(samples)
    assert 1 <= n <= K
    D = data_offset(K)
    entries = b"".join(u32(hdr["duration"]) + u32(len(p)) + u32(IDR_FLAGS if i else P_FLAGS) for p, i in zip(samples, is_idr))
    trun = full("trun", 0, 0x000701, u32(n) + u32(D) + entries)
    traf = box("traf", full("tfhd", 0, 0x020000, u32(1)) + full("tfdt", 1, 0, struct.pack(">Q", hdr["decode_time"])) + trun)
    moof = box("moof", full("mfhd", 0, 0, u32(hdr["sequence"])) + traf)
    free = box("free", bytes(D - 8 - len(moof) - 8))
    data = b"".join(samples)
    return moof + free + box("mdat", data)


def segment_serial(samples, is_idr, hdr, K):
    """the table of include/ferhip.h, offset by offset"""
    n = len(samples)
    D = 104 + 12 * K
    while D % 16:
        D += 1
    M = sum(len(p) for p in samples)
    out = bytearray(D + M)

    def put(at, *vals):
        for v in vals:
            out[at: at + 4] = v if isinstance(v, bytes) else int(v).to_bytes(4, "big")
            at += 4

    put(0, 88 + 12 * n, b"moof")
    put(8, 0x10, b"mfhd", 0, hdr["sequence"])
    put(24, 64 + 12 * n, b"traf")
    put(32, 0x10, b"tfhd", 0x00020000, 1)
    put(48, 0x14, b"tfdt", 0x01000000, hdr["decode_time"] >> 32, hdr["decode_time"] & 0xFFFFFFFF)
    put(68, 20 + 12 * n, b"trun", 0x00000701, n, D)
    at = D
    for k, p in enumerate(samples):
        put(88 + 12 * k, hdr["duration"], len(p), 0x02000000 if is_idr[k] else 0x01010000)
        for b in p:
            out[at] = b
            at += 1
    put(88 + 12 * n, D - 96 - 12 * n, b"free")
    put(D - 8, 8 + M, b"mdat")
    return bytes(out)


def region(samples, is_idr, hdr, K, stride, fill=0xA5):
    """What ferhip_mp4_blocks and the context calls leave in a region of `stride` bytes pre-filled with `fill`, and the
    index entry (offset excluded): the samples are taken until one does not fit (fault 1) or is number K + 1 (fault 2)
    -> (bytes, (nbytes, nsamples, first type, fault))"""
    D = data_offset(K)
    taken, fault, M = 0, 0, 0
    for p in samples:
        if taken >= K:
            fault = 2
            break
        if D + M + len(p) > stride:
            fault = 1
            break
        M += len(p)
        taken += 1
    out = bytearray([fill]) * stride
    if not taken:
        return bytes(out), (0, 0, 0, fault)
    seg = segment(samples[:taken], is_idr[:taken], hdr, K)
    out[: len(seg)] = seg
    return bytes(out), (len(seg), taken, 5 if is_idr[0] else 1, fault)


def init_segment(sps_unit, pps_unit, dw, dh, timescale):
    """ferhip_write_mp4_init: ftyp + moov of one video track; the units are header byte + escaped payload"""
    avcc = box("avcC", avcc_model.config_record(sps_unit, pps_unit))
    avc1 = box("avc1", bytes(6) + struct.pack(">H", 1) + bytes(16) + struct.pack(">HH", dw, dh) + u32(0x00480000) + u32(0x00480000) + u32(0)
               + struct.pack(">H", 1) + bytes(32) + struct.pack(">HH", 0x0018, 0xFFFF) + avcc)
    stbl = box("stbl", full("stsd", 0, 0, u32(1) + avc1) + full("stts", 0, 0, u32(0)) + full("stsc", 0, 0, u32(0))
               + full("stsz", 0, 0, u32(0) + u32(0)) + full("stco", 0, 0, u32(0)))
    dinf = box("dinf", full("dref", 0, 0, u32(1) + full("url ", 0, 1)))
    minf = box("minf", full("vmhd", 0, 1, bytes(8)) + dinf + stbl)
    mdhd = full("mdhd", 0, 0, u32(0) + u32(0) + u32(timescale) + u32(0) + struct.pack(">HH", 0x55C4, 0))
    hdlr = full("hdlr", 0, 0, u32(0) + b"vide" + bytes(12) + b"\0")
    tkhd = full("tkhd", 0, 3, u32(0) + u32(0) + u32(1) + u32(0) + u32(0) + bytes(8) + bytes(8) + MATRIX + u32(dw << 16) + u32(dh << 16))
    trak = box("trak", tkhd + box("mdia", mdhd + hdlr + minf))
    mvhd = full("mvhd", 0, 0, u32(0) + u32(0) + u32(timescale) + u32(0) + u32(0x00010000) + struct.pack(">H", 0x0100) + bytes(10) + MATRIX
                + bytes(24) + u32(2))
    mvex = box("mvex", full("trex", 0, 0, u32(1) + u32(1) + u32(0) + u32(0) + u32(0)))
    return box("ftyp", b"iso6" + u32(0) + b"iso6cmfcavc1") + box("moov", mvhd + trak + mvex)


CONTAINERS = (b"moov", b"trak", b"mdia", b"minf", b"dinf", b"stbl", b"mvex", b"moof", b"traf")


def check_sizes(data, lo=0, hi=None):
    """every box ends inside its container and every container's size is 8 plus its children -> the number of boxes"""
    hi = len(data) if hi is None else hi
    count, pos = 0, lo
    while pos < hi:
        size, kind = int.from_bytes(data[pos: pos + 4], "big"), bytes(data[pos + 4: pos + 8])
        assert size >= 8 and pos + size <= hi, (kind, pos, size)
        count += 1
        if kind in CONTAINERS:
            count += check_sizes(data, pos + 8, pos + size)
        pos += size
    assert pos == hi
    return count


# ---- in

class _Fault(Exception):
    def __init__(self, code):
        self.code = code


def _box_at(r, pos, hi):
    """The box at r[pos] in a container that ends at hi -> (type, start, header bytes, end).  Fewer than 8 bytes left:
    malformed.  size = the u32, type = the next four bytes, h = 8; size 1: h = 16 (fewer than 16 left: malformed) and size =
    the u64 behind the type; size 0: to the container's end; else size < h or an end beyond the container: malformed."""
    if hi - pos < 8:
        raise _Fault(2)
    size, kind, h = int.from_bytes(r[pos: pos + 4], "big"), bytes(r[pos + 4: pos + 8]), 8
    if size == 1:
        if hi - pos < 16:
            raise _Fault(2)
        size, h = int.from_bytes(r[pos + 8: pos + 16], "big"), 16
    elif size == 0:
        size = hi - pos
    if size < h or pos + size > hi:
        raise _Fault(2)
    return kind, pos, h, pos + size


def box_walk(r, lo, hi):
    """the boxes of the container r[lo, hi); pos advances by size >= 8 at every step"""
    out, pos = [], lo
    while pos < hi:
        out.append(_box_at(r, pos, hi))
        pos = out[-1][3]
    return out


def _tfhd(c):
    """content of a tfhd -> default sample size or None"""
    if len(c) < 8:
        raise _Fault(2)
    flags = int.from_bytes(c[1:4], "big")
    if flags & 1:
        raise _Fault(3)
    p, size = 8, None
    for bit in (0x2, 0x8, 0x10, 0x20):
        if flags & bit:
            if p + 4 > len(c):
                raise _Fault(2)
            if bit == 0x10:
                size = int.from_bytes(c[p: p + 4], "big")
            p += 4
    return size


def _trun(c, first, default_size, moof_at, after, budget):
    """content of a trun -> its samples as (offset in the run, size); budget = how many samples the run may still hold"""
    if len(c) < 8:
        raise _Fault(2)
    if c[0] > 1:
        raise _Fault(3)
    flags, count, p = int.from_bytes(c[1:4], "big"), int.from_bytes(c[4:8], "big"), 8
    at = after
    if flags & 1:
        if p + 4 > len(c):
            raise _Fault(2)
        at = moof_at + int.from_bytes(c[p: p + 4], "big", signed=True)
        p += 4
    elif first:
        raise _Fault(3)
    if flags & 4:
        if p + 4 > len(c):
            raise _Fault(2)
        p += 4
    e = 4 * bin(flags & 0xF00).count("1")
    if count * e > len(c) - p:
        raise _Fault(2)
    if not e and count > max(budget, 0):  # entries of no bytes: the run's samples may then number its bytes at the most
        raise _Fault(2)
    if count and not flags & 0x200 and default_size is None:
        raise _Fault(2)
    out = []
    for k in range(count):
        size = default_size
        if flags & 0x200:
            q = p + k * e + (4 if flags & 0x100 else 0)
            size = int.from_bytes(c[q: q + 4], "big")
        out.append((at, size))
        at += size
    return out, at


def _moof(r, start, h, end, budget):
    track = None
    for kind, st, hh, en in box_walk(r, start + h, end):
        if kind != b"traf":
            continue
        kids = box_walk(r, st + hh, en)
        truns = [k for k in kids if k[0] == b"trun"]
        if not truns:
            continue
        if track is not None:
            raise _Fault(3)
        tf = [k for k in kids if k[0] == b"tfhd"]
        if not tf:
            raise _Fault(2)
        default = _tfhd(r[tf[0][1] + tf[0][2]: tf[0][3]])
        track, after = [], None
        for i, (_, a, b, z) in enumerate(truns):
            got, after = _trun(r[a + b: z], i == 0, default, start, after, budget - len(track))
            track += got
    return track or []


def walk(run):
    """-> (list of (offset, size) of the samples that stand, box fault 0 / 2 / 3 / 4)"""
    r = bytes(run)
    done, pending = [], None
    try:
        # the top level is walked box by box: what stands in front of a malformed header stands
        pos = 0
        while pos < len(r):
            kind, start, h, end = _box_at(r, pos, len(r))
            if kind == b"moof":
                if pending is not None:
                    raise _Fault(4)
                pending = _moof(r, start, h, end, len(r) - len(done))
            elif kind == b"mdat" and pending is not None:
                for at, size in pending:
                    if at < start + h or at + size > end:
                        raise _Fault(2)
                done += pending
                pending = None
            pos = end
        if pending is not None:
            raise _Fault(4)
    except _Fault as f:
        return done, f.code
    return done, 0


def demux(run, L=4):
    """-> (the samples that stand as bytes, fault): the box walk's samples up to and with the first one whose length walk
    overruns; the fault is the box walk's, else 1 for such an overrun"""
    r = bytes(run)
    spans, fault = walk(r)
    samples = [r[a: a + n] for a, n in spans]
    for k, p in enumerate(samples):
        if avcc_model.avcc_split(p, L)[1]:
            return samples[: k + 1], fault or 1
    return samples, fault


def demux_runs(runs, L=4):
    """the runs of one stream in order: the first fault ends the stream's walk"""
    samples, fault = [], 0
    for run in runs:
        got, fault = demux(run, L)
        samples += got
        if fault:
            break
    return samples, fault


def units(run, L=4):
    """what the decoder is handed: (nal_unit_type, nal_ref_idc, RBSP) of every sample's units in order, each sample cut as
    the length-prefixed splitter cuts a range"""
    out = []
    for p in demux(run, L)[0]:
        us, fault = avcc_model.avcc_split(p, L)
        out += [(t, r, b) for _, _, t, r, b in us]
        if fault:  # the first fault ends the stream's walk
            break
    return out


def walk_serial(run):
    """walk() restated with one cursor and explicit byte reads, nothing shared with it but the rules"""
    r = bytes(run)
    n = len(r)

    def rd(at, k):
        assert at + k <= n, "a read beyond the run"
        v = 0
        for b in r[at: at + k]:
            v = v << 8 | b
        return v

    def header(pos, hi):
        """-> (type, header bytes, end) or None"""
        if hi - pos < 8:
            return None
        size, h = rd(pos, 4), 8
        if size == 1:
            if hi - pos < 16:
                return None
            size, h = rd(pos + 8, 8), 16
        if size == 0:
            size = hi - pos
        if size < h or size > hi - pos:
            return None
        return r[pos + 4: pos + 8], h, pos + size

    def sound(lo, hi):
        while lo < hi:
            b = header(lo, hi)
            if b is None:
                return False
            lo = b[2]
        return True

    stand, pend, pos, total = [], None, 0, 0
    while pos < n:
        b = header(pos, n)
        if b is None:
            return stand, 2
        kind, h, end = b
        if kind == b"moof":
            if pend is not None:
                return stand, 4
            if not sound(pos + h, end):
                return stand, 2
            pend, seen, q = [], False, pos + h
            while q < end:
                ck, ch, cend = header(q, end)
                if ck == b"traf":
                    if not sound(q + ch, cend):
                        return stand, 2
                    tf, truns, k = None, [], q + ch
                    while k < cend:
                        kk, kh, kend = header(k, cend)
                        if kk == b"tfhd" and tf is None:
                            tf = (k + kh, kend)
                        if kk == b"trun":
                            truns.append((k + kh, kend))
                        k = kend
                    if truns:
                        if seen:
                            return stand, 3
                        seen = True
                        if tf is None or tf[1] - tf[0] < 8:
                            return stand, 2
                        flags = rd(tf[0] + 1, 3)
                        if flags & 1:
                            return stand, 3
                        at, default = tf[0] + 8, None
                        for bit in (2, 8, 16, 32):
                            if flags & bit:
                                if at + 4 > tf[1]:
                                    return stand, 2
                                if bit == 16:
                                    default = rd(at, 4)
                                at += 4
                        cursor = None
                        for a, z in truns:
                            if z - a < 8:
                                return stand, 2
                            if r[a] > 1:
                                return stand, 3
                            flags, count, at = rd(a + 1, 3), rd(a + 4, 4), a + 8
                            if flags & 1:
                                if at + 4 > z:
                                    return stand, 2
                                off = rd(at, 4)
                                cursor = pos + (off - (1 << 32) if off & 0x80000000 else off)
                                at += 4
                            elif cursor is None:
                                return stand, 3
                            if flags & 4:
                                if at + 4 > z:
                                    return stand, 2
                                at += 4
                            step = sum(4 for bit in (0x100, 0x200, 0x400, 0x800) if flags & bit)
                            if count * step > z - at:
                                return stand, 2
                            if step == 0 and total + len(pend) + count > n:
                                return stand, 2
                            if count and not flags & 0x200 and default is None:
                                return stand, 2
                            for i in range(count):
                                size = rd(at + i * step + (4 if flags & 0x100 else 0), 4) if flags & 0x200 else default
                                pend.append((cursor, size))
                                cursor += size
                q = cend
        elif kind == b"mdat" and pend is not None:
            for a, size in pend:
                if a < pos + h or a + size > end:
                    return stand, 2
            stand += pend
            total += len(pend)
            pend = None
        pos = end
    return (stand, 4) if pend is not None else (stand, 0)


def find_avcc(init):
    """-> (offset, length) of the avcC box's content in an initialisation segment, or None"""
    r = bytes(init)
    try:
        lo, hi = 0, len(r)
        for want in (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stsd"):
            hit = [b for b in box_walk(r, lo, hi) if b[0] == want]
            if not hit:
                return None
            lo, hi = hit[0][1] + hit[0][2], hit[0][3]
        lo += 8  # version, flags, entry_count
        entry = box_walk(r, lo, hi)
        if not entry or entry[0][0] not in (b"avc1", b"avc3"):
            return None
        lo, hi = entry[0][1] + entry[0][2] + 78, entry[0][3]
        if lo > hi:
            return None
        hit = [b for b in box_walk(r, lo, hi) if b[0] == b"avcC"]
        if not hit:
            return None
        return hit[0][1] + hit[0][2], hit[0][3] - hit[0][1] - hit[0][2]
    except _Fault:
        return None


# ---- fragments by hand, dressed input, the fault catalogue

def fragment(samples, seq=1, decode_time=0, split=None, second_offset=True, default_size=False, version=0, cts=False, first_flags=False,
             traf_extra=b"", audio_traf=False, gap=b"", mdat="box", tfhd_flags=0x020000, tfhd_extra=b"", second_traf=False, shift=0,
             sizes=None, trun_cut=0, mdat_cut=0):
    """moof + gap + mdat around the samples, built by parts.  split = k: two truns, the second with or without its own
    data_offset; default_size: the sizes stand in the tfhd; version / cts: trun version 1 with composition offsets; mdat =
    "box", "big" (64-bit size) or "zero" (size 0); shift moves every data_offset; sizes overrides the sizes written;
    trun_cut shortens the trun's box by that many bytes; mdat_cut takes bytes off the mdat's end."""
    sizes = [len(p) for p in samples] if sizes is None else sizes
    data = b"".join(samples)
    mh = 16 if mdat == "big" else 8

    def trun(sz, off):
        flags = (0 if default_size else 0x200) | (0x800 if cts else 0) | (0x4 if first_flags else 0) | (0x1 if off is not None else 0)
        c = u32(len(sz)) + (u32(off) if off is not None else b"") + (u32(IDR_FLAGS) if first_flags else b"")
        for k, s in enumerate(sz):
            c += (b"" if default_size else u32(s)) + (u32(k) if cts else b"")
        b = full("trun", version, flags, c)
        if trun_cut:
            b = u32(len(b) - trun_cut) + b[4: len(b) - trun_cut]
        return b

    def moof(off):
        parts = [sizes] if split is None else [sizes[:split], sizes[split:]]
        truns = trun(parts[0], off)
        if split is not None:
            truns += trun(parts[1], off + sum(parts[0]) if second_offset else None)
        tf = full("tfhd", 0, tfhd_flags | (0x10 if default_size else 0), u32(1) + tfhd_extra + (u32(sizes[0]) if default_size else b""))
        traf = box("traf", tf + full("tfdt", 1, 0, struct.pack(">Q", decode_time)) + traf_extra + truns)
        if audio_traf:
            traf = box("traf", full("tfhd", 0, 0x020000, u32(2)) + full("tfdt", 0, 0, u32(0))) + traf
        if second_traf:
            traf += box("traf", full("tfhd", 0, 0x020000, u32(2)) + trun([1], off))
        return box("moof", full("mfhd", 0, 0, u32(seq)) + traf)

    m = moof(0)
    m = moof(len(m) + len(gap) + mh + shift)
    body = data[: len(data) - mdat_cut] if mdat_cut else data
    md = box64("mdat", body) if mdat == "big" else (u32(0) + b"mdat" + body if mdat == "zero" else box("mdat", body))
    return m + gap + md


EMSG = full("emsg", 0, 0, b"urn:x\0v\0" + u32(1) + u32(0) + u32(0) + u32(7) + b"hello")
SIDX = full("sidx", 0, 0, u32(1) + u32(90000) + u32(0) + u32(0) + u32(0))
STYP = box("styp", b"msdh" + u32(0) + b"msdhmsix")


def dress(fragments):
    """fragments = list of lists of samples -> list of (name, run, the samples that stand): the same samples under every
    legal variation of the boxes around them"""
    flat = [p for f in fragments for p in f]
    plain = [fragment(f, seq=1 + k) for k, f in enumerate(fragments)]
    out = [("plain", b"".join(plain), flat)]
    for name, filler in (("styp", STYP), ("sidx", SIDX), ("free", box("free", bytes(5))), ("emsg", EMSG), ("unknown", box("zzzz", b"\x01\x02\x03"))):
        out.append((name + " between fragments", filler + filler.join(plain) + filler, flat))
        out.append((name + " between moof and mdat", b"".join(fragment(f, gap=filler) for f in fragments), flat))
    out.append(("a 64-bit mdat size", b"".join(fragment(f, mdat="big") for f in fragments), flat))
    out.append(("a 64-bit free size", box64("free", bytes(3)) + b"".join(plain), flat))
    out.append(("a last box of size 0", b"".join(plain[:-1]) + fragment(fragments[-1], mdat="zero"), flat))
    for f in fragments:
        if len(f) >= 2:
            out.append(("two truns, both with a data_offset", fragment(f, split=1), f))
            out.append(("two truns, the second without a data_offset", fragment(f, split=len(f) - 1, second_offset=False), f))
            break
    out.append(("a tfhd default size, truns without sizes", b"".join(fragment([p], default_size=True) for p in flat), flat))
    out.append(("tfhd with every optional field", b"".join(_tfhd_all(f) for f in fragments), flat))
    out.append(("trun version 1 with composition offsets", b"".join(fragment(f, version=1, cts=True) for f in fragments), flat))
    out.append(("first_sample_flags", b"".join(fragment(f, first_flags=True) for f in fragments), flat))
    out.append(("extra children in traf", b"".join(fragment(f, traf_extra=box("sbgp", bytes(8)) + box("uuid", bytes(16))) for f in fragments), flat))
    out.append(("an audio-like traf without a trun", b"".join(fragment(f, audio_traf=True) for f in fragments), flat))
    out.append(("init segment in front", init_segment(b"\x67\x42\x00\x1e\xab", b"\x68\xce\x38\x80", 64, 48, 90000) + b"".join(plain), flat))
    return out


def _tfhd_all(samples):
    """a fragment whose tfhd carries sample_description_index (0x2), default duration (0x8), size (0x10) and flags (0x20),
    with per-sample sizes in the trun all the same: the trun's sizes win"""
    sizes = [len(p) for p in samples]
    data = b"".join(samples)

    def moof(off):
        tf = full("tfhd", 0, 0x02003A, u32(1) + u32(1) + u32(3000) + u32(12345) + u32(P_FLAGS))
        tr = full("trun", 0, 0x201, u32(len(sizes)) + u32(off) + b"".join(u32(s) for s in sizes))
        return box("moof", full("mfhd", 0, 0, u32(9)) + box("traf", tf + tr))

    m = moof(len(moof(0)) + 8)
    return m + box("mdat", data)


def catalogue(L=4):
    """-> list of (name, run, samples that stand, fault): at least one case per rule and fault value"""
    rng = np.random.default_rng(1412)

    def smp(n, hdr=0x41):
        return avcc_model.unit(rng.integers(4, 256, n).astype(np.uint8), L, hdr)

    a, b, c = [smp(40, 0x65), smp(21)], [smp(33), smp(7), smp(19)], [smp(11)]
    fa, fb = fragment(a), fragment(b, seq=2)
    out = []

    def case(name, run, stand, fault):
        out.append((name, bytes(run), list(stand), fault))

    case("clean", fa + fb, a + b, 0)
    case("empty run", b"", [], 0)
    case("a size below 8", fa + u32(7) + b"free" + fb, a, 2)
    case("a size of 1 with fewer than 16 bytes", fa + u32(1) + b"free" + bytes(4), a, 2)
    case("a 64-bit size below 16", fa + u32(1) + b"free" + struct.pack(">Q", 15) + fb, a, 2)
    case("fewer than 8 bytes left", fa + b"\0\0\0", a, 2)
    case("a box beyond the run", fa + u32(4000) + b"free" + fb, a, 2)
    m = bytearray(fb)
    m[24:28] = u32(int.from_bytes(m[24:28], "big") + 4)  # the traf, 4 bytes past the moof's end
    case("a child beyond its parent", fa + bytes(m), a, 2)
    m = bytearray(fb)
    traf_size = int.from_bytes(m[24:28], "big")
    m[32:36] = u32(traf_size)  # the tfhd as large as the whole traf and more
    case("a grandchild beyond its parent", fa + bytes(m), a, 2)
    case("trun entries beyond the trun", fa + fragment(b, seq=2, trun_cut=4), a, 2)
    case("a trun too short for its data_offset", fa + box("moof", box("traf", full("tfhd", 0, 0x020000, u32(1)) + full("trun", 0, 0x201, u32(0))))
         + box("mdat"), a, 2)
    case("a sample beyond the mdat", fa + fragment(b, seq=2, mdat_cut=1), a, 2)
    case("a sample in front of the mdat's content", fa + fragment(b, seq=2, shift=-1), a, 2)
    case("a sample size that reaches beyond the mdat", fa + fragment(b, seq=2, sizes=[33, 7, 0xFFFFFFF0]), a, 2)
    case("a moof without an mdat", fa + fb[: fb.index(b"mdat") - 4], a, 4)
    case("a moof behind a pending moof", fa + fb[: fb.index(b"mdat") - 4] + fragment(c, seq=3), a, 4)
    case("an mdat without a moof is skipped", box("mdat", b"junk") + fa, a, 0)
    case("a base-data-offset flag", fa + fragment(b, seq=2, tfhd_flags=0x000001, tfhd_extra=bytes(8)), a, 3)
    case("a second traf with a trun", fa + fragment(b, seq=2, second_traf=True), a, 3)
    case("a trun of version 2", fa + fragment(b, seq=2, version=2), a, 3)
    nooff = box("moof", box("traf", full("tfhd", 0, 0x020000, u32(1)) + full("trun", 0, 0x200, u32(1) + u32(7)))) + box("mdat", bytes(7))
    case("a first trun without a data_offset", fa + nooff, a, 3)
    nosz = box("moof", box("traf", full("tfhd", 0, 0x020000, u32(1)) + full("trun", 0, 0x001, u32(2) + u32(56)))) + box("mdat", bytes(16))
    case("no sizes anywhere", fa + nosz, a, 2)
    many = box("moof", box("traf", full("tfhd", 0, 0x020010, u32(1) + u32(0)) + full("trun", 0, 0x001, u32(0xFFFFFFFF) + u32(60)))) + box("mdat", bytes(4))
    case("a count without entries beyond what the run may hold", fa + many, a, 2)
    room = len(fa) + 64 - len(a)
    few = box("moof", box("traf", full("tfhd", 0, 0x020010, u32(1) + u32(0)) + full("trun", 0, 0x001, u32(room) + u32(64)))) + box("mdat")
    assert len(fa + few) - len(a) == room and room < 0xFFFF
    case("as many empty samples as the run may hold", fa + few, a + [b""] * room, 0)
    more = few[:50] + (room + 1).to_bytes(2, "big") + few[52:]
    case("one empty sample more", fa + more, a, 2)
    case("traf without a tfhd", fa + box("moof", box("traf", full("trun", 0, 0x201, u32(0) + u32(0)))) + box("mdat"), a, 2)
    case("a tfhd too short for its fields", fa + box("moof", box("traf", full("tfhd", 0, 0x020010, u32(1)) + full("trun", 0, 0x201, u32(0) + u32(0))))
         + box("mdat"), a, 2)
    case("a moof without a track, then its mdat", box("moof", full("mfhd", 0, 0, u32(1))) + box("mdat", b"x") + fa, a, 0)
    case("a sample of size 0", fragment([b""] + a), [b""] + a, 0)
    bad = [smp(12), avcc_model.unit(bytes(9), L)[:-3], smp(5)]  # the middle sample's length reaches 3 bytes beyond it
    case("a length-walk overrun inside a sample", fa + fragment(bad, seq=2), a + bad[:2], 1)
    return out


# ---- the known-answer payloads of the GPU test, and the configurations they run in

KAT_LENGTHS = (0, 1, 2, 3, 15, 16, 17) + tuple(range(4090, 4101)) + (8191, 8192, 8193, 20011)
KAT_CONFIGS = tuple((K, m) for K in (1, 2, 3, 6) for m in range(1, K + 1))


def kat_payloads():
    """payloads dense in 00 00 0x patterns, at the lengths of KAT_LENGTHS, then with a pattern at every phase around the
    seam of two 4096-byte chunks"""
    rng = np.random.default_rng(1449)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 255], np.uint8)
    out = [alphabet[rng.integers(0, alphabet.size, n)] for n in KAT_LENGTHS]
    for x in range(4):
        for at in range(4096 - 4, 4096 + 2):
            p = np.full(4096 + 37 + x, 0xAB, np.uint8)
            p[at: at + 3] = (0, 0, x)
            out.append(p)
    for p in out:
        p.setflags(write=False)
    return out


def sample_of(entry):
    """an Annex-B entry of one unit (00 00 00 01, header byte, escaped payload) -> the same unit behind its 4-byte length"""
    e = bytes(entry)
    assert e[:4] == b"\0\0\0\1"
    return u32(len(e) - 4) + e[4:]


def cursor_phases(sizes, m):
    """the byte phases (mod 16) at which the samples of `sizes`, in segments of m, are written"""
    out = set()
    for g in range(0, len(sizes), m):
        at = 0
        for n in sizes[g: g + m]:
            out.add(at % 16)
            at += n
    return out


def units_of_samples(samples, L=4):
    """the units the decoder is handed of the samples demux() or demux_runs() gives: a sample whose walk overruns is the last"""
    out = []
    for p in samples:
        us, fault = avcc_model.avcc_split(p, L)
        out += [(t, r, b) for _, _, t, r, b in us]
        if fault:
            break
    return out


def cut_runs(data):
    """a stream's bytes cut into runs behind every mdat (a run is a whole number of top-level boxes and of fragments); bytes
    whose top level does not walk stay one run"""
    r = bytes(data)
    try:
        boxes = box_walk(r, 0, len(r))
    except _Fault:
        return [r]
    out, lo = [], 0
    for kind, _, _, end in boxes:
        if kind == b"mdat":
            out.append(r[lo:end])
            lo = end
    if lo < len(r):
        out.append(r[lo:])
    return out
