"""NumPy model of the decoder's Annex-B splitter (split_stream, csrc/fer_dec_syntax_host.h) as a set of local predicates, the
layout the device splitter (csrc/fer_nalsplit.hip) gives its output, and the corpus that pins both.

For a range s[0..n):
  a unit begins at st = z + 4 for every z with s[z..z+3] = 00 00 00 01 and z + 3 < n, in order;
  it ends at en = the smallest i >= st with s[i] = s[i+1] = 0, s[i+2] in {0, 1} and i + 2 < n, else at n;
  en <= st is no unit; the header byte is s[st]; the payload is s[st+1..en) without every s[p] = 03 with p - 2 >= st + 1 and
  s[p-2] = s[p-1] = 0; a unit with an empty payload ends the range: it and everything behind it are dropped.
Flags are computed for all bytes at once, ends by searchsorted, dropped bytes by a mask.
"""
import numpy as np

CHUNK = 4096  # bytes of a range's 16-byte-aligned image that one workgroup takes


def _flags(s):
    """-> (code [n] bool: 00 00 00 01 begins here, term [n] bool: a terminator begins here, drop03 [n] bool: 03 behind two zeros)"""
    n = s.size
    z = s == 0
    code = np.zeros(n, bool)
    term = np.zeros(n, bool)
    drop = np.zeros(n, bool)
    if n >= 4:
        code[: n - 3] = z[: n - 3] & z[1: n - 2] & z[2: n - 1] & (s[3:] == 1)
    if n >= 3:
        term[: n - 2] = z[: n - 2] & z[1: n - 1] & (s[2:] <= 1)
        drop[2:] = (s[2:] == 3) & z[1: n - 1] & z[: n - 2]
    return code, term, drop


def split_raw(data):
    """every unit of the range that is not empty, before the empty-payload cut -> list of (st, en, type, ref_idc, rbsp bytes)"""
    s = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    n = s.size
    code, term, drop = _flags(s)
    st = np.flatnonzero(code) + 4
    tpos = np.flatnonzero(term)
    k = np.searchsorted(tpos, st, "left")
    en = np.where(k < tpos.size, tpos[np.minimum(k, max(tpos.size - 1, 0))] if tpos.size else n, n)
    ok = en > st
    st, en = st[ok], en[ok]
    # the header byte never counts as a zero of the pattern: p - 2 = st leaves the 03 in place (p - 1 = st cannot match,
    # the byte in front of st is the 01 of the start code)
    p = st + 2
    drop[p[p < n]] = False
    out = []
    for a, b in zip(st.tolist(), en.tolist()):
        seg = s[a + 1: b]
        out.append((a, b, int(s[a]) & 0x1F, (int(s[a]) & 0x7F) >> 5, seg[~drop[a + 1: b]].tobytes()))
    return out


def split(data):
    """-> list of (nal_unit_type, nal_ref_idc, rbsp bytes): what split_stream leaves in its output"""
    out = []
    for _, _, t, r, p in split_raw(data):
        if not p:
            break
        out.append((t, r, p))
    return out


def layout(ranges):
    """The device splitter's output for a list of ranges -> (units, spans, total): units = the table after the cut, a list of
    (range, type, ref_idc, bytes, offset); spans = (offset, rbsp bytes) of EVERY unit, the cut ones included (they are cut
    from the table, not from the buffer); total = the buffer's size.  Every unit starts at the next multiple of 16."""
    units, spans, off = [], [], 0
    for r, data in enumerate(ranges):
        cut = False
        for _, _, t, ref, p in split_raw(data):
            cut |= not p
            if not cut:
                units.append((r, t, ref, len(p), off))
            spans.append((off, p))
            off += (len(p) + 15) & ~15
    return units, spans, off


def events(data):
    """the event classes that occur in a range (names as in REQUIRED), from the model's own arrays"""
    s = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    n = s.size
    code, term, drop = _flags(s)
    raw = split_raw(s)
    ev = set()
    if not code.any():
        ev.add("no_start_code")
    if len(raw) >= 2:
        ev.add("several_units")
    if len(raw) >= 100 and n <= 2 * CHUNK:
        ev.add("hundreds_of_units_per_chunk")
    st_all = np.flatnonzero(code) + 4
    if st_all.size > len(raw):
        ev.add("empty_unit_skipped")
    for k, (st, en, _, _, p) in enumerate(raw):
        if en == n:
            ev.add("ends_at_range_end")
            if n >= 2 and s[n - 1] == 0 and en - st > 1:
                ev.add("ends_at_range_end_with_trailing_zeros")
        elif s[en + 2] == 1:
            ev.add("ended_by_three_byte_code")
            if not code[en]:
                ev.add("three_byte_code_begins_no_unit")
        else:
            ev.add("ended_by_zeros")
        if en + 3 == n:
            ev.add("terminator_ends_with_range")
        if en == n and n >= 2 and s[n - 2] == 0 and s[n - 1] == 0:
            ev.add("terminator_one_past_range")
        d = drop[st + 1: en]
        if d.any():
            ev.add("dropped_03")
            q = np.flatnonzero(d) + st + 1
            if np.any(np.diff(q) == 3):
                ev.add("dropped_03_twice_in_a_row")
            for b in (16, 1024, CHUNK):
                for cut in (1, 2):  # the boundary lies `cut` bytes into the three-byte pattern
                    if np.any((q - 2 + cut) % b == 0):
                        ev.add(f"drop_across_{b}_{cut}")
        if st + 2 < en and s[st] == 0 and s[st + 1] == 0 and s[st + 2] == 3:
            ev.add("03_behind_header_zero_kept")
        if not p:
            ev.add("header_only_unit")
            if k + 1 < len(raw):
                ev.add("units_behind_header_only_unit")
        if (st + 1) // CHUNK + 2 <= (en - 1) // CHUNK:
            ev.add("unit_spans_chunks")
    for z in np.flatnonzero(code):
        for b in (16, 1024, CHUNK):
            for cut in (1, 2, 3):
                if (z + cut) % b == 0:
                    ev.add(f"code_across_{b}_{cut}")
        if z >= 1 and s[z - 1] == 0:
            ev.add("five_byte_code")
    return ev


REQUIRED = {"no_start_code", "several_units", "hundreds_of_units_per_chunk", "empty_unit_skipped", "ends_at_range_end",
            "ends_at_range_end_with_trailing_zeros", "ended_by_three_byte_code", "three_byte_code_begins_no_unit", "ended_by_zeros",
            "terminator_ends_with_range", "terminator_one_past_range", "dropped_03", "dropped_03_twice_in_a_row",
            "03_behind_header_zero_kept", "header_only_unit", "units_behind_header_only_unit", "unit_spans_chunks", "five_byte_code"}
REQUIRED |= {f"code_across_{b}_{c}" for b in (16, 1024, CHUNK) for c in (1, 2, 3)}
REQUIRED |= {f"drop_across_{b}_{c}" for b in (16, 1024, CHUNK) for c in (1, 2)}

ALPHABET = np.array([0] * 9 + [1] * 3 + [3] * 3 + [2] + [0x41, 0x65, 0xAB, 0xFF], np.uint8)  # 00 45 %, 01 15 %, 03 15 %, 02 5 %, other 20 %


def draw(rng, n):
    """n bytes from the weighted alphabet: start codes, terminators and 00 00 03 all occur"""
    return ALPHABET[rng.integers(0, ALPHABET.size, n)]


def _b(*parts):
    out = []
    for p in parts:
        out += list(p) if not isinstance(p, int) else [p]
    return np.array(out, np.uint8)


_corpus = None
SC = (0, 0, 0, 1)


def corpus():
    """-> list of ranges (uint8 arrays); built once, never modified by its users"""
    global _corpus
    if _corpus is not None:
        return _corpus
    rng = np.random.default_rng(20241017)
    out = []
    for n in range(9):  # lengths 0..8: zeros, a start code cut short, drawn bytes
        out.append(np.zeros(n, np.uint8))
        out.append(_b(SC, 0x65, 0x11, 0x22, 0x33, 0x44)[:n])
        out.append(draw(rng, n))
    out.append(np.full(300, 0xAB, np.uint8))                         # no start code at all
    out.append(_b(0, 0, 1, 0x65, 1, 2, 3, 0, 0, 1, 0x41, 9))          # ... three-byte codes only
    out.append(_b(0, SC, 0x65, 0x80, 0x81))                           # 00 00 00 00 01
    out.append(_b(SC, 0x67, 1, 2, 0, 0, 1, 0x68, 7, 7, SC, 0x65, 5, 6))  # a three-byte code between two units
    out.append(_b(SC, 0x65, 1, 2, 3))                                 # ends with the range
    out.append(_b(SC, 0x65, 1, 2, 0))                                 # ... with one and two trailing zeros
    out.append(_b(SC, 0x65, 1, 2, 0, 0))                              # (00 00 whose third byte would be one past the end)
    out.append(_b(SC, 0x65, 1, 2, 0, 0, 0))                           # a terminator whose third byte is the last byte
    out.append(_b(SC, 0x65, 1, 2, 0, 0, 1))
    out.append(_b(SC, 0x65, 9, 0, 0, 3, 0, 0, 3, 7))                  # 00 00 03 00 00 03
    out.append(_b(SC, 0x65, 9, 0, 0, 3))                              # an 03 as the last byte is dropped whatever follows
    out.append(_b(SC, 0x00, 0, 3, 5, 5))                              # an 03 right behind a header byte 00 and one zero
    out.append(_b(SC, 0x00, 0, 3, 0, 0, 3, 1))
    out.append(_b(SC, 0x67, 1, 2, SC, 0x68, SC, 0x65, 4, 4, 4))        # a header-only unit in the middle of a range
    out.append(_b(SC, SC, 0x65, 1))                                   # an empty unit: a code right behind a code
    out.append(_b(SC, 0, 0, 1, 0x65, 1, SC, 0x41, 2))                  # ... and a unit that is 00 00 01
    # every start code and every 00 00 03 across a boundary of 16, 1024 and 4096 bytes at each split position (and flush
    # with it on either side); the device splitter's boundaries lie in the 16-byte-aligned image of a range, so the
    # misalignments of the known-answer test move them all once more
    for b in (16, 1024, CHUNK):
        for k in range(0, 5):
            r = np.full(b + 12, 0xAB, np.uint8)
            r[:5] = _b(SC, 0x65)
            r[b - k: b - k + 4] = SC          # k bytes of the code in front of the boundary
            r[b - k + 4] = 0x41
            if b - k >= 8:
                out.append(r)
        for k in range(0, 4):
            r = np.full(b + 9, 0xCD, np.uint8)
            r[:5] = _b(SC, 0x65)
            r[b - k: b - k + 3] = (0, 0, 3)   # k bytes of 00 00 03 in front of the boundary
            if b - k >= 8:
                out.append(r)
    # a chunk of five-byte units (header + four bytes behind a four-byte code: several hundred units in 4096 bytes)
    out.append(np.tile(_b(SC, 0x41, 1, 2, 3, 4), 600))
    # a unit of a few chunks around drawn bytes without terminators
    body = draw(rng, 3 * CHUNK + 77)
    body[body == 0] = 0x80
    out.append(np.concatenate([_b(SC, 0x65), body, _b(SC, 0x41, 1, 1)]))
    # drawn ranges
    for k in range(48):
        out.append(draw(rng, int(rng.integers(9, 3 * CHUNK))))
    for k in range(8):  # ... with long units: zeros thinned out
        r = draw(rng, int(rng.integers(CHUNK, 4 * CHUNK)))
        thin = rng.random(r.size) < 0.9
        r[(r == 0) & thin] = 0x77
        r[:5] = _b(SC, 0x65)
        out.append(r)
    seen = set()
    for r in out:
        r.setflags(write=False)
        seen |= events(r)
    missing = REQUIRED - seen
    assert not missing, f"the corpus no longer produces: {sorted(missing)}"
    _corpus = out
    return _corpus
