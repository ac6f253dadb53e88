"""Length-prefixed (AVCC) NAL framing on the device, out and in: FERHIP_AU_AVCC of ferhip_pack_nal / ferhip_fetch_nal /
ferhip_frame_nal_blocks_fmt and ferhip_write_avcc_config, the splitter of ferhip_split_avcc_blocks, and the live decoder in
AVCC input (ferhip_decs_set_input, ferhip_decs_set_config), against tests/avcc_model.py (pinned by
test_avcc_model_host.py) and against the Annex-B calls on the same NAL units.  Every comparison is byte-exact."""
from pathlib import Path

import numpy as np
import pytest

import avcc_model as am
import nal_model
import nal_split_model as sm

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
FILL = 0xA5
E_ARG, E_STATE, E_UNSUP = -1, -3, -4
IDR, SLICE, NONE = 5, 1, -1
CHUNK = 4096

_cache = {}


def _r16(n):
    return (int(n) + 15) & ~15


# ---- 1. framing

def _framing_payloads():
    rng = np.random.default_rng(5)
    alphabet = np.array([0, 1, 2, 3, 255], np.uint8)
    out = []
    for n in (0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7):
        out.append(np.zeros(n, np.uint8))  # all-zero payloads draw the most 03 bytes
        out.append(alphabet[rng.integers(0, alphabet.size, n)])
    for at in range(CHUNK - 2, CHUNK + 3):  # 00 00 0x around a chunk edge
        for x in range(4):
            p = np.full(CHUNK + 40, 0xAB, np.uint8)
            p[at: at + 3] = (0, 0, x)
            out.append(p)
    types = (5, 1, 7, 8)
    return out, [types[k % 4] for k in range(len(out))]


def test_framing_kat(pkg):
    payloads, types = _framing_payloads()
    annexb = [nal_model.frame_nal(t, p) for p, t in zip(payloads, types)]
    want = [am.annexb_to_avcc(a) for a in annexb]
    assert all(len(w) == len(a) and w[4:] == a[4:] for w, a in zip(want, annexb))
    assert want[0] == bytes([0, 0, 0, 1, 0x25]) and int.from_bytes(want[-1][:4], "big") == len(want[-1]) - 4
    total = sum(_r16(len(w)) for w in want)
    cap = total + 48
    rc, out, idx = pkg.frame_nal_blocks_raw(payloads, types, cap=cap, fill=FILL, flags=pkg.AU_AVCC)
    assert rc == 0
    rc0, out0, idx0 = pkg.frame_nal_blocks_raw(payloads, types, cap=cap, fill=FILL)
    assert rc0 == 0 and np.array_equal(idx, idx0), "the index of the two framings"
    rc1, out1, idx1 = pkg.frame_nal_blocks_raw(payloads, types, cap=cap, fill=FILL, flags=0)
    assert rc1 == 0 and np.array_equal(out1, out0) and np.array_equal(idx1, idx0), "flags 0 is ferhip_frame_nal_blocks"
    off = 0
    touched = np.zeros(cap, bool)
    for k, w in enumerate(want):
        assert (int(idx[k]["offset"]), int(idx[k]["bytes"]), int(idx[k]["nal_type"])) == (off, len(w), types[k]), f"entry {k}"
        assert bytes(out[off: off + len(w)]) == w, f"entry {k} ({len(w)} bytes)"
        assert bytes(out0[off: off + len(w)]) == annexb[k], f"entry {k}: Annex-B"
        touched[off: off + len(w)] = True
        off += _r16(len(w))
    assert (int(idx[-1]["offset"]), int(idx[-1]["bytes"])) == (total, len(want))
    assert np.all(out[~touched] == FILL), "a byte outside the entries was written"
    # the two outputs differ only in the 4-byte prefixes
    diff = np.flatnonzero(out != out0)
    starts = np.array([int(e["offset"]) for e in idx[:-1]])
    assert np.all(np.isin(diff - starts[np.searchsorted(starts, diff, "right") - 1], (0, 1, 2, 3)))
    # cap one byte short of the total: the last entry is absent, no byte at or beyond cap is touched
    rc, out, idx = pkg.frame_nal_blocks_raw(payloads, types, cap=total - 1, fill=FILL, flags=pkg.AU_AVCC)
    assert rc == 0 and np.array_equal(idx[:-1], idx0[:-1])
    assert (int(idx[-1]["offset"]), int(idx[-1]["bytes"])) == (total, len(want) - 1)
    last = int(idx[len(want) - 1]["offset"])
    assert np.all(out[last:] == FILL)
    assert bytes(out[int(idx[len(want) - 2]["offset"]):][: len(want[-2])]) == want[-2]
    # other flag bits are refused
    for bad in (pkg.AU_PARAM_SETS, pkg.AU_AVCC | pkg.AU_PARAM_SETS, 2, 8):
        assert pkg.frame_nal_blocks_raw(payloads[:2], types[:2], flags=bad)[0] == E_ARG


# ---- 2. encoder

EW, EH = 48, 32
EFSZ = EW * EH * 3 // 2
ES = 3


def _eframe(pkg, s, t):
    return pkg.gen_frame(EW, EH, t, 900 + 13 * s, 3)


def _encode_48x32(pkg):
    """three streams, pictures I P P I P, stream 1 absent in the second call -> per call, per flags (0, PARAM_SETS) the Annex-B
    entries of every stream (b"" for an absent one), and per stream its configuration record; computed once"""
    if "enc" in _cache:
        return _cache["enc"]
    g = pkg.FerHip(EW, EH, ES, qp=12, window=16, maxdiff=3, intra_every=30)
    types = [IDR, SLICE, SLICE, IDR, SLICE]
    calls = []
    for t, nt in enumerate(types):
        pics = [None if (t == 1 and s == 1) else _eframe(pkg, s, t) for s in range(ES)]
        _, got = g.encode_live(pics, [nt] * ES)
        assert got == [NONE if p is None else nt for p in pics]
        calls.append({f: g.fetch_nal(f)[0] for f in (0, pkg.AU_PARAM_SETS)})
    assert g.status() == [0] * ES
    rec = [g.avcc_config(s) for s in range(ES)]
    g.close()
    _cache["enc"] = (calls, rec)
    return _cache["enc"]


def _nal(unit):
    assert unit[:4] == b"\x00\x00\x00\x01"
    return unit[4:]


def test_encoder_avcc(pkg):
    g = pkg.FerHip(EW, EH, ES, qp=12, window=16, maxdiff=3, intra_every=30)
    # the configuration record follows the display size and the rate settings as the SPS and PPS writers do
    def check_records():
        recs = []
        for s in range(ES):
            sps, pps = g.sps_pps(s)
            recs.append(g.avcc_config(s))
            assert recs[-1] == am.config_record(_nal(sps), _nal(pps)), f"stream {s}"
        return recs
    r0 = check_records()
    assert r0[0] == r0[1] == r0[2]
    g.set_rate(1, qp=20)  # base[1] changes: the stream's PPS does
    r1 = check_records()
    assert r1[0] == r0[0] and r1[1] != r0[1]
    g.set_display_size(EW - 6, EH - 2)  # the SPS crops
    r2 = check_records()
    assert r2[0] != r1[0] and r2[1] != r1[1]
    lib = g.lib
    buf = np.zeros(256, np.uint8)
    assert lib.ferhip_write_avcc_config(g.ctx, 0, buf.ctypes.data, len(r2[0]) - 1) == 0 and not buf.any()
    assert lib.ferhip_write_avcc_config(g.ctx, 0, buf.ctypes.data, len(r2[0])) == len(r2[0])
    assert lib.ferhip_write_avcc_config(g.ctx, ES, buf.ctypes.data, 256) == 0 and lib.ferhip_write_avcc_config(g.ctx, -1, buf.ctypes.data, 256) == 0
    g.set_display_size(EW, EH)
    cap = 1 << 16
    dst, index = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (ES + 1))
    fill = np.full(cap, FILL, np.uint8)

    def pack(flags):
        dst.upload(fill)
        g.pack_nal_device(dst.ptr, index.ptr, cap, flags)
        g.sync()
        return dst.download(), index.download(dtype=pkg.AU)

    for t, nt in enumerate([IDR, SLICE, SLICE]):
        present = [not (t == 1 and s == 1) for s in range(ES)]
        _, got = g.encode_live([_eframe(pkg, s, t) if present[s] else None for s in range(ES)], [nt] * ES)
        for ps in (0, pkg.AU_PARAM_SETS):
            units, ntypes = g.fetch_nal(ps)
            rc, hbuf, hidx = g.fetch_nal_raw(cap, ps)
            assert rc == 0
            want = [am.annexb_to_avcc(u) for u in units]
            assert [len(sm.split_raw(np.frombuffer(u, np.uint8))) for u in units] == [(3 if ps and nt == IDR else 1) * int(p) for p in present]
            got_units, got_types = g.fetch_nal(ps | pkg.AU_AVCC)
            assert got_units == want and got_types == ntypes, f"picture {t} flags {ps}: ferhip_fetch_nal"
            rc, abuf, aidx = g.fetch_nal_raw(cap, ps | pkg.AU_AVCC)
            assert rc == 0 and np.array_equal(aidx, hidx), "the index of the two framings"
            a0, i0 = pack(ps)
            a1, i1 = pack(ps | pkg.AU_AVCC)
            a2, i2 = pack(ps)
            assert np.array_equal(a0, a2) and np.array_equal(i0, i2), "Annex-B, AVCC, Annex-B again"
            assert np.array_equal(i0, i1) and np.array_equal(i0, hidx)
            touched = np.zeros(cap, bool)
            for s in range(ES):
                o = int(i1[s]["offset"])
                assert bytes(a1[o: o + len(want[s])]) == want[s], f"picture {t} stream {s} flags {ps}: ferhip_pack_nal"
                assert bytes(a0[o: o + len(units[s])]) == units[s]
                touched[o: o + len(want[s])] = True
            assert np.all(a1[~touched] == FILL)
            if ps and nt == IDR:  # the parameter sets of the entry are those of the record
                for s in range(ES):
                    raw = sm.split_raw(np.frombuffer(units[s], np.uint8))
                    sps, pps = (units[s][a:b] for a, b, _, _, _ in raw[:2])
                    assert g.avcc_config(s) == am.config_record(sps, pps)
    assert g.status() == [0] * ES
    g.close()
    dst.free()
    index.free()


# ---- 3. splitter

def _check_split(ranges, L, rc, out, units, count, fault, cap):
    want_units, total, want_fault = am.layout(ranges, L)
    assert rc == 0 and total <= cap
    assert count == len(want_units)
    got = [(int(u["range"]), int(u["nal_type"]), int(u["ref_idc"]), int(u["bytes"]), int(u["offset"])) for u in units]
    assert got == want_units
    assert [int(f) for f in fault] == want_fault
    want = np.full(out.size, FILL, np.uint8)
    k = 0
    for r, data in enumerate(ranges):
        for _, _, _, _, p in am.avcc_split(data, L)[0]:
            off = want_units[k][4]
            want[off: off + len(p)] = np.frombuffer(p, np.uint8)
            k += 1
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])} of {total}"


@pytest.mark.parametrize("L", [1, 2, 4])
def test_split_kat(pkg, L):
    ranges = [r for _, r in am.corpus(L)]
    total = am.layout(ranges, L)[1]
    for misalign in range(16):
        rc, out, units, count, fault = pkg.split_avcc_blocks_raw(ranges, L, misalign, cap=total + 80, fill=FILL)
        _check_split(ranges, L, rc, out, units, count, fault, total + 80)
    # an empty range between full ones, one range per call, odd alignments
    for k, (name, r) in enumerate(am.corpus(L)):
        trio = [ranges[1], np.zeros(0, np.uint8), r]
        t = am.layout(trio, L)[1]
        rc, out, units, count, fault = pkg.split_avcc_blocks_raw(trio, L, (5 * k + 3) % 16, cap=t + 32, fill=FILL)
        _check_split(trio, L, rc, out, units, count, fault, t + 32)


def test_split_kat_arguments_and_capacities(pkg):
    u = am.unit
    r = [np.frombuffer(u([1, 2], 4, 0x67) + u([3], 4, 0x68) + u([4, 4], 4, 0x65), np.uint8)]
    for L in (0, 3, 5, -1):
        assert pkg.split_avcc_blocks_raw(r, L)[0] == E_ARG
    for misalign in (-1, 16):
        assert pkg.split_avcc_blocks_raw(r, 4, misalign)[0] == E_ARG
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(r, 4, 3, units_cap=2, fill=FILL)
    assert rc == E_ARG and count == 3 and [int(x["nal_type"]) for x in units] == [7, 8]
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(r, 4, 3, units_cap=0, fill=FILL)
    assert rc == E_ARG and count == 3
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(r, 4, 3, cap=32, fill=FILL)  # room for two of the three units
    assert rc == E_ARG and count == 3 and bytes(out[:2]) == b"\x01\x02" and out[16] == 3 and np.all(out[17:] == FILL)
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(r, 4, 3, cap=33, fill=FILL)  # ... and one byte of the third
    assert rc == E_ARG and count == 3 and out[32] == 4 and out.size == 33
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(r, 4, 3, cap=48, fill=FILL)
    assert rc == 0 and count == 3 and bytes(out[32:34]) == b"\x04\x04" and list(fault) == [0]
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw([np.zeros(0, np.uint8)] * 2, 2, 5, fill=FILL)
    assert rc == 0 and count == 0 and np.all(out == FILL) and list(fault) == [0, 0]
    assert pkg.split_avcc_blocks_raw([], 4)[0] == E_ARG
    # more units than the splitter's first table holds: 400 three-byte units in each of two ranges
    many = np.frombuffer(b"".join(u([k & 0xFF, 7], 1, 0x41) for k in range(400)), np.uint8)
    ranges = [many, many[:-1]]
    units_want, total, faults = am.layout(ranges, 1)
    assert len(units_want) == 799 and faults == [0, 1]
    rc, out, units, count, fault = pkg.split_avcc_blocks_raw(ranges, 1, 9, cap=total, fill=FILL)
    _check_split(ranges, 1, rc, out, units, count, fault, total)


# ---- 4. live decoder

class _Feeder:
    """a call's chunks in device memory, each at an odd address (stream s starts 2 s + 1 bytes past a multiple of 16)"""

    def __init__(self, pkg, S, room):
        self.pitch = ((room + 63) & ~15)
        self.buf = pkg.DeviceBuffer(S * self.pitch + 64)

    def put(self, chunks):
        ptrs, lens = [], []
        for s, c in enumerate(chunks):
            if not c:
                ptrs.append(None)
                lens.append(0)
                continue
            off = s * self.pitch + 2 * s + 1
            assert len(c) + 2 * s + 1 <= self.pitch
            self.buf.upload(np.frombuffer(c, np.uint8), off)
            ptrs.append(self.buf.ptr + off)
            lens.append(len(c))
        return ptrs, lens


def _run(pkg, dec, calls, fmts=None, device_in=False, configs=None):
    """calls: a list of chunk lists; fmts[c] = (format, length size) of call c, None = the decoder's default is never
    touched -> per call (pictures [list of arrays per stream], pics, status); slots past a stream's pictures keep the fill"""
    S, P, fsz = dec.S, dec.P, dec.fsz
    feeder = _Feeder(pkg, S, max([len(c) for call in calls for c in call if c] + [16])) if device_in else None
    out = []
    for k, chunks in enumerate(calls):
        if fmts is not None:
            dec.set_input(*fmts[k])
        target = np.full((P, S, fsz), FILL, np.uint8)
        if device_in:
            ptrs, lens = feeder.put(chunks)
            _, pics, st = dec.decode_dev(ptrs, lens, target)
        else:
            _, pics, st = dec.decode(chunks, target)
        for s in range(S):
            assert (target[pics[s]:, s] == FILL).all(), f"stream {s}: a slot past its pictures was written"
        out.append(([target[: pics[s], s].copy() for s in range(S)], pics, st))
    if feeder:
        feeder.buf.free()
    return out


def _same(a, b, what=""):
    assert len(a) == len(b)
    for c, ((pa, na, sa), (pb, nb, sb)) in enumerate(zip(a, b)):
        assert na == nb and sa == sb, f"{what} call {c}: pictures {na} / {nb}, status {sa} / {sb}"
        for s in range(len(pa)):
            assert np.array_equal(pa[s], pb[s]), f"{what} call {c} stream {s}"


def _units(stream):
    """the NAL units of an Annex-B stream, each as header byte + escaped payload"""
    s = np.frombuffer(stream, np.uint8)
    return [s[a:b].tobytes() for a, b, _, _, _ in sm.split_raw(s)]


def _frame(units, L):
    """a chunk of units: Annex-B (L = 0) or length-prefixed"""
    if not units:
        return None
    return b"".join((b"\x00\x00\x00\x01" if L == 0 else len(u).to_bytes(L, "big")) + u for u in units)


def _schedules(units):
    """units[s] = the stream's units -> {name: (calls of unit lists, max slices per call)}"""
    S = len(units)
    is_ps = lambda u: u[0] & 31 in (7, 8)
    n = max(len(u) for u in units)
    one = [[u[k: k + 1] for u in units] for k in range(n)]
    lead = [next(k for k, x in enumerate(u) if not is_ps(x)) for u in units]
    ps_first = [[u[:lead[s]] for s, u in enumerate(units)], [u[lead[s]:] for s, u in enumerate(units)]]
    slices = max(sum(not is_ps(x) for x in u) for u in units)
    return {"one_unit_per_call": (one, 1), "everything_in_one_call": ([list(units)], slices), "parameter_sets_first": (ps_first, slices)}


def _sources(pkg):
    """-> {name: (W, H, units per stream)}: the committed golden streams and the 48x32 encodes"""
    if "src" not in _cache:
        a = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
        b = (GOLD / "qcif_skip_5f_qp12.264").read_bytes()
        calls, _ = _encode_48x32(pkg)
        enc = [b"".join(c[pkg.AU_PARAM_SETS][s] for c in calls) for s in range(ES)]
        _cache["src"] = {"golden": (176, 144, [_units(x) for x in (a, b, a)]), "encoded_48x32": (EW, EH, [_units(x) for x in enc])}
    return _cache["src"]


@pytest.mark.parametrize("source", ["golden", "encoded_48x32"])
def test_live_decode_avcc_equals_annexb(pkg, source):
    W, H, units = _sources(pkg)[source]
    S = len(units)
    for name, (sched, P) in _schedules(units).items():
        def calls(L):
            return [[_frame(us, L) for us in call] for call in sched]
        dec = pkg.LiveDecoder(S, W, H, P)
        ref = _run(pkg, dec, calls(0))
        dec.close()
        assert sum(sum(n) for _, n, _ in ref) == sum(sum(u[0] & 31 in (1, 5) for u in us) for us in units), name
        assert all(st == [0] * S for _, _, st in ref)
        assert 255 < max(len(u) for us in units for u in us) < 65536  # too long for one-byte lengths, short enough for two
        for L, device_in in ((4, False), (4, True), (2, True), (2, False)):
            dec = pkg.LiveDecoder(S, W, H, P)
            dec.set_input(pkg.IN_AVCC, L)
            _same(ref, _run(pkg, dec, calls(L), device_in=device_in), f"{name} L={L} device_in={device_in}:")
            dec.close()


def test_live_decode_dev_grows_the_table_and_the_store(pkg):
    """2000 access unit delimiters in front of every stream's SPS + PPS + IDR: more units than a fresh splitter's table
    holds, so the job is repeated; only that second pass sees the bytes of all units -- 16 of the store for every short
    unit, more than the first store has -- and the job is repeated once more.  The next call finds the buffers as they
    were left.  Two-byte lengths: units of this fixture are longer than the 255 bytes a one-byte length can state
    (test_live_decode_avcc_equals_annexb asserts it)."""
    W, H, units = _sources(pkg)["encoded_48x32"]
    S, N, L = 2, 2000, 2
    real = [us[:3] for us in units[:S]]
    assert all([u[0] & 31 for u in r] == [7, 8, 5] for r in real)
    assert max(len(u) for r in real for u in r) < 65536
    aud = (2).to_bytes(L, "big") + b"\x09\xF0"
    first = [aud * N + _frame(r, L) for r in real]
    table, total, faults = am.layout([np.frombuffer(c, np.uint8) for c in first], L)
    need = sum(_r16(len(c)) for c in first)
    assert len(table) == S * (N + 3) > max(64, 4 * S) and faults == [0] * S, "the first table"
    assert sum(_r16(t[3]) for t in table[:64]) <= need + need // 4 + 4096 - 64 < total, "the first store: enough for the first pass only"
    calls = [first, [_frame(us[3:4], L) for us in units[:S]]]
    dec = pkg.LiveDecoder(S, W, H, 1)
    dec.set_input(pkg.IN_AVCC, L)
    host = _run(pkg, dec, calls)
    dec.close()
    assert all(n == [1] * S and st == [0] * S for _, n, st in host)
    dec = pkg.LiveDecoder(S, W, H, 1)
    dec.set_input(pkg.IN_AVCC, L)
    _same(host, _run(pkg, dec, calls, device_in=True))
    dec.close()


def test_live_decode_set_config_and_set_input_arguments(pkg):
    W, H, units = _sources(pkg)["encoded_48x32"]
    _, recs = _encode_48x32(pkg)
    S = ES
    slices = [[u for u in us if u[0] & 31 in (1, 5)] for us in units]
    P = len(slices[0])
    dec = pkg.LiveDecoder(S, W, H, P)
    ref = _run(pkg, dec, [[_frame(us, 0) for us in units]])
    dec.close()
    assert ref[0][1] == [5, 4, 5] and ref[0][2] == [0] * S
    for device_in in (False, True):
        dec = pkg.LiveDecoder(S, W, H, P)
        for s in range(S):  # in Annex-B input a record of any length size is taken
            assert dec.set_config(s, recs[s][:4] + bytes([0xFC | 1]) + recs[s][5:]) == 0
        dec.set_input(pkg.IN_AVCC, 4)
        for s in range(S):
            assert dec.set_config(s, recs[s]) == 0
        _same(ref, _run(pkg, dec, [[_frame(us, 4) for us in slices]], device_in=device_in), f"set_config, device_in={device_in}:")
        dec.close()
    dec = pkg.LiveDecoder(S, W, H, P)
    lib, rec = pkg.load_library(), recs[0]
    assert lib.ferhip_decs_set_input(dec.h, 2, 4) == E_ARG and lib.ferhip_decs_set_input(dec.h, -1, 4) == E_ARG
    for L in (0, 3, 5, 8):
        assert lib.ferhip_decs_set_input(dec.h, pkg.IN_AVCC, L) == E_ARG
    assert lib.ferhip_decs_set_input(dec.h, pkg.IN_ANNEXB, 77) == 0  # ignored in Annex-B
    dec.set_input(pkg.IN_AVCC, 4)
    assert dec.set_config(0, rec[:4] + bytes([0xFC | 1]) + rec[5:]) == E_ARG, "a record with another length size"
    assert dec.set_config(0, rec[:4] + bytes([0xFC | 0]) + rec[5:]) == E_ARG
    assert dec.set_config(S, rec) == E_ARG and dec.set_config(-1, rec) == E_ARG
    assert dec.set_config(0, bytes([2]) + rec[1:]) == E_ARG, "configurationVersion"
    for cut in (0, 5, 6, 7, 8, len(rec) - 5, len(rec) - 1):
        assert dec.set_config(0, rec[:cut]) == E_ARG, f"truncated to {cut} bytes"
    assert dec.set_config(0, rec[:5] + bytes([0xE0]) + rec[8 + int.from_bytes(rec[6:8], "big"):]) == E_ARG, "no SPS"
    assert dec.set_config(0, rec[:8 + int.from_bytes(rec[6:8], "big")] + bytes([0])) == E_ARG, "no PPS"
    assert dec.set_config(0, rec) == 0
    # an SPS of another picture size: FERHIP_E_UNSUP, as in a chunk
    g = pkg.FerHip(64, 32, 1, qp=12, window=16, maxdiff=3, intra_every=30)
    other = g.avcc_config(0)
    g.close()
    assert dec.set_config(1, other) == E_UNSUP
    dec.close()


def test_live_decode_overrun_is_isolated(pkg):
    W, H, units = _sources(pkg)["encoded_48x32"]
    S, L = ES, 4
    def aus(us):
        out, cur = [], []
        for u in us:
            cur.append(u)
            if u[0] & 31 in (1, 5):
                out.append(cur)
                cur = []
        return out
    au = [aus(us) for us in units]
    v = au[1]  # stream 1 sat out the second picture: I P I P
    assert [x[-1][0] & 31 for x in v] == [5, 1, 5, 1] and [x[-1][0] & 31 for x in au[0]] == [5, 1, 1, 5, 1]
    # up to two access units per stream and call: streams 0, 2 = I P | P | I P, stream 1 = I | P | I P
    good = [[au[0][0] + au[0][1], v[0], au[2][0] + au[2][1]], [au[0][2], v[1], au[2][2]], [au[0][3] + au[0][4], v[2] + v[3], au[2][3] + au[2][4]]]
    framed = [[_frame(c, L) for c in call] for call in good]
    clean_dec = pkg.LiveDecoder(S, W, H, 2)
    clean_dec.set_input(pkg.IN_AVCC, L)
    clean = _run(pkg, clean_dec, framed)
    clean_dec.close()
    assert [n for _, n, _ in clean] == [[2, 1, 2], [1, 1, 1], [2, 2, 2]] and all(st == [0] * S for _, _, st in clean)
    # the damage: call 1 of stream 1 = its P picture, then the same unit again one byte short
    bad = [list(c) for c in framed]
    bad[1][1] = framed[1][1] + framed[1][1][:-1]
    bad.insert(2, [None, framed[1][1], None])  # a P slice behind the fault: refused until the next IDR
    without = [[c[0], None, c[2]] for c in bad]
    for device_in in (False, True):
        dec = pkg.LiveDecoder(S, W, H, 2)
        dec.set_input(pkg.IN_AVCC, L)
        got = _run(pkg, dec, bad, device_in=device_in)
        dec.close()
        dec = pkg.LiveDecoder(S, W, H, 2)
        dec.set_input(pkg.IN_AVCC, L)
        alone = _run(pkg, dec, without, device_in=device_in)
        dec.close()
        assert [st for _, _, st in got] == [[0, 0, 0], [0, E_ARG, 0], [0, E_STATE, 0], [0, 0, 0]], f"device_in={device_in}"
        assert [n for _, n, _ in got] == [[2, 1, 2], [1, 1, 1], [0, 0, 0], [2, 2, 2]]
        assert np.array_equal(got[1][0][1], clean[1][0][1]), "the picture in front of the overrun is delivered"
        assert np.array_equal(got[3][0][1], clean[2][0][1]), "the stream is back at its next IDR"
        for c in range(4):
            for s in (0, 2):
                assert np.array_equal(got[c][0][s], alone[c][0][s]), f"call {c} stream {s}: as without stream 1"
            assert alone[c][1][1] == 0 and alone[c][2] == [0] * S
    # stray bytes behind the last unit are an overrun too, and the units in front of them decode
    for device_in in (False, True):
        dec = pkg.LiveDecoder(S, W, H, 2)
        dec.set_input(pkg.IN_AVCC, L)
        got = _run(pkg, dec, [[framed[0][0], framed[0][1] + b"\x00\x00", framed[0][2]]], device_in=device_in)
        dec.close()
        assert got[0][1] == [2, 1, 2] and got[0][2] == [0, E_ARG, 0]
        _same([(got[0][0], None, None)], [(clean[0][0], None, None)])


def test_live_decode_alternates_annexb_and_avcc(pkg):
    W, H, units = _sources(pkg)["golden"]
    S = len(units)
    is_slice = lambda u: u[0] & 31 in (1, 5)
    aus = []
    for us in units:
        out, cur = [], []
        for u in us:
            cur.append(u)
            if is_slice(u):
                out.append(cur)
                cur = []
        aus.append(out)
    n = max(len(a) for a in aus)
    sched = [[a[k] if k < len(a) else [] for a in aus] for k in range(n)]
    dec = pkg.LiveDecoder(S, W, H, 1)
    ref = _run(pkg, dec, [[_frame(us, 0) for us in call] for call in sched])
    dec.close()
    assert sum(sum(p) for _, p, _ in ref) == 13
    fmts = [(pkg.IN_ANNEXB, 4), (pkg.IN_AVCC, 4), (pkg.IN_AVCC, 2), (pkg.IN_ANNEXB, 0), (pkg.IN_AVCC, 4)]
    calls = [[_frame(us, 0 if f == pkg.IN_ANNEXB else L) for us in call] for call, (f, L) in zip(sched, fmts)]
    for device_in in (False, True):
        dec = pkg.LiveDecoder(S, W, H, 1)
        _same(ref, _run(pkg, dec, calls, fmts=fmts[:n], device_in=device_in), f"device_in={device_in}:")
        dec.close()


# ---- 5. loopback

def test_loopback_without_the_bus(pkg):
    """encode -> ferhip_pack_nal(FERHIP_AU_AVCC | FERHIP_AU_PARAM_SETS) -> ferhip_decs_decode_dev in AVCC input, all in device
    memory: the luma equals the encoder's own reconstruction (chroma: the decoder follows the reference in keeping
    ChromaACLevel of the previous macroblock)"""
    W, H, S, T = 176, 144, 3, 4
    FSZ = W * H * 3 // 2
    feeds = np.stack([np.stack([pkg.gen_frame(W, H, t, 500 + 7 * s, 2) for t in range(T)]) for s in range(S)])
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    cap = S * (((g.nmb * 1024 + 4096 + 15) & ~15) + 64)
    dst, index = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (S + 1))
    dec = pkg.LiveDecoder(S, W, H, 1)
    dec.set_input(pkg.IN_AVCC, 4)
    out_d = pkg.DeviceBuffer(S * FSZ)
    decoded = 0
    for t in range(T):
        present = [not (t == 2 and s == 1) for s in range(S)]
        g.encode_live([feeds[s, t] if present[s] else None for s in range(S)], [5 if t == 0 else 1] * S)
        g.pack_nal_device(dst.ptr, index.ptr, cap, pkg.AU_PARAM_SETS | pkg.AU_AVCC)
        g.sync()
        idx = index.download(dtype=pkg.AU)  # the 16 (S + 1) index bytes are all that crosses the bus
        assert int(idx[S]["offset"]) <= cap and int(idx[S]["bytes"]) == sum(present)
        ptrs = [dst.ptr + int(idx[s]["offset"]) if idx[s]["bytes"] else None for s in range(S)]
        out_d.upload(np.full(S * FSZ, FILL, np.uint8))
        _, pics, status = dec.decode_dev(ptrs, [int(b) for b in idx["bytes"][:S]], out_d)
        assert pics == [int(p) for p in present] and status == [0] * S, f"picture {t}"
        got = out_d.download().reshape(1, S, FSZ)
        recon = np.asarray(g.get_recon()).reshape(S, FSZ)
        for s in range(S):
            if not present[s]:
                assert (got[0, s] == FILL).all()
                continue
            assert np.array_equal(got[0, s, : W * H], recon[s, : W * H]), f"picture {t} stream {s}: the encoder's reconstruction"
            decoded += 1
    assert decoded == 11 and g.status() == [0] * S
    for x in (dec, g):
        x.close()
    for b in (dst, index, out_d):
        b.free()
