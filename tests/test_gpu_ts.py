"""Transport stream packets on the device (ferhip_pack_ts, ferhip_fetch_ts, ferhip_ts_blocks, ferhip_write_ts_psi,
csrc/fer_ts.hip) against tests/ts_model.py (pinned on the host by test_ts_model_host.py) applied to the entries that
tests/nal_model.py and ferhip_fetch_nal give; the device demultiplexer (ferhip_unts_blocks) against the same model followed by
the Annex-B splitter's layout (tests/nal_split_model.py); and the live decoder on packets in host and in device memory
(ferhip_decs_decode_ts) against ferhip_decs_decode on the Annex-B form of the same units.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import nal_model
import nal_split_model as sm
import ts_model as tm

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = 5, 1, -1
E_ARG, E_STATE = -1, -3
FILL = 0xA5

_cache = {}


def _hdrs(pkg, n, cc0=14):
    """pts and pcr with bit 32 set, counters that wrap within a few packets"""
    k = np.arange(n)
    return pkg.ts_hdr(n, pts=(1 << 32) + 0x12345678 + 3000 * k, pcr=(1 << 32) + 0x0FEDCBA9 + 7 * k, pid=0x100 + k % 0x1E00, pmt_pid=0x20 + k % 0xE0,
                      cc=(cc0 + 5 * k) & 15, psi_cc=(15 + k) & 15)


def _hdr_dict(h):
    return {f: int(h[f]) for f in ("pts", "pcr", "pid", "pmt_pid", "cc", "psi_cc")}


def _kat_payloads():
    if "kat" in _cache:
        return _cache["kat"]
    rng = np.random.default_rng(1880)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 255], np.uint8)
    out = [np.full(n, 0xAB, np.uint8) for n in (0, 150, 151, 152, 333, 334, 335, 336)]  # L = 25 + n
    out += [np.zeros(n, np.uint8) for n in (1, 2, 3, 150, 151, 400, 4095, 4096, 4097)]
    out += [alphabet[rng.integers(0, alphabet.size, n)] for n in (97, 152, 1000, 4096, 2 * 4096 + 7, 3 * 4096 - 1)]
    # 00 00 0x whose inserted 03 is PES byte 175 (the last of packet 0), 176 (the first of packet 1), 359 and 360 (around the
    # seam of packets 1 and 2), and at every phase around the edge of a 4096-byte chunk of the payload
    for x in range(4):
        for e in (150, 151, 334, 335):
            p = np.full(700, 0xAB, np.uint8)
            p[e - 2: e + 1] = (0, 0, x)
            assert nal_model.frame_nal(1, p)[5 + e] == 3
            out.append(p)
        for at in range(4096 - 4, 4096 + 2):
            p = np.full(4096 + 100, 0xAB, np.uint8)
            p[at: at + 3] = (0, 0, x)
            out.append(p)
    for p in out:
        p.setflags(write=False)
    _cache["kat"] = out
    return out


def _check(out, idx, per_stream, types, cap, fill=FILL, what=""):
    """the whole buffer and index against the model's layout: a stream whose packets do not end within cap is absent, and
    every byte the model does not place holds the fill value"""
    index = tm.layout(per_stream, types)
    want = np.full(out.size, fill, np.uint8)
    written = 0
    for s, pk in enumerate(per_stream):
        off, nbytes = index[s][:2]
        assert tuple(int(v) for v in idx[s]) == index[s], f"{what}: index[{s}] = {idx[s]}, expected {index[s]}"
        if not pk or off + nbytes > cap:
            continue
        written += 1
        want[off: off + nbytes] = np.frombuffer(pk, np.uint8)
    total = index[-1]
    assert tuple(int(v) for v in idx[len(per_stream)]) == (total[0], written, 0, total[3], 0), f"{what}: index[S]"
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])}"
    return index


def test_kat_blocks_equal_the_model(pkg):
    payloads = _kat_payloads()
    n = len(payloads)
    types = [(1, 5)[k & 1] for k in range(n)]
    hdr = _hdrs(pkg, n)
    per_stream = [tm.mux(nal_model.frame_nal(types[k], payloads[k]), types[k], _hdr_dict(hdr[k])) for k in range(n)]
    assert [len(pk) // 188 for pk in per_stream[:8]] == [1, 1, 1, 2, 2, 2, 2, 3]
    assert [tm.npackets(25 + m) for m in (0, 150, 151, 152, 334, 335, 336)] == [1, 1, 1, 2, 2, 2, 3]
    assert any(pk[188 * k + 3] & 15 == 0 and k for pk in per_stream for k in range(len(pk) // 188)), "a counter wraps"
    index = tm.layout(per_stream, types)
    total = index[-1][0]
    rc, out, idx = pkg.ts_blocks_raw(payloads, types, hdr, cap=total + 64, fill=FILL)
    assert rc == 0
    _check(out, idx, per_stream, types, total + 64, what="all")
    # one byte short of the last stream, and of one in the middle: that stream is absent, nothing beyond cap is touched
    last_end = index[n - 1][0] + index[n - 1][1]
    rc, out, idx = pkg.ts_blocks_raw(payloads, types, hdr, cap=last_end - 1, fill=FILL)
    assert rc == 0
    _check(out, idx, per_stream, types, last_end - 1, what="cap one byte short")
    assert int(idx[n]["bytes"]) == n - 1
    rc, out, idx = pkg.ts_blocks_raw(payloads, types, hdr, cap=last_end, fill=FILL)
    assert rc == 0 and int(idx[n]["bytes"]) == n
    _check(out, idx, per_stream, types, last_end, what="cap exact")
    mid_end = index[n // 2][0] + index[n // 2][1]
    rc, out, idx = pkg.ts_blocks_raw(payloads, types, hdr, cap=mid_end - 1, fill=FILL)
    assert rc == 0 and int(idx[n]["bytes"]) == n // 2
    _check(out, idx, per_stream, types, mid_end - 1, what="cap one byte short of a stream in the middle")


def test_kat_one_payload_per_call_and_refusals(pkg):
    payloads = _kat_payloads()
    for k in (0, 2, 3, 7, 21, 22, len(payloads) - 1):
        hdr = _hdrs(pkg, 1, cc0=15)
        pk = tm.mux(nal_model.frame_nal(5, payloads[k]), 5, _hdr_dict(hdr[0]))
        rc, out, idx = pkg.ts_blocks_raw([payloads[k]], [5], hdr, cap=len(pk) + 40, fill=FILL)
        assert rc == 0
        _check(out, idx, [pk], [5], len(pk) + 40, what=f"payload {k}")
    hdr = _hdrs(pkg, 2)
    two = [payloads[3], payloads[4]]
    assert pkg.ts_blocks_raw(two, [1, 5], hdr)[0] == 0
    for field, v in (("pts", 1 << 33), ("pcr", 1 << 33), ("pid", 0x0F), ("pid", 0x1FFF), ("pmt_pid", 0x0F), ("pmt_pid", 0x1FFF), ("cc", 16),
                     ("psi_cc", 16), ("reserved", 1)):
        h = hdr.copy()
        h[field][1] = v
        assert pkg.ts_blocks_raw(two, [1, 5], h)[0] == E_ARG, field
    h = hdr.copy()
    h["pmt_pid"][1] = h["pid"][1]
    assert pkg.ts_blocks_raw(two, [1, 5], h)[0] == E_ARG
    for field, v in (("pts", (1 << 33) - 1), ("pid", 0x10), ("pid", 0x1FFE), ("cc", 15)):
        h = hdr.copy()
        h[field][1] = v
        assert pkg.ts_blocks_raw(two, [1, 5], h)[0] == 0, field
    lib = pkg.load_library()
    lens, nt, idx = np.array([4], np.uint32), np.array([1], np.int32), np.zeros(2, pkg.TS_AU)
    src, out = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    assert lib.ferhip_ts_blocks(src.ctypes.data, 16, lens.ctypes.data, nt.ctypes.data, 1, None, out.ctypes.data, 256, idx.ctypes.data) == E_ARG
    assert lib.ferhip_ts_blocks(src.ctypes.data, 16, lens.ctypes.data, nt.ctypes.data, 1, hdr.ctypes.data, None, 256, idx.ctypes.data) == E_ARG
    assert lib.ferhip_ts_blocks(src.ctypes.data, 16, lens.ctypes.data, nt.ctypes.data, 1, hdr.ctypes.data, out.ctypes.data, 256, None) == E_ARG
    assert lib.ferhip_ts_blocks(src.ctypes.data, 16, lens.ctypes.data, nt.ctypes.data, 1, hdr.ctypes.data, out.ctypes.data, 256, idx.ctypes.data) == 0


def test_write_ts_psi(pkg):
    for pid, pmt, cc in ((0x100, 0x1000, 0), (0x10, 0x1FFE, 15), (0x1ABC, 0x20, 7)):
        assert pkg.write_ts_psi(pid, pmt, cc) == tm.psi(pid, pmt, cc)
    p = pkg.write_ts_psi(0x100, 0x1000, 3)
    assert p[17:21] == bytes.fromhex("2AB104B2") and p[188 + 22: 188 + 26] == bytes.fromhex("15BD4D56")
    for bad in ((0x0F, 0x1000, 0), (0x100, 0x1FFF, 0), (0x100, 0x100, 0), (0x100, 0x1000, 16), (0x100, 0x1000, -1), (-1, 0x1000, 0)):
        assert pkg.write_ts_psi(*bad) == b"", bad
    assert pkg.write_ts_psi(0x100, 0x1000, 0, cap=375) == b""


# ---- pictures

W, H, S = 64, 48, 3
QP = 8


def _frames():
    if "frames" not in _cache:
        a = np.random.default_rng(4864).integers(0, 256, (S, 3, W * H * 3 // 2)).astype(np.uint8)  # noise: nothing is predicted
        a.setflags(write=False)
        _cache["frames"] = a
    return _cache["frames"]


FLAG_SETS = ((0, "plain"), (1, "parameter sets"), (8, "PSI"), (9, "parameter sets and PSI"))


def test_pictures_equal_the_model_on_fetch_nal_entries(pkg):
    """IDR, P, and P with stream 1 absent, under all four flag combinations: ferhip_fetch_ts and ferhip_pack_ts + copy against
    the model on ferhip_fetch_nal's entries; the counters run on in the caller's hands"""
    feeds = _frames()
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    cap = 1 << 18
    dst, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(24 * (S + 1))
    hdr0 = pkg.ts_hdr(S, pid=0x100 + np.arange(S), pmt_pid=0x1000 + np.arange(S))
    assert g.lib.ferhip_pack_ts(g.ctx, 0, hdr0.ctypes.data, dst.ptr, cap, dix.ptr) == E_STATE and g.fetch_ts_raw(hdr0, cap)[0] == E_STATE
    cc = {f: np.full(S, 14, np.int64) for f, _ in FLAG_SETS}
    psi_cc = {f: np.full(S, 15, np.int64) for f, _ in FLAG_SETS}
    kinds = []
    for t in range(3):
        present = [not (t == 2 and s == 1) for s in range(S)]
        # (noise: left to itself the encoder would code every picture as an I picture)
        rbsp, nt = g.encode_live([feeds[s][t] if present[s] else None for s in range(S)], [pkg.NAL_SLICE if t else pkg.NAL_IDR] * S)
        kinds.append(list(nt))
        if t == 0:
            assert all(len(nal_model.frame_nal(5, np.frombuffer(r, np.uint8))) - 5 > 4096 for r in rbsp), "an IDR unit exceeds one 4096-byte chunk"
        rtp_before = g.fetch_rtp(pkg.rtp_hdr(S), 128, 1)[0]
        nal_before = g.fetch_nal(1)
        for flags, name in FLAG_SETS:
            what = f"picture {t}, {name}"
            entries, types = g.fetch_nal(flags & 1)
            hdr = pkg.ts_hdr(S, pts=(1 << 32) + 3000 * t, pcr=(1 << 32) - 5 + 3000 * t, pid=0x100 + np.arange(S), pmt_pid=0x1000 + np.arange(S),
                             cc=cc[flags] & 15, psi_cc=psi_cc[flags] & 15)
            per_stream = [tm.mux(entries[s], types[s], _hdr_dict(hdr[s]), bool(flags & 8)) if entries[s] else b"" for s in range(S)]
            index = tm.layout(per_stream, types)
            total = index[-1][0]
            rc, buf, idx = g.fetch_ts_raw(hdr, cap, flags, fill=FILL)
            assert rc == 0, what
            for s in range(S + 1):
                assert tuple(int(v) for v in idx[s]) == index[s], f"{what}: index[{s}]"
            got = [bytes(buf[index[s][0]: index[s][0] + index[s][1]]) for s in range(S)]
            assert got == per_stream, f"{what}: ferhip_fetch_ts"
            assert np.all(buf[total:] == FILL)
            again = g.fetch_ts_raw(hdr, cap, flags, fill=FILL)
            assert again[0] == 0 and np.array_equal(again[1], buf) and np.array_equal(again[2], idx), f"{what}: a repeated call"
            assert g.fetch_ts(hdr, flags)[0] == per_stream
            # device to device, then copied: the whole buffer
            dst.upload(np.full(cap, FILL, np.uint8))
            g.pack_ts_device(hdr, dst.ptr, cap, dix.ptr, flags)
            g.sync()
            _check(dst.download(), dix.download(dtype=pkg.TS_AU), per_stream, types, cap, what=what)
            for s in range(S):
                npk = index[s][3]
                with_psi = bool(flags & 8) and types[s] == IDR
                assert (per_stream[s][:376] == pkg.write_ts_psi(int(hdr["pid"][s]), int(hdr["pmt_pid"][s]), int(hdr["psi_cc"][s]))) == with_psi, what
                cc[flags][s] += npk - (2 if with_psi else 0)
                psi_cc[flags][s] += with_psi
            if flags == 9:  # one byte short of the last stream that is there: fetch fills the index and refuses
                last = max(s for s in range(S) if per_stream[s])
                short = index[last][0] + index[last][1] - 1
                rc, _, idx = g.fetch_ts_raw(hdr, short, flags)
                assert rc == E_ARG and [tuple(int(v) for v in r) for r in idx[:S]] == index[:S]
                dst.upload(np.full(cap, FILL, np.uint8))
                g.pack_ts_device(hdr, dst.ptr, short, dix.ptr, flags)
                g.sync()
                _check(dst.download(), dix.download(dtype=pkg.TS_AU), per_stream, types, short, what=what + ", one byte short")
        assert g.fetch_nal(1) == nal_before and g.fetch_rtp(pkg.rtp_hdr(S), 128, 1)[0] == rtp_before, "the other framings are unchanged"
    assert kinds == [[IDR] * S, [SLICE] * S, [SLICE, NONE, SLICE]]
    assert g.status() == [0] * S
    g.close()


def test_context_refusals(pkg):
    feeds = _frames()
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    lib = g.lib
    cap = 1 << 17
    dst, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(24 * (S + 1))
    hdr = pkg.ts_hdr(S, pts=5, pcr=6, pid=0x100 + np.arange(S), pmt_pid=0x1000, cc=3, psi_cc=4)

    def pack(flags=0, h=hdr, d=dst.ptr, c=cap, i=dix.ptr):
        return lib.ferhip_pack_ts(g.ctx, flags, h.ctypes.data if h is not None else None, d, c, i)

    assert pack() == E_STATE
    g.encode_live([feeds[s][0] for s in range(S)])
    assert pack() == 0 and pack(9) == 0
    for kw in (dict(flags=2), dict(flags=4), dict(flags=16), dict(flags=9 | 32), dict(h=None), dict(d=dst.ptr + 8), dict(i=dix.ptr + 4),
               dict(i=None), dict(d=None)):
        assert pack(**kw) == E_ARG, kw
    assert lib.ferhip_pack_ts(None, 0, hdr.ctypes.data, dst.ptr, cap, dix.ptr) == E_ARG
    for field, v in (("pts", 1 << 33), ("pcr", 1 << 33), ("pid", 0x0F), ("pid", 0x1FFF), ("pmt_pid", 0x0F), ("pmt_pid", 0x1FFF), ("cc", 16),
                     ("psi_cc", 16), ("reserved", 1), ("pmt_pid", 0x100 + S - 1)):
        h = hdr.copy()
        h[field][S - 1] = v
        assert pack(h=h) == E_ARG and g.fetch_ts_raw(h, cap)[0] == E_ARG, field
    assert pack(d=None, c=0) == 0
    # a stream whose PIDs change gets its PSI row again
    a = g.fetch_ts(hdr, 8)[0]
    h = hdr.copy()
    h["pid"][1], h["pmt_pid"][1] = 0x1234, 0x0456
    b = g.fetch_ts(h, 8)[0]
    assert a[0] == b[0] and a[2] == b[2] and b[1][:376] == tm.psi(0x1234, 0x0456, 4) and a[1][:376] == tm.psi(0x101, 0x1000, 4)
    assert g.fetch_ts(hdr, 8)[0] == a
    # a call in which every stream is absent: nothing at all
    g.encode_live([None] * S)
    rc, _, idx = g.fetch_ts_raw(hdr, 0, 9)
    assert rc == 0 and [tuple(int(v) for v in r) for r in idx] == [(0, 0, 0, 0, 0)] * (S + 1)
    g.close()


# ---- the way in, known answers: ferhip_unts_blocks against the model

GOLDENS = ("qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264")


def _golden_ts(with_psi=True):
    from conftest import golden_bytes
    k = ("gold_ts", with_psi)
    if k not in _cache:
        _cache[k] = [b"".join(tm.mux_stream(golden_bytes(n), dict(tm.HDR, pid=0x100 + i, pmt_pid=0x1000 + i), with_psi)) for i, n in enumerate(GOLDENS)]
    return _cache[k]


def _lay(pkg, per_stream, chunk=3):
    """every stream's packets in runs of up to `chunk` packets, interleaved, at odd offsets -> (base, rows)"""
    buf, rows = bytearray(b"\xEE" * 3), []
    at = [0] * len(per_stream)
    k = 0
    while any(at[s] < len(d) for s, d in enumerate(per_stream)):
        for s, d in enumerate(per_stream):
            if at[s] < len(d):
                n = min(188 * (1 + (k + s) % chunk), len(d) - at[s])
                rows.append((len(buf), n, s))
                buf += d[at[s]: at[s] + n] + b"\xEE" * (1 + k % 3)
                at[s] += n
                k += 1
    return bytes(buf), np.array(rows, pkg.TS_RUN) if rows else np.zeros(0, pkg.TS_RUN)


def _check_unts(pkg, base, rows, streams, pids, expect, misalign, what):
    """streams[s] = the bytes stream s's runs name, in order; the whole store, the table, fault[] and cc_next[] against
    ts_model.demux followed by the Annex-B splitter's layout"""
    model = [tm.demux(d, pid, e) for d, pid, e in zip(streams, pids, expect)]
    ranges = [es for es, _, _ in model]
    want_units, spans, total = sm.layout(ranges)
    cap = total + 48
    rc, out, units, count, fault, nxt = pkg.unts_blocks_raw(base, rows, pids, expect, misalign, cap=cap, units_cap=len(want_units) + 2, fill=FILL)
    assert rc == 0, what
    assert [int(f) for f in fault] == [f for _, f, _ in model], f"{what}: fault[]"
    assert [int(n) for n in nxt] == [n for _, _, n in model], f"{what}: cc_next[]"
    assert count == len(want_units), f"{what}: {count} units, expected {len(want_units)}"
    got = [(int(u["range"]), int(u["nal_type"]), int(u["ref_idc"]), int(u["bytes"]), int(u["offset"])) for u in units[:count]]
    assert got == want_units, what
    want = np.full(out.size, FILL, np.uint8)
    for off, p in spans:
        want[off: off + len(p)] = np.frombuffer(p, np.uint8)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])} of {total}"
    return model


@pytest.mark.parametrize("misalign", (0, 1, 15))
def test_unts_kat_golden_dressed_and_multi_program(pkg, misalign):
    from conftest import golden_bytes
    per_stream = _golden_ts()
    pids = [0x100 + i for i in range(4)]
    base, rows = _lay(pkg, per_stream)
    model = _check_unts(pkg, base, rows, per_stream, pids, [14, -1, 14, -1], misalign, f"goldens, misalign {misalign}")
    assert all(f == 0 for _, f, _ in model)
    assert [tm.units_of(es) for es, _, _ in model] == [tm.stream_units(golden_bytes(n)) for n in GOLDENS]
    # one stream alone in one run, and a stream without runs between two others
    _check_unts(pkg, per_stream[3], np.array([(0, len(per_stream[3]), 0)], pkg.TS_RUN), per_stream[3:], pids[3:], [-1], misalign, "one stream")
    base, rows = _lay(pkg, [per_stream[0], b"", per_stream[3]], chunk=70)
    _check_unts(pkg, base, rows, [per_stream[0], b"", per_stream[3]], [0x100, 0x55, 0x103], [14, 9, 14], misalign, "an empty stream")
    # dressed input: foreign PIDs, null packets, afc-2 packets, a PES header with a DTS, stuffing in middle packets
    dressed = [tm.dress(tm.access_units_of(golden_bytes(n)), 0x100, 5)[0] for n in (GOLDENS[0], GOLDENS[3])]
    base, rows = _lay(pkg, dressed, chunk=5)
    model = _check_unts(pkg, base, rows, dressed, [0x100, 0x100], [5, -1], misalign, "dressed")
    assert [tm.units_of(es) for es, _, _ in model] == [tm.stream_units(golden_bytes(n)) for n in (GOLDENS[0], GOLDENS[3])]
    # a multi-program buffer: three programs' packets interleaved, read by three slots through the same runs
    progs = per_stream[:3]
    parts = [[d[o: o + 188] for o in range(0, len(d), 188)] for d in progs]
    mixed = bytearray()
    while any(parts):
        for q in parts:
            mixed += b"".join(q[:2])
            del q[:2]
    mixed = bytes(mixed)
    half = (len(mixed) // 376) * 188
    rows = np.array([(o, n, s) for s in range(3) for o, n in ((0, half), (half, len(mixed) - half))], pkg.TS_RUN)
    model = _check_unts(pkg, mixed, rows, [mixed] * 3, pids[:3], [14, 14, -1], misalign, "multi-program")
    assert [es for es, _, _ in model] == [tm.demux(d, pid, 14)[0] for d, pid in zip(progs, pids)]


def test_unts_kat_fault_catalogue(pkg):
    cat = tm.catalogue()
    streams = [data for _, data, _, _, _, _ in cat]
    pids = [pid for _, _, pid, _, _, _ in cat]
    expect = [e for _, _, _, e, _, _ in cat]
    for misalign in (0, 1, 15):
        base, rows = _lay(pkg, streams, chunk=2)
        model = _check_unts(pkg, base, rows, streams, pids, expect, misalign, f"catalogue, misalign {misalign}")
        for (name, _, _, _, fault, stands), (es, f, nxt) in zip(cat, model):
            assert f == fault and es == stands and (nxt == -1) == (fault != 0), name
    # every third entry alone: a fault's place in the table does not matter
    for name, data, pid, e, fault, stands in cat[::3]:
        _check_unts(pkg, data, np.array([(0, len(data), 0)], pkg.TS_RUN), [data], [pid], [e], 1, name)
    # a stream longer than one step of the walk with its fault behind the first 64 packets
    long = _golden_ts(False)[0]
    assert len(long) // 188 > 200
    for k in (70, 127, 128):
        lost = long[: 188 * k] + long[188 * (k + 1):]
        m = _check_unts(pkg, lost, np.array([(0, len(lost), 0)], pkg.TS_RUN), [lost], [0x100], [14], 0, f"packet {k} lost")
        assert m[0][1] == tm.GAP


def test_unts_arguments_and_capacities(pkg):
    per_stream = _golden_ts()[:2]
    pids = [0x100, 0x101]
    base, rows = _lay(pkg, per_stream)
    rc, out, units, count, fault, nxt = pkg.unts_blocks_raw(base, rows, pids)
    assert rc == 0 and count > 8
    total = int(units[count - 1]["offset"]) + ((int(units[count - 1]["bytes"]) + 15) & ~15)
    # a store one byte short, a table one row short: FERHIP_E_ARG and the true count
    rc, _, _, count2, _, _ = pkg.unts_blocks_raw(base, rows, pids, cap=total - 1, fill=FILL)
    assert rc == E_ARG and count2 == count
    rc, _, _, count2, _, _ = pkg.unts_blocks_raw(base, rows, pids, units_cap=count - 1)
    assert rc == E_ARG and count2 == count
    for field, k, v in (("stream", 0, 2), ("offset", 1, len(base) - 3), ("bytes", 2, 187), ("bytes", 2, 189)):
        bad = rows.copy()
        bad[field][k] = v
        assert pkg.unts_blocks_raw(base, bad, pids)[0] == E_ARG, field
    assert pkg.unts_blocks_raw(base, rows, [0x100, 0x2000])[0] == E_ARG
    assert pkg.unts_blocks_raw(base, rows, pids, misalign=16)[0] == E_ARG and pkg.unts_blocks_raw(base, rows, [])[0] == E_ARG
    assert pkg.unts_blocks_raw(base, rows, pids, cc_expect=[16, -1])[0] == E_ARG
    rc, _, _, count, fault, nxt = pkg.unts_blocks_raw(b"", np.zeros(0, pkg.TS_RUN), [1, 2, 3], [5, -1, 7])
    assert rc == 0 and count == 0 and list(fault) == [0, 0, 0] and list(nxt) == [5, -1, 7]


# ---- the live decoder

DW, DH = 176, 144


def _gold_aus():
    """three streams (a, b, a) as access units (entry, type)"""
    if "aus" not in _cache:
        from conftest import golden_bytes
        a, b = tm.access_units_of(golden_bytes(GOLDENS[0])), tm.access_units_of(golden_bytes(GOLDENS[3]))
        _cache["aus"] = [a, b, a]
    return _cache["aus"]


class _Sender:
    """multiplexes access units per stream with running counters and lays the packets of a call out in interleaved runs"""

    def __init__(self, n, with_psi=True):
        self.h = [dict(tm.HDR, pid=0x100 + s, pmt_pid=0x1000 + s, cc=(3 + 7 * s) & 15) for s in range(n)]
        self.pids = [h["pid"] for h in self.h]
        self.with_psi = with_psi

    def packets(self, s, aus):
        out, h = b"", self.h[s]
        for entry, t in aus:
            pk = tm.mux(entry, t, h, self.with_psi)
            psi = self.with_psi and t == 5
            h["cc"] = (h["cc"] + len(pk) // 188 - 2 * psi) & 15
            h["psi_cc"] = (h["psi_cc"] + psi) & 15
            out += pk
        return out


def _ts_call(pkg, dec, base, rows, pids, target, device):
    """decode_ts with the packets in host memory, or (device) in device memory at an odd address"""
    if not device:
        return dec.decode_ts(base, rows, pids, target)
    buf = pkg.DeviceBuffer(len(base) + 16)
    buf.upload(np.frombuffer(base, np.uint8), offset=5)
    try:
        return dec.decode_ts(buf.ptr + 5, rows, pids, target, base_on_device=True)
    finally:
        buf.free()


def _decode_calls(pkg, dec, calls, snd=None, device=False, rtp=None):
    """calls: per call a list per stream of access units; snd = a _Sender: through decode_ts, rtp = (module, sender): through
    decode_rtp, else Annex-B through decode"""
    out = []
    for call in calls:
        target = np.full((dec.P, dec.S, dec.fsz), FILL, np.uint8)
        if snd:
            base, rows = _lay(pkg, [snd.packets(s, aus) for s, aus in enumerate(call)])
            _, pics, st = _ts_call(pkg, dec, base, rows, snd.pids, target, device)
        else:
            _, pics, st = dec.decode([b"".join(e for e, _ in aus) or None for aus in call], target)
        for s in range(dec.S):
            assert (target[pics[s]:, s] == FILL).all()
        out.append(([target[: pics[s], s].copy() for s in range(dec.S)], pics, st))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for c, ((pa, na, sa), (pb, nb, sb)) in enumerate(zip(a, b)):
        assert na == nb and sa == sb, f"{what} call {c}: pictures {na} / {nb}, status {sa} / {sb}"
        for s in range(len(pa)):
            assert np.array_equal(pa[s], pb[s]), f"{what} call {c} stream {s}"


def test_live_decode_ts_equals_annexb(pkg):
    aus = _gold_aus()
    n_s, n = len(aus), max(len(a) for a in aus)
    schedules = {"one_picture_per_call": ([[a[k: k + 1] for a in aus] for k in range(n)], 1),
                 "everything_in_one_call": ([list(aus)], n),
                 "two_then_the_rest": ([[a[:2] for a in aus], [a[2:] for a in aus]], n)}
    for name, (calls, maxpic) in schedules.items():
        dec = pkg.LiveDecoder(n_s, DW, DH, maxpic)
        ref = _decode_calls(pkg, dec, calls)
        dec.close()
        assert sum(sum(npic) for _, npic, _ in ref) == sum(len(a) for a in aus) and all(st == [0] * n_s for _, _, st in ref)
        for device in (False, True):
            dec = pkg.LiveDecoder(n_s, DW, DH, maxpic)
            _same(ref, _decode_calls(pkg, dec, calls, _Sender(n_s), device), f"{name} device={device}")
            dec.close()
    # mixed with the other decode calls on one decoder: Annex-B, TS, RTP, TS
    import rtp_model as rm
    calls = schedules["one_picture_per_call"][0]
    dec = pkg.LiveDecoder(n_s, DW, DH, 1)
    ref = _decode_calls(pkg, dec, calls)
    dec.close()
    for device in (False, True):
        dec = pkg.LiveDecoder(n_s, DW, DH, 1)
        snd = _Sender(n_s)
        seq = [100 * s for s in range(n_s)]
        got = []
        for k, call in enumerate(calls):
            if k == 2:  # RTP packets of the same units
                buf, rows = bytearray(), []
                for s, a in enumerate(call):
                    for entry, _ in a:
                        pk = rm.packetise(rm.access_units_of(entry)[0], 1400, dict(rm.HDR, seq=seq[s]))
                        seq[s] += len(pk)
                        for p in pk:
                            rows.append((len(buf), len(p), s))
                            buf += p
                target = np.full((dec.P, dec.S, dec.fsz), FILL, np.uint8)
                _, pics, st = dec.decode_rtp(bytes(buf), np.array(rows, pkg.RTP_PKT), target)
                got.append(([target[: pics[s], s].copy() for s in range(dec.S)], pics, st))
            else:
                got += _decode_calls(pkg, dec, [call], snd if k & 1 else None, device)
        dec.close()
        _same(ref, got, f"alternating device={device}")


@pytest.mark.parametrize("device", (False, True))
def test_live_decode_ts_faults_are_isolated(pkg, device):
    aus = _gold_aus()
    n_s = len(aus)
    v = aus[0]  # I P P P, every slice in many packets
    clean_calls = [[a[:1] for a in aus], [v[1:3], aus[1][1:2], v[1:3]], [v[3:4], aus[1][2:3], v[3:4]]]
    dec = pkg.LiveDecoder(n_s, DW, DH, 2)
    clean = _decode_calls(pkg, dec, clean_calls, _Sender(n_s), device)
    dec.close()
    assert [npic for _, npic, _ in clean] == [[1, 1, 1], [2, 1, 2], [1, 1, 1]] and all(st == [0] * n_s for _, _, st in clean)

    def damage(kind, data):
        """in the second access unit of call 1 (stream 0): a lost packet, a repeated packet, a scrambled packet"""
        first = len(tm.mux(*v[1], tm.HDR)) // 188
        k = first + 2
        assert len(data) // 188 > k + 2
        p = data[188 * k: 188 * (k + 1)]
        if kind == "gap":
            return data[: 188 * k] + data[188 * (k + 1):]
        if kind == "duplicate":
            return data[: 188 * k] + p + data[188 * k:]
        return data[: 188 * k] + p[:3] + bytes([p[3] | 0x80]) + p[4:] + data[188 * (k + 1):]

    for kind in ("gap", "duplicate", "malformed"):
        dec = pkg.LiveDecoder(n_s, DW, DH, 2)
        snd = _Sender(n_s)
        _decode_calls(pkg, dec, clean_calls[:1], snd, device)
        per = [snd.packets(s, a) for s, a in enumerate(clean_calls[1])]
        per[0] = damage(kind, per[0])
        target = np.full((2, n_s, dec.fsz), FILL, np.uint8)
        _, pics, st = _ts_call(pkg, dec, *_lay(pkg, per), snd.pids, target, device)
        assert (pics, st) == ([1, 1, 2], [E_ARG, 0, 0]), kind
        assert np.array_equal(target[0, 0], clean[1][0][0][0]), f"{kind}: the picture in front of the fault is delivered"
        for s in (1, 2):
            assert np.array_equal(target[: pics[s], s], clean[1][0][s]), f"{kind}: stream {s} is untouched"
        # a P slice behind the fault is refused until the next IDR slice; any counter is taken (the expectation was cleared)
        snd.h[0]["cc"] = 9
        nxt = _decode_calls(pkg, dec, [[v[3:4], aus[1][2:3], v[3:4]]], snd, device)[0]
        assert nxt[1] == [0, 1, 1] and nxt[2] == [E_STATE, 0, 0], kind
        assert np.array_equal(nxt[0][1], clean[2][0][1]) and np.array_equal(nxt[0][2], clean[2][0][2])
        back = _decode_calls(pkg, dec, [[v[:1], [], []]], snd, device)[0]
        assert back[1] == [1, 0, 0] and back[2] == [0, 0, 0] and np.array_equal(back[0][0], clean[0][0][0]), kind
        dec.close()


def test_live_decode_ts_arguments_and_the_expectation(pkg):
    aus = _gold_aus()
    n_s = len(aus)
    dec = pkg.LiveDecoder(n_s, DW, DH, 1)
    snd = _Sender(n_s)
    base, rows = _lay(pkg, [snd.packets(s, a[:1]) for s, a in enumerate(aus)])
    pids = np.array(snd.pids, np.uint16)
    for field, v in (("stream", n_s), ("bytes", 187)):
        bad = rows.copy()
        bad[field][3] = v
        with pytest.raises(pkg.FerHipError, match="code -1"):
            dec.decode_ts(base, bad, pids)
    with pytest.raises(pkg.FerHipError, match="code -1"):
        dec.decode_ts(base, rows, [0x100, 0x2000, 0x102])
    pics, st = (C.c_int * n_s)(), (C.c_int * n_s)()
    lib = dec.lib
    assert lib.ferhip_decs_decode_ts(dec.h, None, 0, rows.ctypes.data, rows.size, pids.ctypes.data, None, 0, pics, st) == E_ARG
    assert lib.ferhip_decs_decode_ts(dec.h, base, 0, rows.ctypes.data, rows.size, None, None, 0, pics, st) == E_ARG
    assert lib.ferhip_decs_decode_ts(dec.h, base, 0, rows.ctypes.data, rows.size, pids.ctypes.data, None, 0, None, st) == E_ARG
    # more slices than max_pictures: refused as a whole, nothing taken, the expectation stays
    two = _Sender(n_s)
    b2, r2 = _lay(pkg, [two.packets(s, a[:2]) for s, a in enumerate(aus)])
    for device in (False, True):
        with pytest.raises(pkg.FerHipError, match="code -1"):
            _ts_call(pkg, dec, b2, r2, pids, None, device)
    _, pics, st = dec.decode_ts(base, rows, pids)
    assert (pics, st) == ([1] * n_s, [0] * n_s)
    # the expectation survives the call: the same packets again are a gap for every stream, from device memory too (one
    # expectation for both paths); behind reset_stream any counter is taken
    _, pics, st = _ts_call(pkg, dec, base, rows, pids, None, True)
    assert (pics, st) == ([0] * n_s, [E_ARG] * n_s)
    for s in range(n_s):
        dec.reset_stream(s)
    _, pics, st = _ts_call(pkg, dec, base, rows, pids, None, True)
    assert (pics, st) == ([1] * n_s, [0] * n_s)
    # the next access units carry on from what the device path left
    base, rows = _lay(pkg, [snd.packets(s, a[1:2]) for s, a in enumerate(aus)])
    _, pics, st = dec.decode_ts(base, rows, pids)
    assert (pics, st) == ([1] * n_s, [0] * n_s)
    _, pics, st = dec.decode_ts(b"", np.zeros(0, pkg.TS_RUN), pids)
    assert (pics, st) == ([0] * n_s, [0] * n_s)
    dec.close()


def test_loopback_without_the_bus(pkg):
    """an encoder's packets are decoded where ferhip_pack_ts left them: only the table of runs crosses the bus"""
    feeds = _frames()
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    cap = 1 << 18
    dst, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(24 * (S + 1))
    dec = pkg.LiveDecoder(S, W, H, 1)
    pids = 0x200 + np.arange(S)
    cc, psi_cc = np.full(S, 13, np.int64), np.zeros(S, np.int64)
    for t in range(3):
        g.encode_live([feeds[s][t] for s in range(S)], [pkg.NAL_SLICE if t else pkg.NAL_IDR] * S)
        hdr = pkg.ts_hdr(S, pts=3000 * t, pcr=3000 * t, pid=pids, pmt_pid=0x1000, cc=cc & 15, psi_cc=psi_cc & 15)
        g.pack_ts_device(hdr, dst.ptr, cap, dix.ptr, pkg.AU_PARAM_SETS | pkg.TS_PSI)
        g.sync()
        idx = dix.download(dtype=pkg.TS_AU)
        assert int(idx["offset"][S]) <= cap and int(idx["bytes"][S]) == S
        rows = np.array([(int(idx["offset"][s]), int(idx["bytes"][s]), s) for s in range(S)], pkg.TS_RUN)
        got, pics, st = dec.decode_ts(dst.ptr, rows, pids, base_on_device=True)
        assert pics == [1] * S and st == [0] * S, f"picture {t}"
        assert np.array_equal(got[0], g.get_recon()), f"picture {t}"
        psi = (idx["nal_type"][:S] == IDR)
        cc += idx["npkts"][:S] - 2 * psi
        psi_cc += psi
    assert int(cc.min()) > 13 + 32, "the counters wrapped on the way"
    dec.close()
    g.close()
