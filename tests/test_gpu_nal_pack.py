"""Annex-B framing on the device (ferhip_pack_nal, ferhip_fetch_nal, ferhip_frame_nal_blocks, csrc/fer_nalpack.hip) against
the closed form of tests/nal_model.py (pinned to the byte loops by test_nal_model_host.py), the library's host
ferhip_write_nal and, for whole streams, Oracle.encode_stream."""
import numpy as np
import pytest

import nal_model

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = 5, 1, -1
E_ARG, E_STATE = -1, -3
FILL = 0xA5

_cache = {}


def _expected():
    """the model's framing of every corpus payload, computed once"""
    if "corpus" not in _cache:
        _cache["corpus"] = [nal_model.frame_nal(t, p) for p, t in nal_model.corpus()]
    return _cache["corpus"]


def _r16(n):
    return (int(n) + 15) & ~15


def _check_layout(out, idx, want, cap):
    """index: offsets multiples of 16, the exclusive sum of the 16-rounded sizes, sizes exact; out: every entry equals
    `want`, and every byte outside the entries (rounding gaps, tail of the buffer) still holds the fill value"""
    n = len(want)
    off = 0
    touched = np.zeros(out.size, bool)
    for k in range(n):
        e = idx[k]
        assert int(e["offset"]) == off and off % 16 == 0, f"entry {k}: offset {int(e['offset'])}, expected {off}"
        assert int(e["bytes"]) == len(want[k]), f"entry {k}: {int(e['bytes'])} bytes, expected {len(want[k])}"
        assert bytes(out[off: off + len(want[k])]) == want[k], f"entry {k} ({len(want[k])} bytes) differs"
        touched[off: off + len(want[k])] = True
        off += _r16(len(want[k]))
    assert int(idx[n]["offset"]) == off and int(idx[n]["bytes"]) == n
    assert off <= cap
    assert np.all(out[:cap][~touched[:cap]] == FILL), "a byte outside the entries was written"


def test_kat_corpus_one_call(pkg):
    corpus, want = nal_model.corpus(), _expected()
    cap = sum(_r16(len(w)) for w in want) + 48
    rc, out, idx = pkg.frame_nal_blocks_raw([p for p, _ in corpus], [t for _, t in corpus], cap=cap, fill=FILL)
    assert rc == 0
    assert [int(t) for t in idx["nal_type"][:-1]] == [t for _, t in corpus]
    _check_layout(out, idx, want, cap)
    # ... and the library's own byte loop, every payload
    write_nal = pkg.load_library().ferhip_write_nal
    buf = np.empty(max(p.size for p, _ in corpus) * 3 // 2 + 16, np.uint8)
    for k, (p, t) in enumerate(corpus):
        src = np.ascontiguousarray(p)
        n = write_nal(1, t, src.ctypes.data, src.size, buf.ctypes.data)
        off = int(idx[k]["offset"])
        assert bytes(out[off: off + int(idx[k]["bytes"])]) == buf[:n].tobytes(), f"payload {k} differs from ferhip_write_nal"


def test_kat_corpus_one_payload_per_call(pkg):
    corpus, want = nal_model.corpus(), _expected()
    for k, (p, t) in enumerate(corpus):
        cap = _r16(len(want[k])) + 32
        rc, out, idx = pkg.frame_nal_blocks_raw([p], [t], cap=cap, fill=FILL)
        assert rc == 0, f"payload {k}"
        _check_layout(out, idx, [want[k]], cap)


def test_kat_payload_longer_than_the_grid(pkg):
    """more than 64 chunks: a workgroup walks several chunks of the payload; beside it an empty and a one-chunk payload"""
    rng = np.random.default_rng(7)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 4, 0xFF], np.uint8)
    long = alphabet[rng.integers(0, 8, 2 * 64 * nal_model.CHUNK + nal_model.CHUNK + 5)]
    payloads = [np.zeros(0, np.uint8), long, alphabet[rng.integers(0, 8, 1000)], np.zeros(nal_model.CHUNK * 65 + 1, np.uint8)]
    types = [1, 5, 1, 5]
    want = [nal_model.frame_nal(t, p) for p, t in zip(payloads, types)]
    cap = sum(_r16(len(w)) for w in want) + 16
    rc, out, idx = pkg.frame_nal_blocks_raw(payloads, types, cap=cap, fill=FILL)
    assert rc == 0
    _check_layout(out, idx, want, cap)
    assert pkg.frame_nal_blocks(payloads, types) == want


# ---- pictures

W, H = 176, 144
# calls x streams; intra_every 2 counts a stream's own pictures, so with AUTO types (smooth content):
#   call      0 1 2 3
#   stream 0  I P I .
#   stream 1  I P . I
#   stream 2  I . P I
#   stream 3  . . I P     its first picture comes in call 2, after set_rate(3, qp = 20)
#   stream 4  I P I P
# every call has an absent stream; call 1 has only P pictures and absent streams
TABLE = np.array([[1, 1, 1, 0, 1], [1, 1, 0, 0, 1], [1, 0, 1, 1, 1], [0, 1, 1, 1, 1]], np.uint8)
QP, QP3 = 12, 20


def _frames(pkg, S, T, w=W, h=H, noise=2):
    k = ("frames", S, T, w, h, noise)
    if k not in _cache:
        a = np.stack([np.stack([pkg.gen_frame(w, h, t, 500 + 7 * s, noise) for t in range(T)]) for s in range(S)])
        a.setflags(write=False)
        _cache[k] = a
    return _cache[k]


def _copy_rbsp(g):
    """the last picture's RBSP of every stream through ferhip_copy_rbsp"""
    stride = g.nmb * 1024 + 4096
    dst = np.zeros((g.S, stride), np.uint8)
    lens = np.zeros(g.S, np.uint32)
    g.copy_rbsp_host(dst, lens, stride)
    g.sync()
    return [bytes(dst[s, : lens[s]]) for s in range(g.S)]


def _run_table(pkg, S=5):
    """the four calls of TABLE -> per call: (nal types, rbsp via copy_rbsp, fetch_nal(0), fetch_nal(AU_PARAM_SETS), sps+pps of
    every stream at that time); per stream: the pictures it was given"""
    if "table" in _cache:
        return _cache["table"]
    feeds = _frames(pkg, S, 4)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=2)
    pos = [0] * S
    calls = []
    for c in range(4):
        if c == 2:
            g.set_rate(3, qp=QP3)  # before the first picture of stream 3: its PPS carries pic_init_qp = 14 + 20
        pics = []
        for s in range(S):
            pics.append(feeds[s][pos[s]] if TABLE[c, s] else None)
            pos[s] += int(TABLE[c, s])
        rbsp, nt = g.encode_live(pics)
        via_copy = _copy_rbsp(g)
        assert via_copy == rbsp
        plain, plain_t = g.fetch_nal()
        with_ps, ps_t = g.fetch_nal(pkg.AU_PARAM_SETS)
        again, _ = g.fetch_nal()  # packing twice, and after a flagged pack
        assert again == plain
        assert _copy_rbsp(g) == rbsp, "packing changed the RBSP"
        calls.append(dict(nt=nt, rbsp=via_copy, plain=plain, plain_t=plain_t, with_ps=with_ps, ps_t=ps_t,
                          ps=[g.sps_pps(s) for s in range(S)]))
    assert g.status() == [0] * S
    _cache["table"] = (g, calls, [feeds[s][: pos[s]] for s in range(S)])
    return _cache["table"]


def test_pictures_fetch_equals_write_nal(pkg):
    g, calls, _ = _run_table(pkg)
    for c, r in enumerate(calls):
        for s in range(g.S):
            if not TABLE[c, s]:
                assert r["nt"][s] == NONE and r["plain"][s] == b"" and r["plain_t"][s] == 0
                assert r["with_ps"][s] == b"" and r["ps_t"][s] == 0
                continue
            unit = g.write_nal(r["nt"][s], r["rbsp"][s])
            assert r["plain"][s] == unit, f"call {c} stream {s}"
            assert r["plain_t"][s] == r["nt"][s] == r["ps_t"][s]
            if r["nt"][s] == IDR:
                sps, pps = r["ps"][s]
                assert r["with_ps"][s] == sps + pps + unit, f"call {c} stream {s}: SPS + PPS + slice"
            else:
                assert r["with_ps"][s] == unit, f"call {c} stream {s}: a P entry carries no parameter sets"
    types = ["".join({5: "I", 1: "P", -1: "."}[calls[c]["nt"][s]] for c in range(4)) for s in range(g.S)]
    assert types == ["IPI.", "IP.I", "I.PI", "..IP", "IPIP"]
    # stream 3 carries its own PPS
    assert calls[2]["ps"][3][1] != calls[2]["ps"][0][1]
    assert calls[2]["with_ps"][3].startswith(calls[2]["ps"][3][0] + calls[2]["ps"][3][1])


def test_pictures_streams_equal_oracle(pkg, fo):
    """sps_pps(s) + the concatenated units of stream s = Oracle.encode_stream of exactly the pictures it was given.
    The oracle streams of this test hold no emulation prevention byte at all (counted: 0 in each of the five streams, like
    the committed QCIF goldens), so this test pins the plumbing -- which stream, which type, which bytes, which order --
    and the known-answer tests above pin the escaping."""
    g, calls, given = _run_table(pkg)
    for s in range(g.S):
        o = fo.Oracle(W, H, qp=QP3 if s == 3 else QP, window=16, maxdiff=3, intra_every=2)
        ref, _ = o.encode_stream(given[s])
        o.close()
        sps, pps = calls[3]["ps"][s]
        mine = sps + pps + b"".join(calls[c]["plain"][s] for c in range(4))
        assert mine == ref, f"stream {s}"
        print(f"stream {s}: {len(ref)} bytes, {ref.count(bytes([0, 0, 3]))} emulation prevention bytes")


def test_device_path_17_streams(pkg):
    S = 17
    feeds = _frames(pkg, S, 2)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    stride = g.nmb * 1024 + 4096
    cap = S * _r16(stride) + 64
    dst = pkg.DeviceBuffer(cap)
    index = pkg.DeviceBuffer(16 * (S + 1))
    fill = np.full(cap, FILL, np.uint8)
    for t, present in enumerate(([1] * S, [int(s % 5 != 2) for s in range(S)])):
        g.set_frames_live(feeds[:, t], present)
        _, _, _, nt = g.encode_picture_device([0 if p else NONE for p in present])
        before = _copy_rbsp(g)
        for flags in (0, pkg.AU_PARAM_SETS):
            want = []
            for s in range(S):
                if not present[s]:
                    want.append(b"")
                    continue
                unit = g.write_nal(nt[s], before[s])
                want.append(b"".join(g.sps_pps(s)) + unit if flags and nt[s] == IDR else unit)
            outs = []
            for rep in range(2):
                dst.upload(fill)
                g.pack_nal_device(dst.ptr, index.ptr, cap, flags)
                g.sync()
                out, idx = dst.download(), index.download(dtype=pkg.AU)
                outs.append(out)
                off = 0
                touched = np.zeros(cap, bool)
                for s in range(S):
                    assert (int(idx[s]["offset"]), int(idx[s]["bytes"])) == (off, len(want[s])), f"picture {t} stream {s}"
                    assert int(idx[s]["nal_type"]) == (nt[s] if present[s] else 0)
                    assert bytes(out[off: off + len(want[s])]) == want[s], f"picture {t} stream {s} flags {flags}"
                    touched[off: off + len(want[s])] = True
                    off += _r16(len(want[s]))
                assert (int(idx[S]["offset"]), int(idx[S]["bytes"])) == (off, sum(present))
                assert np.all(out[~touched] == FILL)
            assert np.array_equal(outs[0], outs[1])
            assert _copy_rbsp(g) == before, "packing changed the RBSP"
    assert [t for t in nt if t != NONE] == [SLICE] * sum(present)
    assert g.status() == [0] * S
    g.close()


def test_edges(pkg):
    S = 3
    feeds = _frames(pkg, S, 3)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    dst = pkg.DeviceBuffer(1 << 20)
    index = pkg.DeviceBuffer(16 * (S + 1))
    lib = g.lib
    # before the context's first picture
    assert lib.ferhip_pack_nal(g.ctx, 0, dst.ptr, 1 << 20, index.ptr) == E_STATE
    assert g.fetch_nal_raw(1 << 20)[0] == E_STATE
    g.set_rate(1, qp=20)
    rbsp, nt = g.encode_live([feeds[s][0] for s in range(S)])
    units = [g.write_nal(nt[s], rbsp[s]) for s in range(S)]
    offs = np.concatenate(([0], np.cumsum([_r16(len(u)) for u in units]))).astype(int)
    total = int(offs[S])
    # bad arguments
    assert lib.ferhip_pack_nal(g.ctx, 0, dst.ptr + 8, 1 << 20, index.ptr) == E_ARG
    assert lib.ferhip_pack_nal(g.ctx, 2, dst.ptr, 1 << 20, index.ptr) == E_ARG
    # cap one byte short of the total: the last entry stays out, the others and the index are exact
    fill = np.full(total + 64, FILL, np.uint8)
    dst.upload(fill)
    assert lib.ferhip_pack_nal(g.ctx, 0, dst.ptr, total - 1, index.ptr) == 0
    g.sync()
    out, idx = dst.download(total + 64), index.download(dtype=pkg.AU)
    for s in range(S):
        assert (int(idx[s]["offset"]), int(idx[s]["bytes"]), int(idx[s]["nal_type"])) == (offs[s], len(units[s]), nt[s])
    assert (int(idx[S]["offset"]), int(idx[S]["bytes"])) == (total, S - 1)
    for s in range(S - 1):
        assert bytes(out[offs[s]: offs[s] + len(units[s])]) == units[s]
    assert np.all(out[offs[S - 1]:] == FILL), "the entry that does not fit, or a byte at or beyond cap, was written"
    # a cap that cuts the second entry's 16-byte slots: only the first entry is written
    dst.upload(fill)
    assert lib.ferhip_pack_nal(g.ctx, 0, dst.ptr, int(offs[2]) - 1, index.ptr) == 0
    g.sync()
    out, idx = dst.download(total + 64), index.download(dtype=pkg.AU)
    assert (int(idx[S]["offset"]), int(idx[S]["bytes"])) == (total, 1)
    assert [int(b) for b in idx["bytes"][:S]] == [len(u) for u in units]
    assert bytes(out[: len(units[0])]) == units[0] and np.all(out[offs[1]:] == FILL)
    rc, _, hidx = g.fetch_nal_raw(total - 1)
    assert rc == E_ARG and int(hidx[S]["offset"]) == total and [int(b) for b in hidx["bytes"][:S]] == [len(u) for u in units]
    with pytest.raises(pkg.FerHipError, match="code -1"):
        g.fetch_nal(cap=total - 1)
    assert g.fetch_nal(cap=total)[0] == units
    # cap 0: nothing is written, the index is true
    dst.upload(fill)
    assert lib.ferhip_pack_nal(g.ctx, 0, None, 0, index.ptr) == 0
    assert lib.ferhip_pack_nal(g.ctx, 0, dst.ptr, 0, index.ptr) == 0
    g.sync()
    idx = index.download(dtype=pkg.AU)
    assert (int(idx[S]["offset"]), int(idx[S]["bytes"])) == (total, 0)
    assert np.all(dst.download(total + 64) == FILL)
    # a call in which every stream is absent: total 0
    rbsp0, nt0 = g.encode_live([None] * S)
    assert rbsp0 == [b""] * S
    got, types = g.fetch_nal(pkg.AU_PARAM_SETS)
    assert got == [b""] * S and types == [0] * S
    rc, _, hidx = g.fetch_nal_raw(0)
    assert rc == 0 and int(hidx[S]["offset"]) == 0 and int(hidx[S]["bytes"]) == 0
    # reset_stream with the flag: the next IDR of the slot carries the PPS of its new base QP
    rbsp, nt = g.encode_live([feeds[s][1] for s in range(S)])
    g.fetch_nal(pkg.AU_PARAM_SETS)  # the table has been in use before the reset
    old_pps = g.sps_pps(1)[1]
    g.reset_stream(1)
    g.set_rate(1, qp=17)
    rbsp, nt = g.encode_live([feeds[s][2] for s in range(S)])
    assert nt == [SLICE, IDR, SLICE]
    sps, pps = g.sps_pps(1)
    assert pps != old_pps
    got, types = g.fetch_nal(pkg.AU_PARAM_SETS)
    assert got[1] == sps + pps + g.write_nal(IDR, rbsp[1])
    assert got[0] == g.write_nal(SLICE, rbsp[0]) and got[2] == g.write_nal(SLICE, rbsp[2])
    assert g.status() == [0] * S
    g.close()


def test_one_larger_picture(pkg):
    """1280x720 I picture at QP 12, two streams: a stream spans many chunks (and more of them than a payload has workgroups)"""
    w, h, S = 1280, 720, 2
    feeds = _frames(pkg, S, 1, w, h, noise=6)
    g = pkg.FerHip(w, h, S, qp=12, window=16, maxdiff=3, intra_every=30)
    g.set_frames(feeds[:, 0])
    rbsp, nt = g.encode_picture([IDR] * S)
    assert nt == [IDR] * S and g.status() == [0] * S
    print("RBSP bytes:", [len(r) for r in rbsp])
    assert min(len(r) for r in rbsp) > 2 * nal_model.CHUNK
    got, types = g.fetch_nal()
    assert types == nt
    for s in range(S):
        assert got[s] == g.write_nal(IDR, rbsp[s]), f"stream {s}"
    g.close()
