"""Fragmented MP4 segments on the device (ferhip_mp4_open / _append / _close / _fetch, ferhip_mp4_blocks,
ferhip_write_mp4_init, csrc/fer_mp4.hip) against tests/mp4_model.py (pinned on the host by test_mp4_model_host.py) applied to
the samples that tests/nal_model.py and ferhip_fetch_nal(FERHIP_AU_AVCC) give, and the live decoder on fragments in host
memory (ferhip_decs_decode_mp4) against ferhip_decs_decode on the same units as length-prefixed chunks.  Everything is
bit-exact, the bytes the kernels must not touch included."""
import numpy as np
import pytest

import avcc_model
import mp4_model as mm
import nal_model

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = 5, 1, -1
E_ARG, E_STATE = -1, -3
FILL = 0xA5

_cache = {}


def _kat():
    """-> (payloads, types, samples): sample k = the length-prefixed entry of payload k"""
    if "kat" not in _cache:
        payloads = mm.kat_payloads()
        types = [(SLICE, IDR)[k % 3 == 0] for k in range(len(payloads))]
        samples = [mm.sample_of(nal_model.frame_nal(t, p)) for t, p in zip(types, payloads)]
        _cache["kat"] = (payloads, types, samples)
    return _cache["kat"]


def _hdrs(pkg, n):
    k = np.arange(n)
    return pkg.mp4_hdr(n, decode_time=(1 << 32) + 0x12345678 + 90000 * k, sequence=0x01020304 + k, duration=3000 + k)


def _hdr_dict(h):
    return {f: int(h[f]) for f in ("decode_time", "sequence", "duration")}


def _check_regions(out, idx, groups, group_types, hdr, K, stride, what):
    """every region and every index entry against the model; out is [nseg][stride]"""
    nseg = len(groups)
    streams = total = faults = 0
    for g in range(nseg):
        want, (nbytes, ns, first, fault) = mm.region(groups[g], [t == IDR for t in group_types[g]], _hdr_dict(hdr[g]), K, stride, FILL)
        off = g * stride if (ns or fault) else 0
        assert tuple(int(v) for v in idx[g]) == (off, nbytes, ns, first, fault), f"{what}: index[{g}] = {idx[g]}"
        bad = np.flatnonzero(out[g] != np.frombuffer(want, np.uint8))
        assert bad.size == 0, f"{what}: region {g}: {bad.size} bytes differ, the first at {int(bad[0])}"
        streams += ns > 0
        total += ns
        faults |= fault
    assert tuple(int(v) for v in idx[nseg]) == (0, streams, total, 0, faults), f"{what}: index[S] = {idx[nseg]}"


def _groups(items, m):
    return [items[g: g + m] for g in range(0, len(items), m)]


@pytest.mark.parametrize("K", (1, 2, 3, 6))
def test_kat_blocks_equal_the_model(pkg, K):
    payloads, types, samples = _kat()
    assert len(nal_model.frame_nal(5, payloads[-1])) > 4096 and any(len(s) > 3 * 4096 for s in samples)
    for m in range(1, K + 1):
        groups, gtypes = _groups(samples, m), _groups(types, m)
        stride = (mm.data_offset(K) + max(sum(len(p) for p in g) for g in groups) + 15 + 16) & ~15
        hdr = _hdrs(pkg, len(groups))
        rc, out, idx = pkg.mp4_blocks_raw(payloads, types, m, K, hdr, stride, fill=FILL)
        assert rc == 0
        _check_regions(out, idx, groups, gtypes, hdr, K, stride, f"K {K}, m {m}")
        assert int(idx[len(groups)]["fault"]) == 0
    # the front of a region: the free box's content is zero, whatever the buffer held
    D = mm.data_offset(K)
    n = int(idx[0]["nsamples"])
    assert bytes(out[0][88 + 12 * n + 4: 88 + 12 * n + 8]) == b"free" and not out[0][88 + 12 * n + 8: D - 8].any()


def test_kat_one_payload_per_call_and_refusals(pkg):
    payloads, types, samples = _kat()
    for k in (0, 1, 6, 7, 17, len(payloads) - 1):
        hdr = _hdrs(pkg, 1)
        stride = (mm.data_offset(1) + len(samples[k]) + 15 + 16) & ~15
        rc, out, idx = pkg.mp4_blocks_raw([payloads[k]], [types[k]], 1, 1, hdr, stride, fill=FILL)
        assert rc == 0
        _check_regions(out, idx, [[samples[k]]], [[types[k]]], hdr, 1, stride, f"payload {k}")
    two, tt, hdr = [payloads[3], payloads[4]], [1, 5], _hdrs(pkg, 1)
    D = mm.data_offset(2)
    assert pkg.mp4_blocks_raw(two, tt, 2, 2, hdr, 4096)[0] == 0
    assert pkg.mp4_blocks_raw(two, tt, 2, 2, hdr, D + 16)[0] == 0  # the smallest stride
    for m, K, stride in ((2, 0, 4096), (2, 4097, 1 << 16), (0, 2, 4096), (2, 2, 4096 + 8), (2, 2, D)):
        assert pkg.mp4_blocks_raw(two, tt, m, K, hdr, stride)[0] == E_ARG, (m, K, stride)
    lib = pkg.load_library()
    lens, nt, idx = np.array([4], np.uint32), np.array([1], np.int32), np.zeros(2, pkg.MP4_SEG)
    src, out = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    args = [src.ctypes.data, 16, lens.ctypes.data, nt.ctypes.data, 1, 1, 1, hdr.ctypes.data, out.ctypes.data, 256, idx.ctypes.data]
    assert lib.ferhip_mp4_blocks(*args) == 0
    for k, v in ((2, None), (3, None), (7, None), (8, None), (10, None), (4, 0), (9, 1 << 31)):  # (refused before out is touched)
        bad = list(args)
        bad[k] = v
        assert lib.ferhip_mp4_blocks(*bad) == E_ARG, k


def test_overflow_faults_and_leaves_the_rest_alone(pkg):
    payloads, types, samples = _kat()
    K, m = 3, 3
    D = mm.data_offset(K)
    # three segments of three samples; the middle one is made to need a multiple of 16 exactly
    pick = [3, 4, 5, 20, 7, 8, 9, 10, 11]
    pl, tt, sm = [payloads[k] for k in pick], [types[k] for k in pick], [samples[k] for k in pick]
    need = [D + sum(len(p) for p in g) for g in _groups(sm, m)]
    pad = -need[1] % 16
    pl[5] = np.concatenate([pl[5], np.full(pad, 0x77, np.uint8)])
    sm[5] = mm.sample_of(nal_model.frame_nal(tt[5], pl[5]))
    groups, gtypes = _groups(sm, m), _groups(tt, m)
    need = [D + sum(len(p) for p in g) for g in groups]
    assert need[1] % 16 == 0 and need[1] > need[0] and need[1] > need[2]
    hdr = _hdrs(pkg, 3)
    rc, out, idx = pkg.mp4_blocks_raw(pl, tt, m, K, hdr, need[1], fill=FILL)
    assert rc == 0 and [int(f) for f in idx["fault"]] == [0, 0, 0, 0]
    _check_regions(out, idx, groups, gtypes, hdr, K, need[1], "a stride exactly large enough")
    # 16 bytes short for the middle segment's last sample: fault 1, two samples, the tail and both neighbours untouched
    rc, out, idx = pkg.mp4_blocks_raw(pl, tt, m, K, hdr, need[1] - 16, fill=FILL)
    assert rc == 0 and [int(f) for f in idx["fault"]] == [0, 1, 0, 1] and [int(n) for n in idx["nsamples"]] == [3, 2, 3, 8]
    _check_regions(out, idx, groups, gtypes, hdr, K, need[1] - 16, "16 bytes short")
    # a second sample that does not fit and a third that would: from the faulted sample on nothing more is added
    p3, t3 = [payloads[21], payloads[7], payloads[0]], [IDR, SLICE, SLICE]
    s3 = [mm.sample_of(nal_model.frame_nal(t, p)) for t, p in zip(t3, p3)]
    stride = (D + len(s3[0]) + 8 + 15) & ~15
    assert len(s3[2]) == 5 and stride - D - len(s3[0]) >= 8
    rc, out, idx = pkg.mp4_blocks_raw(p3, t3, m, K, hdr[:1], stride, fill=FILL)
    assert rc == 0 and tuple(int(v) for v in idx[0]) == (0, D + len(s3[0]), 1, IDR, 1)
    _check_regions(out, idx, [s3], [t3], hdr, K, stride, "short for the second sample")
    # a first sample that does not fit: offset and fault only, nothing written
    rc, out, idx = pkg.mp4_blocks_raw(pl, tt, m, K, hdr, D + 16, fill=FILL)
    assert rc == 0 and tuple(int(v) for v in idx[1]) == (D + 16, 0, 0, 0, 1) and np.all(out[1] == FILL)
    _check_regions(out, idx, groups, gtypes, hdr, K, D + 16, "the smallest stride")
    # K + 1 samples: fault 2, beside clean segments (the last one is shorter)
    pl4, tt4, sm4 = pl + pl[:2], tt + tt[:2], sm + sm[:2]
    rc, out, idx = pkg.mp4_blocks_raw(pl4, tt4, 4, K, hdr, 1 << 15, fill=FILL)
    assert rc == 0 and [int(f) for f in idx["fault"]] == [2, 2, 0, 2] and [int(n) for n in idx["nsamples"]] == [3, 3, 3, 9]
    _check_regions(out, idx, _groups(sm4, 4), _groups(tt4, 4), hdr, K, 1 << 15, "K + 1 samples")


# ---- pictures

W, H, S = 64, 48, 9
QP = 8
STRIDE = 1 << 16
KINDS = (IDR, SLICE, SLICE, SLICE, IDR, SLICE)


def _frames():
    if "frames" not in _cache:
        a = np.random.default_rng(5190).integers(0, 256, (S, len(KINDS), W * H * 3 // 2)).astype(np.uint8)  # noise: nothing is predicted
        a.setflags(write=False)
        _cache["frames"] = a
    return _cache["frames"]


def _present(t, s):
    return s != 7 and not (s == 3 and t in (1, 2, 4))


def _encode(g, pkg, t, present=_present):
    feeds = _frames()
    return g.encode_live([feeds[s][t] if present(t, s) else None for s in range(S)], [KINDS[t]] * S)


def _want_segment(per_picture, s, hdr, K):
    """per_picture = list of (entries, types) of ferhip_fetch_nal -> the model's segment of stream s, b"" without a sample"""
    samples = [e[s] for e, _ in per_picture if e[s]]
    idr = [t[s] == IDR for e, t in per_picture if e[s]]
    return mm.segment(samples, idr, hdr, K) if samples else b""


@pytest.mark.parametrize("ps", (0, 1))
def test_context_segments_equal_the_model_on_fetch_nal_entries(pkg, ps):
    """IDR P P | P IDR P in two segments back to back, stream 3 absent in some calls and stream 7 throughout: the first
    segment through ferhip_mp4_close and a copy of the regions, the second through ferhip_mp4_fetch"""
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    K = 3
    dst, dix = pkg.DeviceBuffer(S * STRIDE), pkg.DeviceBuffer(24 * (S + 1))
    hdr = pkg.mp4_hdr(S, decode_time=(1 << 33) + 1000 * np.arange(S), sequence=1 + np.arange(S), duration=3000)
    per = []
    dst.upload(np.full(S * STRIDE, FILL, np.uint8))
    g.mp4_open(hdr, K, dst.ptr, STRIDE, ps)
    for t in range(3):
        _, nt = _encode(g, pkg, t)
        assert [n for n in nt] == [KINDS[t] if _present(t, s) else NONE for s in range(S)]
        g.mp4_append()
        per.append(g.fetch_nal(pkg.AU_AVCC | ps))  # behind the append: the other framings change nothing
    g.mp4_close_device(dix.ptr)
    g.sync()
    out, idx = dst.download().reshape(S, STRIDE), dix.download(dtype=pkg.MP4_SEG)
    assert len(per[0][0][0]) > 4096, "an IDR sample exceeds one 4096-byte chunk"
    if ps:
        sps, pps = g.sps_pps(0)
        assert per[0][0][0].startswith(mm.u32(len(sps) - 4) + sps[4:] + mm.u32(len(pps) - 4) + pps[4:])
    nsamples = []
    for s in range(S):
        want = _want_segment(per, s, _hdr_dict(hdr[s]), K)
        n = sum(1 for e, _ in per if e[s])
        nsamples.append(n)
        first = next((t[s] for e, t in per if e[s]), 0)
        assert tuple(int(v) for v in idx[s]) == ((s * STRIDE, len(want), n, first, 0) if n else (0, 0, 0, 0, 0)), f"index[{s}]"
        assert bytes(out[s][: len(want)]) == want and np.all(out[s][len(want):] == FILL), f"stream {s}"
        if want:
            got, fault = mm.demux(want)
            assert fault == 0 and got == [e[s] for e, _ in per if e[s]]
    assert nsamples == [3, 3, 3, 1, 3, 3, 3, 0, 3]
    assert tuple(int(v) for v in idx[S]) == (0, 8, sum(nsamples), 0, 0)
    # the second segment: the caller advances the header
    hdr2 = hdr.copy()
    hdr2["decode_time"] += np.array(nsamples, np.uint64) * 3000
    hdr2["sequence"] += 1
    dst.upload(np.full(S * STRIDE, FILL, np.uint8))
    g.mp4_open(hdr2, K, dst.ptr, STRIDE, ps)
    per = []
    for t in range(3, 6):
        _encode(g, pkg, t)
        per.append(g.fetch_nal(pkg.AU_AVCC | ps))
        g.mp4_append()
    rc, buf, idx = g.mp4_fetch_raw(S * STRIDE, fill=FILL)
    assert rc == 0
    at = 0
    regions = dst.download().reshape(S, STRIDE)
    for s in range(S):
        want = _want_segment(per, s, _hdr_dict(hdr2[s]), K)
        n = sum(1 for e, _ in per if e[s])
        first = next((t[s] for e, t in per if e[s]), 0)
        assert tuple(int(v) for v in idx[s]) == ((at, len(want), n, first, 0) if n else (0, 0, 0, 0, 0)), f"segment 2: index[{s}]"
        assert bytes(buf[at: at + len(want)]) == want, f"segment 2: stream {s}"
        assert bytes(regions[s][: len(want)]) == want and np.all(regions[s][len(want):] == FILL), "fetch is close plus copies"
        at += len(want)
    assert np.all(buf[at:] == FILL) and [int(idx[s]["first_nal_type"]) for s in (0, 3)] == [SLICE, SLICE]
    assert g.status() == [0] * S
    g.close()


def test_context_mixing_reset_and_call_order(pkg):
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    lib = g.lib
    K = 4
    dst, dix = pkg.DeviceBuffer(S * STRIDE), pkg.DeviceBuffer(24 * (S + 1))
    hdr = pkg.mp4_hdr(S, decode_time=7, sequence=3, duration=1001)

    def op(flags=0, k=K, h=hdr, d=dst.ptr, st=STRIDE, c=g.ctx):
        return lib.ferhip_mp4_open(c, flags, k, h.ctypes.data if h is not None else None, d, st)

    D = mm.data_offset(K)
    for kw in (dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=1 | 16), dict(k=0), dict(k=4097), dict(h=None), dict(d=None),
               dict(d=dst.ptr + 8), dict(st=STRIDE + 8), dict(st=D), dict(st=1 << 31), dict(c=None)):
        assert op(**kw) == E_ARG, kw
    assert lib.ferhip_mp4_append(g.ctx) == E_STATE and lib.ferhip_mp4_close(g.ctx, dix.ptr) == E_STATE
    assert g.mp4_fetch_raw(STRIDE)[0] == E_STATE
    assert lib.ferhip_mp4_append(None) == E_ARG and lib.ferhip_mp4_close(None, dix.ptr) == E_ARG
    assert op() == 0 and op() == E_STATE
    assert lib.ferhip_mp4_append(g.ctx) == E_STATE, "before the context's first picture"
    assert lib.ferhip_mp4_close(g.ctx, None) == E_ARG and lib.ferhip_mp4_close(g.ctx, dix.ptr + 4) == E_ARG
    assert lib.ferhip_mp4_fetch(g.ctx, None, 16, dix.ptr) == E_ARG
    dst.upload(np.full(S * STRIDE, FILL, np.uint8))
    per = []
    for t in range(4):
        if t == 2:
            g.reset_stream(4)  # inside the segment: the stream's next sample is an IDR slice
        g.encode_live([_frames()[s][t] for s in range(S)], [pkg.NAL_IDR if t == 0 else pkg.NAL_AUTO if (t, s) == (2, 4) else pkg.NAL_SLICE for s in range(S)])
        # the other framings in between, in front of and behind the append
        per.append(g.fetch_nal(pkg.AU_AVCC))
        g.fetch_rtp(pkg.rtp_hdr(S), 128, 1)
        g.mp4_append()
        assert lib.ferhip_mp4_append(g.ctx) == E_STATE, "twice behind one encode call"
        g.fetch_ts(pkg.ts_hdr(S), 9)
        g.fetch_nal(pkg.AU_PARAM_SETS)
    assert per[2][1][4] == IDR and per[2][1][0] == SLICE
    # short of room: the index is filled, the call is refused, and the segment is closed all the same
    rc, _, idx = g.mp4_fetch_raw(100)
    assert rc == E_ARG and [int(n) for n in idx["nsamples"]] == [4] * S + [4 * S]
    assert lib.ferhip_mp4_close(g.ctx, dix.ptr) == E_STATE
    out = dst.download().reshape(S, STRIDE)
    at = 0
    for s in range(S):
        want = _want_segment(per, s, _hdr_dict(hdr[s]), K)
        assert int(idx[s]["offset"]) == at and int(idx[s]["bytes"]) == len(want)
        assert bytes(out[s][: len(want)]) == want and np.all(out[s][len(want):] == FILL), f"stream {s}"
        at += len(want)
    # K + 1 pictures and a stride too small for a second one, in a context
    small = (mm.data_offset(1) + max(len(e) for e in per[3][0]) + 15 + 16) & ~15
    g.mp4_open(hdr, 1, dst.ptr, small, 0)
    dst.upload(np.full(S * STRIDE, FILL, np.uint8))
    g.mp4_append()
    g.encode_live([_frames()[s][4] for s in range(S)], [pkg.NAL_SLICE] * S)
    g.mp4_append()
    rc, buf, idx = g.mp4_fetch_raw(S * small, fill=FILL)
    assert rc == 0 and [int(f) for f in idx["fault"]] == [2] * S + [2] and [int(n) for n in idx["nsamples"]] == [1] * S + [S]
    flat = dst.download()
    for s in range(S):
        want = mm.segment([per[3][0][s]], [False], _hdr_dict(hdr[s]), 1)
        assert bytes(flat[s * small: s * small + len(want)]) == want and np.all(flat[s * small + len(want): (s + 1) * small] == FILL)
    assert np.all(flat[S * small:] == FILL)
    # destroy with a segment open
    g.mp4_open(hdr, 2, dst.ptr, STRIDE, 1)
    g.mp4_append()
    g.close()


def test_write_mp4_init(pkg):
    g = pkg.FerHip(W, H, 2, qp=QP)
    for s in range(2):
        sps, pps = g.sps_pps(s)
        ini = g.mp4_init(s, 90000)
        assert ini == mm.init_segment(sps[4:], pps[4:], W, H, 90000)
        off, n = mm.find_avcc(ini)
        assert ini[off: off + n] == g.avcc_config(s)
        mm.check_sizes(ini)
    assert g.mp4_init(2, 90000) == b"" and g.mp4_init(-1, 90000) == b"" and g.mp4_init(0, 0) == b""
    full = len(g.mp4_init(0, 30))
    assert g.mp4_init(0, 30, cap=full - 1) == b"" and len(g.mp4_init(0, 30, cap=full)) == full
    g.close()
    g = pkg.FerHip(64, 48, 1, qp=QP)
    g.set_display_size(50, 38)
    sps, pps = g.sps_pps(0)
    assert g.mp4_init(0, 25) == mm.init_segment(sps[4:], pps[4:], 50, 38, 25)
    g.close()


# ---- the way in: fragments in host memory into the live decoder

GOLDENS = ("qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264")
HDR = dict(decode_time=(1 << 32) + 90000, sequence=0x01020304, duration=3000)


def _gold_samples(name):
    import ts_model as tm
    from conftest import golden_bytes
    if ("gs", name) not in _cache:
        aus = tm.access_units_of(golden_bytes(name))
        _cache[("gs", name)] = ([avcc_model.annexb_to_avcc(e) for e, _ in aus], [t for _, t in aus])
    return _cache[("gs", name)]


def _gold_run(name, m=2, K=3):
    samples, types = _gold_samples(name)
    return b"".join(mm.segment(samples[g: g + m], [t == IDR for t in types[g: g + m]], dict(HDR, sequence=g), K) for g in range(0, len(samples), m))


def _lay(pkg, per_stream_runs):
    """every stream's runs interleaved at odd offsets -> (base, rows)"""
    buf, rows = bytearray(b"\xEE" * 3), []
    k = 0
    while any(per_stream_runs):
        for s, runs in enumerate(per_stream_runs):
            if runs:
                r = runs.pop(0)
                rows.append((len(buf), len(r), s))
                buf += r + b"\xEE" * (1 + k % 3)
                k += 1
    return bytes(buf), np.array(rows, pkg.MP4_RUN) if rows else np.zeros(0, pkg.MP4_RUN)


# ---- the live decoder

DW, DH = 176, 144


def _gold_aus():
    """three streams (a, b, a) as access units (sample, type)"""
    if "aus" not in _cache:
        a, b = (list(zip(*_gold_samples(n))) for n in (GOLDENS[0], GOLDENS[3]))
        _cache["aus"] = [a, b, a]
    return _cache["aus"]


def _fragments_of(aus, seq=1):
    """one fragment for the access units of a call, b"" for none"""
    return mm.segment([p for p, _ in aus], [t == IDR for _, t in aus], dict(HDR, sequence=seq), max(len(aus), 1)) if aus else b""


def _mp4_call(pkg, dec, base, rows, target, L=4):
    return dec.decode_mp4(base, rows, L, target)


def _decode_calls(pkg, dec, calls, mp4=False):
    """calls: per call a list per stream of access units; through decode_mp4, else the same units as length-prefixed chunks"""
    out = []
    for call in calls:
        target = np.full((dec.P, dec.S, dec.fsz), FILL, np.uint8)
        if mp4:
            base, rows = _lay(pkg, [mm.cut_runs(_fragments_of(aus)) if aus else [] for aus in call])
            _, pics, st = _mp4_call(pkg, dec, base, rows, target)
        else:
            dec.set_input(pkg.IN_AVCC, 4)
            _, pics, st = dec.decode([b"".join(p for p, _ in aus) or None for aus in call], target)
            dec.set_input(pkg.IN_ANNEXB, 4)
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


def test_live_decode_mp4_equals_length_prefixed_chunks(pkg):
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
        dec = pkg.LiveDecoder(n_s, DW, DH, maxpic)
        _same(ref, _decode_calls(pkg, dec, calls, True), name)
        dec.close()
    # mixed with the other decode calls on one decoder
    calls = schedules["one_picture_per_call"][0]
    dec = pkg.LiveDecoder(n_s, DW, DH, 1)
    ref = _decode_calls(pkg, dec, calls)
    dec.close()
    dec = pkg.LiveDecoder(n_s, DW, DH, 1)
    got = []
    for k, call in enumerate(calls):
        got += _decode_calls(pkg, dec, [call], bool(k & 1))
    dec.close()
    _same(ref, got, "alternating")


def test_live_decode_mp4_faults_are_isolated(pkg):
    aus = _gold_aus()
    n_s = len(aus)
    v = aus[0]  # I P P P
    clean_calls = [[a[:1] for a in aus], [v[1:3], aus[1][1:2], v[1:3]], [v[3:4], aus[1][2:3], v[3:4]]]
    dec = pkg.LiveDecoder(n_s, DW, DH, 2)
    clean = _decode_calls(pkg, dec, clean_calls, True)
    dec.close()
    assert [npic for _, npic, _ in clean] == [[1, 1, 1], [2, 1, 2], [1, 1, 1]] and all(st == [0] * n_s for _, _, st in clean)
    fa, fb = _fragments_of(v[1:2], 2), _fragments_of(v[2:3], 3)
    D = mm.data_offset(1)

    def damage(kind):
        """stream 0's second fragment of call 1"""
        b = bytearray(fb)
        if kind == "truncated":
            return fa + bytes(b[: D - 8])
        if kind == "malformed":
            b[D - 8: D - 4] = mm.u32(len(fb) - D + 7)  # the mdat one byte short of its sample
        if kind == "unsupported":
            b[76] = 2  # the trun's version
        if kind == "overrun":
            b[D: D + 4] = mm.u32(len(v[2][0]))  # the unit claims four bytes more than the sample holds
        return fa + bytes(b)

    for kind in ("truncated", "malformed", "unsupported", "overrun"):
        dec = pkg.LiveDecoder(n_s, DW, DH, 2)
        _decode_calls(pkg, dec, clean_calls[:1], True)
        per = [mm.cut_runs(damage(kind)), mm.cut_runs(_fragments_of(clean_calls[1][1])), mm.cut_runs(_fragments_of(clean_calls[1][2]))]
        assert mm.demux_runs(per[0])[1] == {"truncated": 4, "malformed": 2, "unsupported": 3, "overrun": 1}[kind]
        target = np.full((2, n_s, dec.fsz), FILL, np.uint8)
        _, pics, st = _mp4_call(pkg, dec, *_lay(pkg, per), target)
        assert (pics, st) == ([1, 1, 2], [E_ARG, 0, 0]), kind
        assert np.array_equal(target[0, 0], clean[1][0][0][0]), f"{kind}: the picture in front of the fault is delivered"
        for s in (1, 2):
            assert np.array_equal(target[: pics[s], s], clean[1][0][s]), f"{kind}: stream {s} is untouched"
        # a P slice behind the fault is refused until the next IDR slice
        nxt = _decode_calls(pkg, dec, [[v[3:4], aus[1][2:3], v[3:4]]], True)[0]
        assert nxt[1] == [0, 1, 1] and nxt[2] == [E_STATE, 0, 0], kind
        assert np.array_equal(nxt[0][1], clean[2][0][1]) and np.array_equal(nxt[0][2], clean[2][0][2])
        back = _decode_calls(pkg, dec, [[v[:1], [], []]], True)[0]
        assert back[1] == [1, 0, 0] and back[2] == [0, 0, 0] and np.array_equal(back[0][0], clean[0][0][0]), kind
        dec.close()


def test_live_decode_mp4_arguments(pkg):
    import ctypes as C
    aus = _gold_aus()
    n_s = len(aus)
    dec = pkg.LiveDecoder(n_s, DW, DH, 1)
    base, rows = _lay(pkg, [mm.cut_runs(_fragments_of(a[:1])) for a in aus])
    bad = rows.copy()
    bad["stream"][1] = n_s
    with pytest.raises(pkg.FerHipError, match="code -1"):
        dec.decode_mp4(base, bad)
    for L in (0, 3, 8):
        with pytest.raises(pkg.FerHipError, match="code -1"):
            dec.decode_mp4(base, rows, L)
    pics, st = (C.c_int * n_s)(), (C.c_int * n_s)()
    lib = dec.lib
    assert lib.ferhip_decs_decode_mp4(dec.h, None, 0, rows.ctypes.data, rows.size, 4, None, 0, pics, st) == E_ARG
    assert lib.ferhip_decs_decode_mp4(dec.h, base, 0, None, rows.size, 4, None, 0, pics, st) == E_ARG
    assert lib.ferhip_decs_decode_mp4(dec.h, base, 0, rows.ctypes.data, rows.size, 4, None, 0, None, st) == E_ARG
    assert lib.ferhip_decs_decode_mp4(None, base, 0, rows.ctypes.data, rows.size, 4, None, 0, pics, st) == E_ARG
    # more slices than max_pictures: refused as a whole, nothing taken
    b2, r2 = _lay(pkg, [mm.cut_runs(_fragments_of(a[:2])) for a in aus])
    with pytest.raises(pkg.FerHipError, match="code -1"):
        _mp4_call(pkg, dec, b2, r2, None)
    # fragments in device memory are not taken yet: refused as unsupported, nothing taken
    E_UNSUP = -4
    assert lib.ferhip_decs_decode_mp4(dec.h, 16, 1, rows.ctypes.data, rows.size, 4, None, 0, pics, st) == E_UNSUP
    _, pics, st = _mp4_call(pkg, dec, base, rows, None)
    assert (pics, st) == ([1] * n_s, [0] * n_s)
    ini = mm.init_segment(b"\x67\x42\x00\x1e\xab", b"\x68\xce\x38\x80", 64, 48, 90000)
    assert pkg.mp4_find_avcc(ini) == mm.find_avcc(ini) and pkg.mp4_find_avcc(ini[:-60]) is None and pkg.mp4_find_avcc(b"") is None
    _, pics, st = dec.decode_mp4(b"", np.zeros(0, pkg.MP4_RUN))
    assert (pics, st) == ([0] * n_s, [0] * n_s)
    dec.close()


@pytest.mark.parametrize("ps", (1, 0))
def test_loopback_through_fetch(pkg, ps):
    """an encoder's segments as ferhip_mp4_fetch brings them to the host are decoded from there.  Without parameter sets in
    the samples the decoder gets them from the initialisation segment."""
    feeds = _frames()
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    K = 3
    dst = pkg.DeviceBuffer(S * STRIDE)
    dec = pkg.LiveDecoder(S, W, H, K)
    if not ps:
        for s in range(S):
            ini = g.mp4_init(s, 90000)
            off, n = pkg.mp4_find_avcc(ini)
            assert dec.set_config(s, ini[off: off + n]) == 0
    hdr = pkg.mp4_hdr(S, decode_time=0, sequence=1, duration=3000)
    for seg in range(2):
        g.mp4_open(hdr, K, dst.ptr, STRIDE, ps)
        recon = []
        for t in range(3 * seg, 3 * seg + 3):
            g.encode_live([feeds[s][t] for s in range(S)], [KINDS[t]] * S)
            g.mp4_append()
            recon.append(g.get_recon())
        rc, buf, idx = g.mp4_fetch_raw(S * STRIDE)
        assert rc == 0 and [int(n) for n in idx["nsamples"]] == [3] * S + [3 * S] and int(idx[S]["fault"]) == 0
        rows = np.array([(int(idx["offset"][s]), int(idx["bytes"][s]), s) for s in range(S)], pkg.MP4_RUN)
        got, pics, st = dec.decode_mp4(buf, rows)
        assert pics == [3] * S and st == [0] * S, f"segment {seg}"
        for k in range(3):
            assert np.array_equal(got[k], recon[k]), f"segment {seg}, picture {k}"
        hdr["decode_time"] += 9000
        hdr["sequence"] += 1
    dec.close()
    g.close()
