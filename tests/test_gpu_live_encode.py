"""The live encoder (FERHIP_NAL_NONE, ferhip_set_frames_live / ferhip_upload_frames_live, ferhip_reset_stream): the streams of
a context need not tick together.  A stream's output must be a function of the pictures it was given alone, so every
stream is compared NAL by NAL, and its reconstruction picture by picture, with Oracle.encode_stream of exactly the frames
it got -- whatever calls it sat out and whatever the other streams did."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
from quality_model import plane_sse, ssim_windows

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
IDR, SLICE, NONE = 5, 1, -1
E_ARG = -1
NOISE = 0xA5

# calls x streams, 1 = the stream has a picture in that call.  With intra_every 4 and AUTO types (smooth content, so the
# SAD test never asks for an IDR) the picture types are:
#   call      0 1 2 3 4 5 6 7 8 9
#   stream 0  I P P P I P . P P I      present except in the call nobody takes part in
#   stream 1  . I P P . P . I P P      absent on the first call: its first picture is its IDR
#   stream 2  . . . I P P . P I P      absent on the first three calls
#   stream 3  I P . P . . . P I P      absent for 1 call and for 3 calls in a row between P pictures
#   stream 4  I P . . P P . I P P      absent for 2 calls between P pictures, and on call 6 where its IDR would have fallen
# call 0 has only I and absent streams, call 5 only P and absent streams, call 6 only absent streams.
TABLE = np.array([[1, 0, 0, 1, 1],
                  [1, 1, 0, 1, 1],
                  [1, 1, 0, 0, 0],
                  [1, 1, 1, 1, 0],
                  [1, 0, 1, 0, 1],
                  [1, 1, 1, 0, 1],
                  [0, 0, 0, 0, 0],
                  [1, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1]], np.uint8)
TYPES = ["IPPPIP.PPI", ".IPP.P.IPP", "...IPP.PIP", "IP.P...PIP", "IP..PP.IPP"]

_content_cache = {}
_oracle_cache = {}


def _content(pkg, W, H, T, seed, noise=2, static=False):
    """[T][fsz], computed once per module and never modified"""
    k = (W, H, T, seed, noise, static)
    if k not in _content_cache:
        a = np.stack([pkg.gen_frame(W, H, 0 if static else t, seed, noise) for t in range(T)])
        a.setflags(write=False)
        _content_cache[k] = a
    return _content_cache[k]


def _oracle(fo, key, frames, W, H, qp, intra_every, window=16):
    """(Annex-B stream, recon [T][fsz], brojTipova) of Oracle.encode_stream(frames); cached under `key`"""
    k = (key, W, H, qp, intra_every, window, len(frames))
    if k not in _oracle_cache:
        o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=3, intra_every=intra_every)
        stream, rec = o.encode_stream(frames)
        stats = list(o.stats())
        o.close()
        _oracle_cache[k] = (stream, rec, stats)
    return _oracle_cache[k]


def _annexb(g, s, pics):
    sps, pps = g.sps_pps(s)
    return sps + pps + b"".join(g.write_nal(nt, rb) for nt, rb in pics)


class _Run:
    """Drives a context through a presence table.  feeds[s] = the pictures of stream s in order; a stream takes its next
    picture in every call it is present in.  Absent slots of the source carry 0xA5 noise.  After every call: absent
    streams return b"" / NAL_NONE and their get_recon is their previous reconstruction."""

    def __init__(self, pkg, g, feeds, ingest="host", rbsp="host"):
        self.pkg, self.g, self.feeds, self.ingest, self.rbsp = pkg, g, feeds, ingest, rbsp
        S = g.S
        self.pos = [0] * S
        self.pics = [[] for _ in range(S)]   # (nal type, rbsp) of every coded picture
        self.recs = [[] for _ in range(S)]   # its reconstruction
        self.last_rec = [None] * S
        self.bufs = []
        stride = g.nmb * 1024 + 4096
        if rbsp == "device":
            self.keep = pkg.DeviceBuffer(S * stride)
            self.lens = pkg.DeviceBuffer(S * 4)
            self.bufs += [self.keep, self.lens]
        if ingest in ("device", "device+4"):
            self.dev = pkg.DeviceBuffer(S * g.fsz + 16)
            self.bufs.append(self.dev)
        if ingest == "upload":
            self.pin = pkg.DeviceBuffer(S * g.fsz, pinned=True)
            self.bufs.append(self.pin)

    def call(self, present, nal_types=None):
        g, S = self.g, self.g.S
        src = np.full((S, g.fsz), NOISE, np.uint8)
        for s in range(S):
            if present[s]:
                src[s] = self.feeds[s][self.pos[s]]
        if self.ingest == "host":
            g.set_frames_live(src, present)
        elif self.ingest in ("device", "device+4"):
            off = 4 if self.ingest == "device+4" else 0
            self.dev.upload(src, offset=off)
            g.set_frames_live(self.dev.ptr + off, present)
        else:
            g.sync()  # the pinned buffer is reused: the previous upload has been consumed
            self.pin.upload(src)
            g.upload_frames_live(self.pin.ptr, present)
            g.set_frames_uploaded()
        req = [0 if present[s] else NONE for s in range(S)] if nal_types is None else nal_types
        if self.rbsp == "host":
            rb, nt = g.encode_picture(req)
        else:
            stride = g.nmb * 1024 + 4096
            _, st, _, nt = g.encode_picture_device(req)
            assert st == stride
            g.copy_rbsp_device(self.keep.ptr, self.lens.ptr)
            g.sync()
            ln = self.lens.download(dtype=np.uint32)
            kb = self.keep.download().reshape(S, stride)
            rb = [bytes(kb[s, :ln[s]]) for s in range(S)]
        rec = g.get_recon()
        for s in range(S):
            if present[s]:
                assert nt[s] in (IDR, SLICE) and len(rb[s]) > 0, f"stream {s}: present but nothing coded"
                self.pics[s].append((nt[s], rb[s]))
                self.recs[s].append(rec[s].copy())
                self.last_rec[s] = rec[s].copy()
                self.pos[s] += 1
            else:
                assert nt[s] == NONE, f"stream {s}: absent, nal type {nt[s]}"
                assert rb[s] == b"", f"stream {s}: absent, {len(rb[s])} RBSP bytes"
                if self.last_rec[s] is not None:
                    assert np.array_equal(rec[s], self.last_rec[s]), f"stream {s}: absent, its reconstruction moved"
        return nt

    def check(self, fo, keys, W, H, qp, intra_every, streams=None, base_of=None):
        g = self.g
        for s in (range(g.S) if streams is None else streams):
            n = self.pos[s]
            ref, ref_rec, _ = _oracle(fo, keys[s], self.feeds[s][:n], W, H, qp if base_of is None else base_of[s], intra_every)
            got = _annexb(g, s, self.pics[s])
            assert got == ref, f"stream {s}: bitstream differs from the oracle's encode of its own {n} pictures"
            for t in range(n):
                assert np.array_equal(self.recs[s][t], ref_rec[t]), f"stream {s} picture {t}: reconstruction"

    def free(self):
        for b in self.bufs:
            b.free()


def _type_string(run, table, s):
    it = iter(run.pics[s])
    return "".join({IDR: "I", SLICE: "P"}[next(it)[0]] if table[c][s] else "." for c in range(len(table)))


def _gaps_run(pkg, fo, S, rbsp, tune=()):
    W, H, T = 80, 48, 10
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=4)
    for k, v in tune:
        g.tune(k, v)
    feeds = [_content(pkg, W, H, T, 1234 + s) for s in range(S)]
    run = _Run(pkg, g, feeds, rbsp=rbsp)
    table = TABLE[:, np.arange(S) % 5]
    for c in range(len(table)):
        if c == 4:
            # ferhip_select_nal_type leaves the absent streams out and decides what the encode call then uses
            src = np.full((S, g.fsz), NOISE, np.uint8)
            for s in range(S):
                if table[c][s]:
                    src[s] = feeds[s][run.pos[s]]
            g.set_frames_live(src, table[c])
            sel = (C.c_int * S)(*[0 if table[c][s] else NONE for s in range(S)])
            assert g.lib.ferhip_select_nal_type(g.ctx, sel) == 0
            nt = run.call(table[c])
            assert list(sel) == nt
        else:
            nt = run.call(table[c])
        if c == 6:
            assert nt == [NONE] * S
    for s in range(S):
        assert _type_string(run, table, s) == TYPES[s % 5], f"stream {s}: the table no longer covers its cases"
    assert g.status() == [0] * S
    run.check(fo, [("gap", 1234 + s) for s in range(S)], W, H, 12, 4)
    run.free()
    g.close()


@pytest.mark.parametrize("rbsp", ["host", "device"])
def test_streams_with_gaps_match_the_oracle(pkg, fo, rbsp):
    _gaps_run(pkg, fo, 5, rbsp)


@pytest.mark.parametrize("speculate", [0, 1])
@pytest.mark.parametrize("wgs", [1, 3072])
def test_gaps_across_all_ticket_queues(pkg, fo, speculate, wgs):
    """17 streams: all eight ticket queues of k_me_resolve hold rows of present and of absent streams; status stays 0
    (no chain timeout, bit 5, no unresolved vectors, bit 6)"""
    _gaps_run(pkg, fo, 17, "host", tune=((pkg.TUNE_SPECULATE, speculate), (pkg.TUNE_RESOLVE_WGS, wgs)))


def test_stale_mb_type_is_the_streams_own_across_a_gap(pkg, fo):
    """Golden qcif_skip_5f_qp12 (static content, intra_every 3: I P P I P) in stream 0, which sits out two calls right before
    its second IDR; stream 1 codes moving content in those calls.  The Intra16x16 size estimate of that IDR reads the mb_type
    of the stream's own last picture (the reference's stale-mb_type quirk), so stream 0 must still give the golden bytes."""
    W, H = 176, 144
    golden = (GOLD / "qcif_skip_5f_qp12.264").read_bytes()
    f0 = _content(pkg, W, H, 5, 1234, noise=0, static=True)
    f1 = _content(pkg, W, H, 7, 4321)
    assert all((f0[0][:W * H].reshape(H // 16, 16, W // 16, 16) != f1[t][:W * H].reshape(H // 16, 16, W // 16, 16)).any(axis=(1, 3)).all()
               for t in range(7)), "stream 1's pictures differ from stream 0's in every macroblock"
    g = pkg.FerHip(W, H, 2, qp=12, window=16, maxdiff=3, intra_every=3)
    run = _Run(pkg, g, [f0, f1])
    for c, p0 in enumerate([1, 1, 1, 0, 0, 1, 1]):
        run.call([p0, 1])
        if c == 4:
            mbt = g.read("MBTYPE").reshape(2, -1)
            assert (mbt[0] != mbt[1]).any(), "the two streams hold different macroblock types before stream 0's IDR"
    assert _type_string(run, [[1, 1]] * 3 + [[0, 1]] * 2 + [[1, 1]] * 2, 0) == "IPP..IP"
    assert g.status() == [0, 0]
    assert _annexb(g, 0, run.pics[0]) == golden, "stream 0: not the golden stream"
    run.check(fo, [("skipq", 0), ("moveq", 0)], W, H, 12, 3)
    g.close()


@pytest.mark.parametrize("W,H,ingest", [(16, 16, "host"), (16, 16, "device"), (16, 16, "device+4"),
                                        (208, 112, "host"), (208, 112, "device"), (208, 112, "device+4"), (208, 112, "upload")])
def test_carry_and_masked_ingest_at_awkward_sizes(pkg, fo, W, H, ingest):
    """16x16: planes of 256 and 64 bytes, far less than one wavefront's 16-byte words; 208x112: 1456 words of luma, no
    multiple of 64.  Stream 1 is absent on every other call, so its reference is carried while the sets swap under it;
    the 0xA5 noise in its slot of the source must not reach any stream."""
    S, T = 3, 6
    g = pkg.FerHip(W, H, S, qp=20, window=16, maxdiff=3, intra_every=30)
    feeds = [_content(pkg, W, H, T, 77 + s) for s in range(S)]
    run = _Run(pkg, g, feeds, ingest=ingest)
    for c in range(T):
        run.call([1, c % 2 == 0, 1])
    assert run.pos == [6, 3, 6]
    assert g.status() == [0] * S
    run.check(fo, [("awk", 77 + s) for s in range(S)], W, H, 20, 30)
    run.free()
    g.close()


# ---- rate modes: the settings of test_gpu_rate_control.py (ABR_SET[0]) and test_gpu_quality.py (QSET[0])
def _rate_run(pkg, patterns, T, ncalls):
    """streams 0 (ABR) and 1 (QUALITY) follow patterns[s](call) until each has coded T pictures; streams 2 and 3 stay in
    CQP (26, the context's, and 20) and are present in every call"""
    W, H, S = 80, 48, 4
    g = pkg.FerHip(W, H, S, qp=26, window=16, maxdiff=3, intra_every=5)
    g.set_rate(0, pkg.RC_ABR, qp=26, qp_min=0, qp_max=51, max_step=2, ip_offset=3, window=0, target_bits=6000)
    g.set_rate(1, pkg.RC_QUALITY, qp=26, qp_min=0, qp_max=51, max_step=2, ip_offset=3, target_sse=60000)
    g.set_rate(3, pkg.RC_CQP, qp=20)
    feeds = [_content(pkg, W, H, ncalls, 900 + s) for s in range(S)]
    run = _Run(pkg, g, feeds)
    qps = [[] for _ in range(S)]
    for c in range(ncalls):
        present = [run.pos[s] < T and patterns[s](c) for s in (0, 1)] + [1, 1]
        before = g.last_qp()
        run.call(present)
        after = g.last_qp()
        for s in range(S):
            if present[s]:
                qps[s].append(after[s])
            else:
                assert after[s] == before[s], f"stream {s}: absent, ferhip_get_qp moved from {before[s]} to {after[s]}"
    assert run.pos[0] == T and run.pos[1] == T, "the patterns leave room for T pictures"
    assert g.status() == [0] * S
    return g, run, qps


def test_rate_modes_see_only_their_own_pictures(pkg, fo):
    T = 12
    gd, dense, qd = _rate_run(pkg, [lambda c: True, lambda c: True], T, T)
    gaps = [lambda c: c % 3 != 1 and c not in (5, 6), lambda c: c % 4 != 2 and c != 0]
    gg, gapped, qg = _rate_run(pkg, gaps, T, 22)
    for s, mode in ((0, "ABR"), (1, "QUALITY")):
        assert len(set(qd[s])) > 1, f"{mode}: the controller never moved"
        assert qg[s] == qd[s], f"{mode}: QPs with gaps {qg[s]} != dense {qd[s]}"
        assert gapped.pics[s] == dense.pics[s], f"{mode}: bytes differ between the gapped and the dense run"
        assert all(np.array_equal(a, b) for a, b in zip(gapped.recs[s], dense.recs[s]))
    for run in (dense, gapped):
        run.check(fo, [None, None, ("cqp", 902), ("cqp", 903)], 80, 48, 26, 5, streams=(2, 3), base_of={2: 26, 3: 20})
    gd.close()
    gg.close()


def _check_record(q, s, src, rec, W, H):
    want = plane_sse(src, rec, W, H)
    assert list(q.sse[0, s]) == list(want), f"stream {s}: sse {list(q.sse[0, s])} != numpy {list(want)}"
    v = ssim_windows(src, rec, W, H)
    assert q.ssim_windows[0, s] == (W // 4 - 1) * (H // 4 - 1) == v.size
    assert abs(q.ssim[0, s] - v.mean()) <= 1e-12, f"stream {s}: ssim {q.ssim[0, s]!r} != numpy {v.mean()!r}"


@pytest.mark.parametrize("gaps", [True, False])
def test_quality_ring_with_gaps(pkg, gaps):
    W, H, S = 80, 48, 3
    table = [[1, 0, 1], [1, 1, 1], [1, 1, 0], [1, 0, 0], [0, 0, 0], [1, 1, 1], [0, 1, 1]] if gaps else [[1, 1, 1]] * 5
    g = pkg.FerHip(W, H, S, qp=28, window=16, maxdiff=3, intra_every=30)
    g.set_quality(pkg.QM_SSE | pkg.QM_SSIM)
    feeds = [_content(pkg, W, H, len(table), 31 + s) for s in range(S)]
    run = _Run(pkg, g, feeds)
    rows = []
    for c, present in enumerate(table):
        coded = list(run.pos)
        nt = run.call(present)
        if not any(present):
            continue  # a call nobody takes part in changes nothing: no row
        q = g.quality(1)
        rows.append(q)
        qp = g.last_qp()
        for s in range(S):
            assert q.picture[0, s] == coded[s], f"call {c} stream {s}: picture {q.picture[0, s]}, the stream has coded {coded[s]}"
            assert q.qp[0, s] == qp[s]
            if present[s]:
                assert q.nal_type[0, s] == nt[s] and q.rbsp_bytes[0, s] == len(run.pics[s][-1][1])
                _check_record(q, s, feeds[s][coded[s]], run.recs[s][-1], W, H)
            else:
                assert q.nal_type[0, s] == 0 and q.rbsp_bytes[0, s] == 0
                assert list(q.sse[0, s]) == [0, 0, 0] and q.ssim_sum[0, s] == 0.0 and q.ssim_windows[0, s] == 0
    ring = g.quality(len(table))
    assert ring.sse.shape[0] == len(rows)
    for k, q in enumerate(rows):
        for f in ("sse", "ssim_sum", "ssim_windows", "qp", "nal_type", "rbsp_bytes", "picture"):
            assert np.array_equal(getattr(ring, f)[k], getattr(q, f)[0]), (k, f)
    if not gaps:
        assert [list(ring.picture[k]) for k in range(len(rows))] == [[k] * S for k in range(len(rows))]
    assert g.status() == [0] * S
    g.close()


def test_reset_stream(pkg, fo):
    W, H, S = 80, 48, 3
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=4)
    for bad in (-1, S):
        with pytest.raises(pkg.FerHipError, match=f"code {E_ARG}$"):
            g.reset_stream(bad)
    old = _content(pkg, W, H, 6, 1234, noise=0, static=True)   # skip-heavy: slot 1 ends with P_Skip macroblock types
    new = _content(pkg, W, H, 4, 5150)
    feeds = [_content(pkg, W, H, 10, 60), np.concatenate([old, new]), _content(pkg, W, H, 10, 62)]
    run = _Run(pkg, g, feeds)
    for c in range(6):
        run.call([1, 1, 1])
    assert (g.read("MBTYPE").reshape(S, -1)[1] != 0).any(), "slot 1 leaves macroblock types behind"
    assert g.stats()[1].sum() > 0
    first = _annexb(g, 1, run.pics[1])
    ref, _, _ = _oracle(fo, ("reset-old", 0), old, W, H, 12, 4)
    assert first == ref
    g.reset_stream(1)
    assert list(g.stats()[1]) == [0] * 5 and g.status() == [0] * S and g.last_qp()[1] == 12
    assert (g.read("MBTYPE").reshape(S, -1)[1] == 0).all()
    with pytest.raises(pkg.FerHipError):
        g.set_rate(1, pkg.RC_CQP, qp=40)  # a base above 37 is refused before a stream's first picture: the slot is there again
    g.set_rate(1, pkg.RC_CQP, qp=30)      # accepted, and sets the base: the PPS of the new feed says 30
    run.pics[1], run.recs[1], run.last_rec[1] = [], [], None
    feeds[1] = new
    run.pos[1] = 0
    for c in range(4):
        run.call([1, 1, 1])
    assert g.status() == [0] * S
    ref, ref_rec, ref_stats = _oracle(fo, ("reset-new", 0), new, W, H, 30, 4)
    assert _annexb(g, 1, run.pics[1]) == ref, "slot 1 after the reset: not a fresh stream at qp 30"
    assert all(np.array_equal(run.recs[1][t], ref_rec[t]) for t in range(4))
    assert list(g.stats()[1]) == ref_stats, "brojTipova of slot 1 restarted from zero"
    assert g.last_qp()[1] == 30
    run.check(fo, [("reset", 60), None, ("reset", 62)], W, H, 12, 4, streams=(0, 2))
    g.close()
