"""Long runs on the GPU, bit for bit against the oracle (inputs and their reasons: tests/long_run.py, pinned on the host by
test_long_run_host.py): the encoder across the frame_num / pic_order_cnt_lsb wrap and through runs of IDR pictures, the
decoders across the seam between two parse windows.  The pictures are tiny; the cost is launches.  The lengths cannot
shrink: 513 pictures make the wrap, 257 the seam of a full window."""
import ctypes as C

import numpy as np
import pytest

import long_run as lr

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = lr.IDR, lr.SLICE, lr.NONE
FILL = 0xA5


# ---- C1: the P run through the C loop


def test_p_run_across_the_frame_num_wrap(pkg, fo):
    r = lr.P_RUN
    frames, ora = lr.p_run_frames(), lr.p_run_oracle()
    g = pkg.FerHip(r["W"], r["H"], 2, qp=r["qp"], window=r["window"], maxdiff=r["maxdiff"], intra_every=r["intra_every"])
    streams, rec = g.encode_streams(frames, want_recon=True)
    assert g.status() == [0, 0]
    stats = g.stats()
    g.close()
    for s, (stream, orec, ostats) in enumerate(ora):
        if streams[s] != stream:
            mine, theirs = lr.split_annexb(streams[s]), lr.split_annexb(stream)
            bad = next((k for k, (a, b) in enumerate(zip(mine, theirs)) if a != b), min(len(mine), len(theirs)))
            pytest.fail(f"stream {s}: NAL unit {bad} (picture {bad - 2}) differs from the oracle's, {len(mine)} against {len(theirs)} units")
        same = (rec[:, s] == orec).all(axis=1)
        assert same.all(), f"stream {s}: reconstruction of picture {int(np.nonzero(~same)[0][0])}"
        assert list(stats[s]) == ostats, f"stream {s}: stats"


# ---- C2: three schedules picture by picture


def test_schedules_picture_by_picture(pkg, fo):
    S = 3
    g = pkg.FerHip(lr.SCHED_W, lr.SCHED_H, S, qp=lr.SCHED_QP, window=lr.SCHED_WINDOW, maxdiff=3, intra_every=100000)
    feeds = [lr.schedule_feed(s) for s in range(S)]
    ora = [lr.schedule_oracle(s) for s in range(S)]
    pos = [0] * S
    for n, row in enumerate(lr.SCHEDULE):
        pics = [None if row[s] == NONE else feeds[s][pos[s]] for s in range(S)]
        rbsp, nt = g.encode_live(pics, list(row))
        rec = g.get_recon()
        assert list(nt) == list(row), f"call {n}: NAL types"
        for s in range(S):
            if row[s] == NONE:
                assert rbsp[s] == b"", f"call {n} stream {s}: an absent picture has no RBSP"
                if pos[s]:
                    assert np.array_equal(rec[s], ora[s]["pictures"][pos[s] - 1][2]), f"call {n} stream {s}: an absent picture moved the reconstruction"
                continue
            ot, orb, orec = ora[s]["pictures"][pos[s]]
            assert ot == row[s]
            if rbsp[s] != orb:
                hdr = lr.parse_header(rbsp[s], row[s]), lr.parse_header(orb, row[s])
                pytest.fail(f"call {n} stream {s} (its picture {pos[s]}): RBSP differs; header fields {hdr[0]} against the oracle's {hdr[1]}, "
                            f"{len(rbsp[s])} against {len(orb)} bytes")
            assert np.array_equal(rec[s], orec), f"call {n} stream {s} (its picture {pos[s]}): reconstruction"
            pos[s] += 1
    assert g.status() == [0] * S
    stats = g.stats()
    g.close()
    for s in range(S):
        assert pos[s] == len(ora[s]["pictures"])
        assert list(stats[s]) == ora[s]["stats"], f"stream {s}: stats"


# ---- C3: batch decode across windows


def _decode_streams_into(pkg, streams, max_pictures, fsz):
    """ferhip_decode_streams into a buffer filled with 0xA5 (ferhip.decode_streams allocates its own) -> (out, pictures)"""
    lib = pkg.load_library()
    S = len(streams)
    out = np.full((max_pictures, S, fsz), FILL, np.uint8)
    arr = (C.c_char_p * S)(*streams)
    lens = (C.c_size_t * S)(*[len(s) for s in streams])
    pics = (C.c_int * S)()
    W, H = C.c_int(), C.c_int()
    rc = lib.ferhip_decode_streams(arr, lens, S, out.ctypes.data, max_pictures, pics, C.byref(W), C.byref(H))
    assert rc == 0, f"ferhip_decode_streams: {rc}"
    return out, list(pics), W.value, H.value


def _check_batch(out, pictures, want, what):
    """want[s]: the oracle's pictures of stream s, [T_s][fsz]; every slot behind a stream's end still holds the fill"""
    assert pictures == [len(w) for w in want], what
    for s, w in enumerate(want):
        same = (out[:len(w), s] == w).all(axis=1)
        assert same.all(), f"{what} stream {s}: picture {int(np.nonzero(~same)[0][0])} of {len(w)} differs from the oracle's"
        assert (out[len(w):, s] == FILL).all(), f"{what} stream {s}: a slot behind its last picture was written"


def test_batch_decode_across_windows(pkg, fo):
    r = lr.P_RUN
    (a, arec, _), (b, brec, _) = lr.p_run_oracle()
    fsz = r["W"] * r["H"] * 3 // 2
    streams = [a, lr.cut_pictures(b, 300), lr.cut_pictures(b, 10)]
    assert b.startswith(streams[1]) and streams[1].startswith(streams[2])
    # the oracle decoder gives the oracle encoder's reconstruction (test_long_run_host.py): that is the expected picture
    out, pictures, W, H = _decode_streams_into(pkg, streams, 530, fsz)
    assert (W, H) == (r["W"], r["H"])
    _check_batch(out, pictures, [arec, brec[:300], brec[:10]], "max_pictures 530")
    out, pictures, _, _ = _decode_streams_into(pkg, streams, 300, fsz)
    _check_batch(out, pictures, [arec[:300], brec[:300], brec[:10]], "max_pictures 300")


# ---- C4: synthesized batches


def _synth_batch(keys):
    return [lr.synth_stream(*k)[0] for k in keys], [lr.synth_oracle(*k)[0] for k in keys]


@pytest.mark.parametrize("family", sorted(lr.FAMILIES))
def test_synth_batch_of_seven_offsets(pkg, fo, family):
    """seven streams whose cycles stand at the seven phases: whichever picture a window ends at, every hand-over is there"""
    streams, want = _synth_batch(lr.SYNTH_BATCHES[family])
    out, pictures, W, H = _decode_streams_into(pkg, streams, lr.SYNTH_T, lr.SYNTH_W * lr.SYNTH_H * 3 // 2)
    assert (W, H) == (lr.SYNTH_W, lr.SYNTH_H)
    _check_batch(out, pictures, want, family)


@pytest.mark.parametrize("family", sorted(lr.FAMILIES))
def test_synth_long_stream(pkg, fo, family):
    """600 pictures of one stream: more than two full windows"""
    streams, want = _synth_batch([lr.SYNTH_LONG[family]])
    out, pictures, _, _ = _decode_streams_into(pkg, streams, lr.SYNTH_T_LONG, lr.SYNTH_W * lr.SYNTH_H * 3 // 2)
    _check_batch(out, pictures, want, family)


def test_synth_long_stream_nal_by_nal(pkg, fo):
    """the streaming decoder has no window: the same 600 pictures, one NAL unit per call"""
    key = lr.SYNTH_LONG["held"]
    stream, want = lr.synth_stream(*key)[0], lr.synth_oracle(*key)[0]
    d = pkg.Decoder()
    k = 0
    for nal in pkg.split_nals(stream):
        t, idc, rbsp = pkg.unescape_nal(nal)
        pic = d.nal(t, idc, rbsp)
        if pic is not None:
            assert np.array_equal(pic, want[k]), f"picture {k}"
            k += 1
    d.close()
    assert k == key[2]


@pytest.mark.parametrize("where", ["host", "device"])
def test_live_decoder_two_windows_in_one_call(pkg, fo, where):
    """one ferhip_decs_decode call that carries all 300 pictures of seven streams: the window loop runs inside the call, and
    the result is the batch decoder's"""
    streams, want = _synth_batch(lr.SYNTH_BATCHES["held"])
    T, S, fsz = lr.SYNTH_T, lr.PERIOD, lr.SYNTH_W * lr.SYNTH_H * 3 // 2
    batch, bp, _, _ = _decode_streams_into(pkg, streams, T, fsz)
    d = pkg.LiveDecoder(S, lr.SYNTH_W, lr.SYNTH_H, max_pictures=T)
    if where == "host":
        out, pictures, status = d.decode(streams, out=np.full((T, S, fsz), FILL, np.uint8))
    else:
        buf = pkg.DeviceBuffer(T * S * fsz)
        buf.upload(np.full(T * S * fsz, FILL, np.uint8))
        _, pictures, status = d.decode(streams, out=buf)
        out = buf.download().reshape(T, S, fsz)
        buf.free()
    d.close()
    assert status == [0] * S and pictures == bp == [T] * S
    _check_batch(out, pictures, want, f"live, {where} output")
    assert np.array_equal(out, batch)
