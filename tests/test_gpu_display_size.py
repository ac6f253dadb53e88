"""Pictures of any even size: padded ingest (ferhip_set_frames_display, ferhip_upload_frames_display), the cropping SPS,
cropped reconstruction read-back, and the live decoder's crop report and windowed output.  The yardsticks are the numpy
padding model (tests/pad_model.py, pinned in tests/test_pad_model_host.py) and the oracle: a display-size encode must be,
slice for slice, the oracle's encode of the numpy-padded pictures, and the oracle decoder ignores cropping, so windowed
output is the oracle's pictures windowed by numpy."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import pad_model as pm

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
E_ARG, E_STATE = -1, -3
POISON = 0xEE  # fills source slots that must not be read and output slots that must not be written; sources stay below it
S = 3


def _rand_pics(rng, n, dw, dh):
    return rng.integers(0, 200, (n, dw * dh * 3 // 2), dtype=np.uint8)


def _model(pics, dw, dh, W, H):
    return np.stack([pm.pad_picture(p, dw, dh, W, H) for p in pics])


# ---------------------------------------------------------------- 1. ingest known-answer test
INGEST = [(16, 16, 2, 2), (16, 16, 16, 2), (32, 32, 18, 30), (64, 48, 50, 38), (80, 48, 66, 48), (80, 48, 80, 34), (48, 32, 48, 32)]


@pytest.fixture(scope="module", params=INGEST, ids=lambda p: "%dx%d<-%dx%d" % p)
def ingest(pkg, request):
    W, H, dw, dh = request.param
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    yield enc, W, H, dw, dh
    enc.close()


def _cur(enc):
    return enc.read("CUR").reshape(enc.S, enc.fsz)


def test_ingest_host_source(ingest):
    enc, W, H, dw, dh = ingest
    pics = _rand_pics(np.random.default_rng(1), S, dw, dh)
    enc.set_frames_display(pics)
    assert np.array_equal(_cur(enc), _model(pics, dw, dh, W, H))


@pytest.mark.parametrize("mis,mask", [pytest.param(0, None, id="0"), pytest.param(1, None, id="1"), pytest.param(2, None, id="2"),
                                      pytest.param(7, None, id="7"), pytest.param(3, [1, 0, 1], id="3-present101")])
def test_ingest_device_source_at_any_alignment(pkg, ingest, mis, mask):
    enc, W, H, dw, dh = ingest
    rng = np.random.default_rng(2 + mis)
    want = pics = _rand_pics(rng, S, dw, dh)
    if mask:  # an absent stream keeps its picture, and its slot is never read
        before = _rand_pics(rng, S, dw, dh)
        enc.set_frames_display(before)
        want = np.stack([pics[s] if mask[s] else before[s] for s in range(S)])
        pics = np.stack([pics[s] if mask[s] else np.full_like(pics[s], POISON) for s in range(S)])
    buf = pkg.DeviceBuffer(pics.nbytes + 32)
    buf.upload(np.full(pics.nbytes + 32, POISON, np.uint8))
    buf.upload(pics, offset=mis)
    assert buf.ptr % 16 == 0
    enc.set_frames_display(buf.ptr + mis, present=mask)
    got = _cur(enc)
    buf.free()
    assert np.array_equal(got, _model(want, dw, dh, W, H))


def test_ingest_upload_path(pkg, ingest):
    enc, W, H, dw, dh = ingest
    pics = _rand_pics(np.random.default_rng(3), S, dw, dh)
    pin = pkg.DeviceBuffer(pics.nbytes, pinned=True)
    pin.upload(pics)
    enc.upload_frames_display(pin.ptr)
    enc.set_frames_uploaded()
    got = _cur(enc)
    pin.free()
    assert np.array_equal(got, _model(pics, dw, dh, W, H))


@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 0, 1]])
@pytest.mark.parametrize("path", ["host", "device", "upload"])
def test_ingest_masked(pkg, ingest, mask, path):
    enc, W, H, dw, dh = ingest
    rng = np.random.default_rng(4 + sum(mask))
    before = _rand_pics(rng, S, dw, dh)
    enc.set_frames_display(before)
    pics = _rand_pics(rng, S, dw, dh)
    for s in range(S):
        if not mask[s]:
            pics[s] = POISON  # an absent stream's slot must never be read
    if path == "host":
        enc.set_frames_display(pics, present=mask)
    elif path == "device":
        buf = pkg.DeviceBuffer(pics.nbytes + 16)
        buf.upload(pics, offset=1)
        enc.set_frames_display(buf.ptr + 1, present=mask)
        enc.sync()
        buf.free()
    else:
        pin = pkg.DeviceBuffer(pics.nbytes, pinned=True)
        pin.upload(pics)
        enc.upload_frames_display(pin.ptr, present=mask)
        enc.set_frames_uploaded()
        enc.sync()
        pin.free()
    got = _cur(enc)
    want = _model([pics[s] if mask[s] else before[s] for s in range(S)], dw, dh, W, H)
    assert np.array_equal(got, want)  # absent streams keep their previous pictures
    assert not (got == POISON).any()


def test_ingest_display_and_coded_uploads_alternate_in_flight(pkg, ingest):
    enc, W, H, dw, dh = ingest
    rng = np.random.default_rng(5)
    coded = rng.integers(0, 200, (S, enc.fsz), dtype=np.uint8)
    disp = _rand_pics(rng, S, dw, dh)
    pc, pd = pkg.DeviceBuffer(coded.nbytes, pinned=True), pkg.DeviceBuffer(disp.nbytes, pinned=True)
    pc.upload(coded)
    pd.upload(disp)
    for order in ("cd", "dc", "dd"):
        for k in order:  # both uploads in flight before either is made current
            if k == "c":
                enc.upload_frames(pc.ptr)
            else:
                enc.upload_frames_display(pd.ptr)
        for k in order:
            enc.set_frames_uploaded()
            want = coded if k == "c" else _model(disp, dw, dh, W, H)
            assert np.array_equal(_cur(enc), want), (order, k)
    pc.free()
    pd.free()


# ---------------------------------------------------------------- 2. encode parity with the oracle on numpy-padded pictures
def _encode_display(pkg, fo, W, H, dw, dh, qp, frames, window=16):
    """frames [T][S][dw*dh*3/2] through a display-size context, picture by picture, AUTO types.
    -> dict(streams = Annex-B per stream, every check of section 2 asserted on the way, oracle pictures per stream)"""
    T = frames.shape[0]
    enc = pkg.FerHip(W, H, S, qp=qp, window=window, maxdiff=3, intra_every=30)
    enc.set_display_size(dw, dh)
    sps_model = pm.sps_nal(W, H, dw, dh)
    assert enc.sps_pps()[0] == sps_model, "ferhip_write_sps differs from the SPS model"
    padded = np.stack([_model(frames[t], dw, dh, W, H) for t in range(T)])
    ref, ref_nals, ref_rec = [], [], []
    for s in range(S):
        o = fo.Oracle(W, H, qp=qp, window=window, maxdiff=3, intra_every=30)
        st, rec = o.encode_stream(padded[:, s])
        o.close()
        ref.append(st)
        ref_nals.append(pm.split_nals(st))
        ref_rec.append(rec)
    streams = [sps_model + enc.sps_pps(s)[1] for s in range(S)]
    types = []
    for t in range(T):
        enc.set_frames_display(frames[t])
        rbsp, nt = enc.encode_picture()
        types.append(nt)
        framed, ftypes = enc.fetch_nal(pkg.AU_PARAM_SETS)
        rd, rf = enc.get_recon_display(), enc.get_recon()
        for s in range(S):
            want = ref_nals[s][2 + t]
            wt, _, wrbsp = pkg.unescape_nal(want)
            assert nt[s] == wt, f"picture {t} stream {s}: NAL type {nt[s]}, oracle {wt}"
            assert rbsp[s] == wrbsp, f"picture {t} stream {s}: slice RBSP differs from the oracle's"
            slice_nal = enc.write_nal(nt[s], rbsp[s])
            assert slice_nal == want
            assert ftypes[s] == nt[s]
            assert framed[s] == (sps_model + enc.sps_pps(s)[1] + slice_nal if nt[s] == pkg.NAL_IDR else slice_nal)
            assert np.array_equal(rf[s], ref_rec[s][t]), f"picture {t} stream {s}: reconstruction"
            assert np.array_equal(rd[s], pm.window(ref_rec[s][t], W, H, 0, 0, dw, dh)), f"picture {t} stream {s}: cropped reconstruction"
            streams[s] += slice_nal
    assert enc.status() == [0] * S
    enc.close()
    for s in range(S):
        # the whole stream, cropping SPS included, under the oracle decoder: the oracle's own pictures
        n, pics, st = fo.decode_stream_md5(streams[s])
        assert n == T and (st["W"], st["H"]) == (W, H)
        assert np.array_equal(np.stack(pics), ref_rec[s])
        assert streams[s] == pm.swap_sps(ref[s], sps_model)
    return dict(streams=streams, pictures=ref_rec, types=types)


def _gen(fo, dw, dh, T, seed0=500):
    return np.stack([np.stack([fo.gen_frame(dw, dh, t, seed0 + s, 2) for s in range(S)]) for t in range(T)])


@pytest.fixture(scope="module")
def coded(pkg, fo):
    """the 64x48 <- 50x38 IPPP run at qp 12: sections 3 and 4 decode its streams"""
    return _encode_display(pkg, fo, 64, 48, 50, 38, 12, _gen(fo, 50, 38, 5))


def test_encode_parity_qp12(coded):
    assert [t[0] for t in coded["types"]] == [5, 1, 1, 1, 1]


def test_encode_parity_qp28(pkg, fo):
    r = _encode_display(pkg, fo, 64, 48, 50, 38, 28, _gen(fo, 50, 38, 5))
    assert [t[0] for t in r["types"]] == [5, 1, 1, 1, 1]


def test_encode_parity_auto_types_with_a_scene_cut(pkg, fo):
    dw, dh = 162, 130
    frames = _gen(fo, dw, dh, 4)
    frames[2:, 1] = 255 - frames[2:, 1]  # stream 1 cuts at picture 2: its luma SAD against the reference picture exceeds 16 per sample
    r = _encode_display(pkg, fo, 176, 144, dw, dh, 28, frames)
    assert [t[1] for t in r["types"]] == [5, 1, 5, 1] and [t[0] for t in r["types"]] == [5, 1, 1, 1]


# ---------------------------------------------------------------- 3. decode: crop report and windowed output
W3, H3 = 64, 48
CROP_B = (4, 10, 2, 8)  # left, right, top, bottom of the stream whose SPS is swapped for a model SPS


@pytest.fixture(scope="module")
def dec_streams(coded):
    """three 64x48 streams and the oracle's pictures of each: 0 as the encoder wrote it (cropped to 50x38), 1 with left / top
    offsets swapped in, 2 as stream 0 of the encoder again"""
    st = [coded["streams"][0], pm.swap_sps(coded["streams"][1], pm.sps_nal(W3, H3, crop=CROP_B)), coded["streams"][2]]
    return st, [coded["pictures"][k] for k in range(3)], [(0, 14, 0, 10), CROP_B, (0, 14, 0, 10)]


def _live(pkg, streams, P, win=None, out="host", dev_chunks=False, out_mis=0, late=()):
    """Feed every stream P access units per call (streams in `late` sit out the first call) -> pictures per stream, and the
    crops read after the first call.  Every slot that must stay unwritten is checked for the poison fill."""
    n = len(streams)
    dec = pkg.LiveDecoder(n, W3, H3, P)
    if win:
        dec.set_display(*win)
    osz = dec.fsz
    aus = [pkg.access_units(s) for s in streams]
    pos, got, crops, call = [0] * n, [[] for _ in range(n)], None, 0
    dbuf = pkg.DeviceBuffer(P * n * osz + 32) if out != "host" else None
    while any(pos[s] < len(aus[s]) for s in range(n)):
        take = [0 if (call == 0 and s in late) else min(P, len(aus[s]) - pos[s]) for s in range(n)]
        chunks = [b"".join(aus[s][pos[s]:pos[s] + take[s]]) or None for s in range(n)]
        for s in range(n):
            pos[s] += take[s]
        if dev_chunks:
            cb = pkg.DeviceBuffer(sum(len(c) + 16 for c in chunks if c) + 16)
            ptrs, lens, o = [], [], 3  # chunks at odd addresses
            for c in chunks:
                if c:
                    cb.upload(np.frombuffer(c, np.uint8), offset=o)
                ptrs.append(cb.ptr + o if c else None)
                lens.append(len(c) if c else 0)
                o += (len(c) if c else 0) + 5
        if dbuf:
            dbuf.upload(np.full(P * n * osz + 32, POISON, np.uint8))
            target = dbuf if out_mis == 0 else dbuf.ptr + out_mis
        else:
            target = np.full((P, n, osz), POISON, np.uint8)
        if dev_chunks:
            _, pics, status = dec.decode_dev(ptrs, lens, target)
            cb.free()
        else:
            _, pics, status = dec.decode(chunks, target)
        assert status == [0] * n
        assert pics == take
        if dbuf:
            raw = dbuf.download()
            assert (raw[:out_mis] == POISON).all() and (raw[out_mis + P * n * osz:] == POISON).all()
            o = raw[out_mis:out_mis + P * n * osz].reshape(P, n, osz)
        else:
            o = target
        for s in range(n):
            got[s] += [o[k, s].copy() for k in range(pics[s])]
            assert (o[pics[s]:, s] == POISON).all(), f"stream {s}: a slot past its pictures was written"
        if call == 0:
            crops = [dec.get_crop(s) if s not in late else None for s in range(n)]
        call += 1
    dec.close()
    if dbuf:
        dbuf.free()
    return [np.stack(g) for g in got], crops


def test_decode_reports_crop_and_full_output_is_unchanged(pkg, dec_streams):
    streams, ref, crops = dec_streams
    got, c = _live(pkg, streams, 1)
    assert c == crops
    for s in range(3):
        assert np.array_equal(got[s], ref[s]), f"stream {s}"


WINDOWS = [(0, 0, 50, 38), (4, 2, 50, 38), (14, 10, 2, 2), (0, 0, 64, 48)]


def _windowed(ref, win):
    return np.stack([pm.window(p, W3, H3, *win) for p in ref])


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("mode", ["host", "device", "device+4", "dev_chunks_host", "dev_chunks_device+4", "device+1", "device+3"])
def test_decode_windowed_output(pkg, dec_streams, win, mode):
    streams, ref, _ = dec_streams
    got, _ = _live(pkg, streams, 1, win, out="host" if mode.endswith("host") else "device", dev_chunks=mode.startswith("dev_chunks"),
                   out_mis=int(mode.partition("+")[2] or 0))
    for s in range(3):
        assert np.array_equal(got[s], _windowed(ref[s], win)), f"stream {s}"


@pytest.mark.parametrize("out", ["host", "device"])
def test_decode_windowed_two_pictures_per_call_one_stream_absent(pkg, dec_streams, out):
    streams, ref, crops = dec_streams
    win = (4, 2, 50, 38)
    got, c = _live(pkg, streams, 2, win, out=out, late=(1,))
    assert c == [crops[0], None, crops[2]]
    for s in range(3):
        assert np.array_equal(got[s], _windowed(ref[s], win)), f"stream {s}"


def test_decode_set_display_back_to_the_default(pkg, dec_streams):
    streams, ref, _ = dec_streams
    dec = pkg.LiveDecoder(1, W3, H3, 1)
    aus = pkg.access_units(streams[0])
    dec.set_display(0, 0, 50, 38)
    o, pics, st = dec.decode([aus[0]])
    assert pics == [1] and np.array_equal(o[0, 0], pm.window(ref[0][0], W3, H3, 0, 0, 50, 38))
    dec.set_display(0, 0, W3, H3)
    o, pics, st = dec.decode([aus[1]])
    assert pics == [1] and o.shape[2] == W3 * H3 * 3 // 2 and np.array_equal(o[0, 0], ref[0][1])
    dec.close()


def test_decode_cut_cropless_and_nonsense_sps_report_zeros(pkg, fo, coded):
    base, ref = coded["streams"][0], coded["pictures"][0]
    full = pm.sps_rbsp(W3, H3, 50, 38)
    import pslice_synth as ps
    cut = ps.nal_unit(7, 1, full[:7])  # ends inside the offsets
    assert cut[-1] != 0
    cases = [cut, pm.sps_nal(W3, H3), pm.sps_nal(W3, H3, crop=(32, 32, 0, 0)), pm.sps_nal(W3, H3, crop=(0, 0, 40, 8))]
    streams = [pm.swap_sps(base, sps) for sps in cases]
    dec = pkg.LiveDecoder(len(streams), W3, H3, 8)
    o, pics, st = dec.decode(streams)
    assert st == [0] * len(streams) and pics == [5] * len(streams)
    for s in range(len(streams)):
        assert dec.get_crop(s) == (0, 0, 0, 0)
        assert np.array_equal(o[:5, s], ref), f"case {s}"
    dec.close()


# ---------------------------------------------------------------- 4. loopback without the bus
def test_loopback_device_to_device(pkg, fo):
    W, H, dw, dh = 64, 48, 50, 38
    frames = _gen(fo, dw, dh, 1, seed0=900)
    a = pkg.FerHip(W, H, S, qp=20, window=16)
    a.set_display_size(dw, dh)
    a.set_frames_display(frames[0])
    a.encode_picture_device()
    cap = S * (a.nmb * 1024 + 4096 + 128)
    nal, idx = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (S + 1))
    a.pack_nal_device(nal.ptr, idx.ptr, cap, pkg.AU_PARAM_SETS)
    a.sync()
    index = idx.download(dtype=np.uint8).view(pkg.AU)
    dec = pkg.LiveDecoder(S, W, H, 1)
    dec.set_display(0, 0, dw, dh)
    out = pkg.DeviceBuffer(S * dec.fsz)
    _, pics, st = dec.decode_dev([nal.ptr + int(index["offset"][s]) for s in range(S)], [int(index["bytes"][s]) for s in range(S)], out)
    assert pics == [1] * S and st == [0] * S
    assert [dec.get_crop(s) for s in range(S)] == [(0, W - dw, 0, H - dh)] * S
    b = pkg.FerHip(W, H, S, qp=20, window=16)
    b.set_display_size(dw, dh)
    b.set_frames_display(out.ptr)  # dw*dh*3/2 = 2850 bytes per slot: streams 1 and 2 start misaligned
    got = _cur(b)
    rec = a.get_recon_display()
    assert np.array_equal(out.download().reshape(S, -1), rec)
    assert np.array_equal(got, _model(rec, dw, dh, W, H))
    for x in (nal, idx, out):
        x.free()
    dec.close()
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. arguments and state
def test_encoder_arguments_and_state(pkg):
    lib = pkg.load_library()
    enc = pkg.FerHip(64, 48, 1, qp=20, window=16)
    f = lib.ferhip_set_display_size
    for dw, dh in [(51, 38), (50, 37), (48, 38), (66, 38), (50, 32), (50, 50), (0, 38), (-2, 38), (64, 0)]:
        assert f(enc.ctx, dw, dh) == E_ARG, (dw, dh)
    assert f(None, 50, 38) == E_ARG
    assert f(enc.ctx, 50, 34) == 0 and f(enc.ctx, 64, 48) == 0  # (W, H) is the default again
    plain = pkg.FerHip(64, 48, 1, qp=20, window=16)
    assert enc.sps_pps() == plain.sps_pps()
    plain.close()
    assert f(enc.ctx, 50, 38) == 0
    buf = np.zeros(64 * 48 * 3 // 2, np.uint8)
    assert lib.ferhip_set_frames_display(enc.ctx, None, 1, None) == E_ARG
    assert lib.ferhip_set_frames_display(None, buf.ctypes.data, 1, None) == E_ARG
    assert lib.ferhip_upload_frames_display(enc.ctx, None, None) == E_ARG
    assert lib.ferhip_upload_frames_display(None, buf.ctypes.data, None) == E_ARG
    assert lib.ferhip_get_recon_display(enc.ctx, None, 1) == E_ARG
    assert lib.ferhip_get_recon_display(None, buf.ctypes.data, 1) == E_ARG
    enc.dw, enc.dh, enc.dfsz = 50, 38, 50 * 38 * 3 // 2
    enc.set_frames_display(buf[:enc.dfsz])
    enc.encode_picture()
    assert f(enc.ctx, 50, 38) == E_STATE and f(enc.ctx, 64, 48) == E_STATE  # a picture has been coded
    assert f(enc.ctx, 51, 38) == E_ARG
    enc.close()


def test_decoder_arguments_and_state(pkg, coded):
    lib = pkg.load_library()
    dec = pkg.LiveDecoder(2, W3, H3, 1)
    crop = (C.c_int * 4)()
    assert lib.ferhip_decs_get_crop(dec.h, 0, crop) == E_STATE  # no SPS yet
    assert lib.ferhip_decs_get_crop(dec.h, -1, crop) == E_ARG
    assert lib.ferhip_decs_get_crop(dec.h, 2, crop) == E_ARG
    assert lib.ferhip_decs_get_crop(dec.h, 0, None) == E_ARG
    assert lib.ferhip_decs_get_crop(None, 0, crop) == E_ARG
    f = lib.ferhip_decs_set_display
    for win in [(1, 0, 50, 38), (0, 1, 50, 38), (0, 0, 51, 38), (0, 0, 50, 37), (16, 0, 50, 38), (0, 12, 50, 38), (0, 0, 0, 38),
                (0, 0, 50, 0), (0, 0, 66, 38), (0, 0, 50, 50), (-2, 0, 50, 38), (0, -2, 50, 38)]:
        assert f(dec.h, *win) == E_ARG, win
    assert f(None, 0, 0, 50, 38) == E_ARG
    assert f(dec.h, 14, 10, 50, 38) == 0 and f(dec.h, 62, 46, 2, 2) == 0 and f(dec.h, 0, 0, W3, H3) == 0
    aus = pkg.access_units(coded["streams"][0])
    _, pics, st = dec.decode([aus[0], None])
    assert pics == [1, 0]
    assert dec.get_crop(0) == (0, 14, 0, 10)
    assert lib.ferhip_decs_get_crop(dec.h, 1, crop) == E_STATE  # stream 1 still has none
    dec.reset_stream(0)
    assert lib.ferhip_decs_get_crop(dec.h, 0, crop) == E_STATE  # forgotten with the parameter sets
    dec.close()


def test_untouched_context_reproduces_the_committed_golden(pkg):
    case = "qcif_ippp_4f_qp12_w16"
    m = json.loads((GOLD / "goldens.json").read_text())[case]
    gold = (GOLD / f"{case}.264").read_bytes()
    frames = np.stack([pkg.gen_frame(m["W"], m["H"], t, m["seed"], m["noise"]) for t in range(m["T"])])
    g = pkg.FerHip(m["W"], m["H"], 1, qp=m["qp"], window=m["window"], maxdiff=m["maxdiff"], intra_every=m["intra_every"])
    assert g.sps_pps()[0] == pm.split_nals(gold)[0]
    streams, rec = g.encode_streams(frames[:, None], want_recon=True)
    assert streams[0] == gold
    assert hashlib.sha256(rec.tobytes()).hexdigest() == m["recon_sha256"]
    g.close()
