"""The encoder and the decoders at every QP 0..51 (tests/qp_sweep.py), bit exact against the oracle.

ferhip_create takes params.qp 0..51 and ferhip_set_rate lets every picture be coded at any QP 0..51; the other whole-picture
tests reach a handful of those values and none below 10, and the block KATs of test_gpu_stages.py call the scalar transforms, not
the row forms (fwd_row / inv_row with the RowQ tables) that k_intra_mb and k_p_resid run.  Here every QP is met on whole pictures:

  a  the create route: a context per QP over the streams of qp_sweep.py
  b  the rate route: one context of 52 x 2 streams, every pair at its own QP through ferhip_set_rate
     (on both routes k_rc_plan writes QPy | QPc << 8 from c_qpc_tab of fer_rate.hip before every picture; k_qpc of fer_api.hip,
     which fills it at create, is only ever read through ferhip_chroma_qp: test_qp_sweep_host.py pins that one)
  c  all four decode entry points on the streams the device encoder wrote in (a)
  d  the block entry points (the scalar forms) on extreme, impulse, flat and random blocks at every QP
  e  ferhip_mb_unit (the scalar forms again, driven as the macroblock drivers do) with residuals over the whole +-255 at every QP
     (the row forms are reached by whole pictures only, (a) and (b): the mutant list in DESIGN.md)

tests/test_qp_sweep_host.py shows on the oracle alone what these runs reach.  Test ids group the QPs by q % 4, q % 13 or
q % 26 (the dearer a QP, the fewer an id), so each mixes low and high values.
"""
import ctypes as C

import numpy as np
import pytest

import qp_sweep as qs
import transform_model as tm
from enc_parity import compare_stream, device_run
from nal_model import frame_nal
from picture_oracle import check_pictures, encode_by_picture, oracle_pictures
from test_gpu_mbunit import _qpc

pytestmark = pytest.mark.gpu

GROUPS = range(4)       # q % 4: thirteen QPs an id
GROUPS13 = range(13)    # q % 13: four QPs an id, where a QP costs more (an oracle run, a decoder per stream)
GROUPS26 = range(26)    # q % 26: q and q + 26
YS = qs.W * qs.H
PLANES = (("Y", 0, YS), ("Cb", YS, YS + YS // 4), ("Cr", YS + YS // 4, YS * 3 // 2))
_device = {}


def _group(g, n=4):
    return [q for q in qs.QPS if q % n == g]


def _device_run(pkg, qp):
    """the streams of qp_sweep.py, one context created at this QP; run once per QP and shared by the tests.  The context is closed
    at once; what stays is about 0.2 MB a QP (four pictures of five streams: RBSP, reconstruction, side arrays), 10 MB for all 52.
    Whichever test first asks for a QP pays its encode and the oracle's runs of that QP: in file order that is (a), and the times
    in DESIGN.md are those of one whole-suite run in that order; test_batch_decoder_on_every_stream run alone pays for all 52
    itself (DESIGN.md has that time too)."""
    if qp not in _device:
        seqs = np.stack([qs.frames(s) for s in qs.STREAMS], 1)   # [4][S][fsz]
        _device[qp] = device_run(pkg, qs.W, qs.H, seqs, qp, qs.WINDOW)
    return _device[qp]


# ---------------------------------------------------------------- a. the create route
@pytest.mark.parametrize("group", GROUPS26)
def test_encoder_matches_oracle_at_every_qp(pkg, fo, group):
    """test_encoder_matches_oracle_on_hard_content's comparison (enc_parity.compare_stream, its three exclusions and no others) at
    every QP.  Under the level guard this pins the device against the reference; on the streams above it (seed 20 below QP 9,
    seed 22 below 5, seed 21 below 3) the comparison is the same, and what it pins is the device against the oracle, which
    writes the low 12 bits of an escape suffix (R3 of DESIGN.md) -- not the reference."""
    for qp in _group(group, 26):
        dev = _device_run(pkg, qp)
        for s, name in enumerate(qs.STREAMS):
            r = qs.run(fo, name, qp)
            compare_stream(dev, s, r["pics"], f"qp {qp} stream {name}")
            assert dev["streams"][s] == r["stream"], f"qp {qp} stream {name}: SPS / PPS / NAL framing"
        assert dev["status"] == [0] * len(qs.STREAMS), qp


# ---------------------------------------------------------------- b. the rate route
RATE_STREAMS = ("mild", 21)
RATE_TYPES = (5, 1, 5, 1)
MAX_BASE = 37   # the largest QP a stream's PPS can carry (pic_init_qp = 14 + base <= 51)


_rate = {}


def _rate_run(pkg):
    """One context of 52 x 2 streams created at QP 26, stream pair q ("mild", seed 21) coded at QP q through ferhip_set_rate:
    CQP q before the first picture for q <= 37; CQP 37 before picture 0 and CQP q before picture 1 for q > 37 (a base above 37 is
    refused) -> per stream the pictures (nal type, rbsp, recon, ferhip_get_qp after the picture), the Annex-B stream with the
    stream's own parameter sets (ferhip_write_pps_stream), status; run once and shared"""
    if not _rate:
        qps = [q for q in qs.QPS for _ in RATE_STREAMS]
        S = len(qps)
        frames = np.stack([qs.frames(n) for _ in qs.QPS for n in RATE_STREAMS], 1)   # [4][S][fsz]
        sched = [[min(q, MAX_BASE) for q in qps], [q if q > MAX_BASE else None for q in qps], [None] * S, [None] * S]
        g = pkg.FerHip(qs.W, qs.H, S, qp=26, window=qs.WINDOW, maxdiff=3, intra_every=1000)
        try:
            res = encode_by_picture(g, frames, sched, types=[[nt] * S for nt in RATE_TYPES])
            status = g.status()
            stream = [b"".join(g.sps_pps(s)) + b"".join(g.write_nal(nt, rb) for nt, rb, _, _ in res[s]) for s in range(S)]
        finally:
            g.close()
        _rate.update(res=res, stream=stream, status=status)
    return _rate


def test_set_rate_context_reports_the_schedule(pkg):
    """ferhip_get_qp after every picture, and status() all zero"""
    r = _rate_run(pkg)
    assert r["status"] == [0] * len(r["res"])
    for q in qs.QPS:
        for k in range(len(RATE_STREAMS)):
            got = [p[3] for p in r["res"][q * len(RATE_STREAMS) + k]]
            assert got == [min(q, MAX_BASE), q, q, q], f"stream pair {q}: ferhip_get_qp {got}"


@pytest.mark.parametrize("group", GROUPS13)
def test_set_rate_codes_every_qp_side_by_side(pkg, fo, group):
    """Stream pair q of _rate_run().  q <= 37: q is the stream's base, and the whole stream, its PPS included, is the oracle's at
    qp = q.  q > 37: the first picture at 37 (the largest base), then q from picture 1 on with slice_qp_delta = q - 37 - 14:
    compared picture by picture, header apart from slice_qp_delta, slice data, reconstruction (picture_oracle.check_pictures;
    the oracle codes the same QP schedule and types IDR, P, IDR, P)."""
    r = _rate_run(pkg)
    for q in _group(group, 13):
        for k, name in enumerate(RATE_STREAMS):
            s = q * len(RATE_STREAMS) + k
            want = [min(q, MAX_BASE)] + [q] * 3
            ora, _ = oracle_pictures(fo, qs.frames(name), want, qs.W, qs.H, window=qs.WINDOW, intra_every=1000, types=RATE_TYPES)
            check_pictures(r["res"][s], want[0], ora, f"stream {s} ({name}, qp {q})")
            if q <= MAX_BASE:
                ref = qs.parameter_sets(fo, q) + b"".join(frame_nal(nt, rb) for nt, rb, _ in ora)
                assert r["stream"][s] == ref, f"stream {s} ({name}, qp {q}): the whole stream, parameter sets included"


# ---------------------------------------------------------------- c. the decoders on the device encoder's streams
def _wanted(fo, name, qp, stream):
    """the oracle decoder's pictures of this stream (the record of qp_sweep.run() where the device wrote the oracle's bytes)"""
    r = qs.run(fo, name, qp)
    if stream == r["stream"]:
        return r["decoded"]
    n, dec, _ = fo.decode_stream_md5(stream)
    assert n == 4
    return np.stack(dec)


def _check_decoded(pkg, fo, name, qp, s, got, what):
    """got [4][fsz] against the oracle decoder plane by plane; under the guard the luma also against the encoder's
    reconstruction, as far as qp_sweep.luma_pictures() says a decoder gives it back"""
    dev = _device_run(pkg, qp)
    want = _wanted(fo, name, qp, dev["streams"][s])
    for t in range(4):
        for plane, a, b in PLANES:
            bad = np.flatnonzero(got[t][a:b] != want[t][a:b])
            assert bad.size == 0, f"{what}: qp {qp} stream {name} picture {t} {plane}: {bad.size} samples differ, first at {bad[:8]}"
    for t in range(qs.luma_pictures(fo, name, qp)):
        assert np.array_equal(got[t][:YS], dev["pics"][t]["recon"][s][:YS]), f"{what}: qp {qp} stream {name} picture {t}: the encoder's luma"


def test_batch_decoder_on_every_stream(pkg, fo):
    """all 52 x 5 streams of (a) in one ferhip_decode_streams call"""
    keys = [(q, s) for q in qs.QPS for s in range(len(qs.STREAMS))]
    streams = [_device_run(pkg, q)["streams"][s] for q, s in keys]
    out, pics, w, h = pkg.decode_streams(streams, 4)
    assert pics == [4] * len(keys) and (w, h) == (qs.W, qs.H)
    for k, (q, s) in enumerate(keys):
        _check_decoded(pkg, fo, qs.STREAMS[s], q, s, out[:, k], "decode_streams")


def _rate_streams(pkg, group, n=4):
    """(name, qp, index in the context, stream) of the "mild" and seed-21 streams of the group's QPs"""
    return [(name, q, qs.STREAMS.index(name), _device_run(pkg, q)["streams"][qs.STREAMS.index(name)])
            for q in _group(group, n) for name in RATE_STREAMS]


@pytest.mark.parametrize("group", GROUPS13)
def test_decode_nal_by_nal(pkg, fo, group):
    """ferhip_dec_nal, a decoder of its own per stream"""
    for name, qp, s, stream in _rate_streams(pkg, group, 13):
        d = pkg.Decoder()
        try:
            got = [p for p in (d.nal(*pkg.unescape_nal(nal)) for nal in pkg.split_nals(stream)) if p is not None]
        finally:
            d.close()
        assert len(got) == 4
        _check_decoded(pkg, fo, name, qp, s, got, "ferhip_dec_nal")


@pytest.mark.parametrize("group", GROUPS)
def test_legacy_rbsp_decode(pkg, fo, group, tmp_path):
    """RBSP_decode(NALunit) under the reference's name, output appended to `yuvoutput` (test_legacy_rbsp_decode_seam's driver)"""
    lib = pkg.load_library()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]

    class NALunit(C.Structure):
        _fields_ = [("forbidden_zero_bit", C.c_ubyte), ("nal_ref_idc", C.c_uint), ("nal_unit_type", C.c_uint),
                    ("NumBytesInRBSP", C.c_uint), ("rbsp_byte", C.POINTER(C.c_ubyte))]

    class Frame(C.Structure):
        _fields_ = [("Lwidth", C.c_int), ("Lheight", C.c_int), ("Cwidth", C.c_int), ("Cheight", C.c_int),
                    ("L", C.POINTER(C.c_ubyte)), ("C", C.POINTER(C.c_ubyte) * 2)]

    frame = Frame.in_dll(lib, "frame")   # the SPS call sizes and allocates it, as in the reference
    frame.L = None
    frame.C[0] = None
    frame.C[1] = None
    lib.RBSP_decode.argtypes = [NALunit]
    lib.RBSP_decode.restype = None
    buf = (C.c_ubyte * 65536)()
    head = b"YUV4MPEG2 C420jpeg W%d H%d F24:1 Ip A1:1\n" % (qs.W, qs.H)
    fsz = YS * 3 // 2
    for k, (name, qp, s, stream) in enumerate(_rate_streams(pkg, group)):
        out = tmp_path / f"dec{k}.y4m"
        lib.ferhip_fileio_reset()
        fout = libc.fopen(str(out).encode(), b"wb")
        assert fout
        C.c_void_p.in_dll(lib, "yuvoutput").value = fout
        try:
            for nal in pkg.split_nals(stream):
                t, idc, rbsp = pkg.unescape_nal(nal)
                C.memmove(buf, rbsp, len(rbsp))
                lib.RBSP_decode(NALunit(0, idc, t, len(rbsp), C.cast(buf, C.POINTER(C.c_ubyte))))
        finally:
            libc.fclose(fout)
            C.c_void_p.in_dll(lib, "yuvoutput").value = None
            lib.ferhip_fileio_reset()
        data = out.read_bytes()
        assert data[:len(head)] == head and len(data) == len(head) + 4 * (6 + fsz), f"qp {qp} stream {name}: {len(data)} bytes of Y4M"
        body = data[len(head):]
        assert all(body[t * (6 + fsz):t * (6 + fsz) + 6] == b"FRAME\n" for t in range(4))
        got = [np.frombuffer(body[t * (6 + fsz) + 6:(t + 1) * (6 + fsz)], np.uint8) for t in range(4)]
        _check_decoded(pkg, fo, name, qp, s, got, "RBSP_decode")


@pytest.mark.parametrize("group", GROUPS)
def test_live_decode(pkg, fo, group):
    """ferhip_decs_decode: the group's streams side by side in one live decoder, one access unit of every stream a call"""
    cases = _rate_streams(pkg, group)
    chunks = [pkg.access_units(stream) for _, _, _, stream in cases]
    assert all(len(c) == 4 for c in chunks)
    S = len(cases)
    d = pkg.LiveDecoder(S, qs.W, qs.H, 1)
    got = []
    try:
        for t in range(4):
            out = np.full((1, S, YS * 3 // 2), 0xA5, np.uint8)
            _, pics, status = d.decode([c[t] for c in chunks], out)
            assert pics == [1] * S and status == [0] * S, (t, pics, status)
            got.append(out[0])
    finally:
        d.close()
    for k, (name, qp, s, _) in enumerate(cases):
        _check_decoded(pkg, fo, name, qp, s, [g[k] for g in got], "ferhip_decs_decode")


# ---------------------------------------------------------------- d. block KATs at every QP
@pytest.mark.parametrize("group", GROUPS13)
def test_block_entry_points_at_every_qp(pkg, fo, group):
    """forward_residual / inverse_residual with both keep_dc values and the four DC operations on transform_model.kat_cases():
    the 32 extreme sign patterns, impulses, flat blocks, random full-range blocks; the inverses on the forward outputs and on
    random levels within the largest level of the QP; the DC operations on DCs from the forward outputs and the all-equal extremes"""
    from h264_fer_amd.ferhip import block_op, forward_residual, inverse_residual
    for qp in _group(group, 13):
        for op, keep, blocks in tm.kat_cases(qp):
            if op == "forward_residual":
                got, want = forward_residual(qp, blocks, keep), fo.forward_residual(qp, blocks, keep)
            elif op == "inverse_residual":
                got, want = inverse_residual(qp, blocks, keep), fo.inverse_residual(qp, blocks, keep)
            else:
                got, want = block_op(op, blocks, qp), fo.block_op(op, blocks, qp)
                if op.endswith("chroma"):   # a 2x2 operation: slots 0..3 of the record
                    got, want = got[:, :4], want[:, :4]
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, f"qp {qp} {op} keep_dc {keep}: {bad.size} blocks differ, first {blocks[bad[0]].tolist()} -> {got[bad[0]].tolist()} for {want[bad[0]].tolist()}"


# ---------------------------------------------------------------- e. ferhip_mb_unit at every QP
MBU_N = 8            # macroblocks per ferhip_mb_unit call
MBU_W, MBU_H = 64, 32
BLK_XY = ((0, 0), (4, 0), (0, 4), (4, 4), (8, 0), (12, 0), (8, 4), (12, 4), (0, 8), (4, 8), (0, 12), (4, 12), (8, 8), (12, 8), (8, 12), (12, 12))


def _mb_planes(frame):
    Y = frame[:MBU_W * MBU_H].reshape(MBU_H, MBU_W)
    Cb = frame[MBU_W * MBU_H:MBU_W * MBU_H * 5 // 4].reshape(MBU_H // 2, MBU_W // 2)
    Cr = frame[MBU_W * MBU_H * 5 // 4:].reshape(MBU_H // 2, MBU_W // 2)
    return Y, Cb, Cr


def _mb_of(planes, k):
    Y, Cb, Cr = planes
    y, x = (k // 4) * 16, (k % 4) * 16
    return Y[y:y + 16, x:x + 16], Cb[y // 2:y // 2 + 8, x // 2:x // 2 + 8], Cr[y // 2:y // 2 + 8, x // 2:x // 2 + 8]


@pytest.mark.parametrize("group", GROUPS)
def test_mb_unit_at_every_qp(pkg, fo, group):
    """FERHIP_MBU_QT for Intra16x16, inter and Intra4x4 macroblocks, with and without reconstruction, eight macroblocks a call,
    the prediction independent of the source (both uniform 0..255: residuals over the whole +-255); then DEC16, DEC4 of every
    block and DECC on the levels it produced.  Against Oracle.quantization_transform, as
    test_quantization_transform_and_decoding_drivers_kat does at seven QPs."""
    o = fo.Oracle(MBU_W, MBU_H)
    try:
        for qp in _group(group):
            rng = np.random.default_rng(5200 + qp)
            for mb_type, slice_type, cls in ((1, 2, 1), (0, 0, 2), (0, 2, 0)):  # I16 in an I slice, P_L0_16x16, I4x4
                for rec in (0, 1):
                    frame = rng.integers(0, 256, MBU_W * MBU_H * 3 // 2, dtype=np.uint8)
                    pred = rng.integers(0, 256, MBU_W * MBU_H * 3 // 2, dtype=np.uint8).astype(np.int32)
                    src, prd = _mb_planes(frame), _mb_planes(pred)
                    jobs, want = [], []
                    for k in range(MBU_N):
                        sY, sCb, sCr = _mb_of(src, k)
                        pY, pCb, pCr = _mb_of(prd, k)
                        jobs.append(dict(op=pkg.MBU_QT, cls=cls, qp=qp, qpc=_qpc(qp), reconstruct=rec, srcY=sY, srcCb=sCb, srcCr=sCr,
                                         predY=pY, predCb=pCb, predCr=pCr))
                        o.set_frame(frame)
                        o.set_mb(k, mb_type, slice_type, qp)
                        o.set_levels(lumaLevel=np.zeros(256), dc16=np.zeros(16), ac16=np.zeros(256), cdc=np.zeros(8), cac=np.zeros(128))
                        o.quantization_transform(pY, pCb, pCr, rec)
                        want.append((o.levels(), [a.copy() for a in _mb_of(_mb_planes(o.frame()), k)]))
                    res = pkg.mb_unit(jobs)
                    dec, dec_want = [], []
                    for k, (r, (lv, (oY, oCb, oCr))) in enumerate(zip(res, want)):
                        tag = f"qp {qp} class {cls} reconstruct {rec} macroblock {k}"
                        if cls == 2:
                            assert np.array_equal(r["lumaLevel"], lv["lumaLevel"]), tag
                        if cls == 1:
                            assert np.array_equal(r["dc16"], lv["dc16"]), tag
                            assert np.array_equal(r["ac16"].reshape(16, 16)[:, :15], lv["ac16"].reshape(16, 16)[:, :15]), tag
                        assert np.array_equal(r["cdc"], lv["cdc"]), tag
                        assert np.array_equal(r["cac"].reshape(8, 16)[:, :15], lv["cac"].reshape(8, 16)[:, :15]), tag
                        if not rec:
                            continue
                        if cls != 0:
                            assert np.array_equal(r["recY"].reshape(16, 16), oY), tag
                        assert np.array_equal(r["recCb"].reshape(8, 8), oCb) and np.array_equal(r["recCr"].reshape(8, 8), oCr), tag
                        pY, pCb, pCr = _mb_of(prd, k)
                        if cls == 1:
                            dec.append(dict(op=pkg.MBU_DEC16, qp=qp, qpc=_qpc(qp), predY=pY, dc16=r["dc16"], ac16=r["ac16"]))
                            dec_want.append((tag + " DEC16", "recY", (0, 0, 16), oY))
                        if cls == 2:
                            for blk, (x0, y0) in enumerate(BLK_XY):
                                dec.append(dict(op=pkg.MBU_DEC4, qp=qp, qpc=_qpc(qp), blk=blk, predY=pY, lumaLevel=r["lumaLevel"]))
                                dec_want.append((tag + f" DEC4 block {blk}", "recY", (x0, y0, 4), oY))
                        dec.append(dict(op=pkg.MBU_DECC, qp=qp, qpc=_qpc(qp), predCb=pCb, predCr=pCr, cdc=r["cdc"], cac=r["cac"]))
                        dec_want.append((tag + " DECC", "recCb", (0, 0, 8), oCb))
                        dec_want.append((tag + " DECC", "recCr", (0, 0, 8), oCr))
                    if dec:
                        out = iter(pkg.mb_unit(dec))
                        d = None
                        for tag, field, (x0, y0, n), plane in dec_want:
                            if field != "recCr":
                                d = next(out)
                            side = 16 if field == "recY" else 8
                            assert np.array_equal(d[field].reshape(side, side)[y0:y0 + n, x0:x0 + n], plane[y0:y0 + n, x0:x0 + n]), tag
    finally:
        o.close()
