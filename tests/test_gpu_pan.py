"""GPU parity on panned content (tests/pan_content.py): vectors, predictors and vector differences hundreds of quarter samples
long, bit exact against the oracle.

Every other encoder parity test moves its pictures by a few samples, so k_me_spec's far centres, the reach of k_me_walk's
diamond, k_me_resolve's long vector words and its P_Skip verdict at a long predicted vector, the merge / mvd / motion compensation
of k_p_resid far over the right and bottom edges, the long se(v) codes of k_cavlc and the decoders' side of all that never had
input.  tests/test_pan_content_host.py shows on the oracle alone that the runs below reach them; here the device only has to agree,
picture by picture: RBSP bytes, reconstruction, MBTYPE, MV, MVD, CBP, TC, the counters, status() all zero; then the motion lists
and the bucket walk of a far pair, and all four decode entry points on the device's own streams.

Side arrays are compared where the reference defines them, as in test_gpu_hard_content.py: CBP, TC and MVD outside P_Skip
macroblocks, TC on the blocks the CBP sends through the writer.  MVD is compared with the differences derived from the oracle's
vectors and types by the predictor rules (pan_content.mvd_of); the RBSP carries the same numbers once more.
"""
import numpy as np
import pytest

import pan_content as pc
from enc_parity import coded_tc_mask as _coded_tc_mask
from test_gpu_me_lists import run_case
from test_gpu_walk_dense import walk_check

pytestmark = pytest.mark.gpu

# launch shapes of the seventeen-stream context: (key, value) pairs for tune()
SHAPES = {"speculate": (("TUNE_SPECULATE", 1),), "no_speculation": (("TUNE_SPECULATE", 0),),
          "one_workgroup": (("TUNE_RESOLVE_WGS", 1), ("TUNE_RESOLVE_GROUP", 4))}
_device = {}


def _device_run(pkg, case, shape=None):
    """All pictures of every stream through set_frames / encode_picture with explicit types -> per picture a dict of what the
    device produced ([S] leading), the counters, status and the Annex-B streams; run once per (case, shape) and shared."""
    if (case, shape) not in _device:
        names, qp, window, maxdiff = case
        W, H = pc.SEQS[names[0]][:2]
        S = len(names)
        seqs = np.stack([pc.frames(n) for n in names], 1)   # [T][S][fsz]
        types = pc.nal_types(len(seqs))
        g = pkg.FerHip(W, H, S, qp=qp, window=window, maxdiff=maxdiff, intra_every=1000)
        try:
            for key, value in SHAPES[shape] if shape else ():
                g.tune(getattr(pkg, key), value)
            nmb = g.nmb
            pics = []
            for t, nt in enumerate(types):
                g.set_frames(seqs[t])
                rbsp, got = g.encode_picture(nal_types=[nt] * S)
                assert got == [nt] * S
                r = dict(rbsp=rbsp, recon=g.get_recon(), mb_type=g.read("MBTYPE").reshape(S, nmb), cbp=g.read("CBP").reshape(S, nmb, 2),
                         tc=g.read("TC").reshape(S, nmb, 24))
                if nt == 1:
                    r.update(mv=g.read("MV").reshape(S, nmb, 4, 2).astype(np.int64), mvd=g.read("MVD").reshape(S, nmb, 4, 2).astype(np.int64))
                pics.append(r)
            out = dict(pics=pics, stats=g.stats(), status=g.status(),
                       streams=[b"".join(g.sps_pps(s)) + b"".join(g.write_nal(nt, p["rbsp"][s]) for nt, p in zip(types, pics))
                                for s in range(S)])
        finally:
            g.close()
        _device[(case, shape)] = out
    return _device[(case, shape)]


def _compare(dev, fo, case):
    names, qp, window, maxdiff = case
    mbw = pc.SEQS[names[0]][0] // 16
    for s, name in enumerate(names):
        ref = pc.oracle_run(fo, name, qp, window, maxdiff)
        for t, (d, o) in enumerate(zip(dev["pics"], ref)):
            tag = f"{name} picture {t}"
            mt, cbp = o["mb_type"], o["cbp"]
            assert np.array_equal(d["mb_type"][s], mt), f"{tag}: MBTYPE at {np.flatnonzero(d['mb_type'][s] != mt)[:8]}"
            coded = mt != pc.P_SKIP
            if t:
                bad = np.flatnonzero((d["mv"][s] != o["mv"]).any((1, 2)))
                assert bad.size == 0, f"{tag}: MV at {bad[:8]}: {d['mv'][s][bad[0]].tolist()} for {o['mv'][bad[0]].tolist()}"
                want = pc.mvd_of(o["mv"], mt, mbw)
                bad = np.flatnonzero(((d["mvd"][s] != want).any((1, 2))) & coded)
                assert bad.size == 0, f"{tag}: MVD at {bad[:8]}: {d['mvd'][s][bad[0]].tolist()} for {want[bad[0]].tolist()}"
            assert np.array_equal(d["cbp"][s][coded], cbp[coded]), f"{tag}: CBP at {np.flatnonzero((d['cbp'][s] != cbp).any(1) & coded)[:8]}"
            m = _coded_tc_mask(mt, cbp) & coded[:, None]
            dtc = d["tc"][s].astype(np.int32)
            assert np.array_equal(dtc[m], o["tc"][m]), f"{tag}: TC at macroblocks {np.flatnonzero(((dtc != o['tc']) & m).any(1))[:8]}"
            bad = np.flatnonzero(d["recon"][s] != o["recon"])
            assert bad.size == 0, f"{tag}: {bad.size} reconstructed samples differ, first at {bad[:8]}"
            assert d["rbsp"][s] == o["rbsp"], f"{tag}: RBSP {len(d['rbsp'][s])} vs {len(o['rbsp'])} bytes"
        assert list(dev["stats"][s]) == list(ref[-1]["stats"]), f"{name}: brojTipova"
    assert dev["status"] == [0] * len(names)


@pytest.mark.parametrize("case", [c for c in pc.ENC_CASES if c[0] != pc.MANY], ids=pc.case_id)
def test_encoder_matches_oracle_on_panned_content(pkg, fo, case):
    _compare(_device_run(pkg, case), fo, case)


MANY_CASE = [c for c in pc.ENC_CASES if c[0] == pc.MANY][0]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_seventeen_streams_take_the_ticket_queues(pkg, fo, shape):
    """S >= 16: one ticket queue per XCD; every stream another pan, two of them still; three launch shapes"""
    _compare(_device_run(pkg, MANY_CASE, shape), fo, MANY_CASE)


def test_a_stream_of_the_seventeen_alone_gives_the_same_bytes(pkg, fo):
    names, qp, window, maxdiff = MANY_CASE
    k = 13
    alone = _device_run(pkg, ((names[k],), qp, window, maxdiff))
    many = _device_run(pkg, MANY_CASE, "speculate")
    assert alone["streams"][0] == many["streams"][k]
    for a, m in zip(alone["pics"], many["pics"]):
        assert np.array_equal(a["recon"][0], m["recon"][k])


# ---------------------------------------------------------------- the motion lists and the walk
@pytest.mark.parametrize("name,window", [("qcif_se40", 16), ("qcif_se40", 32), ("wide", 16)])
def test_lists_on_a_far_pair(pkg, fo, name, window):
    """ST3, V0, the guessed centres, SPEC_L1, SPEC_L2 and the resolved vector (test_gpu_me_lists.check_stream) where the true
    centres are hundreds of samples away: nearly every guess is a miss, and a few are hits"""
    W, H = pc.SEQS[name][:2]
    c, _, _ = run_case(pkg, fo, "pan:" + name, W, H, window, 3)
    assert c["hit"] > 0 and c["miss"] > 0, c
    assert c["nolist"] < c["parts"], c


@pytest.mark.parametrize("window", [16, 32])
def test_walk_on_a_far_pair(pkg, fo, window):
    f = pc.frames("qcif_se40")
    walk_check(pkg, fo, "pan:qcif_se40", f[0], f[1], window)


# ---------------------------------------------------------------- the decoders
DEC_CASE = {"qcif_se40": (pc.QUAD, 12, 16, 3), "qcif_ne90": (pc.QUAD, 12, 16, 3), "tall": (("tall",), 12, 16, 3)}
FILL = 0xA5


def _decoded(pkg, fo, name):
    """-> (the device encoder's stream of the sequence, the oracle decoder's pictures of it [T][fsz], which must also be the
    encoder's reconstructions)"""
    case = DEC_CASE[name]
    dev = _device_run(pkg, case)
    s = case[0].index(name)
    stream = dev["streams"][s]
    n, dec, _ = fo.decode_stream_md5(stream)
    assert n == len(dev["pics"])
    want = np.stack(dec)
    assert np.array_equal(want, np.stack([p["recon"][s] for p in dev["pics"]])), "the oracle decoder leaves the encoder's reconstruction"
    return stream, want


@pytest.mark.parametrize("name", pc.DEC_CASES)
def test_decode_streams(pkg, fo, name):
    stream, want = _decoded(pkg, fo, name)
    T = len(want)
    out, pics, w, h = pkg.decode_streams([stream, stream], T)
    assert pics == [T, T] and (w, h) == pc.SEQS[name][:2]
    for s in range(2):
        assert np.array_equal(out[:, s], want), f"stream {s}: pictures {np.flatnonzero((out[:, s] != want).any(1))}"


@pytest.mark.parametrize("name", pc.DEC_CASES)
def test_decode_nal_by_nal(pkg, fo, name):
    stream, want = _decoded(pkg, fo, name)
    d = pkg.Decoder()
    try:
        k = 0
        for nal in pkg.split_nals(stream):
            pic = d.nal(*pkg.unescape_nal(nal))
            if pic is not None:
                assert np.array_equal(pic, want[k]), f"picture {k}"
                k += 1
    finally:
        d.close()
    assert k == len(want)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", pc.DEC_CASES)
def test_live_decode(pkg, fo, name, where):
    """ferhip_decs_decode on host chunks / ferhip_decs_decode_dev on chunks in device memory (at an odd address), one access unit
    a call"""
    stream, want = _decoded(pkg, fo, name)
    W, H = pc.SEQS[name][:2]
    chunks = pkg.access_units(stream)
    assert len(chunks) == len(want)
    d = pkg.LiveDecoder(1, W, H, 1)
    buf = pkg.DeviceBuffer(max(len(c) for c in chunks) + 64) if where == "device" else None
    try:
        for k, c in enumerate(chunks):
            out = np.full((1, 1, W * H * 3 // 2), FILL, np.uint8)
            if buf:
                buf.upload(np.frombuffer(c, np.uint8), 1)
                _, pics, status = d.decode_dev([buf.ptr + 1], [len(c)], out)
            else:
                _, pics, status = d.decode([c], out)
            assert pics == [1] and status == [0], (k, pics, status)
            assert np.array_equal(out[0, 0], want[k]), f"picture {k}"
    finally:
        d.close()
        if buf:
            buf.free()
