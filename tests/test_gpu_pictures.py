"""Pictures by descriptor: ferhip_set_pictures, ferhip_get_recon_pictures and the live decoder's pitched output layout
(ferhip_decs_set_layout) -- a pointer and a row pitch per stream and plane, I420 or NV12, at any byte alignment.  The
yardsticks are the numpy model (tests/pic_model.py, pinned in tests/test_pic_model_host.py) and the oracle: an encode fed
through descriptors must be, slice for slice, the oracle's encode of the model's gathered pictures."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import pad_model as pm
import pic_model as pic

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
E_ARG = -1
S = 3
SIZES = [(48, 32), (64, 32)]  # chroma width 24 = 8 (mod 16): words of two runs; and 32
FMTS = [pic.I420, pic.NV12]
EXTRA = [0, 1, 3, 61]         # pitch = row bytes + ...
OFFS = [0, 1, 2, 3, 5, 15]    # plane base, bytes past a 16-byte boundary
FMT_ID = {pic.I420: "i420", pic.NV12: "nv12"}


def _crow(fmt, dw):
    return dw // 2 if fmt == pic.I420 else dw


class Pool:
    """Host arrays and their device twins.  Stream 0 (and 1): the planes in one allocation; stream 2: one allocation per
    plane.  Every plane starts `off` bytes past a 16-byte boundary, well inside its allocation: what surrounds it and what
    lies in its pitch gaps is `fill`."""

    def __init__(self, pkg, cap):
        self.pkg, self.cap = pkg, cap
        self.dev = [pkg.DeviceBuffer(cap) for _ in range(5)]
        assert all(d.ptr % 16 == 0 for d in self.dev)

    def layout(self, fmt, dw, dh, extra, offs, present=(1, 1, 1)):
        """-> model descriptors [(buffer, offset, pitch)...] per stream; offs = the plane offsets, used in turn"""
        py, pc = dw + extra, _crow(fmt, dw) + extra
        np_ = 3 if fmt == pic.I420 else 2
        sizes = [py * dh] + [pc * (dh // 2)] * (np_ - 1)
        pitches = [py] + [pc] * (np_ - 1)
        pics, k = [], 0
        for s in range(S):
            if not present[s]:
                pics.append(None)
                continue
            planes, pos = [], 32
            for n in range(np_):
                o = offs[k % len(offs)]
                k += 1
                if s == 2:
                    planes.append((2 + n, 32 + o, pitches[n]))
                    assert 32 + o + sizes[n] + 32 <= self.cap
                else:
                    planes.append((s, pos + o, pitches[n]))
                    pos = (pos + o + sizes[n] + 15) // 16 * 16 + 32
                    assert pos <= self.cap
            pics.append(planes)
        return pics

    def host(self, fill):
        return [np.full(self.cap, fill, np.uint8) for _ in range(5)]

    def upload(self, bufs):
        for d, b in zip(self.dev, bufs):
            d.upload(b)

    def download(self):
        return [d.download() for d in self.dev]

    def descs(self, pics):
        """model descriptors -> what pkg.pic_table takes, with device addresses"""
        return [None if p is None else ([self.dev[b].ptr + o for b, o, _ in p], [t for _, _, t in p]) for p in pics]

    def free(self):
        for d in self.dev:
            d.free()


def _cur(enc):
    return enc.read("CUR").reshape(enc.S, enc.fsz)


def _fill_pictures(bufs, pics, fmt, frames, dw, dh):
    return pic.scatter(bufs, pics, fmt, frames, dw, dh)


# ---------------------------------------------------------------- 1. ingest known-answer test
@pytest.fixture(scope="module")
def pool(pkg):
    p = Pool(pkg, 16384)
    yield p
    p.free()


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID.get)
@pytest.mark.parametrize("ddh", [0, 2, 14])
@pytest.mark.parametrize("ddw", [0, 2, 14])
@pytest.mark.parametrize("W,H", SIZES)
def test_ingest_bytes(pkg, pool, W, H, ddw, ddh, fmt):
    dw, dh = W - ddw, H - ddh
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    rng = np.random.default_rng(W * 7 + ddw * 3 + ddh + fmt)
    for extra in EXTRA:
        for k, off in enumerate(OFFS):
            frames = rng.integers(1, 255, (S, dw * dh * 3 // 2), dtype=np.uint8)
            offs = OFFS[k:] + OFFS[:k]  # the first plane at `off`, the others at the offsets that follow it
            pics = pool.layout(fmt, dw, dh, extra, offs)
            got = []
            for fill in (0x00, 0xFF):
                bufs = _fill_pictures(pool.host(fill), pics, fmt, frames, dw, dh)
                pool.upload(bufs)
                enc.set_pictures(pool.descs(pics), fmt)
                got.append(_cur(enc))
                want = np.stack(pic.gather(bufs, pics, fmt, dw, dh, W, H))
                assert np.array_equal(got[-1], want), (extra, off, fill)
            assert np.array_equal(got[0], got[1]), (extra, off)  # nothing outside the rows reaches the pictures
            assert np.array_equal(got[0], np.stack([pm.pad_picture(f, dw, dh, W, H) for f in frames]))
    enc.close()


def test_tight_i420_descriptors_equal_the_display_size_ingest(pkg):
    """A packed [S][dw*dh*3/2] array is a descriptor table with pitches dw, dw/2, dw/2: both ingest kernels run the same body
    over it and must fill the same picture set, at an odd base address and a chroma width of 8 (mod 16)."""
    W, H, dw, dh = 80, 48, 66, 48
    dys, fsz = dw * dh, dw * dh * 3 // 2
    frames = np.random.default_rng(23).integers(1, 255, (S, fsz), dtype=np.uint8)
    buf = pkg.DeviceBuffer(S * fsz + 32)
    buf.upload(np.full(S * fsz + 32, 0xEE, np.uint8))
    buf.upload(frames, offset=3)
    base = [buf.ptr + 3 + s * fsz for s in range(S)]
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    enc.set_pictures([([b, b + dys, b + dys + dys // 4], [dw, dw // 2, dw // 2]) for b in base], pic.I420)
    by_desc = _cur(enc)
    enc.set_frames(np.zeros((S, enc.fsz), np.uint8))
    enc.set_frames_display(buf.ptr + 3)
    by_display = _cur(enc)
    enc.close()
    buf.free()
    assert np.array_equal(by_desc, by_display)
    assert np.array_equal(by_desc, np.stack([pm.pad_picture(f, dw, dh, W, H) for f in frames]))


# ---------------------------------------------------------------- 2. absent streams
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID.get)
@pytest.mark.parametrize("W,H,dw,dh", [(48, 32, 46, 18), (64, 32, 64, 32)])
def test_absent_stream_keeps_its_picture(pkg, pool, W, H, dw, dh, fmt):
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    rng = np.random.default_rng(11)
    first = rng.integers(1, 255, (S, dw * dh * 3 // 2), dtype=np.uint8)
    pics = pool.layout(fmt, dw, dh, 3, [1, 5, 2])
    pool.upload(_fill_pictures(pool.host(0xEE), pics, fmt, first, dw, dh))
    enc.set_pictures(pool.descs(pics), fmt)
    before = _cur(enc)
    second = rng.integers(1, 255, (S, dw * dh * 3 // 2), dtype=np.uint8)
    pool.upload(_fill_pictures(pool.host(0xEE), pics, fmt, second, dw, dh))
    table = pkg.pic_table(pool.descs(pics))
    table[1].plane[0] = None  # absent; the rest of its descriptor is garbage that would be refused or fault if it were used
    table[1].plane[1], table[1].plane[2] = 0x10, None
    table[1].pitch[0], table[1].pitch[1], table[1].pitch[2] = 1, 0, 0xFFFFFFFF
    table[1].reserved = 0xDEAD
    enc.set_pictures(list(table), fmt)
    after = _cur(enc)
    assert np.array_equal(after[1], before[1])
    assert np.array_equal(after[1], pm.pad_picture(first[1], dw, dh, W, H))
    for s in (0, 2):
        assert np.array_equal(after[s], pm.pad_picture(second[s], dw, dh, W, H))
    enc.close()


# ---------------------------------------------------------------- 3. argument errors
def test_argument_errors(pkg, pool):
    lib = pkg.load_library()
    W, H, dw, dh = 48, 32, 46, 30
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    for fmt in FMTS:
        pics = pool.layout(fmt, dw, dh, 0, [0])
        for f in (lib.ferhip_set_pictures, lib.ferhip_get_recon_pictures):
            def call(edit=None, fm=fmt):
                t = pkg.pic_table(pool.descs(pics))
                if edit:
                    edit(t)
                return f(enc.ctx, t, fm)
            assert call() == 0
            assert call(fm=2) == E_ARG and call(fm=-1) == E_ARG                                   # unknown format
            assert call(lambda t: setattr(t[0], "reserved", 1)) == E_ARG                          # reserved != 0
            assert call(lambda t: t[2].pitch.__setitem__(0, dw - 1)) == E_ARG                     # pitch below the row
            assert call(lambda t: t[0].pitch.__setitem__(1, _crow(fmt, dw) - 1)) == E_ARG
            assert call(lambda t: t[1].plane.__setitem__(1, None)) == E_ARG                       # NULL chroma plane
            assert call(lambda t: t[1].plane.__setitem__(2, None)) == (E_ARG if fmt == pic.I420 else 0)  # NV12 ignores plane[2]
            assert f(enc.ctx, None, fmt) == E_ARG and f(None, pkg.pic_table(pool.descs(pics)), fmt) == E_ARG
    enc.close()


# ---------------------------------------------------------------- 4. encode parity with the oracle, 5. reconstruction out
def _gen(fo, dw, dh, T, seed0=700):
    return np.stack([np.stack([fo.gen_frame(dw, dh, t, seed0 + s, 2) for s in range(S)]) for t in range(T)])


@pytest.mark.parametrize("fmt,W,H,dw,dh,extra", [(pic.NV12, 64, 48, 62, 34, 61), (pic.I420, 64, 48, 64, 48, 3)],
                         ids=["nv12_62x34_pitched", "i420_coded_size"])
def test_encode_parity_and_recon_out(pkg, fo, fmt, W, H, dw, dh, extra):
    """IDR + 2 P pictures of moving textured content, fed through descriptors: every slice is the oracle's encode of the
    model's gathered pictures (with the cropping SPS when dw x dh is not the coded size), and the reconstruction written
    through descriptors is the model's scatter of ferhip_get_recon_display"""
    T, qp = 3, 12
    frames = _gen(fo, dw, dh, T)
    p = Pool(pkg, 32768)
    pics = p.layout(fmt, dw, dh, extra, [5, 1, 15, 3])
    enc = pkg.FerHip(W, H, S, qp=qp, window=16, maxdiff=3, intra_every=30)
    enc.set_display_size(dw, dh)
    sps_model = pm.sps_nal(W, H, dw, dh)
    assert enc.sps_pps()[0] == sps_model
    hosts = [_fill_pictures(p.host(0xEE), pics, fmt, frames[t], dw, dh) for t in range(T)]
    padded = np.stack([np.stack(pic.gather(hosts[t], pics, fmt, dw, dh, W, H)) for t in range(T)])
    ref_nals, ref_rec, ref = [], [], []
    for s in range(S):
        o = fo.Oracle(W, H, qp=qp, window=16, maxdiff=3, intra_every=30)
        st, rec = o.encode_stream(padded[:, s])
        o.close()
        ref.append(st)
        ref_nals.append(pm.split_nals(st))
        ref_rec.append(rec)
    streams = [sps_model + enc.sps_pps(s)[1] for s in range(S)]
    types = []
    for t in range(T):
        p.upload(hosts[t])
        enc.set_pictures(p.descs(pics), fmt)
        rbsp, nt = enc.encode_picture()
        types.append(nt[0])
        for s in range(S):
            want = ref_nals[s][2 + t]
            wt, _, wrbsp = pkg.unescape_nal(want)
            assert nt[s] == wt and rbsp[s] == wrbsp, f"picture {t} stream {s}: slice differs from the oracle's"
            streams[s] += enc.write_nal(nt[s], rbsp[s])
        rd = enc.get_recon_display()
        for s in range(S):
            assert np.array_equal(rd[s], pm.window(ref_rec[s][t], W, H, 0, 0, dw, dh))
        # the way back, into pattern-filled buffers of both formats and another pitch and alignment
        for ofmt in FMTS:
            opics = p.layout(ofmt, dw, dh, 3 if ofmt == fmt else 61, [3, 2, 1, 15], present=(1, 0, 1))
            pattern = [((np.arange(p.cap) + 7 * b) % 251).astype(np.uint8) for b in range(5)]
            p.upload(pattern)
            enc.get_recon_pictures(p.descs(opics), ofmt)
            got = p.download()
            want = pic.scatter(pattern, opics, ofmt, rd, dw, dh)
            for g, w_ in zip(got, want):
                assert np.array_equal(g, w_), f"picture {t} format {ofmt}: gaps, surroundings or samples differ"
    assert types == [5, 1, 1]
    assert enc.status() == [0] * S
    for s in range(S):
        assert streams[s] == pm.swap_sps(ref[s], sps_model)
    enc.close()
    p.free()


# ---------------------------------------------------------------- 6. the live decoder's pitched layout
GW, GH = 176, 144
GOLDEN = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_skip_5f_qp12.264"]
FILL = 0xC3


@pytest.fixture(scope="module")
def golden_default(pkg):
    """the golden streams' access units, and every picture in the default layout (full coded pictures, host output)"""
    streams = [(GOLD / n).read_bytes() for n in GOLDEN]
    aus = [pkg.access_units(s)[:4] for s in streams]
    dec = pkg.LiveDecoder(S, GW, GH, 4)
    o, pics, st = dec.decode([b"".join(a) for a in aus])
    dec.close()
    assert pics == [4] * S and st == [0] * S
    return aus, o.copy()


def _dev_chunks(pkg, chunks):
    cb = pkg.DeviceBuffer(sum(len(c) + 16 for c in chunks if c) + 16)
    ptrs, lens, o = [], [], 3
    for c in chunks:
        if c:
            cb.upload(np.frombuffer(c, np.uint8), offset=o)
        ptrs.append(cb.ptr + o if c else None)
        lens.append(len(c) if c else 0)
        o += (len(c) if c else 0) + 5
    return cb, ptrs, lens


def _decode_pitched(pkg, aus, fmt, py, pc, win, dev_chunks, mis=1, late=(1,)):
    """two access units per call into pattern-filled device slots; streams in `late` sit out the first call.
    -> list over calls of (slot array [P][S][slot], pictures)"""
    P = 2
    dec = pkg.LiveDecoder(S, GW, GH, P)
    if win:
        dec.set_display(*win)
    dec.set_layout(fmt, py, pc)
    slot = dec.fsz
    assert slot == pic.slot_bytes(fmt, py, pc, (win or (0, 0, GW, GH))[3])
    buf = pkg.DeviceBuffer(P * S * slot + 32)
    pos, calls, call = [0] * S, [], 0
    while any(pos[s] < len(aus[s]) for s in range(S)):
        take = [0 if (call == 0 and s in late) else min(P, len(aus[s]) - pos[s]) for s in range(S)]
        chunks = [b"".join(aus[s][pos[s]:pos[s] + take[s]]) or None for s in range(S)]
        for s in range(S):
            pos[s] += take[s]
        buf.upload(np.full(P * S * slot + 32, FILL, np.uint8))
        if dev_chunks:
            cb, ptrs, lens = _dev_chunks(pkg, chunks)
            _, pics, st = dec.decode_dev(ptrs, lens, buf.ptr + mis)
            cb.free()
        else:
            _, pics, st = dec.decode(chunks, buf.ptr + mis)
        assert st == [0] * S and pics == take
        raw = buf.download()
        assert (raw[:mis] == FILL).all() and (raw[mis + P * S * slot:] == FILL).all()
        calls.append((raw[mis:mis + P * S * slot].reshape(P, S, slot), pics))
        call += 1
    dec.close()
    buf.free()
    return calls


@pytest.mark.parametrize("dev_chunks", [False, True], ids=["decode", "decode_dev"])
@pytest.mark.parametrize("win", [None, (6, 10, 150, 118)], ids=["full", "window"])
@pytest.mark.parametrize("pitch", ["+0", "+3", "256"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID.get)
def test_decoder_layout(pkg, golden_default, fmt, pitch, win, dev_chunks):
    aus, full = golden_default
    x0, y0, dw, dh = win or (0, 0, GW, GH)
    py, pc = {"+0": (dw, _crow(fmt, dw)), "+3": (dw + 3, _crow(fmt, dw) + 3), "256": (256, 256)}[pitch]
    calls = _decode_pitched(pkg, aus, fmt, py, pc, win, dev_chunks)
    slot = pic.slot_bytes(fmt, py, pc, dh)
    done = [0] * S
    for o, pics in calls:
        for s in range(S):
            for k in range(2):
                blank = np.full(slot, FILL, np.uint8)
                if k >= pics[s]:
                    assert np.array_equal(o[k, s], blank), f"stream {s}: an undecoded slot was written"
                    continue
                tight = pm.window(full[done[s] + k, s], GW, GH, x0, y0, dw, dh)
                want = pic.scatter([blank], [pic.slot_pic(fmt, py, pc, dh)], fmt, [tight], dw, dh)[0]
                assert np.array_equal(o[k, s], want), f"stream {s} picture {done[s] + k}"
            done[s] += pics[s]
    assert done == [4] * S


def test_decoder_layout_arguments_and_reset(pkg, golden_default):
    aus, full = golden_default
    lib = pkg.load_library()
    dec = pkg.LiveDecoder(S, GW, GH, 1)
    f = lib.ferhip_decs_set_layout
    assert f(None, pic.NV12, 256, 256) == E_ARG and f(dec.h, 2, 256, 256) == E_ARG and f(dec.h, -1, 256, 256) == E_ARG
    chunks = [a[0] for a in aus]
    host = np.full((1, S, dec.cfsz), FILL, np.uint8)
    dec.set_layout(pic.NV12, GW, GW)
    with pytest.raises(pkg.FerHipError):  # a layout other than the default with host output
        dec.decode(chunks, np.full((1, S, dec.fsz), FILL, np.uint8))
    buf = pkg.DeviceBuffer(S * 256 * GH * 2)
    for fmt, py, pc in [(pic.I420, GW - 1, GW // 2), (pic.I420, GW, GW // 2 - 1), (pic.NV12, GW, GW - 1)]:  # pitches below a row
        dec.set_layout(fmt, py, pc)
        with pytest.raises(pkg.FerHipError):
            dec.decode(chunks, buf)
    dec.set_layout(pic.I420, GW, GW // 2)  # the default again: host output works, today's bytes
    assert dec.fsz == dec.cfsz
    o, pics, st = dec.decode(chunks, host)
    assert pics == [1] * S and st == [0] * S and np.array_equal(o[0], full[0])
    dec.set_display(6, 10, 150, 118)
    dec.set_layout(pic.I420, 150, 75)  # the default of the window
    o, pics, st = dec.decode([a[1] for a in aus])
    assert pics == [1] * S
    for s in range(S):
        assert np.array_equal(o[0, s], pm.window(full[1, s], GW, GH, 6, 10, 150, 118))
    dec.close()
    buf.free()


# ---------------------------------------------------------------- 7. loopback: decoder slots feed an encoder in place
def test_loopback_nv12_slots_feed_the_encoder(pkg, fo):
    T, qp = 4, 20
    streams = [(GOLD / n).read_bytes() for n in GOLDEN]
    aus = [pkg.access_units(s)[:T] for s in streams]
    dec = pkg.LiveDecoder(S, GW, GH, T)
    dec.set_layout(pic.NV12, 256, 256)
    slot = dec.fsz
    out = pkg.DeviceBuffer(T * S * slot + 16)
    _, pics, st = dec.decode([b"".join(a) for a in aus], out.ptr + 1)  # slots at odd addresses
    assert pics == [T] * S and st == [0] * S
    enc = pkg.FerHip(GW, GH, S, qp=qp, window=16, maxdiff=3, intra_every=30)
    got = [b"".join(enc.sps_pps(s)) for s in range(S)]
    for t in range(T):
        base = [out.ptr + 1 + (t * S + s) * slot for s in range(S)]
        enc.set_pictures([([b, b + 256 * GH], [256, 256]) for b in base], pic.NV12)
        rbsp, nt = enc.encode_picture()
        for s in range(S):
            got[s] += enc.write_nal(nt[s], rbsp[s])
    assert enc.status() == [0] * S
    for s in range(S):
        n, decoded, _ = fo.decode_stream_md5(b"".join(aus[s]))
        assert n == T
        o = fo.Oracle(GW, GH, qp=qp, window=16, maxdiff=3, intra_every=30)
        want, _ = o.encode_stream(np.stack(decoded))
        o.close()
        assert got[s] == want, f"stream {s}"
    enc.close()
    dec.close()
    out.free()
