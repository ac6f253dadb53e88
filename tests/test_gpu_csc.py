"""Packed 4:2:2 and 32-bit RGB pictures, converted on the device: FERHIP_FMT_YUY2, UYVY, BGRA and RGBA through
ferhip_set_pictures, ferhip_get_recon_pictures and the live decoder's output layout (ferhip_decs_set_layout).  The
yardsticks are the numpy model of the definition in include/ferhip.h (tests/csc_model.py, pinned in
tests/test_csc_model_host.py), tests/pad_model.py for the padding, and the oracle: an encode fed with packed pictures must be,
slice for slice, the oracle's encode of the model's converted and padded pictures."""
from pathlib import Path

import numpy as np
import pytest

import csc_model as csc
import pad_model as pm

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
E_ARG = -1
S = 3
SIZES = [(48, 32), (64, 32)]  # chroma width 24 = 8 (mod 16): half a strip of 4:2:2 at the end of a row, uint2 chroma stores; and 32
OFFS = [0, 4, 8, 12]          # plane base, bytes past a 16-byte boundary
EXTRA = [0, 4, 60]            # pitch = row bytes + ...
FMT_ID = {csc.YUY2: "yuy2", csc.UYVY: "uyvy", csc.BGRA: "bgra", csc.RGBA: "rgba"}
MAT_ID = {csc.BT601: "bt601", csc.BT709: "bt709"}
I420 = 0


class Pool:
    """Host arrays and their device twins, one allocation per stream.  A stream's plane starts `off` bytes past a 16-byte
    boundary, well inside its allocation: what surrounds it and what lies in its pitch gaps is the caller's fill."""

    def __init__(self, pkg, cap):
        self.pkg, self.cap = pkg, cap
        self.dev = [pkg.DeviceBuffer(cap) for _ in range(S)]
        assert all(d.ptr % 16 == 0 for d in self.dev)

    def layout(self, fmt, dw, dh, extra, offs, present=(1, 1, 1)):
        """-> model descriptors per stream; stream s takes offs[s % len(offs)]"""
        pitch = csc.row_bytes(fmt, dw) + extra
        assert 32 + 12 + pitch * dh + 32 <= self.cap
        return [[(s, 32 + offs[s % len(offs)], pitch)] if present[s] else None for s in range(S)]

    def host(self, fill):
        return [np.full(self.cap, fill, np.uint8) for _ in range(S)]

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


@pytest.fixture(scope="module")
def pool(pkg):
    p = Pool(pkg, 16384)
    yield p
    p.free()


def _cur(enc):
    return enc.read("CUR").reshape(enc.S, enc.fsz)


def _random_rows(rng, bufs, pics, fmt, dw, dh):
    """random bytes in every row of every present picture (A of an RGB pixel included), the rest as it was"""
    out = [b.copy() for b in bufs]
    for p in pics:
        if p is None:
            continue
        b, off, pitch = p[0]
        for y in range(dh):
            n = csc.row_bytes(fmt, dw)
            out[b][off + y * pitch:off + y * pitch + n] = rng.integers(0, 256, n, dtype=np.uint8)
    return out


def _refill(rows, pics, fmt, dw, dh, fill):
    """the pictures' rows of `rows` in buffers that hold `fill` everywhere else"""
    out = [np.full(r.size, fill, np.uint8) for r in rows]
    for p in pics:
        if p is None:
            continue
        b, off, pitch = p[0]
        n = csc.row_bytes(fmt, dw)
        for y in range(dh):
            out[b][off + y * pitch:off + y * pitch + n] = rows[b][off + y * pitch:off + y * pitch + n]
    return out


# ---------------------------------------------------------------- 1. ingest known-answer test
# the RGB formats under both matrices on the first size, under BT.601 on the other
INGEST = [(W, H, f, m) for (W, H) in SIZES for f in csc.FMTS for m in (csc.BT601, csc.BT709)
          if m == csc.BT601 or (f in (csc.BGRA, csc.RGBA) and (W, H) == SIZES[0])]


@pytest.mark.parametrize("ddh", [0, 2, 14])
@pytest.mark.parametrize("ddw", [0, 2, 14])
@pytest.mark.parametrize("W,H,fmt,matrix", INGEST, ids=[f"{w}x{h}-{FMT_ID[f]}-{MAT_ID[m]}" for w, h, f, m in INGEST])
def test_ingest_bytes(pkg, pool, W, H, fmt, matrix, ddw, ddh):
    dw, dh = W - ddw, H - ddh
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    enc.set_csc(matrix)
    rng = np.random.default_rng(W * 7 + ddw * 3 + ddh + fmt * 5 + matrix)
    for extra in EXTRA:
        for k, off in enumerate(OFFS):
            pics = pool.layout(fmt, dw, dh, extra, OFFS[k:] + OFFS[:k])  # stream 0 at `off`, the others at the offsets that follow it
            rows = _random_rows(rng, pool.host(0), pics, fmt, dw, dh)
            got = []
            for fill in (0x00, 0xFF):
                bufs = _refill(rows, pics, fmt, dw, dh, fill)
                pool.upload(bufs)
                enc.set_pictures(pool.descs(pics), fmt)
                got.append(_cur(enc))
                conv = csc.to_i420(bufs, pics, fmt, matrix, dw, dh)
                want = np.stack([pm.pad_picture(f, dw, dh, W, H) for f in conv])
                assert np.array_equal(got[-1], want), (extra, off, fill)
            assert np.array_equal(got[0], got[1]), (extra, off)  # nothing outside the rows reaches the pictures
    enc.close()


# ---------------------------------------------------------------- 2. absent streams
@pytest.mark.parametrize("fmt", csc.FMTS, ids=FMT_ID.get)
@pytest.mark.parametrize("W,H,dw,dh", [(48, 32, 46, 18), (64, 32, 64, 32)])
def test_absent_stream_keeps_its_picture(pkg, pool, W, H, dw, dh, fmt):
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    rng = np.random.default_rng(11 + fmt)
    pics = pool.layout(fmt, dw, dh, 4, [4, 8, 12])
    first = _random_rows(rng, pool.host(0xEE), pics, fmt, dw, dh)
    pool.upload(first)
    enc.set_pictures(pool.descs(pics), fmt)
    before = _cur(enc)
    second = _random_rows(rng, pool.host(0xEE), pics, fmt, dw, dh)
    pool.upload(second)
    table = pkg.pic_table(pool.descs(pics))
    table[1].plane[0] = None  # absent; the rest of its descriptor is garbage that would be refused or fault if it were used
    table[1].plane[1], table[1].plane[2] = 0x10, 0x13
    table[1].pitch[0], table[1].pitch[1], table[1].pitch[2] = 1, 3, 0xFFFFFFFF
    table[1].reserved = 0xDEAD
    enc.set_pictures(list(table), fmt)
    after = _cur(enc)
    c1 = csc.to_i420(first, pics, fmt, csc.BT601, dw, dh)
    c2 = csc.to_i420(second, pics, fmt, csc.BT601, dw, dh)
    assert np.array_equal(after[1], before[1])
    assert np.array_equal(after[1], pm.pad_picture(c1[1], dw, dh, W, H))
    for s in (0, 2):
        assert np.array_equal(after[s], pm.pad_picture(c2[s], dw, dh, W, H))
    enc.close()


# ---------------------------------------------------------------- 3. refusals
def test_refusals_change_nothing(pkg, pool):
    lib = pkg.load_library()
    W, H, dw, dh = 48, 32, 46, 30
    enc = pkg.FerHip(W, H, S, qp=20, window=16)
    enc.set_display_size(dw, dh)
    rng = np.random.default_rng(3)
    for fmt in csc.FMTS:
        rowb = csc.row_bytes(fmt, dw)
        pics = pool.layout(fmt, dw, dh, 8, [0])
        bufs = _random_rows(rng, pool.host(0x5A), pics, fmt, dw, dh)
        pool.upload(bufs)
        enc.set_pictures(pool.descs(pics), fmt)
        cur = _cur(enc)
        bufs = _random_rows(rng, bufs, pics, fmt, dw, dh)  # other pictures: an ingest that ran after all would show
        pool.upload(bufs)
        for f in (lib.ferhip_set_pictures, lib.ferhip_get_recon_pictures):
            def call(edit=None, fm=fmt):
                t = pkg.pic_table(pool.descs(pics))
                if edit:
                    edit(t)
                return f(enc.ctx, t, fm)
            for o in (1, 2, 3):                                                                  # plane[0] off the dword grid
                assert call(lambda t, o=o: t[1].plane.__setitem__(0, t[1].plane[0] + o)) == E_ARG
            for o in (1, 2, 3):                                                                  # pitch with a remainder mod 4
                assert call(lambda t, o=o: t[2].pitch.__setitem__(0, rowb + 8 + o)) == E_ARG
            assert call(lambda t: t[0].pitch.__setitem__(0, rowb - 4)) == E_ARG                   # pitch below the row
            assert call(lambda t: setattr(t[0], "reserved", 1)) == E_ARG                          # reserved != 0
            for bad in (2, 3, 6, 7, 10, -1):                                                     # no formats
                assert call(fm=bad) == E_ARG
            assert f(enc.ctx, None, fmt) == E_ARG and f(None, pkg.pic_table(pool.descs(pics)), fmt) == E_ARG
            assert np.array_equal(_cur(enc), cur)
            for got, want in zip(pool.download(), bufs):
                assert np.array_equal(got, want)
    dec = pkg.LiveDecoder(S, 176, 144, 1)
    for bad in (2, -1):
        assert lib.ferhip_set_csc(enc.ctx, bad) == E_ARG and lib.ferhip_decs_set_csc(dec.h, bad) == E_ARG
    assert lib.ferhip_set_csc(None, 0) == E_ARG and lib.ferhip_decs_set_csc(None, 0) == E_ARG
    for good in (csc.BT709, csc.BT601):
        assert lib.ferhip_set_csc(enc.ctx, good) == 0 and lib.ferhip_decs_set_csc(dec.h, good) == 0
    for bad in (2, 3, 6, 7, 10, -1):
        assert lib.ferhip_decs_set_layout(dec.h, bad, 1024, 0) == E_ARG
    dec.close()
    enc.close()


# ---------------------------------------------------------------- 4. encode parity with the oracle, 5. reconstruction out
EMIT = [(csc.YUY2, csc.BT601), (csc.UYVY, csc.BT601), (csc.BGRA, csc.BT601), (csc.BGRA, csc.BT709), (csc.RGBA, csc.BT601), (csc.RGBA, csc.BT709)]


@pytest.mark.parametrize("fmt,matrix", [(csc.BGRA, csc.BT709), (csc.UYVY, csc.BT601)], ids=["bgra_bt709", "uyvy"])
def test_encode_parity_and_recon_out(pkg, fo, pool, fmt, matrix):
    """IDR + 2 P pictures of moving textured content, written into packed buffers by the model and fed through descriptors:
    every slice is the oracle's encode of the model's converted and padded pictures, with the cropping SPS.  Then the
    reconstruction in all four formats is the model's conversion of ferhip_get_recon_display, gaps and surroundings included"""
    W, H, dw, dh, T, qp = 48, 32, 46, 18, 3, 12
    frames = np.stack([np.stack([fo.gen_frame(dw, dh, t, 700 + s, 2) for s in range(S)]) for t in range(T)])
    pics = pool.layout(fmt, dw, dh, 60, [4, 12, 8])
    enc = pkg.FerHip(W, H, S, qp=qp, window=16, maxdiff=3, intra_every=30)
    enc.set_display_size(dw, dh)
    enc.set_csc(matrix)
    sps_model = pm.sps_nal(W, H, dw, dh)
    assert enc.sps_pps()[0] == sps_model
    hosts = [csc.from_i420(pool.host(0xEE), pics, fmt, matrix, frames[t], dw, dh) for t in range(T)]
    padded = np.stack([np.stack([pm.pad_picture(f, dw, dh, W, H) for f in csc.to_i420(hosts[t], pics, fmt, matrix, dw, dh)]) for t in range(T)])
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
        pool.upload(hosts[t])
        enc.set_pictures(pool.descs(pics), fmt)
        assert np.array_equal(_cur(enc), padded[t])
        rbsp, nt = enc.encode_picture()
        types.append(nt[0])
        for s in range(S):
            wt, _, wrbsp = pkg.unescape_nal(ref_nals[s][2 + t])
            assert nt[s] == wt and rbsp[s] == wrbsp, f"picture {t} stream {s}: slice differs from the oracle's"
            streams[s] += enc.write_nal(nt[s], rbsp[s])
    assert types == [5, 1, 1]
    assert enc.status() == [0] * S
    for s in range(S):
        assert streams[s] == pm.swap_sps(ref[s], sps_model)
    rd = enc.get_recon_display()
    for s in range(S):
        assert np.array_equal(rd[s], pm.window(ref_rec[s][T - 1], W, H, 0, 0, dw, dh))
    # the way back, into pattern-filled buffers
    pattern = [((np.arange(pool.cap) + 7 * b) % 251).astype(np.uint8) for b in range(S)]
    for ofmt, omat in EMIT:
        enc.set_csc(omat)
        for extra in EXTRA:
            for k in range(len(OFFS)):
                opics = pool.layout(ofmt, dw, dh, extra, OFFS[k:] + OFFS[:k], present=(1, 1, 0) if k == 1 else (1, 1, 1))
                pool.upload(pattern)
                enc.get_recon_pictures(pool.descs(opics), ofmt)
                want = csc.from_i420(pattern, opics, ofmt, omat, rd, dw, dh)
                for g, w_ in zip(pool.download(), want):
                    assert np.array_equal(g, w_), f"{FMT_ID[ofmt]} {MAT_ID[omat]} +{extra} offsets {k}: gaps, surroundings or samples differ"
    enc.close()


# ---------------------------------------------------------------- 6. the live decoder's packed layouts
GW, GH = 176, 144
GOLDEN = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_skip_5f_qp12.264"]
FILL = 0xC3
WIN = (6, 10, 150, 118)


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


def _decode_packed(pkg, aus, fmt, matrix, pitch, win, dev_chunks, mis, late=(1,)):
    """two access units per call into pattern-filled device slots that start `mis` bytes past a 16-byte boundary; streams
    in `late` sit out the first call.  -> list over calls of (slot array [P][S][slot], pictures)"""
    P = 2
    dec = pkg.LiveDecoder(S, GW, GH, P)
    if win:
        dec.set_display(*win)
    dec.set_csc(matrix)
    dec.set_layout(fmt, pitch, 1)  # pitch_c is ignored
    slot = dec.fsz
    assert slot == csc.slot_bytes(fmt, pitch, (win or (0, 0, GW, GH))[3])
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
@pytest.mark.parametrize("win", [None, WIN], ids=["full", "window"])
@pytest.mark.parametrize("extra,mis", [(0, 0), (12, 4)], ids=["tight_aligned", "+12_base4"])
@pytest.mark.parametrize("fmt,matrix", [(csc.YUY2, csc.BT601), (csc.UYVY, csc.BT601), (csc.BGRA, csc.BT709), (csc.RGBA, csc.BT601)],
                         ids=["yuy2", "uyvy", "bgra_bt709", "rgba_bt601"])
def test_decoder_layout(pkg, golden_default, fmt, matrix, extra, mis, win, dev_chunks):
    aus, full = golden_default
    x0, y0, dw, dh = win or (0, 0, GW, GH)
    pitch = csc.row_bytes(fmt, dw) + extra
    calls = _decode_packed(pkg, aus, fmt, matrix, pitch, win, dev_chunks, mis)
    slot = csc.slot_bytes(fmt, pitch, dh)
    done = [0] * S
    for o, pics in calls:
        for s in range(S):
            for k in range(2):
                blank = np.full(slot, FILL, np.uint8)
                if k >= pics[s]:
                    assert np.array_equal(o[k, s], blank), f"stream {s}: an undecoded slot was written"
                    continue
                tight = pm.window(full[done[s] + k, s], GW, GH, x0, y0, dw, dh)
                want = csc.from_i420([blank], [csc.slot_pic(fmt, pitch, dh)], fmt, matrix, [tight], dw, dh)[0]
                assert np.array_equal(o[k, s], want), f"stream {s} picture {done[s] + k}"
            done[s] += pics[s]
    assert done == [4] * S


@pytest.mark.parametrize("dev_chunks", [False, True], ids=["decode", "decode_dev"])
def test_decoder_layout_refusals_consume_nothing(pkg, golden_default, dev_chunks):
    aus, full = golden_default
    fmt, dw, dh = csc.BGRA, GW, GH
    rowb = csc.row_bytes(fmt, dw)
    dec = pkg.LiveDecoder(S, GW, GH, 1)
    chunks = [a[0] for a in aus]
    cb, ptrs, lens = _dev_chunks(pkg, chunks)
    buf = pkg.DeviceBuffer(S * (rowb + 4) * dh + 32)
    buf.upload(np.full(buf.nbytes, FILL, np.uint8))

    def run(out):
        return dec.decode_dev(ptrs, lens, out) if dev_chunks else dec.decode(chunks, out)
    for pitch, out in [(rowb, buf.ptr + 1), (rowb, buf.ptr + 2), (rowb, buf.ptr + 3),   # a misaligned out
                       (rowb - 4, buf.ptr), (rowb + 2, buf.ptr),                          # pitch_y below the row, off the dword grid
                       (rowb, np.full((1, S, rowb * dh), FILL, np.uint8))]:              # host output
        dec.set_layout(fmt, pitch, 0)
        with pytest.raises(pkg.FerHipError):
            run(out)
    assert (buf.download() == FILL).all()
    dec.set_layout(fmt, rowb + 4, 0)  # the same call with good arguments: the first pictures are still there to take
    _, pics, st = run(buf.ptr + 4)
    assert pics == [1] * S and st == [0] * S
    slot = csc.slot_bytes(fmt, rowb + 4, dh)
    raw = buf.download()
    for s in range(S):
        want = csc.from_i420([np.full(slot, FILL, np.uint8)], [csc.slot_pic(fmt, rowb + 4, dh)], fmt, csc.BT601, [full[0, s]], dw, dh)[0]
        assert np.array_equal(raw[4 + s * slot:4 + (s + 1) * slot], want)
    dec.close()
    cb.free()
    buf.free()


# ---------------------------------------------------------------- 7. loopback: decoder slots feed an encoder in place
def test_loopback_yuy2_slots_feed_the_encoder(pkg, golden_default):
    aus, full = golden_default
    T, pitch = 4, 2 * GW + 32
    dec = pkg.LiveDecoder(S, GW, GH, T)
    dec.set_layout(csc.YUY2, pitch, 0)
    slot = dec.fsz
    out = pkg.DeviceBuffer(T * S * slot + 16)
    _, pics, st = dec.decode([b"".join(a) for a in aus], out.ptr + 4)
    assert pics == [T] * S and st == [0] * S
    enc = pkg.FerHip(GW, GH, S, qp=20, window=16)
    ref = pkg.FerHip(GW, GH, S, qp=20, window=16)
    tight = pkg.DeviceBuffer(S * GW * GH * 3 // 2)
    ysz = GW * GH
    for t in range(T):
        enc.set_pictures([([out.ptr + 4 + (t * S + s) * slot], [pitch]) for s in range(S)], csc.YUY2)
        tight.upload(full[t])
        base = [tight.ptr + s * ysz * 3 // 2 for s in range(S)]
        ref.set_pictures([([b, b + ysz, b + ysz * 5 // 4], [GW, GW // 2, GW // 2]) for b in base], I420)
        assert np.array_equal(_cur(enc), _cur(ref)), f"picture {t}"
        assert np.array_equal(_cur(enc), full[t])
    enc.close()
    ref.close()
    dec.close()
    out.free()
    tight.free()
