"""The Annex-B splitter on the device (ferhip_split_nal_blocks, csrc/fer_nalsplit.hip) against tests/nal_split_model.py
(pinned to split_stream's byte loop by test_nal_split_model_host.py), and the live decoder fed from device memory
(ferhip_decs_decode_dev) against ferhip_decs_decode on the same bytes."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import nal_model
import nal_split_model as sm

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
W, H = 176, 144
FSZ = W * H * 3 // 2
FILL = 0xA5
E_ARG, E_STATE, E_UNSUP, E_DEVICE = -1, -3, -4, -5

_cache = {}


def _check(ranges, rc, out, units, count, cap, first_range=0):
    """table and bytes equal the model's layout; every byte of out outside the units' RBSP still holds the fill value"""
    want_units, spans, total = sm.layout(ranges)
    assert rc == 0 and total <= cap
    assert count == len(want_units)
    got = [(int(u["range"]) - first_range, int(u["nal_type"]), int(u["ref_idc"]), int(u["bytes"]), int(u["offset"])) for u in units]
    assert got == want_units
    want = np.full(out.size, FILL, np.uint8)
    for off, p in spans:
        want[off: off + len(p)] = np.frombuffer(p, np.uint8)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])} of {total}"


def _layout_total(ranges):
    k = id(ranges)
    if k not in _cache:
        _cache[k] = sm.layout(ranges)[2]
    return _cache[k]


@pytest.mark.parametrize("misalign", [0, 1, 7, 15])
def test_kat_corpus_one_call(pkg, misalign):
    corpus = sm.corpus()
    cap = _layout_total(corpus) + 80
    rc, out, units, count = pkg.split_nal_blocks_raw(corpus, misalign, cap=cap, fill=FILL)
    _check(corpus, rc, out, units, count, cap)


def test_kat_corpus_one_range_per_call(pkg):
    for k, r in enumerate(sm.corpus()):
        total = sm.layout([r])[2]
        rc, out, units, count = pkg.split_nal_blocks_raw([r], k % 16, cap=total + 32, fill=FILL)
        _check([r], rc, out, units, count, total + 32)


def test_kat_unit_longer_than_the_grid_and_a_range_of_tiny_units(pkg):
    """one unit of 150 chunks (the grid has 64 workgroups per range: the strided walk), and 600 five-byte units in a row"""
    rng = np.random.default_rng(31)
    big = sm.draw(rng, 150 * sm.CHUNK).copy()
    big[:5] = (0, 0, 0, 1, 0x65)
    while True:  # the drawn bytes stay, except that the third byte of every terminator becomes 03: one unit, many dropped bytes
        z = big[5:] == 0
        t = np.flatnonzero(z[:-2] & z[1:-1] & (big[7:] <= 1))
        if t.size == 0:
            break
        big[t + 7] = 3
    if big[-1] == 0 and big[-2] == 0:
        big[-1] = 0x80
    tiny = np.tile(np.array([0, 0, 0, 1, 0x41, 9, 8, 7, 6], np.uint8), 600)
    ranges = [tiny, big, tiny[:-2]]
    units, _, total = sm.layout(ranges)
    assert len(units) == 1201 and units[600][3] > 400000 and big.size == 614400
    for misalign in (0, 9):
        rc, out, got, count = pkg.split_nal_blocks_raw(ranges, misalign, cap=total + 16, fill=FILL)
        _check(ranges, rc, out, got, count, total + 16)


def test_kat_arguments(pkg):
    r = [np.array([0, 0, 0, 1, 0x67, 1, 2, 0, 0, 0, 1, 0x68, 3, 0, 0, 0, 1, 0x65, 4, 4], np.uint8)]
    for misalign in (-1, 16, 100):
        assert pkg.split_nal_blocks_raw(r, misalign)[0] == E_ARG
    rc, out, units, count = pkg.split_nal_blocks_raw(r, 3, units_cap=2, fill=FILL)
    assert rc == E_ARG and count == 3 and [int(u["nal_type"]) for u in units] == [7, 8]
    rc, out, units, count = pkg.split_nal_blocks_raw(r, 3, units_cap=0, fill=FILL)
    assert rc == E_ARG and count == 3
    rc, out, units, count = pkg.split_nal_blocks_raw(r, 3, cap=32, fill=FILL)  # room for two of the three units
    assert rc == E_ARG and count == 3 and bytes(out[:2]) == b"\x01\x02" and out[16] == 3 and np.all(out[17:] == FILL)
    rc, out, units, count = pkg.split_nal_blocks_raw(r, 3, cap=48, fill=FILL)
    assert rc == 0 and count == 3 and bytes(out[32:34]) == b"\x04\x04"
    # nothing to split
    rc, out, units, count = pkg.split_nal_blocks_raw([np.zeros(0, np.uint8), np.zeros(0, np.uint8)], 5, fill=FILL)
    assert rc == 0 and count == 0 and np.all(out == FILL)
    assert pkg.split_nal_blocks_raw([], 0)[0] == E_ARG


# ---- the live decoder fed from device memory

def _golden_aus(pkg):
    if "aus" not in _cache:
        a = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
        b = (GOLD / "qcif_skip_5f_qp12.264").read_bytes()
        _cache["aus"] = [pkg.access_units(s) for s in (a, b, a)]
    return _cache["aus"]


class _Feeder:
    """a call's chunks in device memory, each at an odd address (stream s starts 2 s + 1 bytes past a multiple of 16)"""

    def __init__(self, pkg, S, room):
        self.pitch = ((room + 63) & ~15)
        self.buf = pkg.DeviceBuffer(S * self.pitch + 64)

    def put(self, chunks):
        ptrs, lens = [], []
        for s, c in enumerate(chunks):
            if not c:
                ptrs.append(None)
                lens.append(0)
                continue
            off = s * self.pitch + 2 * s + 1
            assert len(c) + 2 * s + 1 <= self.pitch
            self.buf.upload(np.frombuffer(c, np.uint8), off)
            ptrs.append(self.buf.ptr + off)
            lens.append(len(c))
        return ptrs, lens

    def free(self):
        self.buf.free()


def _run(pkg, calls, S, P=1, device_in=False, device_out=False, dec=None):
    """calls: a list of chunk lists -> per call (pictures [list of arrays per stream], pics, status); slots past a stream's
    pictures must keep the fill value"""
    own = dec is None
    dec = dec or pkg.LiveDecoder(S, W, H, P)
    feeder = _Feeder(pkg, S, max(len(c) for call in calls for c in call if c)) if device_in else None
    buf = pkg.DeviceBuffer(P * S * FSZ) if device_out else None
    out = []
    for chunks in calls:
        if device_out:
            buf.upload(np.full(P * S * FSZ, FILL, np.uint8))
            target = buf
        else:
            target = np.full((P, S, FSZ), FILL, np.uint8)
        if device_in:
            ptrs, lens = feeder.put(chunks)
            _, pics, st = dec.decode_dev(ptrs, lens, target)
        else:
            _, pics, st = dec.decode(chunks, target)
        o = buf.download().reshape(P, S, FSZ) if device_out else target
        for s in range(S):
            assert (o[pics[s]:, s] == FILL).all(), f"stream {s}: a slot past its pictures was written"
        out.append(([o[: pics[s], s].copy() for s in range(S)], pics, st))
    if own:
        dec.close()
    if feeder:
        feeder.free()
    if buf:
        buf.free()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for c, ((pa, na, sa), (pb, nb, sb)) in enumerate(zip(a, b)):
        assert na == nb and sa == sb, f"call {c}: pictures {na} / {nb}, status {sa} / {sb}"
        for s in range(len(pa)):
            assert np.array_equal(pa[s], pb[s]), f"call {c} stream {s}"


def _calls(aus, schedule):
    pos = [0] * len(aus)
    calls = []
    for call in schedule:
        chunks = []
        for s, n in enumerate(call):
            chunks.append(b"".join(aus[s][pos[s]: pos[s] + n]) or None)
            pos[s] += n
        calls.append(chunks)
    return calls


SCHEDULES = {
    "one_per_call": ([[1, 1, 1]] * 4 + [[0, 1, 0]], 1),
    "gaps_and_late_starts": ([[1, 0, 0], [0, 0, 0], [1, 1, 0], [0, 1, 1], [1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 1, 1]], 1),
    "several_per_call": ([[2, 3, 1], [1, 0, 3], [1, 2, 0]], 3),
}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_live_decode_from_device_memory(pkg, name):
    aus = _golden_aus(pkg)
    schedule, P = SCHEDULES[name]
    calls = _calls(aus, schedule)
    assert sum(len(a) for a in aus) == sum(sum(c) for c in schedule)
    ref = _run(pkg, calls, 3, P)
    assert sum(sum(n) for _, n, _ in ref) == 13 and all(s == [0, 0, 0] for _, _, s in ref)
    _same(ref, _run(pkg, calls, 3, P, device_in=True))
    _same(ref, _run(pkg, calls, 3, P, device_in=True, device_out=True))
    _same(ref, _run(pkg, calls, 3, P, device_out=True))


def test_live_decode_dev_grows_the_table_and_the_store(pkg):
    """2000 access unit delimiters in front of every stream's first access unit: more units than a fresh splitter's table
    holds and, at 16 bytes of the store for every six-byte unit, more RBSP than its first store does, so fer_split_run
    repeats the job with both grown; the next call finds the buffers as they were left"""
    S, N = 2, 2000
    aus = _golden_aus(pkg)[:S]
    first = [b"\x00\x00\x00\x01\x09\xF0" * N + a[0] for a in aus]
    units, _, total = sm.layout([np.frombuffer(c, np.uint8) for c in first])
    need = sum((len(c) + 15) & ~15 for c in first)
    assert len(units) == S * (N + 3) > max(64, 4 * S), "the first table"
    assert total > need + need // 4 + 4096 - 64, "the first store"
    calls = [first, [a[1] for a in aus]]
    host = _run(pkg, calls, S)
    assert all(n == [1] * S and st == [0] * S for _, n, st in host)
    dec = pkg.LiveDecoder(S, W, H, 1)
    _same(host, _run(pkg, calls, S, device_in=True, dec=dec))
    dec.close()


def test_live_decode_dev_arguments(pkg):
    lib = pkg.load_library()
    aus = _golden_aus(pkg)
    dec = pkg.LiveDecoder(2, W, H, 1)
    feeder = _Feeder(pkg, 2, len(aus[0][0]))
    ptrs, lens = feeder.put([aus[0][0], None])
    arr = (C.c_void_p * 2)(*ptrs)
    ln = (C.c_size_t * 2)(*lens)
    pics, status = (C.c_int * 2)(), (C.c_int * 2)()
    assert lib.ferhip_decs_decode_dev(None, arr, ln, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_decode_dev(dec.h, None, ln, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_decode_dev(dec.h, arr, None, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_decode_dev(dec.h, arr, ln, None, 0, None, status) == E_ARG
    assert lib.ferhip_decs_decode_dev(dec.h, arr, ln, None, 0, pics, None) == E_ARG
    # NULL chunks and zero lengths: nothing new
    for a, n in (((None, None), (0, 0)), ((ptrs[0], None), (0, 0)), ((None, None), (lens[0], 7))):
        assert lib.ferhip_decs_decode_dev(dec.h, (C.c_void_p * 2)(*a), (C.c_size_t * 2)(*n), None, 0, pics, status) == 0
        assert list(pics) == [0, 0] and list(status) == [0, 0]
    assert lib.ferhip_decs_decode_dev(dec.h, arr, ln, None, 0, pics, status) == 0  # out = NULL: decoded, nothing copied
    assert list(pics) == [1, 0] and list(status) == [0, 0]
    t = dec.timing()
    assert t["dev_split_bytes"] == len(aus[0][0]) and t["dev_split"] > 0 and t["host_split"] == 0
    # the two calls mix on one decoder: the P picture arrives through host memory
    out, pics, status = dec.decode([aus[0][1], None])
    assert pics == [1, 0] and status == [0, 0]
    ref = _run(pkg, [[aus[0][0]], [aus[0][1]]], 1)
    assert np.array_equal(out[0, 0], ref[1][0][0][0])
    dec.close()
    feeder.free()


def _damage_pair(pkg, victim_calls, neighbour):
    """the victim's calls beside a clean neighbour stream, through host memory and through device memory"""
    n = max(len(victim_calls), len(neighbour))
    calls = [[victim_calls[c] if c < len(victim_calls) else None, neighbour[c] if c < len(neighbour) else None] for c in range(n)]
    host = _run(pkg, calls, 2)
    dev = _run(pkg, calls, 2, device_in=True, device_out=True)
    _same(host, dev)
    return host


def _neighbour_ref(pkg):
    if "nbref" not in _cache:
        nb = _golden_aus(pkg)[1]
        r = _run(pkg, [[a] for a in nb], 1)
        assert all(n == [1] and s == [0] for _, n, s in r)
        _cache["nbref"] = [p[0][0] for p, _, _ in r]
    return _cache["nbref"]


@pytest.mark.parametrize("case", ["syntax", "i_pcm", "other_size_sps", "slice_before_sps"])
def test_fault_cases_agree_with_the_host_path(pkg, case):
    from test_gpu_live_decode import _fault_cases
    victim = _fault_cases(pkg)[case]
    nb, nbref = _golden_aus(pkg)[1], _neighbour_ref(pkg)
    res = _damage_pair(pkg, [v[0] for v in victim], nb)
    assert [st[0] for _, _, st in res[: len(victim)]] == [v[1] for v in victim]
    got = [p[1][0] for p, n, st in res if n[1]]
    assert all(st[1] == 0 for _, _, st in res) and len(got) == len(nbref)
    assert all(np.array_equal(a, b) for a, b in zip(got, nbref)), "the undamaged neighbour"


def test_damage_fuzz_agrees_with_the_host_path(pkg):
    clean = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    nb, nbref = _golden_aus(pkg)[1], _neighbour_ref(pkg)
    rng = np.random.default_rng(17)
    dec_h, dec_d = pkg.LiveDecoder(2, W, H, 1), pkg.LiveDecoder(2, W, H, 1)
    faulted = decoded = 0
    for trial in range(24):
        bad = bytearray(clean)
        lo = 64 + int(rng.integers(0, len(bad) - 200))
        for k in range(int(rng.integers(1, 6))):
            bad[min(lo + int(rng.integers(0, 64)), len(bad) - 1)] = int(rng.integers(0, 256))
        if trial % 3 == 0:  # mint the patterns themselves: a start code, a terminator or 00 00 03 in the middle of slice data
            pat = (b"\x00\x00\x00\x01", b"\x00\x00\x01", b"\x00\x00\x03")[trial // 3 % 3]
            bad[lo: lo + len(pat)] = pat
        aus = pkg.access_units(bytes(bad))
        n = max(len(aus), len(nb))
        calls = [[aus[c] if c < len(aus) else None, nb[c] if c < len(nb) else None] for c in range(n)]
        for d in (dec_h, dec_d):
            d.reset_stream(0)
            d.reset_stream(1)
        host = _run(pkg, calls, 2, dec=dec_h)
        dev = _run(pkg, calls, 2, device_in=True, dec=dec_d)
        _same(host, dev)
        got = [p[1][0] for p, n_, st in host if n_[1]]
        assert all(st[1] == 0 for _, _, st in host) and len(got) == len(nbref), f"trial {trial}"
        assert all(np.array_equal(a, b) for a, b in zip(got, nbref)), f"trial {trial}: the undamaged neighbour"
        any_fault = any(st[0] != 0 for _, _, st in host)
        faulted += any_fault
        decoded += not any_fault
    dec_h.close()
    dec_d.close()
    assert faulted >= 1 and decoded >= 1, (faulted, decoded)


def test_slice_header_longer_than_the_prefix(pkg):
    """a P slice whose ref_pic_list_modification alone is longer than the prefix that comes back with the table: the unit
    is fetched whole and decodes as on the host path"""
    import pslice_synth as ps
    prefix = pkg.SPLIT_PREFIX
    entries = 8 * prefix // 30 + 3  # an entry is ue(0) + ue(16383): 1 + 29 bits
    assert entries < 64  # the parser's own limit on the list
    aus = _golden_aus(pkg)[0]
    rng = np.random.default_rng(4)
    w, _, _ = ps.p_slice(rng, 99, 1, 2, False, 0, [(0, 16383)] * entries)
    assert len(w.b) > 8 * prefix
    ps.mb_layer(w, rng, 99, False, False, 3, 0.25, 0.3)
    long_p = nal_model.frame_nal(1, np.frombuffer(w.rbsp(2), np.uint8), nal_ref_idc=2)
    w2, _, _ = ps.p_slice(rng, 99, 2, 4, False, 0, None)
    ps.mb_layer(w2, rng, 99, False, False, 3, 0.25, 0.3)
    short_p = nal_model.frame_nal(1, np.frombuffer(w2.rbsp(2), np.uint8), nal_ref_idc=2)
    calls = [[aus[0], aus[0]], [long_p, aus[1]], [short_p, long_p]]
    host = _run(pkg, calls, 2)
    assert [n for _, n, _ in host] == [[1, 1]] * 3 and all(st == [0, 0] for _, _, st in host)
    _same(host, _run(pkg, calls, 2, device_in=True))
    _same(host, _run(pkg, calls, 2, device_in=True, device_out=True))
    # ... and cut short inside the list: the header runs past its NAL unit on both paths
    cut = [[aus[0], None], [long_p[: 5 + prefix + 8], None], [aus[0], None]]
    host = _run(pkg, cut, 2)
    assert [st[0] for _, _, st in host] == [0, E_ARG, 0]
    _same(host, _run(pkg, cut, 2, device_in=True))


def test_loopback_without_the_bus(pkg):
    """encode -> ferhip_pack_nal -> ferhip_decs_decode_dev, all in device memory: equals the host-path decode of the fetched
    bytes in full, and the encoder's own reconstruction in luma (chroma: the decoder follows the reference in keeping
    ChromaACLevel of the previous macroblock)"""
    S, T = 3, 4
    feeds = np.stack([np.stack([pkg.gen_frame(W, H, t, 500 + 7 * s, 2) for t in range(T)]) for s in range(S)])
    g = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    cap = S * (((g.nmb * 1024 + 4096 + 15) & ~15) + 64)
    dst, index = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * (S + 1))
    dec_d, dec_h = pkg.LiveDecoder(S, W, H, 1), pkg.LiveDecoder(S, W, H, 1)
    out_d = pkg.DeviceBuffer(S * FSZ)
    decoded = 0
    for t in range(T):
        present = [not (t == 2 and s == 1) for s in range(S)]
        g.encode_live([feeds[s, t] if present[s] else None for s in range(S)], [5 if t == 0 else 1] * S)
        g.pack_nal_device(dst.ptr, index.ptr, cap, pkg.AU_PARAM_SETS)
        g.sync()
        idx = index.download(dtype=pkg.AU)  # the 16 (S + 1) index bytes are all that crosses the bus
        assert int(idx[S]["offset"]) <= cap and int(idx[S]["bytes"]) == sum(present)
        ptrs = [dst.ptr + int(idx[s]["offset"]) if idx[s]["bytes"] else None for s in range(S)]
        out_d.upload(np.full(S * FSZ, FILL, np.uint8))
        _, pics, status = dec_d.decode_dev(ptrs, [int(b) for b in idx["bytes"][:S]], out_d)
        assert pics == [int(p) for p in present] and status == [0] * S, f"picture {t}"
        got = out_d.download().reshape(1, S, FSZ)
        units, _ = g.fetch_nal(pkg.AU_PARAM_SETS)
        want, hp, hs = dec_h.decode([u or None for u in units])
        assert hp == pics and hs == status
        recon = np.asarray(g.get_recon()).reshape(S, FSZ)
        for s in range(S):
            if not present[s]:
                assert (got[0, s] == FILL).all()
                continue
            assert np.array_equal(got[0, s], want[0, s]), f"picture {t} stream {s}: host-path decode"
            assert np.array_equal(got[0, s, : W * H], recon[s, : W * H]), f"picture {t} stream {s}: the encoder's reconstruction"
            decoded += 1
    assert decoded == 11 and g.status() == [0] * S
    for x in (dec_d, dec_h, g):
        x.close()
    for b in (dst, index, out_d):
        b.free()
