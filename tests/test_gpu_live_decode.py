"""The live decoder (ferhip_decs_*, LiveDecoder): S streams fed access unit by access unit, in any pattern of gaps,
late starts and chunk sizes, decode exactly like the oracle decoder; a stream's faults stay in that stream."""
import ctypes as C
import hashlib
from pathlib import Path

import numpy as np
import pytest
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
QCIF = ["qcif_i_2f_qp12", "qcif_ippp_4f_qp12_w16", "qcif_ippp_4f_qp28_w32", "qcif_skip_5f_qp12"]
W, H = 176, 144
FSZ = W * H * 3 // 2
SENTINEL = 0xA5
E_ARG, E_STATE, E_UNSUP, E_DEVICE = -1, -3, -4, -5

# the plans of test_gpu_full.py::test_decoder_sub_partitions_ref_idx_and_list_modification
F4_PLANS = {
    "sub_partitions": [dict(), dict(), dict()],
    "ref_idx": [dict(override=True, active=1), dict(), dict(override=True, active=0), dict(), dict(override=True, active=3)],
    "list_modification": [dict(modification=[]), dict(), dict(modification=[(0, 0)]), dict(modification=[]),
                          dict(modification=[]), dict(modification=[(1, 2), (2, 0)]), dict()],
    "mixed": [dict(override=True, active=1, modification=[]), dict(early_end=True), dict(modification=[], early_end=True),
              dict(override=True, active=0), dict(modification=[(0, 1)], mvd_range=12), dict(mvd_range=40, p_skip=0.05)],
}


def _oracle(fo, stream):
    n, frames, _ = fo.decode_stream_md5(stream)
    return np.stack(frames)


@pytest.fixture(scope="module")
def streams(pkg, fo):
    """-> list of (Annex-B stream, oracle pictures): the four QCIF goldens and the four f4 plans"""
    import pslice_synth as ps
    base = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    out = [(GOLD / f"{c}.264").read_bytes() for c in QCIF]
    out += [ps.make_stream(pkg.split_nals, base, 7, F4_PLANS[p]) for p in sorted(F4_PLANS)]
    return [(s, _oracle(fo, s)) for s in out]


def _run(pkg, aus, schedule, P=1, sentinel_check=False, device_out=False):
    """aus[s] = access units of stream s; schedule = list of calls, each a list of the number of access units each stream
    gives in that call.  -> (pictures of every stream in order, per-call status lists)"""
    S = len(aus)
    dec = pkg.LiveDecoder(S, W, H, P)
    got = [[] for _ in range(S)]
    pos = [0] * S
    statuses = []
    if device_out:
        buf = pkg.DeviceBuffer(P * S * FSZ)
    for call in schedule:
        chunks = []
        for s in range(S):
            n = call[s]
            chunks.append(b"".join(aus[s][pos[s]:pos[s] + n]) if n and pos[s] < len(aus[s]) else None)
            pos[s] += n
        if device_out:
            buf.upload(np.full(P * S * FSZ, SENTINEL, np.uint8))
            _, pics, st = dec.decode(chunks, buf)
            o = buf.download().reshape(P, S, FSZ)
        else:
            o = np.full((P, S, FSZ), SENTINEL, np.uint8)
            _, pics, st = dec.decode(chunks, o)
        statuses.append(st)
        for s in range(S):
            for k in range(pics[s]):
                got[s].append(o[k, s].copy())
            if sentinel_check:
                assert (o[pics[s]:, s] == SENTINEL).all(), f"stream {s}: a slot past its pictures was written"
    dec.close()
    if device_out:
        buf.free()
    return [np.stack(g) if g else np.zeros((0, FSZ), np.uint8) for g in got], statuses


def _one_per_call(aus, start=None):
    start = start or [0] * len(aus)
    ncall = max(st + len(a) for st, a in zip(start, aus))
    return [[1 if start[s] <= c < start[s] + len(aus[s]) else 0 for s in range(len(aus))] for c in range(ncall)]


def test_live_one_picture_per_call(pkg, streams):
    aus = [pkg.access_units(s) for s, _ in streams]
    got, st = _run(pkg, aus, _one_per_call(aus))
    for s, (_, ref) in enumerate(streams):
        assert np.array_equal(got[s], ref), f"stream {s}"
    assert all(x == 0 for c in st for x in c)


def test_live_gaps_and_late_starts(pkg, streams):
    aus = [pkg.access_units(s) for s, _ in streams]
    rng = np.random.default_rng(11)
    pos, schedule, c = [0] * len(aus), [], 0
    while any(p < len(a) for p, a in zip(pos, aus)):
        call = [1 if c >= 3 * s and pos[s] < len(aus[s]) and rng.random() < 0.6 else 0 for s in range(len(aus))]
        for s in range(len(aus)):
            pos[s] += call[s]
        schedule.append(call)
        c += 1
    got, st = _run(pkg, aus, schedule, sentinel_check=True)
    for s, (_, ref) in enumerate(streams):
        assert np.array_equal(got[s], ref), f"stream {s}"


def test_live_several_pictures_per_call(pkg, streams):
    aus = [pkg.access_units(s) for s, _ in streams]
    rng = np.random.default_rng(12)
    pos, schedule = [0] * len(aus), []
    while any(p < len(a) for p, a in zip(pos, aus)):
        call = [int(rng.integers(1, 4)) if pos[s] < len(aus[s]) else 0 for s in range(len(aus))]
        for s in range(len(aus)):
            pos[s] += call[s]
        schedule.append(call)
    got, st = _run(pkg, aus, schedule, P=3, sentinel_check=True)
    for s, (_, ref) in enumerate(streams):
        assert np.array_equal(got[s], ref), f"stream {s}"


def test_live_reproduces_reference_md5_on_staggered_drugi(pkg):
    stream = golden_bytes("drugi.264")
    aus = pkg.access_units(stream)
    assert len(aus) == 1000
    start = [0, 5, 11, 17]
    dec = pkg.LiveDecoder(4, 640, 480, 1)
    hs = [hashlib.md5(b"YUV4MPEG2 C420jpeg W640 H480 F24:1 Ip A1:1\n") for _ in start]
    n = [0] * 4
    out = np.empty((1, 4, 640 * 480 * 3 // 2), np.uint8)
    for c in range(1000 + start[-1]):
        chunks = [aus[c - st] if 0 <= c - st < 1000 else None for st in start]
        _, pics, status = dec.decode(chunks, out)
        assert status == [0] * 4
        for s in range(4):
            assert pics[s] == (1 if chunks[s] else 0)
            if pics[s]:
                hs[s].update(b"FRAME\n")
                hs[s].update(out[0, s].tobytes())
                n[s] += 1
    dec.close()
    assert n == [1000] * 4
    for s in range(4):
        assert hs[s].hexdigest() == "346891974ac8cafcc6bb72706e34f950", f"copy {s}"


def test_live_device_output_matches_host_output(pkg, streams):
    """Device output (out_on_device = 1) into memory of the library's runtime gives the bytes of host output, and slots
    that were not written keep what the buffer held."""
    aus = [pkg.access_units(s) for s, _ in streams]
    rng = np.random.default_rng(13)
    pos, schedule = [0] * len(aus), []
    while any(p < len(a) for p, a in zip(pos, aus)):
        call = [int(rng.integers(0, 3)) if pos[s] < len(aus[s]) else 0 for s in range(len(aus))]
        for s in range(len(aus)):
            pos[s] += call[s]
        schedule.append(call)
    host, st_h = _run(pkg, aus, schedule, P=2, sentinel_check=True)
    dev, st_d = _run(pkg, aus, schedule, P=2, sentinel_check=True, device_out=True)
    assert st_h == st_d
    for s, (_, ref) in enumerate(streams):
        assert np.array_equal(host[s], ref) and np.array_equal(dev[s], ref), f"stream {s}"
    # a buffer that is not 16-byte aligned (one byte into a larger allocation) takes the byte-wise path
    lib = pkg.load_library()
    dec = pkg.LiveDecoder(1, W, H, 1)
    big = pkg.DeviceBuffer(FSZ + 2)
    big.upload(np.full(FSZ + 2, SENTINEL, np.uint8))
    au = aus[1][0]
    pics, st = (C.c_int * 1)(), (C.c_int * 1)()
    assert lib.ferhip_decs_decode(dec.h, (C.c_char_p * 1)(au), (C.c_size_t * 1)(len(au)), C.c_void_p(big.ptr + 1), 1, pics, st) == 0
    dec.close()
    got = big.download()
    big.free()
    assert list(pics) == [1] and list(st) == [0] and got[0] == SENTINEL and got[-1] == SENTINEL
    assert np.array_equal(got[1:-1], streams[1][1][0])


def _p_slice_with_mb_type(pkg, mb_type):
    import pslice_synth as ps
    w, _, _ = ps.p_slice(np.random.default_rng(3), 99, 9, 18, False, 0, None)
    w.ue(0)  # mb_skip_run
    w.ue(mb_type)
    w.ue(0)
    return ps.nal_unit(1, 2, w.rbsp(4))


def _fault_cases(pkg):
    clean = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    aus = pkg.access_units(clean)
    idr_only = pkg.split_nals(aus[0])[2]
    other_sps = pkg.split_nals(golden_bytes("drugi.264")[:4096])[0]
    assert other_sps[4] & 31 == 7
    # victim calls: (chunk, expected status, expected pictures from the clean stream's oracle or None)
    good_then = [(aus[0], 0, 0), (aus[1], 0, 1)]
    after = [(aus[2], E_STATE, None), (aus[3], E_STATE, None), (idr_only, 0, 0), (aus[1], 0, 1), (aus[2], 0, 2), (aus[3], 0, 3)]
    return {
        "syntax": good_then + [(_p_slice_with_mb_type(pkg, 32), E_DEVICE, None)] + after,
        "i_pcm": good_then + [(_p_slice_with_mb_type(pkg, 30), E_UNSUP, None)] + after,
        "other_size_sps": good_then + [(other_sps + aus[2], E_UNSUP, None)] + after,
        "slice_before_sps": [(aus[1], E_STATE, None), (aus[2], E_STATE, None), (aus[0], 0, 0), (aus[1], 0, 1), (aus[2], 0, 2)],
    }


@pytest.mark.parametrize("case", ["syntax", "i_pcm", "other_size_sps", "slice_before_sps"])
def test_live_error_isolation(pkg, fo, streams, case):
    victim = _fault_cases(pkg)[case]
    ref = _oracle(fo, (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes())
    others = [streams[k] for k in (3, 4, 5)]  # qcif_skip_5f, f4 "list_modification", "mixed": beside the victim
    oaus = [pkg.access_units(s) for s, _ in others]
    S = 1 + len(others)
    dec = pkg.LiveDecoder(S, W, H, 1)
    got = [[] for _ in others]
    out = np.full((1, S, FSZ), SENTINEL, np.uint8)
    for c, (chunk, want_status, want_pic) in enumerate(victim):
        chunks = [chunk] + [a[c] if c < len(a) else None for a in oaus]
        out[:] = SENTINEL
        _, pics, status = dec.decode(chunks, out)
        assert status[0] == want_status, f"call {c}"
        assert status[1:] == [0] * len(others)
        if want_pic is None:
            assert pics[0] == 0 and (out[0, 0] == SENTINEL).all(), f"call {c}"
        else:
            assert pics[0] == 1 and np.array_equal(out[0, 0], ref[want_pic]), f"call {c}"
        for k in range(len(others)):
            if pics[k + 1]:
                got[k].append(out[0, k + 1].copy())
    dec.close()
    for k, (_, r) in enumerate(others):
        n = min(len(victim), r.shape[0])
        assert len(got[k]) == n and np.array_equal(np.stack(got[k]), r[:n]), f"neighbour {k}"


def test_live_damage_fuzz(pkg, fo, streams):
    clean = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    ref = _oracle(fo, clean)
    nb = [streams[k] for k in (2, 7)]  # qcif_ippp_4f_qp28_w32, f4 "sub_partitions"
    nb_aus = [pkg.access_units(s) for s, _ in nb]
    dec = pkg.LiveDecoder(3, W, H, 1)
    rng = np.random.default_rng(5)
    faulted = decoded = 0
    for trial in range(24):
        bad = bytearray(clean)
        lo = 64 + int(rng.integers(0, len(bad) - 200))
        for k in range(int(rng.integers(1, 6))):
            bad[min(lo + int(rng.integers(0, 64)), len(bad) - 1)] = int(rng.integers(2, 256))
        for s in range(3):
            dec.reset_stream(s)
        aus = pkg.access_units(bytes(bad))
        got = [[], []]
        any_fault = False
        for c in range(max(len(aus), *[len(a) for a in nb_aus])):
            chunks = [aus[c] if c < len(aus) else None] + [a[c] if c < len(a) else None for a in nb_aus]
            out, pics, status = dec.decode(chunks)
            assert status[1:] == [0, 0]
            any_fault |= status[0] != 0
            for k in range(2):
                if pics[k + 1]:
                    got[k].append(out[0, k + 1].copy())
        for k, (_, r) in enumerate(nb):
            assert np.array_equal(np.stack(got[k]), r), f"trial {trial}: neighbour {k}"
        faulted += any_fault
        decoded += not any_fault
    assert faulted >= 1 and decoded >= 1, (faulted, decoded)
    dec.reset_stream(0)
    got = []
    for au in pkg.access_units(clean):
        out, pics, status = dec.decode([au, None, None])
        assert status == [0, 0, 0] and pics == [1, 0, 0]
        got.append(out[0, 0].copy())
    dec.close()
    assert np.array_equal(np.stack(got), ref)


def test_live_reset_stream(pkg, streams):
    a = pkg.access_units(streams[1][0])
    b = pkg.access_units(streams[3][0])
    dec = pkg.LiveDecoder(2, W, H, 1)
    for au in a[:2]:
        dec.decode([au, au])
    dec.reset_stream(0)
    got0, got1 = [], []
    for c in range(max(len(b), len(a) - 2)):
        out, pics, status = dec.decode([b[c] if c < len(b) else None, a[2 + c] if 2 + c < len(a) else None])
        assert status == [0, 0]
        if pics[0]:
            got0.append(out[0, 0].copy())
        if pics[1]:
            got1.append(out[0, 1].copy())
    dec.close()
    assert np.array_equal(np.stack(got0), streams[3][1])
    assert np.array_equal(np.stack(got1), streams[1][1][2:])
    # after a reset the parameter sets are gone too: a slice alone is refused
    dec = pkg.LiveDecoder(1, W, H, 1)
    dec.decode([a[0]])
    dec.reset_stream(0)
    _, pics, status = dec.decode([a[1]])
    dec.close()
    assert pics == [0] and status == [E_STATE]


def test_live_arguments(pkg, streams):
    lib = pkg.load_library()
    h = C.c_void_p()
    for args in [(0, W, H, 1), (-1, W, H, 1), (1, W + 8, H, 1), (1, W, H - 4, 1), (1, W, H, 0), (1, W, H, -2)]:
        assert lib.ferhip_decs_create(C.byref(h), *args) == E_ARG, args
    assert lib.ferhip_decs_create(None, 1, W, H, 1) == E_ARG
    assert lib.ferhip_decs_create(C.byref(h), 2, W, H, 1) == 0
    au = pkg.access_units(streams[1][0])[0]
    chunks = (C.c_char_p * 2)(au, None)
    lens = (C.c_size_t * 2)(len(au), 0)
    pics, status = (C.c_int * 2)(), (C.c_int * 2)()
    assert lib.ferhip_decs_decode(h, None, lens, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_decode(h, chunks, None, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_decode(h, chunks, lens, None, 0, None, status) == E_ARG
    assert lib.ferhip_decs_decode(h, chunks, lens, None, 0, pics, None) == E_ARG
    assert lib.ferhip_decs_decode(None, chunks, lens, None, 0, pics, status) == E_ARG
    assert lib.ferhip_decs_reset_stream(h, 2) == E_ARG
    assert lib.ferhip_decs_reset_stream(h, -1) == E_ARG
    assert lib.ferhip_decs_reset_stream(None, 0) == E_ARG
    # out = NULL: decoded, nothing copied
    assert lib.ferhip_decs_decode(h, chunks, lens, None, 0, pics, status) == 0
    assert list(pics) == [1, 0] and list(status) == [0, 0]
    # more slices than max_pictures: the stream's first picture is decoded, the second refused
    two = pkg.access_units(streams[1][0])[1] + pkg.access_units(streams[1][0])[2]
    chunks = (C.c_char_p * 2)(two, None)
    lens = (C.c_size_t * 2)(len(two), 0)
    assert lib.ferhip_decs_decode(h, chunks, lens, None, 0, pics, status) == 0
    assert list(pics) == [1, 0] and list(status) == [E_ARG, 0]
    lib.ferhip_decs_destroy(h)
