"""tests/mp4_model.py pinned on the host: the segment builder and the box walk against their byte-serial restatements, a
fragment and an initialisation segment written by hand, box sizes, mux -> demux on the committed streams, every truncation,
dressed input, the fault catalogue's stated outcomes, and the cursor phases of the GPU test's payloads.  No GPU."""
import numpy as np

import avcc_model
import mp4_model as mm
import nal_model
import ts_model as tm
from conftest import golden_bytes

GOLDENS = ["qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264"]
HDR = dict(decode_time=(1 << 32) + 90000, sequence=0x01020304, duration=3000)


def _samples_of(name):
    """the access units of a committed stream as MP4 samples (parameter sets inside the IDR sample), and their types"""
    aus = tm.access_units_of(golden_bytes(name))
    return [avcc_model.annexb_to_avcc(e) for e, _ in aus], [t for _, t in aus]


def test_segment_equals_its_serial_form_and_its_boxes_add_up():
    rng = np.random.default_rng(11)
    for K in (1, 2, 3, 6, 17, 4096):
        for n in sorted({1, min(K, 2), min(K, 5), K if K < 100 else 40}):
            samples = [rng.integers(0, 256, int(rng.integers(0, 300))).astype(np.uint8).tobytes() for _ in range(n)]
            idr = [k % 3 == 0 for k in range(n)]
            seg = mm.segment(samples, idr, HDR, K)
            assert seg == mm.segment_serial(samples, idr, HDR, K), (K, n)
            D = mm.data_offset(K)
            assert D % 16 == 0 and D >= 104 + 12 * K and seg[D - 4: D] == b"mdat" and len(seg) == D + sum(map(len, samples))
            assert mm.check_sizes(seg) == 8
            assert int.from_bytes(seg[84:88], "big") == D, "data_offset"
            got, fault = mm.walk(seg)
            assert fault == 0 and [seg[a: a + m] for a, m in got] == samples and got[0][0] == D
    assert [mm.data_offset(K) for K in (1, 2, 3, 6)] == [128, 128, 144, 176] and {(104 + 12 * K) % 16 for K in (1, 2, 3, 6)} == {0, 4, 12}


def test_fragment_written_by_hand():
    s0, s1 = bytes.fromhex("00000003 65 88 84".replace(" ", "")), bytes.fromhex("00000002 41 9a".replace(" ", ""))
    want = bytes.fromhex("""
        00000070 6d6f6f66
          00000010 6d666864 00000000 00000007
          00000058 74726166
            00000010 74666864 00020000 00000001
            00000014 74666474 01000000 00000001 00000010
            0000002c 7472756e 00000701 00000002 00000080
              00000bb8 00000007 02000000
              00000bb8 00000006 01010000
        00000008 66726565
        00000015 6d646174
        00000003 65 88 84  00000002 41 9a
    """.replace(" ", "").replace("\n", ""))
    assert mm.segment([s0, s1], [True, False], dict(decode_time=(1 << 32) + 16, sequence=7, duration=3000), 2) == want
    assert mm.demux(want) == ([s0, s1], 0) and mm.units(want) == [(5, 3, b"\x88\x84"), (1, 2, b"\x9a")]
    # K = 1: 24 bytes of free box
    one = mm.segment([s0], [True], dict(decode_time=0, sequence=1, duration=1), 1)
    assert one[100:108] == bytes.fromhex("0000001466726565") and one[108:120] == bytes(12) and one[120:128] == bytes.fromhex("0000000f6d646174")


def test_initialisation_segment_written_by_hand():
    sps, pps = bytes.fromhex("6742001eab40"), bytes.fromhex("68ce3880")
    want = bytes.fromhex("""
        0000001c 66747970 69736f36 00000000 69736f36 636d6663 61766331
        00000258 6d6f6f76
          0000006c 6d766864 00000000 00000000 00000000 00015f90 00000000 00010000 0100 0000 00000000 00000000
            00010000 00000000 00000000 00000000 00010000 00000000 00000000 00000000 40000000
            00000000 00000000 00000000 00000000 00000000 00000000 00000002
          000001bc 7472616b
            0000005c 746b6864 00000003 00000000 00000000 00000001 00000000 00000000 00000000 00000000 0000 0000 0000 0000
              00010000 00000000 00000000 00000000 00010000 00000000 00000000 00000000 40000000 00b00000 00900000
            00000158 6d646961
              00000020 6d646864 00000000 00000000 00000000 00015f90 00000000 55c4 0000
              00000021 68646c72 00000000 00000000 76696465 00000000 00000000 00000000 00
              0000010f 6d696e66
                00000014 766d6864 00000001 0000 0000 0000 0000
                00000024 64696e66 0000001c 64726566 00000000 00000001 0000000c 75726c20 00000001
                000000cf 7374626c
                  00000083 73747364 00000000 00000001
                    00000073 61766331 000000000000 0001 0000 0000 00000000 00000000 00000000 00b0 0090 00480000 00480000 00000000 0001
                      0000000000000000000000000000000000000000000000000000000000000000 0018 ffff
                      0000001d 61766343 01 42001e ff e1 0006 6742001eab40 01 0004 68ce3880
                  00000010 73747473 00000000 00000000
                  00000010 73747363 00000000 00000000
                  00000014 7374737a 00000000 00000000 00000000
                  00000010 7374636f 00000000 00000000
          00000028 6d766578 00000020 74726578 00000000 00000001 00000001 00000000 00000000 00000000
    """.replace(" ", "").replace("\n", ""))
    ini = mm.init_segment(sps, pps, 176, 144, 90000)
    assert ini == want
    assert mm.check_sizes(ini) == 20  # (dref, stsd and avc1 hold counts or fields in front of their children)
    off, n = mm.find_avcc(ini)
    assert ini[off: off + n] == avcc_model.config_record(sps, pps)
    for k in range(len(ini)):
        assert mm.find_avcc(ini[:k]) is None
    assert mm.find_avcc(ini.replace(b"avc1", b"avc3")) == (off, n) and mm.find_avcc(ini.replace(b"avc1", b"hvc1")) is None
    assert mm.find_avcc(ini.replace(b"avcC", b"avcD")) is None and mm.find_avcc(b"") is None


def test_mux_then_demux_returns_the_samples_of_the_golden_streams():
    for name in GOLDENS:
        samples, types = _samples_of(name)
        assert len(samples) >= 2 and types[0] == 5
        sps, pps = avcc_model.parameter_sets_of(golden_bytes(name))
        assert samples[0].startswith(mm.u32(len(sps)) + sps + mm.u32(len(pps)) + pps)
        for m in (1, 2, len(samples)):
            run, h = b"", dict(HDR)
            for g in range(0, len(samples), m):
                part = samples[g: g + m]
                seg = mm.segment(part, [t == 5 for t in types[g: g + m]], h, m)
                assert seg == mm.segment_serial(part, [t == 5 for t in types[g: g + m]], h, m) and mm.check_sizes(seg) == 8
                run += seg
                h = dict(h, decode_time=h["decode_time"] + len(part) * h["duration"], sequence=h["sequence"] + 1)
            assert mm.demux(run) == (samples, 0) and mm.walk(run) == mm.walk_serial(run), name
            import nal_split_model as sm
            assert mm.units(run) == sm.split(golden_bytes(name)), "the units of the stream, nothing added"
        ini = mm.init_segment(sps, pps, 176, 144, 90000)
        off, n = mm.find_avcc(ini)
        assert ini[off: off + n] == avcc_model.config_record(sps, pps)
        assert mm.demux(ini + run) == (samples, 0)


def test_every_truncation_of_a_two_fragment_run():
    samples, types = _samples_of(GOLDENS[0])
    f0 = mm.segment(samples[:2], [True, False], HDR, 2)
    f1 = mm.segment(samples[2:], [False] * len(samples[2:]), dict(HDR, sequence=2), 6)
    run = f0 + f1
    for k in range(len(run) + 1):
        got, fault = mm.demux(run[:k])
        assert mm.walk(run[:k]) == mm.walk_serial(run[:k]), k
        whole = k in (0, len(f0), len(run))
        assert (fault == 0) == whole and fault in (0, 2, 4), k
        assert got == (samples if k == len(run) else samples[:2] if k >= len(f0) else []), k


def test_dressed_input_gives_the_same_samples():
    samples, _ = _samples_of(GOLDENS[1])
    variants = mm.dress([samples[:2], samples[2:]])
    names = " | ".join(n for n, _, _ in variants)
    for word in ("styp", "sidx", "free", "emsg", "unknown", "64-bit", "size 0", "two truns", "without a data_offset", "default size", "version 1",
                 "first_sample_flags", "extra children", "audio-like"):
        assert word in names, word
    for name, run, stand in variants:
        assert mm.walk(run) == mm.walk_serial(run), name
        assert mm.demux(run) == (stand, 0), name
        mm.check_sizes(run[: run.rindex(b"mdat") - 4]) if "size 0" in name else None
    assert mm.demux_runs([r for _, r, _ in variants[:3]]) == (samples * 3, 0)


def test_the_fault_catalogue():
    cases = mm.catalogue()
    assert {f for _, _, _, f in cases} == {0, 1, 2, 3, 4}
    names = " | ".join(n for n, _, _, _ in cases)
    for word in ("below 8", "beyond the run", "beyond its parent", "beyond the trun", "beyond the mdat", "without an mdat", "base-data-offset",
                 "second traf", "no sizes", "overrun inside a sample"):
        assert word in names, word
    for name, run, stand, fault in cases:
        assert mm.demux(run) == (stand, fault), name
        assert mm.walk(run) == mm.walk_serial(run), name
    for L in (1, 2):
        for name, run, stand, fault in mm.catalogue(L):
            assert mm.demux(run, L) == (stand, fault), (L, name)
    # the first fault ends the stream's walk: the runs behind it are not taken
    good = cases[0][1]
    bad = next(run for name, run, _, _ in cases if "base-data-offset" in name)
    assert mm.demux_runs([good, bad, good]) == (cases[0][2] + cases[0][2][:2], 3)


def test_drawn_bytes_walk_alike():
    rng = np.random.default_rng(5)
    kinds = [b"moof", b"traf", b"trun", b"tfhd", b"mdat", b"free"]
    for _ in range(3000):
        n = int(rng.integers(0, 300))
        r = bytearray(rng.integers(0, 4, n).astype(np.uint8).tobytes() if rng.integers(2) else rng.integers(0, 256, n).astype(np.uint8).tobytes())
        o = 0
        while o + 8 <= n and rng.integers(8):
            size = 8 + int(rng.integers(n - o)) if rng.integers(6) else int(rng.integers(3))
            r[o: o + 4] = size.to_bytes(4, "big")
            r[o + 4: o + 8] = kinds[int(rng.integers(len(kinds)))]
            o += 8 + int(rng.integers(24))
        assert mm.walk(bytes(r)) == mm.walk_serial(bytes(r))


def test_cursor_phases_of_the_gpu_payloads_cover_all_residues():
    sizes = [len(mm.sample_of(nal_model.frame_nal(5 if k % 3 == 0 else 1, p))) for k, p in enumerate(mm.kat_payloads())]
    phases = set()
    for K, m in mm.KAT_CONFIGS:
        phases |= mm.cursor_phases(sizes, m)
    assert phases == set(range(16))
    assert {(1, 1), (6, 6), (3, 2)} <= set(mm.KAT_CONFIGS)
