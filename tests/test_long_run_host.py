"""tests/long_run.py pinned without a GPU: its slice header model against the oracle's streams and the reference's own bit
writer, the one place where oracle and product leave the reference on purpose (the frame_num wrap), the coverage the long
encoder inputs were built for, the synthesized decode streams against their plan, and the reference decoder's record."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import long_run as lr
import slice_synth as ss

HERE = Path(__file__).resolve().parent
GOLD = HERE / "golden"
IDR, SLICE, NONE = lr.IDR, lr.SLICE, lr.NONE


def _leaf():
    p = HERE.parent / "oracle" / "_ref" / "libfer_leaf.so"
    if not p.exists():
        pytest.skip("oracle/_ref/libfer_leaf.so not built (reference tree absent)")
    return C.CDLL(str(p))


def _leaf_header(ref, nal_type, frame_num, idr_pic_id, poc_lsb):
    """the fields of header_bits() through the reference's own writer (expGolomb_UC, writeRawBits of F/rbsp_IO.cpp and
    F/expgolomb.cpp), in the order shd_write puts them (F/headers_and_parameter_sets.cpp:172-239) -> the bytes it wrote,
    zero padded"""
    fn = {n: getattr(ref, m) for n, m in dict(init="_Z23init_expgolomb_UC_codesv", writer="_Z13initRawWriterPhj", ue="_Z12expGolomb_UCj",
                                              put="_Z12writeRawBitsij", flush="_Z16flushWriteBufferv").items()}
    fn["init"]()
    buf = (C.c_ubyte * 64)()
    fn["writer"](buf, C.c_uint(64))
    idr = nal_type == IDR
    fn["ue"](C.c_uint(0))
    fn["ue"](C.c_uint(2 if idr else 0))
    fn["ue"](C.c_uint(0))
    fn["put"](C.c_int(9), C.c_uint(frame_num))
    if idr:
        fn["ue"](C.c_uint(idr_pic_id))
    fn["put"](C.c_int(10), C.c_uint(poc_lsb))
    for _ in range(2 if idr else 3):
        fn["put"](C.c_int(1), C.c_uint(0))
    fn["flush"]()
    return bytes(buf)


def _pack(bits):
    return np.packbits(np.array([int(b) for b in bits], np.uint8)).tobytes()


# ---- 1. the header model


def _check_headers(pictures, types, what):
    """pictures: [(nal type, rbsp)] the oracle coded; types: the nal types asked of the stream, NONE included"""
    m, k = lr.HeaderModel(), 0
    for n, t in enumerate(types):
        h = m.next(t)
        if h is None:
            continue
        nt, rbsp = pictures[k]
        k += 1
        assert nt == t, f"{what} call {n}: type"
        want = h + lr.SLICE_QP_DELTA_M14
        assert lr.bits_of(rbsp, len(want)) == want, f"{what} call {n}: header at (frame_num, idr_pic_id, poc_lsb) = {m.fields()}"
    assert k == len(pictures)


def test_header_model_equals_the_oracles_headers(fo):
    for s, (stream, _, _) in enumerate(lr.p_run_oracle()):
        nals = [(t, r) for t, r in lr.split_annexb(stream) if t in (IDR, SLICE)]
        assert len(nals) == lr.P_RUN["T"]
        _check_headers(nals, [t for t, _ in nals], f"P run stream {s}")
    for s in range(3):
        _check_headers([(t, r) for t, r, _ in lr.schedule_oracle(s)["pictures"]], [row[s] for row in lr.SCHEDULE], f"schedule stream {s}")


def test_header_model_equals_the_reference_writer_in_range():
    """every header the schedules ask for whose counters are in range, through the reference's own bit writer"""
    ref = _leaf()
    seen = set()
    for s in range(3):
        m = lr.HeaderModel()
        for row in lr.SCHEDULE:
            h = m.next(row[s])
            fn, idr, poc = m.fields()
            if h is None or fn >= 512 or poc >= 1024 or (row[s], fn, idr, poc) in seen:
                continue
            seen.add((row[s], fn, idr, poc))
            assert h == lr.header_bits(row[s], fn, idr, poc, wrap=False)
            got = _leaf_header(ref, row[s], fn, idr, poc)
            assert lr.bits_of(got, len(h)) == h, (row[s], fn, idr, poc)
            assert not any(got[(len(h) + 7) // 8:])
    assert {(SLICE, 511, 0, 1022)} <= seen and {(IDR, 0, i, 0) for i in range(40)} <= seen


# ---- 2. the divergence


def test_reference_writer_corrupts_the_header_past_the_wrap():
    """Where oracle and product knowingly leave the reference.  The reference's writeRawBits adds the value into its bit
    buffer without masking it to the field's width (F/rbsp_IO.cpp:123-127).  Its encoder keeps frame_num and
    pic_order_cnt_lsb as growing ints, so from the 513th picture of a P run on (frame_num 512 in a 9-bit field, poc_lsb 1024
    in a 10-bit field) the carry runs through the fields in front: the three leading ue(0) codes are wiped and the header
    starts with a first_mb_in_slice that is not 0 -- no decoder parses that picture.  The oracle's fo_bw_put and the
    product's build_header mask the value: frame_num and pic_order_cnt_lsb wrap modulo 512 / 1024 as H.264 7.4.3 defines
    them.  That conformant wrap is written on purpose; up to (511, 1022) all three agree."""
    ref = _leaf()
    h = lr.header_bits(SLICE, 511, 0, 1022)
    assert lr.bits_of(_leaf_header(ref, SLICE, 511, 0, 1022), len(h)) == h
    assert h.startswith("111" + "1" * 9)
    want = lr.header_bits(SLICE, 512, 0, 1024)
    assert want == "111" + "0" * 9 + "0" * 10 + "000"  # the wrap: both fields read 0 again
    got = _leaf_header(ref, SLICE, 512, 0, 1024)
    assert got[:len(_pack(want))] != _pack(want)
    bits = lr.bits_of(got, 64)
    assert bits.startswith("000000000001000000000000")  # 11 zeros: first_mb_in_slice is a 23-bit code, 2047 + its suffix
    z = bits.index("1")
    first_mb_in_slice = (1 << z) - 1 + int(bits[z + 1:2 * z + 1], 2)
    assert first_mb_in_slice >= 2047
    # the model's header parses back to the wrapped fields
    assert lr.parse_header(_pack(want + lr.SLICE_QP_DELTA_M14) + b"\x80", SLICE) == (0, 0, 0, None, 0)


# ---- 3. coverage of the encoder inputs, on the oracle alone


def _runs(types):
    """lengths of the runs of P pictures"""
    out, n = [], 0
    for t in types:
        if t == SLICE:
            n += 1
        elif t == IDR:
            out.append(n)
            n = 0
    return out + [n]


def test_encoder_inputs_cross_the_boundaries(fo):
    for s, (stream, _, _) in enumerate(lr.p_run_oracle()):
        types = [t for t, _ in lr.split_annexb(stream) if t in (IDR, SLICE)]
        assert types == [IDR] + [SLICE] * (lr.P_RUN["T"] - 1), f"P run stream {s}: a scene cut"
        assert max(_runs(types)) >= 513
    lagging = 0
    for s in range(3):
        types = [row[s] for row in lr.SCHEDULE]
        m, ids, wraps_fn, wraps_poc, idr_behind_512 = lr.HeaderModel(), set(), 0, 0, 0
        for t in types:
            before = m.frame_num
            if m.next(t) is None:
                continue
            if t == IDR:
                ids.add(m.idr_pic_id)
                idr_behind_512 += before == 512
            else:
                wraps_fn += m.frame_num > 0 and m.frame_num & 511 == 0
                wraps_poc += m.poc_lsb > 0 and m.poc_lsb & 1023 == 0
        assert wraps_fn >= 1 and wraps_poc >= 1, f"schedule stream {s}"
        assert max(_runs(types)) >= (512 if s < 2 else 513), f"schedule stream {s}"  # (the IDR directly behind frame_num 512 ends it)
        if s < 2:
            assert idr_behind_512 == 1 and ids == {0, 1, 2}, f"schedule stream {s}"
        else:
            assert {0, 1, 3, 7, 15, 31} <= ids and ids == set(range(40))
        lagging += NONE in types
    assert lagging == 1 and [row[1] for row in lr.SCHEDULE].count(NONE) == lr.SCHED_CALLS // 7
    # stream 1's wrap falls on another call than stream 0's
    call_of_wrap = []
    for s in (0, 1):
        m = lr.HeaderModel()
        for n, row in enumerate(lr.SCHEDULE):
            m.next(row[s])
            if m.frame_num == 512:
                call_of_wrap.append(n)
                break
    assert call_of_wrap[0] == 512 and call_of_wrap[1] > 512


def test_oracle_decodes_its_own_long_streams(fo):
    r = lr.P_RUN
    for s, (stream, rec, _) in enumerate(lr.p_run_oracle()):
        got = lr.oracle_decode(stream)
        assert got.shape == rec.shape and np.array_equal(got, rec), f"P run stream {s}"
    for s in range(3):
        o = lr.schedule_oracle(s)
        got = lr.oracle_decode(o["stream"])
        rec = np.stack([p[2] for p in o["pictures"]])
        assert got.shape == rec.shape and np.array_equal(got, rec), f"schedule stream {s}"
    assert r["T"] == 530


# ---- 4. the synthesized decode streams

_ALL_SYNTH = sorted({k for b in lr.SYNTH_BATCHES.values() for k in b} | set(lr.SYNTH_LONG.values()))


@pytest.mark.parametrize("family", sorted(lr.FAMILIES))
def test_oracle_decodes_the_synth_plan(fo, family):
    for key in [k for k in _ALL_SYNTH if k[0] == family]:
        stream, _, types = lr.synth_stream(*key)
        pictures, got = lr.synth_oracle(*key)
        assert pictures.shape[0] == len(types) == len(got) == key[2], f"{key}: {pictures.shape[0]} pictures decoded"
        for t, (want, have) in enumerate(zip(types, got)):
            assert np.array_equal(want, have), f"{key} picture {t}: mb_type differs from macroblock {int(np.nonzero(want != have)[0][0])} on"
        same = np.nonzero((pictures[1:] == pictures[:-1]).all(axis=1))[0]
        assert same.size == 0, f"{key}: picture {int(same[0]) + 1} equals its predecessor"
        sat = float(((pictures == 0) | (pictures == 255)).mean())
        print(f"{key}: {len(stream)} bytes, {sat:.3f} of the samples at 0 or 255, sample std {pictures.std():.1f}")
        assert sat <= 0.5 and pictures.std() > 2


def _unstored(p):
    return p.get("modification") == []


def test_every_seam_position_is_hot():
    """From the plan table, not from a decode: whatever picture index t a decode window ends at (the product's is 256 where
    memory allows; nothing here depends on it), the batch of the seven offsets has every phase of the cycle at t - 1 and at
    t.  So some stream of the batch has at that seam each pair of neighbours the window hand-over exists for."""
    for family, batch in lr.SYNTH_BATCHES.items():
        plans = [lr.synth_plan(*k) for k in batch]
        T = batch[0][2]
        cyc = lr.FAMILIES[family]
        for t in list(range(2, T)):
            assert sorted(cyc.index(p[t]) for p in plans) == list(range(lr.PERIOD)), (family, t)
            pairs = [(p[t - 1], p[t]) for p in plans]
            # a tail_chroma_ac picture, then heads (skip / cbp0 macroblocks) that show the inherited delta and block
            assert any(a.get("tail_chroma_ac") and b.get("head") for a, b in pairs), (family, t)
            if family != "override":  # an unstored picture, then one that predicts across it
                assert any(_unstored(a) and b["type"] == "P" for a, b in pairs), (family, t)
            if family != "held":  # an override to two active entries, then a picture whose mb_pred reads ref_idx
                assert any(a.get("override") and a.get("active") == 1 and not b.get("override") for a, b in pairs), (family, t)
    assert lr.SYNTH_T > 257 and 255 < lr.SYNTH_T and lr.SYNTH_T_LONG > 2 * 256


# ---- 5. the reference's record


def _md5_tool():
    spec = importlib.util.spec_from_file_location("make_long_run_md5", GOLD / "make_long_run_md5.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_oracle_equals_the_reference_decoder_on_long_runs(fo):
    """tests/golden/long_run_md5.json holds the md5 of the Y4M file the reference's OWN decoder (oracle/_ref/ref_decode)
    wrote for the P-run streams and for every held and override stream: the oracle gives the same file, and where the binary
    is present it still reproduces the record.  So the reference's decoder accepts the wrapped headers the oracle writes.
    The mixed family carries no record: ref_decode dies with SIGSEGV on the unreduced cycle (at 30 pictures already, cause
    in the reference, not looked for), so those streams are held to the oracle alone."""
    recorded = json.loads((GOLD / "long_run_md5.json").read_text())
    tool = _md5_tool()
    names = dict(tool.streams())
    assert set(names) == set(recorded) and not any("mixed" in n for n in recorded)
    assert sum(n.startswith("p_run") for n in recorded) == 2
    assert {n for n in recorded if not n.startswith("p_run")} == {tool.synth_name(k) for k in _ALL_SYNTH if k[0] in lr.RECORDED_FAMILIES}
    for name, (stream, pictures, W, H) in names.items():
        assert ss.y4m_md5(pictures, W, H) == recorded[name], f"{name}: the oracle"
        if tool.REF_DECODE.exists():
            assert tool.reference_md5(stream) == recorded[name], f"{name}: the reference decoder"
