"""tests/qp_sweep.py pinned without a GPU: the inputs, what they reach at every QP 0..51 (on the oracle alone), the reference
decoder's record of every stream, the decoder against the encoder's reconstruction, and the int32 / int16 headroom of the block
arithmetic (tests/transform_model.py).

test_gpu_qp_sweep.py compares the device with the oracle on these very runs; that comparison is worth what the oracle reaches,
so this test counts it.  The conditions are conditions on the inputs (change seeds or tiles if one is missed, never a condition).
"""
import hashlib
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import qp_sweep as qs
import transform_model as tm

GOLD = Path(__file__).resolve().parent / "golden"
MD5 = {"mild": "58657c40bd06b763bc616c9103086fa3", 20: "f711a8c1b6c25c393e48bfbfcacb4a6d",   # the four pictures of a stream
       21: "cef57bf8d6404eae617c2dfcd04da253", 22: "e3e8f5d8d4203ec9af5ed0a12452c019"}
MD5["noisy"] = "97d56c12017848b67539bc80eb7c7944"
GUARDED_FROM = {"mild": 0, "noisy": 0, 21: 3, 22: 5, 20: 9}   # the stream is under the level guard at every QP from this one on


def test_inputs_are_pinned():
    for s in qs.STREAMS:
        f = qs.frames(s)
        assert f.shape == (4, qs.W * qs.H * 3 // 2) and f.dtype == np.uint8
        assert hashlib.md5(f.tobytes()).hexdigest() == MD5[s], s
    assert tuple(qs.QPS) == tuple(range(52)) and qs.NAL_TYPES == (5, 1, 1, 1)


def _guarded(fo, qp):
    return [s for s in qs.STREAMS if qs.under_guard(fo, s, qp)]


def test_streams_are_under_the_level_guard_where_stated(fo):
    for s, q0 in GUARDED_FROM.items():
        for q in range(q0, 52):
            assert qs.under_guard(fo, s, q), (s, q, qs.run(fo, s, q)["max_level"])
    for q in qs.QPS:
        assert len(_guarded(fo, q)) >= (5 if q >= 9 else 2), q
    print("max_level per QP", qs.STREAMS, ":", [[qs.run(fo, s, q)["max_level"] for s in qs.STREAMS] for q in qs.QPS])


@pytest.mark.parametrize("qp", qs.QPS)
def test_every_qp_reaches_the_paths_under_the_guard(fo, qp):
    i16 = i4 = p_luma = p_chroma2 = level = 0
    for s in _guarded(fo, qp):
        r = qs.run(fo, s, qp)
        mt = r["pics"][0]["mb_type"]
        i4 += int((mt == 0).sum())
        i16 += int(((mt >= 1) & (mt <= 24)).sum())
        for p in r["pics"][1:]:
            coded = p["mb_type"] != 31
            p_luma += int((p["cbp"][coded, 0] != 0).sum())
            p_chroma2 += int((p["cbp"][coded, 1] == 2).sum())
        level = max(level, r["max_level"])
    assert i16 >= 1 and i4 >= 1, (i16, i4)
    assert p_luma >= 1 and p_chroma2 >= 1, (p_luma, p_chroma2)
    assert level >= 16, level


def test_the_sweep_as_a_whole(fo):
    skips = sum(int((p["mb_type"] == 31).sum()) for q in qs.QPS for s in _guarded(fo, q) for p in qs.run(fo, s, q)["pics"][1:])
    assert skips >= 1
    have = [q for q in qs.QPS if _guarded(fo, q)]
    for c in range(9):
        assert sum(q // 6 == c for q in have) >= 3, f"qP / 6 == {c}"
    for c in range(6):
        assert sum(q % 6 == c for q in have) >= 3, f"qP % 6 == {c}"
    # every level the oracle records fits the device's int16 level storage, under the guard or not
    for q in qs.QPS:
        for s in qs.STREAMS:
            assert qs.run(fo, s, q)["max_level"] <= tm.INT16, (s, q)


def _md5_tool():
    spec = importlib.util.spec_from_file_location("make_qp_sweep_md5", GOLD / "make_qp_sweep_md5.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("stream", qs.STREAMS)
def test_oracle_decoder_equals_the_reference_decoder(fo, stream):
    """tests/golden/qp_sweep_md5.json holds the md5 of what the reference's OWN decoder (oracle/_ref/ref_decode) wrote for every
    stream, the ones above the level guard included: the oracle decoder must give the same Y4M file, and where the binary is
    present it must still reproduce the record."""
    recorded = json.loads((GOLD / "qp_sweep_md5.json").read_text())
    assert len(recorded) == len(qs.STREAMS) * len(qs.QPS)
    tool = _md5_tool()
    for q in qs.QPS:
        r = qs.run(fo, stream, q)
        assert qs.y4m_md5(r["decoded"]) == recorded[tool.key(stream, q)], f"qp {q}: the oracle decoder"
        if tool.REF_DECODE.exists():
            assert tool.reference_md5(r["stream"]) == recorded[tool.key(stream, q)], f"qp {q}: the reference decoder"


def test_decoder_gives_the_encoders_luma_under_the_guard(fo):
    """Chroma is left out: the reference decoder re-applies stale ChromaACLevel to macroblocks of CBP 0 (F/residual.cpp:28-49).
    So are the pictures from the first slice that ends in a skip run on (qp_sweep.luma_pictures): 42 pictures of 21 guarded
    streams (the mosaics, QP 4..21) lose their last 1..3 macroblocks to the more_rbsp_data heuristic, or are predicted from such
    a picture, in the reference decoder and in the oracle alike (the md5 record holds both there).  The count is asserted, so the
    statement cannot drift.  At every QP the I picture of every guarded stream and at least one P picture are compared."""
    ys = qs.W * qs.H
    total = 0
    left_out = []   # (stream, qp, picture) behind luma_pictures() whose luma does differ
    for q in qs.QPS:
        p_pictures = 0
        for s in _guarded(fo, q):
            r = qs.run(fo, s, q)
            k = qs.luma_pictures(fo, s, q)
            assert k >= 1
            for t in range(4):
                same = np.array_equal(r["decoded"][t][:ys], r["pics"][t]["recon"][:ys])
                assert same or t >= k, (s, q, t)
                if not same:
                    left_out.append((s, q, t))
            p_pictures += k - 1
        assert p_pictures >= 1, q
        total += p_pictures
    print("P pictures compared:", total, "pictures the heuristic changes:", left_out)
    assert len(left_out) == 42 and len({(s, q) for s, q, _ in left_out}) == 21
    assert {s for s, _, _ in left_out} == {20, 21, 22} and {t for _, _, t in left_out} == {2, 3}


def test_host_chroma_qp_table_is_the_oracles(pkg, fo):
    """k_qpc of fer_api.hip.  What it writes into FerDev::qp at create and at ferhip_reset_stream, k_rc_plan overwrites from
    c_qpc_tab before any picture quantises, so no encoded picture can show a wrong entry; its live reader is ferhip_chroma_qp, the
    QPc of the per-macroblock shims (ferhip_intra_mbs, the legacy quantizationTransform / transformDecoding*).  Host code: no GPU."""
    import ctypes as C
    want = list((C.c_int * 52).in_dll(fo.lib(), "fo_qpc"))
    f = pkg.load_library().ferhip_chroma_qp
    assert [f(q) for q in range(52)] == want
    assert f(-1) == want[0] and f(52) == want[51] and f(1000) == want[51]


# ---------------------------------------------------------------- headroom
def _oracle_op(fo, op, keep, blocks, qp):
    if op == "forward_residual":
        return fo.forward_residual(qp, blocks, keep)
    if op == "inverse_residual":
        return fo.inverse_residual(qp, blocks, keep)
    return fo.block_op(op, blocks, qp)


def test_model_equals_the_oracle_and_stays_in_int32(fo):
    """the int64 model gives the oracle's (int32) results on every KAT input of test_gpu_qp_sweep.py at every QP, and none of
    its intermediates leaves int32: so the C oracle is defined on these inputs and the device's int arithmetic has headroom"""
    peak = 0
    for qp in range(52):
        for op, keep, blocks in tm.kat_cases(qp):
            tr = tm.Track()
            got = tm.MODEL[op](blocks, qp, tr=tr) if keep is None else tm.MODEL[op](blocks, qp, keep, tr)
            assert np.array_equal(got, _oracle_op(fo, op, keep, blocks, qp)), (qp, op, keep)
            assert tr.peak <= tm.INT32, (qp, op, keep, tr.peak)
            peak = max(peak, tr.peak)
    print("largest intermediate over all KAT inputs: %d = %.4f * 2^31" % (peak, peak / 2 ** 31))


def test_levels_fit_int16_and_products_fit_int32():
    """8-bit input: residuals within +-255, so a coefficient is within +-24241 and the unquantised DC within [-16352, 16288]
    (the core maps r != 0 to 64 r - 32, so the negative side reaches 32 further than 64 * 255).  The largest levels and quantiser
    products per QP (DESIGN.md quotes them)."""
    d = tm.forward_core(tm.extreme_sign_patterns())
    assert int(np.abs(d).max()) == 24241
    flat = tm.forward_core(np.stack([np.full(16, -255), np.full(16, 255)]))
    assert (int(flat[0, 0]), int(flat[1, 0])) == (tm.DC_MIN, tm.DC_MAX) == (int(d[:, 0].min()), int(d[:, 0].max()))
    m = tm.max_levels()
    print("per QP: residual level, luma DC level, chroma DC level, product / 2^31")
    for qp in range(52):
        print(qp, int(m[qp, 0]), int(m[qp, 1]), int(m[qp, 2]), "%.4f" % (m[qp, 3] / 2 ** 31))
    assert (m[:, :3] <= tm.INT16).all()
    assert (m[:, 3:] <= tm.INT32).all()
    assert (np.diff(m[:, 0]) <= 0).all() and (np.diff(m[:, 1]) <= 0).all(), "a coarser quantiser never gives a larger level"
    # the largest level of all: the luma DC of sixteen flat blocks of -255 at QP 0, ((64 * -16352 - 32) * 205 + 16384) >> 15
    assert int(m[:, :3].max()) == int(m[0, 1]) == 6547
