"""tests/slice_synth.py pinned without a GPU: the oracle decodes every stream the GPU test uses to the planned pictures
and macroblock types (a wrong nC model or a miswritten field desynchronises the slice and fails here, not on the GPU),
the plans together contain the syntax they were written for, and their pictures are not saturated."""
import ctypes as C
import hashlib
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import slice_synth as ss

GOLD = Path(__file__).resolve().parent / "golden"
_cache = {}


def decoded(fo, name):
    """-> [(stream, coverage, planned mb_types, oracle pictures [T][fsz], oracle mb_types)] of the plan's two streams"""
    if name not in _cache:
        out = []
        for stream, cov, types in ss.plan_streams(name):
            n, frames, got = fo.decode_stream_trace(stream)
            out.append((stream, cov, types, np.stack(frames), got))
        _cache[name] = out
    return _cache[name]


@pytest.mark.parametrize("name", sorted(ss.PLANS))
def test_oracle_decodes_the_plan(fo, name):
    a, b = decoded(fo, name)
    assert a[0] != b[0]
    for k, (stream, cov, types, pictures, got) in enumerate((a, b)):
        assert pictures.shape[0] == len(types) == len(got), f"stream {k}: {pictures.shape[0]} pictures decoded, {len(types)} planned"
        for t, (want, have) in enumerate(zip(types, got)):
            assert np.array_equal(want, have), f"stream {k} picture {t}: mb_type differs from macroblock {int(np.nonzero(want != have)[0][0])} on"
        sat = float(((pictures == 0) | (pictures == 255)).mean())
        print(f"{name}[{k}]: {len(stream)} bytes, {len(types)} pictures, {sat:.3f} of the samples at 0 or 255, sample std {pictures.std():.1f}")
        if ss.PLANS[name][3]:  # small / mixed levels only: a saturated sample hides arithmetic errors
            assert sat < 0.5
            assert pictures.std() > 2  # ... and a flat picture (std 0) shows none


def _md5_tool():
    spec = importlib.util.spec_from_file_location("make_synth_md5", GOLD / "make_synth_md5.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", sorted(ss.PLANS))
def test_oracle_equals_the_reference_decoder(fo, name):
    """tests/golden/synth_decode_md5.json holds the md5 of what the reference's OWN decoder (oracle/_ref/ref_decode, built
    from its translation units) wrote for every stream: the oracle must give the same Y4M file, and where the binary is
    present it must still reproduce the record."""
    recorded = json.loads((GOLD / "synth_decode_md5.json").read_text())
    tool = _md5_tool()
    cfg = dict(ss.CFG_DEFAULT, **ss.PLANS[name][0])
    for k, (stream, _, _, pictures, _) in enumerate(decoded(fo, name)):
        assert ss.y4m_md5(pictures, cfg["mbw"] * 16, cfg["mbh"] * 16) == recorded[f"{name}[{k}]"], f"stream {k}: the oracle"
        if tool.REF_DECODE.exists():
            assert tool.reference_md5(stream) == recorded[f"{name}[{k}]"], f"stream {k}: the reference decoder"


def test_intra_cbp_table_is_the_oracles(fo):
    t = (C.c_int * 48).in_dll(fo.lib(), "fo_code_to_cbp_intra")
    assert list(t) == ss.INTRA_CBP


def test_plans_cover_the_syntax(fo):
    cov = ss.new_coverage()
    for name in ss.PLANS:
        for _, c, _, _, _ in decoded(fo, name):
            ss.merge_coverage(cov, c)
    for cls in range(5):
        assert {tc for tc, _ in cov["coeff_token"][cls]} == set(range(5 if cls == 4 else 17)), f"coeff_token class {cls}"
    assert {(14, 0), (15, 0)} <= cov["level_prefix"]
    assert any(p == 15 and sl > 0 for p, sl in cov["level_prefix"])
    assert cov["max_suffix_length"] == 6 and (15, 6) in cov["level_prefix"]
    assert cov["start_suffix_1"]
    for n, rows in ((16, range(1, 16)), (15, range(1, 15)), (4, range(1, 4))):  # a row = one TotalCoeff < maxNumCoeff
        assert {tc for tc, _ in cov["total_zeros"][n]} == set(rows), f"total_zeros, maxNumCoeff {n}"
    assert cov["max_run_before"] >= 7
    assert cov["i4_modes"] == set(range(9)) and cov["i16_modes"] == set(range(4)) and cov["chroma_modes"] == set(range(4))
    assert cov["i4_coding"] == {(1, -1)} | {(0, r) for r in range(8)}
    assert cov["intra_in_p"] == {(a, b) for a in ss.KINDS for b in ss.KINDS}
    assert cov["mb_types"]["I"] == set(range(25)) and cov["mb_types"]["P"] == set(range(30)) | {ss.P_SKIP}
    assert cov["sub_types"] == set(range(4))
    assert cov["qpy"] == set(range(52)) and cov["wrap_up"] and cov["wrap_down"]


def test_i4_pairs_come_from_both_constrained_settings(fo):
    for name in ("intra_in_p", "intra_in_p_constrained"):
        cov = ss.merge_coverage(ss.merge_coverage(ss.new_coverage(), decoded(fo, name)[0][1]), decoded(fo, name)[1][1])
        assert len(cov["intra_in_p"]) == 25, name


def _tab(fo, name, rows, cols):
    return np.array((C.c_uint8 * (rows * cols)).in_dll(fo.lib(), name)).reshape(rows, cols)


def test_analyze_block_agrees_with_the_writer(fo):
    """the coverage report's own restatement of residual_block_cavlc, against the bit count of the oracle's writer"""
    rng = np.random.default_rng(1)
    tz16, tz4, rbl = _tab(fo, "fo_tz_len", 15, 16), _tab(fo, "fo_tzdc_len", 3, 4), _tab(fo, "fo_rb_len", 6, 7)
    for mode in ss.LEVEL_MODES:
        for n in (4, 15, 16):
            for _ in range(60):
                coef = ss.gen_block(rng, n, int(rng.integers(0, n + 1)), mode, 40)
                a = ss.analyze_block(coef, n)
                _, bits, tc = fo.cavlc_encode_block(coef, n, -1 if n == 4 else 0)
                assert tc == a["tc"]
                ln, code = C.c_int(), C.c_uint()
                fo.lib().fo_coeff_token(4 if n == 4 else 0, tc, a["t1"], C.byref(ln), C.byref(code))
                want = ln.value + a["t1"]
                for p, sl in a["prefixes"]:
                    want += p + 1 + (4 if (p == 14 and sl == 0) else 12 if p == 15 else sl)
                zl = 0
                if a["tz"] is not None:
                    zl = a["tz"]
                    want += int((tz4 if n == 4 else tz16)[tc - 1, zl])
                for r in a["runs"]:
                    want += ((3 if r < 7 else r - 3) if zl > 6 else int(rbl[zl - 1, r]))
                    zl -= r
                assert bits == want, (mode, n, coef)


F4_MD5 = {  # pslice_synth.make_stream(split_nals, qcif_ippp_4f_qp12_w16, 7, plan) before slice_synth.py shared its header writer
    "list_modification": "e79c96110c94b00eee13447061c43f67", "mixed": "994790d2fb9ab428e3e7f7196eced804", "ref_idx": "0cdd3847dce6a4f2fce19f57f1625885", "sub_partitions": "ee8504f696352ae04b681053319283fb"}


def test_pslice_synth_still_writes_the_same_bytes(pkg):
    import pslice_synth as ps
    base = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    plans = {
        "sub_partitions": [dict(), dict(), dict()],
        "ref_idx": [dict(override=True, active=1), dict(), dict(override=True, active=0), dict(), dict(override=True, active=3)],
        "list_modification": [dict(modification=[]), dict(), dict(modification=[(0, 0)]), dict(modification=[]),
                              dict(modification=[]), dict(modification=[(1, 2), (2, 0)]), dict()],
        "mixed": [dict(override=True, active=1, modification=[]), dict(early_end=True), dict(modification=[], early_end=True),
                  dict(override=True, active=0), dict(modification=[(0, 1)], mvd_range=12), dict(mvd_range=40, p_skip=0.05)],
    }
    for name, plan in plans.items():
        assert hashlib.md5(ps.make_stream(pkg.split_nals, base, 7, plan)).hexdigest() == F4_MD5[name], name
