"""Constant tables of the reference that live in translation units which do not compile in this image
(every one of them includes stdafx.h -> <tchar.h>): their INITIALISER DATA is read from the reference's source text and
compared with the oracle's tables and with the tables / formulas of the device code.

The numbers are parsed by build() (oracle/Makefile, target `ref`, oracle/ref_tables.py) into
oracle/_ref/reference_tables.json, a git-ignored build product like oracle/_ref/libfer_leaf.so: skipped where the
reference tree was absent at build time.  Nothing of the reference is stored in the repository.  This narrows the
"encoder parity unpinned" gap of DESIGN.md section 2 -- the tables the encoder's arithmetic rests on are the reference's own -- it does not close it (the control flow around them
stays pinned by restatement and round trip only).
"""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "h264-fer_amd" / "csrc"
REF_TABLES = ROOT / "oracle" / "_ref" / "reference_tables.json"
pytestmark = pytest.mark.skipif(not REF_TABLES.exists(), reason="oracle/_ref/reference_tables.json not built (reference tree absent)")


def _ref(name):
    """numbers of the reference's table `name` (oracle/ref_tables.py)"""
    return np.array(json.loads(REF_TABLES.read_text())[name])


def _text(path):
    raw = Path(path).read_bytes()
    for enc in ("utf-8", "utf-16", "latin-1"):
        try:
            t = raw.decode(enc)
            if "{" in t:
                return t
        except UnicodeError:
            pass
    raise AssertionError(path)


def _init_body(path, name):
    """text between the braces of `name[...]... = { ... };` (comments removed)"""
    t = re.sub(r"//[^\n]*", "", _text(path))
    t = re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    m = re.search(r"\b" + re.escape(name) + r"\s*(?:\[[^\]]*\]\s*)+=\s*\{", t)
    assert m, f"{name} not found in {path}"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(t[i], 0)
        i += 1
    return t[m.end():i - 1]


def _ints(path, name):
    return np.array([int(v) for v in re.findall(r"-?\d+", _init_body(path, name))])


def _oracle_array(fo, name, n):
    return np.array((C.c_int * n).in_dll(fo.lib(), name))


def _dev_u8(name):
    return _ints(CSRC / "fer_dev.h", name)


def _dev_v():  # the three LevelScale classes per qP % 6 the device derives everything from (level_scale in fer_dev.h)
    v = _ints(CSRC / "fer_dev.h", "v")
    assert v.size == 18
    return v.reshape(6, 3)


def _cls(i, j):
    return 0 if ((i | j) & 1) == 0 else (1 if (i & j & 1) else 2)


def test_level_scale_and_level_quantize(fo):
    ls = _ref("LevelScale").reshape(6, 4, 4)
    lq = _ref("LevelQuantize").reshape(6, 4, 4)
    L = fo.lib()
    L.fo_level_scale.restype = L.fo_level_quantize.restype = C.c_int
    v = _dev_v()
    assert np.array_equal(v, _ref("v").reshape(6, 3))
    for m in range(6):
        for i in range(4):
            for j in range(4):
                assert L.fo_level_scale(m, i, j) == ls[m, i, j]
                assert L.fo_level_quantize(m, i, j) == lq[m, i, j]
                w = int(v[m, _cls(i, j)])
                assert 16 * w == ls[m, i, j]                              # level_scale() of fer_dev.h
                assert (65536 + 16 * w) // (2 * 16 * w) == lq[m, i, j]   # FER_LQ() of fer_dev.h; FerDev.lsq in fer_api.hip


def test_zigzag_and_block_origins(fo):
    zz = _ref("ZigZagReordering").reshape(16, 2)   # {y, x}
    assert np.array_equal(_oracle_array(fo, "fo_zigzag", 32).reshape(16, 2), zz)
    assert np.array_equal(_dev_u8("c_zz"), zz[:, 0] * 4 + zz[:, 1])
    izz = _dev_u8("c_izz")                                                       # scan position of raster sample
    assert np.array_equal(izz[_dev_u8("c_zz")], np.arange(16))
    so = _ref("Intra4x4ScanOrder").reshape(16, 2)    # {x, y}
    assert np.array_equal(_oracle_array(fo, "fo_blk_xy", 32).reshape(16, 2), so)
    assert np.array_equal(_dev_u8("c_bx"), so[:, 0]) and np.array_equal(_dev_u8("c_by"), so[:, 1])


def test_chroma_qp_table(fo):
    q = _ref("qPiToQPc")
    assert q.size == 52
    assert np.array_equal(_oracle_array(fo, "fo_qpc", 52), q)
    assert np.array_equal(_ints(CSRC / "fer_api.hip", "k_qpc"), q)
    import importlib
    t = importlib.import_module("test_gpu_mbunit")
    assert tuple(q) == t._QPC


def test_coded_block_pattern_maps(fo):
    for ref_name, fo_name, dev_name in (("codeNum_to_coded_block_pattern_intra", "fo_code_to_cbp_intra", "c_code_cbp_intra"),
                                        ("codeNum_to_coded_block_pattern_inter", "fo_code_to_cbp_inter", "c_code_cbp_inter"),
                                        ("coded_block_pattern_to_codeNum_intra", "fo_cbp_intra_to_code", "c_cbp_intra_code"),
                                        ("coded_block_pattern_to_codeNum_inter", "fo_cbp_inter_to_code", "c_cbp_inter_code")):
        r = _ref(ref_name)
        assert r.size == 48 and sorted(r) == list(range(48))
        assert np.array_equal(_oracle_array(fo, fo_name, 48), r), ref_name
        assert np.array_equal(_dev_u8(dev_name), r), ref_name


def test_intra_to_chroma_pred_mode():
    r = _ref("intraToChromaPredMode")
    assert list(r) == [2, 1, 0, 3]
    assert list(_ints(ROOT / "oracle" / "fo_intra.c", "intraToChroma")) == list(r)
    # the device spells the same map as a conditional chain (fer_intra.hip)
    src = _text(CSRC / "fer_intra.hip")
    assert "mode16 == 0 ? 2 : (mode16 == 1 ? 1 : (mode16 == 2 ? 0 : 3))" in src


def test_macroblock_type_tables():
    """I_Macroblock_Modes / P_and_SP_macroblock_modes (F/h264_globals.cpp:25-132): the columns the hot path uses.
    Intra16x16: mb_type = 1 + Intra16x16PredMode + 4 CodedBlockPatternChroma + 12 [CodedBlockPatternLuma == 15] -- what
    k_intra_mb writes and k_dec_parse reads; P: the partition shapes behind p_part_w / p_part_h (fer_mvpred.h)."""
    rows = _ref("I_Macroblock_Modes_intra16x16").tolist()
    assert len(rows) == 24
    for mbt, pred, cbc, cbl in rows:
        mbt, pred, cbc, cbl = int(mbt), int(pred), int(cbc), int(cbl)
        assert cbl in (0, 15)
        assert mbt == 1 + pred + 4 * cbc + 12 * (cbl == 15)
    prow = _ref("P_and_SP_macroblock_modes_p").tolist()
    shapes = {int(a): (int(n), int(w), int(h)) for a, n, w, h in prow}
    assert shapes == {0: (1, 16, 16), 1: (2, 16, 8), 2: (2, 8, 16), 3: (4, 8, 8), 4: (4, 8, 8)}
    dev = _text(CSRC / "fer_mvpred.h")
    assert "p_part_w(int t) { return (t == 0 || t == 1 || t == FER_P_SKIP) ? 16 : 8; }" in dev
    assert "p_part_h(int t) { return (t == 0 || t == 2 || t == FER_P_SKIP) ? 16 : 8; }" in dev
    # rows 5.. of the P table are the I rows shifted by 5 (mb_type of an intra macroblock in a P slice)
    irows_in_p = _ref("P_and_SP_macroblock_modes_intra16x16").tolist()
    assert [tuple(map(int, r)) for r in irows_in_p] == [tuple(map(int, r)) for r in rows]
