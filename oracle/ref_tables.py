"""oracle/ref_tables.py -- build step of the `ref` target (oracle/Makefile): reads the initialiser data of the reference's
constant tables that live in translation units which do not compile here (every one of them includes stdafx.h ->
<tchar.h>) and writes the numbers to _ref/reference_tables.json beside _ref/libfer_leaf.so, where
tests/test_reference_tables.py reads them.  Like the leaf library it is a build product of the reference tree (git-ignored).
Usage: python3 ref_tables.py REFERENCE_SOURCE_DIR OUTPUT_JSON
"""
import json
import re
import sys
from pathlib import Path


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
    return [int(v) for v in re.findall(r"-?\d+", _init_body(path, name))]


def tables(ref):
    out = {"LevelScale": _ints(ref / "scaleTransform.cpp", "LevelScale"),
           "LevelQuantize": _ints(ref / "quantizationTransform.cpp", "LevelQuantize"),
           "v": _ints(ref / "scaleTransform.cpp", "v"),
           "ZigZagReordering": _ints(ref / "scaleTransform.cpp", "ZigZagReordering"),
           "Intra4x4ScanOrder": _ints(ref / "h264_globals.cpp", "Intra4x4ScanOrder"),
           "qPiToQPc": _ints(ref / "inttransform.cpp", "qPiToQPc"),
           "intraToChromaPredMode": _ints(ref / "intra.cpp", "intraToChromaPredMode")}
    g = ref / "h264_globals.cpp"
    for name in ("codeNum_to_coded_block_pattern_intra", "codeNum_to_coded_block_pattern_inter",
                 "coded_block_pattern_to_codeNum_intra", "coded_block_pattern_to_codeNum_inter"):
        out[name] = _ints(g, name)
    # I_Macroblock_Modes / P_and_SP_macroblock_modes: the Intra16x16 rows as (mb_type, Intra16x16PredMode,
    # CodedBlockPatternChroma, CodedBlockPatternLuma), the P rows as (mb_type, NumMbPart, MbPartWidth, MbPartHeight)
    t = re.sub(r"//[^\n]*", "", _text(g))
    intra16 = r"\{\s*(\d+)\s*,\s*I_16x16_\w+\s*,\s*NA\s*,\s*Intra_16x16\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}"
    body = t[t.index("I_Macroblock_Modes"):]
    out["I_Macroblock_Modes_intra16x16"] = [list(map(int, r)) for r in re.findall(intra16, body)]
    pbody = t[t.index("P_and_SP_macroblock_modes"):t.index("I_Macroblock_Modes")]
    prow = r"\{\s*(\d+)\s*,\s*P_\w+\s*,\s*(\d+)\s*,\s*\w+\s*,\s*\w+\s*,\s*(\d+)\s*,\s*(\d+)\s*\}"
    out["P_and_SP_macroblock_modes_p"] = [list(map(int, r)) for r in re.findall(prow, pbody)]
    out["P_and_SP_macroblock_modes_intra16x16"] = [list(map(int, r)) for r in re.findall(intra16, pbody)]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    Path(sys.argv[2]).write_text(json.dumps(tables(Path(sys.argv[1]))) + "\n")
