"""The illegal and damaged streams pinned without a GPU: their bytes, the record of what the reference's own decoder makes
of them (tests/golden/illegal_decode_record.json), and the oracle held to that record -- on every stream the reference
decodes the oracle gives its pictures, where the reference stops with a fatal error the oracle stops in front of the same
picture, and where the reference dies the oracle only has to return.  The shares at the end keep the GPU test, which
compares the device with the oracle by these classes, from passing on streams that prove nothing."""
import hashlib
import importlib.util
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import damage_corpus as dc
import illegal_cases as ic
import slice_synth as ss

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


def _md5s(frames):
    return [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in frames]


def _tool():
    spec = importlib.util.spec_from_file_location("make_illegal_record", GOLD / "make_illegal_record.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_corpus_is_pinned():
    c = dc.corpus()
    assert len(c) == 144 and len({s for _, _, s in c}) == 144
    for name, golden, stream in c:
        clean = (GOLD / f"{golden}.264").read_bytes()
        assert len(stream) == len(clean) and stream[:64] == clean[:64] and stream != clean, name
        changed = [i for i in range(len(clean)) if stream[i] != clean[i]]
        assert all(stream[i] >= 2 for i in changed), f"{name}: a changed byte could mint a start code"
        if "/bit" in name:
            assert len(changed) == 1 and bin(stream[changed[0]] ^ clean[changed[0]]).count("1") == 1, name
        else:
            assert 1 <= len(changed) <= 5 and changed[-1] - changed[0] < 64, name
    assert dc.corpus_md5() == ic.CORPUS_MD5 == ic.record()["corpus_md5"]
    assert len(ic.record()["tier2"]) == 144
    assert set(ic.record()["tier1"]) == {k for k, *_ in ic.tier1()}


def test_every_illegal_plan_is_decoded_by_the_reference():
    """Tier 1 is legal syntax: the reference exits 0 on every stream (the constrained_intra_pred plan included)."""
    t1 = ic.tier1()
    bad = [k for k, *_, e in t1 if e["class"] != "complete"]
    print(f"tier 1: {len(t1) - len(bad)} of {len(t1)} streams complete")
    assert not bad, bad
    for key, name, W, H, stream, e in t1:
        assert len(e["md5"]) == len(ss.ILLEGAL_PLANS[name][1]), key


def test_oracle_equals_the_record_on_illegal_plans(fo):
    for key, name, W, H, stream, e in ic.tier1():
        v = ic.verdict(fo, key, stream)
        assert v["status"] == fo.DEC_END and _md5s(v["frames"]) == e["md5"], key


def test_oracle_equals_the_record_on_the_damage_corpus(fo):
    differs = []
    for i, name, golden, stream, e in ic.tier2():
        v = ic.verdict(fo, i, stream)  # (that it returns at all is the first thing checked: ctypes passes a signal on)
        if e["class"] == "complete":
            ok = v["status"] == fo.DEC_END and _md5s(v["frames"]) == e["md5"]
        elif e["class"] == "fatal":
            # exactly the pictures in front of the recorded frame, then a stop: at the reference's fatal error, or at a
            # point in that same picture where the reference already ran outside its arrays
            ok = v["status"] in (fo.DEC_FATAL, fo.DEC_UNDEFINED) and len(v["frames"]) == e["frame"] - 1
        else:
            ok = v["status"] in (fo.DEC_END, fo.DEC_FATAL, fo.DEC_UNDEFINED)
        if not ok:
            differs.append(i)
    print(f"oracle differs from the record on {differs}; open list {sorted(ic.OPEN)}")
    assert differs == sorted(ic.OPEN)
    assert len(ic.OPEN) <= 0.05 * 144


def test_reference_decoder_still_gives_the_record():
    """Where oracle/_ref/ref_decode exists (the reference tree was present at build time) it reproduces the record."""
    tool = _tool()
    if not tool.REF_DECODE.exists():
        pytest.skip("oracle/_ref/ref_decode was not built (no reference tree): the record is held against the oracle only")
    t1, t2 = tool.all_streams()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as ex:
        v1 = list(ex.map(tool.reference_verdict, [s for _, s in t1]))
        v2 = list(ex.map(tool.reference_verdict, t2))
    for (k, _), v in zip(t1, v1):
        assert v == ic.record()["tier1"][k], k
    for i, v in enumerate(v2):
        e = ic.record()["tier2"][i]
        # (a stream the reference dies on may die differently from run to run: only the class is held)
        assert v == e or (v["class"] == e["class"] == "undefined"), i


def test_shares_of_the_damage_corpus(fo):
    """Conditions on the reference alone: enough streams of every class that the comparison means something."""
    t2 = ic.tier2()
    clean = {g: _md5s(fo.decode_stream_verdict((GOLD / f"{g}.264").read_bytes())["frames"]) for g in dc.GOLDENS}
    n = len(t2)
    complete = [(i, g, e) for i, _, g, _, e in t2 if e["class"] == "complete"]
    fatal = [e for *_, e in t2 if e["class"] == "fatal"]
    changed = [i for i, g, e in complete if e["md5"] != clean[g]]
    late = [e for e in fatal if e["frame"] > 1]
    print(f"tier 2: {len(complete)} complete + {len(fatal)} fatal of {n} = {(len(complete) + len(fatal)) / n:.1%}; "
          f"{len(changed)} of {len(complete)} complete with a changed picture = {len(changed) / len(complete):.1%}; "
          f"{len(late)} of {len(fatal)} fatal behind at least one picture = {len(late) / len(fatal):.1%}; open list {len(ic.OPEN)} of {n}")
    assert len(complete) + len(fatal) >= 0.75 * n
    assert len(changed) >= 0.10 * len(complete)
    assert len(late) >= 0.15 * len(fatal)
    # and what the GPU test makes of them: classes that owe pictures or a fault, not "undefined"
    kinds = [ic.expectation(e, ic.verdict(fo, i, s), i in ic.OPEN)["kind"] for i, _, _, s, e in t2]
    print({k: kinds.count(k) for k in ("complete", "fatal", "refused", "undefined")})
    assert kinds.count("complete") >= 0.10 * n and kinds.count("fatal") >= 0.5 * n


def _missing(mbw, mb, x0, y0):
    """(no left neighbour, no upper neighbour) of the block at (x0, y0) of macroblock mb"""
    return (mb % mbw) * 16 + x0 == 0, (mb // mbw) * 16 + y0 == 0


NEEDS_UP, NEEDS_LEFT, NEEDS_BOTH = 1, 2, 3


def test_illegal_plans_predict_from_missing_neighbours(fo):
    """On the oracle's trace: every prediction mode that reads a neighbour meets that neighbour missing, in an I slice and
    in a P slice -- Intra4x4 0, 3, 7 without the upper, 1, 8 without the left, 4, 5, 6 without either; Intra16x16 0
    (vertical), 1 (horizontal), 3 (plane); chroma 2 (vertical), 1 (horizontal), 3 (plane)."""
    i4_need = {0: NEEDS_UP, 3: NEEDS_UP, 7: NEEDS_UP, 1: NEEDS_LEFT, 8: NEEDS_LEFT, 4: NEEDS_BOTH, 5: NEEDS_BOTH, 6: NEEDS_BOTH}
    i16_need = {0: NEEDS_UP, 1: NEEDS_LEFT, 3: NEEDS_BOTH}
    chroma_need = {2: NEEDS_UP, 1: NEEDS_LEFT, 3: NEEDS_BOTH}
    seen = set()

    def note(kind, sl, mode, need, no_left, no_up):
        if mode in need and ((need[mode] & NEEDS_UP and no_up) or (need[mode] & NEEDS_LEFT and no_left)):
            seen.add((kind, sl, mode))

    for key, name, W, H, stream, _ in ic.tier1():
        if not name.startswith("any_mode"):
            continue
        v, mbw = ic.verdict(fo, key, stream), W // 16
        for t in range(len(v["frames"])):
            sl, base = ("I", 0) if v["slice_type"][t] == 2 else ("P", 5)
            for mb, ty in enumerate(v["mb_type"][t]):
                k = int(ty) - base
                if k < 0 or k > 24:
                    continue
                no_left, no_up = _missing(mbw, mb, 0, 0)
                note("chroma", sl, int(v["chroma_mode"][t][mb]), chroma_need, no_left, no_up)
                if k == 0:
                    for blk, (x0, y0) in enumerate(ss.BLK_XY):
                        note("i4", sl, int(v["i4mode"][t][mb][blk]), i4_need, *_missing(mbw, mb, x0, y0))
                else:
                    note("i16", sl, (k - 1) & 3, i16_need, no_left, no_up)
    want = {(kind, sl, m) for kind, need in (("i4", i4_need), ("i16", i16_need), ("chroma", chroma_need)) for sl in "IP" for m in need}
    assert seen == want, sorted(want - seen)


def _vector_range(fo, name):
    lo = hi = 0
    for key, n, W, H, stream, _ in ic.tier1():
        if n != name:
            continue
        v = ic.verdict(fo, key, stream)
        for t in range(len(v["frames"])):
            if v["slice_type"][t] == 0:
                inter = (v["mb_type"][t] <= 4) | (v["mb_type"][t] == ss.P_SKIP)
                if inter.any():
                    lo, hi = min(lo, int(v["mv"][t][inter].min())), max(hi, int(v["mv"][t][inter].max()))
    return lo, hi


def test_vectors_inside_and_past_int16(fo):
    """From the oracle's own vectors: mvd_300 and mvd_3000 stay inside 16 bits and far past what a level allows (+-8192 is the
    most, +-2048 at QCIF), mvd_40000 leaves 16 bits in every stream, in a P picture the refusal is read from."""
    for name in ss.VECTORS_INSIDE_INT16:
        lo, hi = _vector_range(fo, name)
        print(name, lo, hi)
        assert -32768 <= lo and hi <= 32767 and max(-lo, hi) > 250, name
    lo, hi = _vector_range(fo, "mvd_3000")
    assert max(-lo, hi) > 8192
    for name in ss.VECTORS_PAST_INT16:
        for key, n, W, H, stream, e in ic.tier1():
            if n == name:
                x = ic.expectation(e, ic.verdict(fo, key, stream))
                print(key, x)
                assert x["kind"] == "refused" and x["reason"] == "motion vector past 16 bits" and 1 <= x["good"], key
    for key, n, W, H, stream, e in ic.tier1():
        if n not in ss.VECTORS_PAST_INT16:
            assert ic.expectation(e, ic.verdict(fo, key, stream))["kind"] == "complete", key


def test_legal_plans_have_nothing_to_refuse(fo):
    """The refusal reasons are read off the oracle's trace: none of them shows on a legal stream."""
    for name in sorted(ss.PLANS):
        for k, (stream, _, _) in enumerate(ss.plan_streams(name)):
            assert ic.refusal(fo.decode_stream_verdict(stream)) == (None, None), (name, k)
    for g in dc.GOLDENS:
        assert ic.refusal(fo.decode_stream_verdict((GOLD / f"{g}.264").read_bytes())) == (None, None), g


def test_oracle_is_clean_under_sanitizers_on_every_stream(fo, tmp_path):
    """A stand-alone build of the oracle's command line with AddressSanitizer and UBSan decodes every illegal and damaged
    stream as a child process: no report, and the same pictures and status as the library the tests load."""
    src = [str(ROOT / "oracle" / f) for f in ("fo_cli.c", "fo_tables.c", "fo_bits.c", "fo_transform.c", "fo_intra.c", "fo_cavlc.c",
                                               "fo_inter.c", "fo_encode.c", "fo_decode.c", "fo_gen.c", "fo_debug.c")]
    exe = tmp_path / "fo_cli_san"
    # (the sanitizer runtimes linked into the program: it runs in whatever environment the suite runs in)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu99", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe)] + src, check=True)
    cases = [(k, s) for k, _, _, _, s, _ in ic.tier1()] + [(i, s) for i, _, _, s, _ in ic.tier2()]
    files = []
    for n, (_, s) in enumerate(cases):
        files.append(tmp_path / f"{n:03d}.264")
        files[-1].write_bytes(s)
    r = subprocess.run([str(exe), "decn"] + [str(f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [json.loads(x) for x in r.stdout.decode().splitlines()]
    assert len(lines) == len(cases)
    for (key, s), got in zip(cases, lines):
        v = ic.verdict(fo, key, s)
        assert (got["pictures"], got["status"]) == (len(v["frames"]), v["status"]), key


def test_sub_mb_type_past_the_table_is_undefined(fo, pkg):
    """sub_mb_type 4: the reference's NumSubMbPart indexes past P_sub_macroblock_modes, so the oracle stops with the
    "reference undefined" code behind the pictures in front (the device reports a syntax fault there)"""
    import pslice_synth as ps
    clean = (GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    first = pkg.access_units(clean)[0]
    w, _, _ = ps.p_slice(np.random.default_rng(3), 99, 1, 2, False, 0, None)
    w.ue(0)  # mb_skip_run
    w.ue(3)  # P_8x8
    for s in (0, 4, 1, 2):
        w.ue(s)
    v = fo.decode_stream_verdict(first + ps.nal_unit(1, 2, w.rbsp(4)))
    assert v["status"] == fo.DEC_UNDEFINED and len(v["frames"]) == 1
