"""The helpers of the neighbourhood-seam tests (tests/seam_nbhd.py), checked without a GPU: the ctypes mirror of fo_ctx is
pinned against the oracle's accessors, the generators are pinned, and what their jobs reach is counted ON THE ORACLE ALONE --
test_gpu_seam_nbhd.py compares the device with the oracle on these very jobs, and that comparison is worth what the oracle
exercises.  The floors are about a fifth of the counts measured (the rule of test_hard_content_host.py; the counts are in
DESIGN.md): conditions on the generators -- change a generator if one is missed, never a floor."""
import ctypes as C
import hashlib

import numpy as np

import seam_nbhd as sn

P_SKIP = 31


def test_mirror_is_pinned(fo):
    """every pointer or value of fo_ctx that has an accessor reads the same through FoCtx; they bracket each field the driver
    reaches through the mirror alone (chroma_qp_offset, refidx, prev_flag .. sub_mb_type, constrained_intra)"""
    o = fo.Oracle(48, 32, qp=23, window=24, maxdiff=5, intra_every=7)
    L, c = o.L, o.c
    o.set_frame(np.zeros(48 * 32 * 3 // 2, np.uint8))
    o.set_dpb(np.zeros(48 * 32 * 3 // 2, np.uint8))
    o.fill_interpolated()
    o.record_me(True)
    m = sn.mirror(o)
    base = c.value
    assert (m.W, m.H, m.Wc, m.Hc, m.mbw, m.mbh, m.nmb) == (48, 32, 24, 16, 3, 2, 6)
    assert (m.qp, m.window, m.maxdiff_set, m.intra_every, m.basic) == (23, 24, 5, 7, 0)
    assert m.MAXDIFF == 2                                      # fo_create's default (F/h264_globals.cpp)
    o.set_mb(4, 9, 2, 37)
    assert (m.cur, m.cur_mb_type, m.slice_type, m.QPy) == (4, 9, 2, 37)
    assert m.L == L.fo_dbg_plane(c, 0) and m.C[1] == L.fo_dbg_plane(c, 2) and m.dL == L.fo_dbg_plane(c, 3) and m.dC[1] == L.fo_dbg_plane(c, 5)
    assert m.mb_type == L.fo_dbg_mb_type(c) and m.cbp_l == L.fo_dbg_cbp(c, 0) and m.cbp_c == L.fo_dbg_cbp(c, 1)
    assert m.tc_l == L.fo_dbg_tc_l(c) and m.tc_c == L.fo_dbg_tc_c(c) and m.i4mode == L.fo_dbg_i4mode(c)
    assert m.mvx == L.fo_dbg_dec_mv(c, 0) and m.mvy == L.fo_dbg_dec_mv(c, 1)
    assert m.refidx and m.refidx not in (m.mvy, m.mb_type)
    assert base + sn.FoCtx.lv.offset == L.fo_dbg_levels(c)
    assert m.interp[0] and m.interp[0] == L.fo_dbg_interp(c, 0) and m.interp[15] == L.fo_dbg_interp(c, 15)
    assert m.kar[0] and m.kar[0] == L.fo_dbg_kar(c, 0, 0) and m.kar[79] == L.fo_dbg_kar(c, 4, 15)
    assert m.sorted[0] == L.fo_dbg_sorted(c, 0)
    assert base + sn.FoCtx.koliko.offset == L.fo_dbg_koliko(c)
    assert base + sn.FoCtx.type_count.offset == L.fo_dbg_type_count(c)
    assert m.dbg_mvx == L.fo_dbg_mv(c, 0) and m.dbg_mvy == L.fo_dbg_mv(c, 1) and m.dbg_mbsize == L.fo_dbg_mbsize(c)
    assert m.me_rec and m.me_rec == L.fo_dbg_me_lists(c)
    assert m.chroma_pred_mode == L.fo_dbg_chroma_mode(c)
    m.refusals, m.block_overrun, m.dbg_max_level = 5, 3, 77
    assert (L.fo_dbg_refusals(c), L.fo_dbg_block_overrun(c), o.max_level()) == (5, 3, 77)
    m.refusals = m.block_overrun = 0
    # the level arrays through the mirror are the accessor's
    o.set_levels(cac=np.arange(128))
    assert list(m.lv.CAC[:]) == list(range(128)) and m.lv.CDC[7] == 0
    o.close()


def _digest(jobs):
    h = hashlib.md5()
    for j in jobs:
        for k in sorted(j):
            v = j[k]
            if k == "mb":
                for n in v:
                    for kk in sorted(n or {}):
                        h.update(np.asarray(n[kk], np.int64).tobytes())
            else:
                h.update(np.asarray(v, np.int64).tobytes())
    return h.hexdigest()


def test_generators_are_pinned():
    enc = sn.encode_jobs(11, 2)
    assert len(enc) == 60 and _digest(enc) == _digest(sn.encode_jobs(11, 2)) != _digest(sn.encode_jobs(12, 2))
    assert [(j["pos"], j["qp"]) for j in enc[::2]] == [(p, q) for p in range(6) for q in sn.ENC_QPS]
    dec = sn.decode_jobs(12, 120)
    assert _digest(dec) == _digest(sn.decode_jobs(12, 120))
    assert all(sn.mode4_legal(j["pos"], b, m) for j in dec if j["mb"][j["pos"]]["mb_type"] in (0, 5) and j["slice_type"] == (2 if j["mb"][j["pos"]]["mb_type"] == 0 else 0)
               for b, m in enumerate(sn.i4_modes(j)))
    mv = sn.mv_jobs(13, 72)
    assert _digest(mv) == _digest(sn.mv_jobs(13, 72)) and {(j["pos"], j["mb_type"]) for j in mv[:36]} == {(p, t) for p in range(6) for t in (0, 1, 2, 3, 4, 31)}
    assert len(sn.OVERFLOW_JOBS) == 5 and len({n for n, _ in sn.OVERFLOW_JOBS}) == 5


def test_encode_jobs_reach_the_decision(fo):
    jobs = sn.encode_jobs(11, 64)
    x = sn.NbOracle(fo)
    refs = [x.encode(j) for j in jobs]
    ret = np.array([r["ret"] for r in refs])
    i16 = np.bincount(ret[ret >= 0], minlength=4)
    i4 = np.bincount(np.concatenate([r["i4mode"] for r in refs if r["ret"] == -1]), minlength=9)
    print("Intra16x16 winners by mode", i16, "Intra4x4 macroblocks", int((ret == -1).sum()), "their block modes", i4)
    assert (ret == -1).sum() >= 156 and (ret >= 0).sum() >= 228
    assert (i16 >= np.array([38, 43, 127, 19])).all(), i16
    assert (i4 >= np.array([765, 549, 407, 207, 275, 70, 74, 71, 75])).all(), i4
    # a mode that reads a missing neighbour is skipped: never chosen, at every pos
    per_pos = np.zeros(6, int)
    for j, r in zip(jobs, refs):
        nb = sn.NB[j["pos"]]
        per_pos[j["pos"]] += 1
        assert not ((r["ret"] == 0 and "B" not in nb) or (r["ret"] == 1 and "A" not in nb) or (r["ret"] == 3 and not ("A" in nb and "B" in nb))), j["pos"]
        assert all(sn.mode4_legal(j["pos"], b, int(m)) for b, m in enumerate(r["i4mode"]))
    assert (per_pos == 320).all()
    dc_only = sum(r["ret"] == 2 for j, r in zip(jobs, refs) if j["pos"] == 0)
    print("pos 0 (DC alone is left of the 16x16 modes): Intra16x16 winners", dc_only)
    assert dc_only >= 39
    # the min4 == 0 early exit, observed on block 0 (whose search reads no sample of its own macroblock)
    early = sum(x.block0_cost(j, int(r["i4mode"][0])) == 0 for j, r in zip(jobs, refs))
    print("block 0 found a mode of cost 0", early)
    assert early >= 77
    # the stale mb_type_array entry: P_Skip changes what the first coded_mb_size returns
    stale = [(j, r) for j, r in zip(jobs, refs) if j["mb"][j["pos"]]["mb_type"] == P_SKIP]
    differs = 0
    for j, r in stale:
        mb = list(j["mb"])
        mb[j["pos"]] = dict(mb_type=0)
        differs += int(x.encode(dict(j, mb=mb))["mbsize"][0] != r["mbsize"][0])
    print("jobs with a stale P_Skip entry", len(stale), "of which the Intra16x16 size differs from any other entry's", differs)
    assert len(stale) >= 121 and differs >= 98
    cbpl = np.bincount([r["cbp_luma"] for r in refs if r["ret"] == -1], minlength=16)
    cbpc = np.bincount([r["cbp_chroma"] for r in refs], minlength=3)
    print("Intra4x4 luma CBP", cbpl, "cbpC", cbpc)
    assert cbpl[1:15].sum() >= 76 and (cbpl[1:15] > 0).sum() >= 3 and (cbpc >= np.array([52, 79, 251])).all()
    rec0 = sum(int((r["recY"] == 0).sum() + (r["recCb"] == 0).sum() + (r["recCr"] == 0).sum()) for r in refs)
    rec255 = sum(int((r["recY"] == 255).sum() + (r["recCb"] == 255).sum() + (r["recCr"] == 255).sum()) for r in refs)
    print("reconstructed samples at 0 / 255", rec0, rec255)
    assert rec0 >= 2773 and rec255 >= 2166
    x.close()


def test_decode_jobs_reach_the_derivation(fo):
    jobs = sn.decode_jobs(12, 1800)
    x = sn.NbOracle(fo)
    kinds = {"A": dict(missing=0, inter=0, i16=0, i4=0), "B": dict(missing=0, inter=0, i16=0, i4=0)}
    constrained, rem_side, upright, cmodes, i16modes = np.zeros(2, int), dict(below=0, above=0, predicted=0), dict(taken=0, substituted=0), np.zeros(4, int), np.zeros(4, int)
    for j in jobs:
        pos, st = j["pos"], j["slice_type"]
        t = j["mb"][pos]["mb_type"]
        cmodes[j["chroma_mode"]] += 1
        if t != (0 if st == 2 else 5):
            i16modes[((t if st == 2 else t - 5) - 1) & 3] += 1
            continue
        r = x.decode(j)
        constrained[j["constrained_intra"]] += 1
        for side, off in (("A", 1), ("B", 3)):
            if side not in sn.NB[pos]:
                kinds[side]["missing"] += 1
                continue
            nt = j["mb"][pos - off]["mb_type"]
            k = nt if st == 2 else nt - 5
            kinds[side]["i4" if k == 0 else "i16" if 1 <= k <= 24 and nt != P_SKIP else "inter"] += 1
        for b in range(16):
            if j["prev_flag"][b]:
                rem_side["predicted"] += 1
            else:
                assert r["i4mode"][b] in (j["rem_mode"][b], j["rem_mode"][b] + 1)
                rem_side["below" if r["i4mode"][b] == j["rem_mode"][b] else "above"] += 1
        if r["i4mode"][5] in (3, 7):                             # block 5: its up-right samples lie in macroblock C
            upright["substituted" if pos == 5 else "taken"] += 1
            assert pos in (3, 4, 5)
    print("Intra4x4 jobs by constrained_intra", constrained, "edge blocks by neighbour", kinds, "rem_mode against the prediction", rem_side)
    print("block 5 with a mode that reads up-right samples", upright, "chroma modes", cmodes, "Intra16x16 modes", i16modes)
    assert (constrained >= 92).all()
    for side in kinds:
        assert kinds[side]["missing"] >= 59 and kinds[side]["inter"] >= 40 and kinds[side]["i16"] >= 26 and kinds[side]["i4"] >= 25, kinds
    assert rem_side["below"] >= 475 and rem_side["above"] >= 1253 and rem_side["predicted"] >= 1237
    assert upright["taken"] >= 11 and upright["substituted"] >= 4
    assert (cmodes >= np.array([179, 88, 60, 31])).all() and (i16modes >= np.array([31, 46, 83, 12])).all()
    x.close()


def _mv_classes(j):
    """the rules a DERIVE job reaches, told from its inputs (the tests of F/mode_pred.cpp:252-371, :381-425)"""
    pos, t, nb = j["pos"], j["mb_type"], sn.NB[j["pos"]]

    def state(side):
        if side not in nb:
            return None
        nt = j["mb"][nb[side]]["mb_type"]
        return "inter" if nt <= 4 or nt == P_SKIP else "intra"

    out = set()
    a, b, c, d = state("A"), state("B"), state("C"), state("D")
    if "intra" in (a, b, c, d):
        out.add("intra neighbour")
    if t == P_SKIP:
        if not ("A" in nb and "B" in nb):
            out.add("skip: zero at the picture edge")
        else:
            va, vb = np.asarray(j["mb"][nb["A"]]["mv"]).reshape(4, 2)[1], np.asarray(j["mb"][nb["B"]]["mv"]).reshape(4, 2)[2]
            out.add("skip: zero beside a zero vector" if (a == "inter" and not va.any()) or (b == "inter" and not vb.any()) else "skip: predicted")
        return out
    if t in (3, 4):
        out.add("8x8 sub type %d" % j["sub_mb_type"][0])
        return out
    if c is None and d is not None:
        out.add("C replaced by D")
        c = d
    if t == 1:
        out.add("16x8 upper takes B" if b == "inter" else "16x8 upper falls through")
        out.add("16x8 lower takes A" if a == "inter" else "16x8 lower falls through")
        return out
    if t == 2:
        out.add("8x16 left takes A" if a == "inter" else "8x16 left falls through")
        out.add("8x16 right takes C" if (state("C") or ("inter" if b == "inter" and "C" not in nb else None)) == "inter" else "8x16 right falls through")
        return out
    # 16x16: the substitution chain of PredictMV_Luma, then one reference alone or the median
    if a is None and b is None:
        a = "inter"
    elif a is None:
        a = "intra"
    b = a if b is None else b
    c = a if c is None else c
    refs = [s == "inter" for s in (a, b, c)]
    out.add("one reference alone: " + "ABC"[refs.index(True)] if sum(refs) == 1 else "median")
    return out


def test_mv_jobs_reach_the_rules(fo):
    jobs = sn.mv_jobs(13, 2880)
    count = {}
    for j in jobs:
        for k in _mv_classes(j):
            count[k] = count.get(k, 0) + 1
    print("DERIVE jobs by rule", dict(sorted(count.items())))
    floors = {"median": 82, "one reference alone: A": 2, "one reference alone: B": 4, "one reference alone: C": 6, "C replaced by D": 48, "intra neighbour": 265,
              "16x8 upper takes B": 30, "16x8 upper falls through": 66, "16x8 lower takes A": 42, "16x8 lower falls through": 53,
              "8x16 left takes A": 40, "8x16 left falls through": 55, "8x16 right takes C": 33, "8x16 right falls through": 62,
              "skip: zero at the picture edge": 64, "skip: zero beside a zero vector": 13, "skip: predicted": 18,
              "8x8 sub type 0": 76, "8x8 sub type 1": 38, "8x8 sub type 2": 40, "8x8 sub type 3": 36}
    for k, f in floors.items():
        assert count.get(k, 0) >= f, (k, count.get(k, 0), f)
    x = sn.NbOracle(fo)
    assert all(x.derive(j)["fits"] == 1 for j in jobs[::9])
    for name, j in sn.OVERFLOW_JOBS:
        r = x.derive(j)
        assert r["fits"] == 0 and (np.abs(r["mv"]) > 32767).sum() >= 1, name
    x.close()
