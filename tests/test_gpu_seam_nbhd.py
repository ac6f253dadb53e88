"""Known-answer tests of the neighbourhood seam (ferhip_intra_mbs, ferhip_mv_mbs of include/ferhip.h): intra prediction
(rows a10, a11, a12 of DESIGN.md) and motion-vector derivation (row a18) of ONE macroblock among hand-made neighbours, bit
for bit against the oracle's fo_intraPredictionEncoding / fo_intraPrediction_dec / fo_DeriveMVs on the same state
(tests/seam_nbhd.py).  What the jobs reach is counted, on the oracle alone, by tests/test_seam_nbhd_host.py."""
import ctypes as C

import numpy as np
import pytest

import seam_nbhd as sn

pytestmark = pytest.mark.gpu

ENC_FIELDS = ("ret", "mb_type", "cbp_luma", "cbp_chroma", "chroma_mode", "mbsize", "i4mode", "prev_flag", "tc_luma", "tc_chroma", "lumaLevel", "dc16",
              "ac16", "cdc", "cac", "recY", "recCb", "recCr", "predL", "predCb", "predCr")
DEC_FIELDS = ("i4mode", "predL", "predCb", "predCr", "recY", "recCb", "recCr")
_cache = {}


def _encode_run(pkg, fo):
    """the ENCODE jobs, the oracle's results and the device's: computed once, shared by the tests below, left unchanged"""
    if "enc" not in _cache:
        jobs = sn.encode_jobs(11, 64)                  # 6 positions x 5 QPs x 64
        x = sn.NbOracle(fo)
        refs = [x.encode(j) for j in jobs]
        x.close()
        _cache["enc"] = (jobs, refs, pkg.ferhip.intra_mbs(jobs))
    return _cache["enc"]


def _same(got, ref, fields, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        for f in fields:
            assert np.array_equal(np.asarray(g[f]), np.asarray(r[f])), (what, k, f, g[f], r[f])


def test_intra_encode_kat(pkg, fo):
    jobs, refs, got = _encode_run(pkg, fo)
    assert len(jobs) == 6 * 5 * 64
    _same(got, refs, ENC_FIELDS, "encode")
    for k, (g, r) in enumerate(zip(got, refs)):
        nf = r["prev_flag"] == 0                       # rem_intra4x4_pred_mode exists where the flag is 0
        assert np.array_equal(g["rem_mode"][nf], r["rem_mode"][nf]), k
        # the oracle's own TotalCoeff arrays, on the blocks its writer coded
        sent = np.concatenate([np.repeat([(r["cbp_luma"] >> i8) & 1 for i8 in range(4)], 4), np.full(8, r["cbp_chroma"] == 2)]).astype(bool)
        tc = np.concatenate([g["tc_luma"], g["tc_chroma"]])
        assert np.array_equal(tc[sent], r["tc_written"][sent]), k
        assert not tc[~sent].any(), k
    assert {r["ret"] for r in refs} == {-1, 0, 1, 2, 3}


def test_intra_decode_kat(pkg, fo):
    jobs, refs, got = _encode_run(pkg, fo)
    x = sn.NbOracle(fo)
    # what the encoder coded, decoded: prediction and reconstruction must come back
    back = [sn.decode_job_of(j, g) for j, g in zip(jobs, got)]
    dec = pkg.ferhip.intra_mbs(back)
    for k, (d, g, r) in enumerate(zip(dec, got, refs)):
        for f in ("predL", "predCb", "predCr", "recY", "recCb", "recCr"):
            assert np.array_equal(d[f], g[f]), ("round trip", k, f)
        if r["ret"] == -1:
            assert np.array_equal(d["i4mode"], g["i4mode"]), ("round trip", k)
    _same(dec[::7], [x.decode(j) for j in back[::7]], DEC_FIELDS, "decode of encode")
    # the generator's own jobs: P and I slices, both constrained_intra values, chroma_qp_offset, every kind of neighbour
    own = sn.decode_jobs(12, 1800)
    assert {(j["slice_type"], j["constrained_intra"]) for j in own} == {(0, 0), (0, 1), (2, 0), (2, 1)}
    assert sum(j["chroma_qp_offset"] != 0 for j in own) > 900
    _same(pkg.ferhip.intra_mbs(own), [x.decode(j) for j in own], DEC_FIELDS, "decode")
    x.close()


def test_intra_mixed_batch(pkg, fo):
    """ENCODE and DECODE jobs in ONE call, every pos under both ops twice, submitted in descending pos with the ops
    alternating: the call sorts them into runs of one (op, pos), launches each run on its range of streams and scatters the
    results back.  Every result is the oracle's, and the one the same job gets when it is submitted alone."""
    F = pkg.ferhip
    enc = [j for j in sn.encode_jobs(21, 1) if j["qp"] in (sn.ENC_QPS[0], sn.ENC_QPS[-1])]
    dec = sn.decode_jobs(22, 12)
    assert len(enc) == len(dec) == 12
    jobs = []
    for pos in range(5, -1, -1):
        for e, d in zip([j for j in enc if j["pos"] == pos], [j for j in dec if j["pos"] == pos]):
            jobs += [e, d]
    assert len(jobs) == 24 and [j["op"] for j in jobs] == [F.INTRA_ENCODE, F.INTRA_DECODE] * 12
    assert [j["pos"] for j in jobs] == [p for p in range(5, -1, -1) for _ in range(4)]
    got = F.intra_mbs(jobs)
    xe, xd = sn.NbOracle(fo), sn.NbOracle(fo)
    for k, (j, g) in enumerate(zip(jobs, got)):
        if j["op"] == F.INTRA_ENCODE:
            _same([g], [xe.encode(j)], ENC_FIELDS, ("mixed encode", k))
        else:
            _same([g], [xd.decode(j)], DEC_FIELDS, ("mixed decode", k))
        alone = F.intra_mbs([j])[0]
        assert alone.keys() == g.keys()
        for f in g:
            assert np.array_equal(np.asarray(g[f]), np.asarray(alone[f])), ("alone", k, f)
    xe.close()
    xd.close()


def test_mv_kat(pkg, fo):
    F = pkg.ferhip
    x = sn.NbOracle(fo)
    jobs = sn.mv_jobs(13, 2880)                        # 6 positions x 6 types x 80
    got = F.mv_mbs(jobs)
    for k, (j, g) in enumerate(zip(jobs, got)):
        r = x.derive(j)
        assert g["fits"] == r["fits"] == 1, k
        assert np.array_equal(g["mv"], r["mv"]), (k, j["pos"], j["mb_type"], g["mv"], r["mv"])
    # the encoder's direction, and back
    pj = sn.predict_jobs(14, 1500)
    pg = F.mv_mbs(pj)
    again = F.mv_mbs([dict(j, op=F.MV_DERIVE, mvd=g["mvd"]) for j, g in zip(pj, pg)])
    for k, (j, g, a) in enumerate(zip(pj, pg, again)):
        assert a["fits"] == 1 and np.array_equal(a["mv"], np.asarray(j["mv"])), (k, j["pos"], j["mb_type"], g["mvd"], a["mv"], j["mv"])
        assert np.array_equal(x.derive(j, mvd=g["mvd"])["mv"], np.asarray(j["mv"])), k
        np_ = {0: 1, 1: 2, 2: 2}.get(j["mb_type"], 4)
        assert not g["mvd"][2 * np_:].any(), k
    # results that leave 16 bits: the reference keeps ints, the device refuses
    for (name, j), g in zip(sn.OVERFLOW_JOBS, F.mv_mbs([j for _, j in sn.OVERFLOW_JOBS])):
        assert x.derive(j)["fits"] == 0, name
        assert g["fits"] == 0, name
    x.close()


class _Frame(C.Structure):
    _fields_ = [("Lwidth", C.c_int), ("Lheight", C.c_int), ("Cwidth", C.c_int), ("Cheight", C.c_int), ("L", C.c_void_p), ("C", C.c_void_p * 2)]


def _cut(cur, mbw, mbh):
    """pos of macroblock cur of an mbw x mbh picture and the picture address of every macroblock of its 3 x 2 neighbourhood
    (-1 outside the picture): the rule of include/ferhip_legacy.h"""
    mbx, mby = cur % mbw, cur // mbw
    A, B, last = mbx > 0, mby > 0, mbx == mbw - 1
    pos = (3 if not A else 5 if last else 4) if B else (0 if not A else 2 if last else 1)
    ox, oy = mbx - pos % 3, mby - pos // 3
    win = [(oy + m // 3) * mbw + ox + m % 3 if 0 <= ox + m % 3 < mbw and 0 <= oy + m // 3 < mbh else -1 for m in range(6)]
    return pos, win


def test_reference_names(pkg, fo):
    """intraPredictionEncoding, intraPrediction, DeriveMVs and ClearMVD on the reference's globals (include/ferhip_legacy.h),
    every macroblock of a 48 x 32 and of a 32 x 32 `frame`, against the batched calls on the neighbourhood cut out by hand; a
    `frame` one macroblock wide is refused."""
    F = pkg.ferhip
    lib = pkg.load_library()
    rng = np.random.default_rng(15)
    MAX = 10000                                                # FERHIP_LEGACY_MAX_MBS

    def gint(name):
        return C.c_int.in_dll(lib, name)

    def garr(name, n, ct=C.c_int, dt=np.int32):
        return np.frombuffer((ct * n).in_dll(lib, name), dt)

    def gptr(name, n):
        return np.ctypeslib.as_array(C.POINTER(C.c_int).in_dll(lib, name), shape=(n,))

    lib.intraPredictionEncoding.argtypes = lib.intraPrediction.argtypes = [C.c_void_p] * 3
    lib.intraPredictionEncoding.restype = C.c_int
    lib.intraPrediction.restype = lib.DeriveMVs.restype = lib.ClearMVD.restype = None
    frame = _Frame.in_dll(lib, "frame")
    mbt_g, tcl_g, tcc_g = garr("mb_type_array", MAX), garr("totalcoeff_array_luma", MAX * 16).reshape(MAX, 16), garr("totalcoeff_array_chroma", 2 * MAX * 4).reshape(2, MAX, 4)
    flag_g, rem_g, ll_g = garr("prev_intra4x4_pred_mode_flag", 16, C.c_ubyte, np.uint8), garr("rem_intra4x4_pred_mode", 16), garr("LumaLevel", 256)
    mvd_g, sub_g, size_g = garr("mvd_l0", 32).reshape(4, 4, 2), garr("sub_mb_type", 4), garr("ferhip_legacy_mbsize", 2)
    names = ("CurrMbAddr", "QPy", "mb_type", "ferhip_legacy_slice_type", "ferhip_legacy_constrained_intra_pred", "intra_chroma_pred_mode")
    saved = (frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight, frame.L, frame.C[0], frame.C[1], [gint(n).value for n in names])
    pL, pCr, pCb = np.zeros(256, np.int32), np.zeros(64, np.int32), np.zeros(64, np.int32)
    try:
        for (W, H) in ((48, 32), (32, 32)):
            mbw, mbh = W // 16, H // 16
            nmb = mbw * mbh
            src = sn._sources()[1]
            pic = [np.ascontiguousarray(src[0][16:16 + H, 32:32 + W]), np.ascontiguousarray(src[1][8:8 + H // 2, 16:16 + W // 2]),
                   np.ascontiguousarray(src[2][8:8 + H // 2, 16:16 + W // 2])]
            buf = [p.copy() for p in pic]
            frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight = W, H, W // 2, H // 2
            frame.L, frame.C[0], frame.C[1] = (b.ctypes.data for b in buf)
            lib.AllocateMemory()
            cbpl_g, cbpc_g, i4_g, ref_g = gptr("CodedBlockPatternLumaArray", nmb), gptr("CodedBlockPatternChromaArray", nmb), gptr("Intra4x4PredMode", nmb * 16).reshape(nmb, 16), gptr("refIdxL0", nmb)
            mvx = C.POINTER(C.POINTER(C.POINTER(C.c_int))).in_dll(lib, "mvL0x")
            mvy = C.POINTER(C.POINTER(C.POINTER(C.c_int))).in_dll(lib, "mvL0y")

            def put_state(states):
                for r, n in enumerate(states):
                    mbt_g[r], cbpl_g[r], cbpc_g[r] = n["mb_type"], n["cbp_luma"], n["cbp_chroma"]
                    tcl_g[r], tcc_g[:, r], i4_g[r] = n["tc_luma"], n["tc_chroma"].reshape(2, 4), n["i4mode"]
                    for q in range(4):
                        for j in range(4):
                            mvx[r][q][j], mvy[r][q][j] = int(n["mv"][2 * q]), int(n["mv"][2 * q + 1])

            def job_of(cur, states, **kw):
                pos, win = _cut(cur, mbw, mbh)
                Y, U, V = np.zeros((32, 48), np.uint8), np.zeros((16, 24), np.uint8), np.zeros((16, 24), np.uint8)
                for m, r in enumerate(win):
                    if r >= 0:
                        x, y, wx, wy = (r % mbw) * 16, (r // mbw) * 16, (m % 3) * 16, (m // 3) * 16
                        Y[wy:wy + 16, wx:wx + 16] = buf[0][y:y + 16, x:x + 16]
                        U[wy // 2:wy // 2 + 8, wx // 2:wx // 2 + 8] = buf[1][y // 2:y // 2 + 8, x // 2:x // 2 + 8]
                        V[wy // 2:wy // 2 + 8, wx // 2:wx // 2 + 8] = buf[2][y // 2:y // 2 + 8, x // 2:x // 2 + 8]
                mb = [states[win[m]] if m < pos and win[m] >= 0 else None for m in range(6)]
                return dict(pos=pos, mb=mb, Y=Y, Cb=U, Cr=V, **kw)

            def mb_luma(cur):
                x, y = (cur % mbw) * 16, (cur // mbw) * 16
                return buf[0][y:y + 16, x:x + 16].astype(np.int32).ravel()

            for st in (2, 0):                                   # I states: ENCODE and its DECODE; P states: DECODE of the generator's kind, vectors
                states = [sn.nb_state(rng, st) for _ in range(nmb)]
                for cur in range(nmb):
                    for b, p in zip(buf, pic):
                        b[:] = p
                    put_state(states)
                    gint("CurrMbAddr").value, gint("QPy").value, gint("ferhip_legacy_slice_type").value = cur, 27, st
                    if st == 2:
                        stale = int(rng.choice([31, 0, 7]))
                        job = job_of(cur, states, op=F.INTRA_ENCODE, slice_type=2, qp=27)
                        job["mb"][job["pos"]] = dict(mb_type=stale)
                        want = F.intra_mbs([job])[0]
                        mbt_g[cur] = stale
                        ret = lib.intraPredictionEncoding(pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data)
                        assert ret == want["ret"] and gint("intra_chroma_pred_mode").value == want["chroma_mode"], (W, cur)
                        assert np.array_equal(pL, want["predL"]) and np.array_equal(pCb, want["predCb"]) and np.array_equal(pCr, want["predCr"]), (W, cur)
                        assert np.array_equal(i4_g[cur], want["i4mode"]) and np.array_equal(flag_g, want["prev_flag"]) and np.array_equal(size_g, want["mbsize"])
                        assert np.array_equal(rem_g[flag_g == 0], want["rem_mode"][flag_g == 0]) and mbt_g[cur] == 0
                        if ret == -1:
                            assert np.array_equal(mb_luma(cur), want["recY"]) and np.array_equal(ll_g, want["lumaLevel"]), (W, cur)
                        else:
                            assert np.array_equal(buf[0], pic[0]), (W, cur)
                        assert np.array_equal(buf[1], pic[1]) and np.array_equal(buf[2], pic[2])
                        djob = sn.decode_job_of(job, want)
                    else:
                        djob = None
                        for cand in sn.decode_jobs(100 + cur, 60):   # a legal job of the generator's for this pos, on this picture and state
                            if cand["pos"] == _cut(cur, mbw, mbh)[0] and cand["slice_type"] == 0:
                                djob = dict(cand, **job_of(cur, states, op=F.INTRA_DECODE, slice_type=0, qp=27))
                                djob["mb"][djob["pos"]] = cand["mb"][cand["pos"]]
                                djob["chroma_qp_offset"] = 0
                                if lib.ferhip_intra_mbs(F.nbhd_jobs([djob]), (F.IntraResult * 1)(), 1) == 0:   # legal among THESE neighbours too
                                    break
                        assert djob is not None
                    for b, p in zip(buf, pic):
                        b[:] = p
                    want = F.intra_mbs([djob])[0]
                    t = djob["mb"][djob["pos"]]["mb_type"]
                    gint("mb_type").value, gint("intra_chroma_pred_mode").value = t, djob["chroma_mode"]
                    gint("ferhip_legacy_constrained_intra_pred").value = djob["constrained_intra"]
                    flag_g[:], rem_g[:], ll_g[:] = djob["prev_flag"], djob["rem_mode"], djob["lumaLevel"]
                    i4_g[cur] = 0
                    lib.intraPrediction(pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data)
                    assert np.array_equal(pL, want["predL"]) and np.array_equal(pCb, want["predCb"]) and np.array_equal(pCr, want["predCr"]), (W, cur, st)
                    if t == (0 if st == 2 else 5):
                        assert np.array_equal(i4_g[cur], want["i4mode"]) and np.array_equal(mb_luma(cur), want["recY"]), (W, cur, st)
                    else:
                        assert np.array_equal(buf[0], pic[0])
                    if st == 0:                                  # DeriveMVs of every type at this macroblock
                        for t in (0, 1, 2, 3, 4, 31):
                            put_state(states)
                            mj = dict(op=F.MV_DERIVE, pos=djob["pos"], mb=djob["mb"], mb_type=t, sub_mb_type=rng.integers(0, 4, 4).astype(np.int32),
                                      mvd=rng.integers(-50, 51, 8).astype(np.int32))
                            want = F.mv_mbs([mj])[0]
                            assert want["fits"] == 1
                            gint("mb_type").value, sub_g[:] = t, mj["sub_mb_type"]
                            mvd_g[:] = 99
                            lib.ClearMVD()
                            assert not mvd_g.any()
                            mvd_g[:, 0] = mj["mvd"].reshape(4, 2)
                            ref_g[cur] = 5
                            lib.DeriveMVs()
                            got = np.array([[mvx[cur][q][j], mvy[cur][q][j]] for q in range(4) for j in range(4)]).reshape(4, 4, 2)
                            assert (got == want["mv"].reshape(4, 1, 2)).all() and ref_g[cur] == 0, (W, cur, t)
        # a picture one macroblock wide: the message, nothing moves
        frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight = 16, 32, 8, 16
        lib.AllocateMemory()
        i4_g = gptr("Intra4x4PredMode", 32)
        i4_g[:] = 7
        pL[:] = -5
        gint("CurrMbAddr").value, gint("mb_type").value = 1, 0
        assert lib.intraPredictionEncoding(pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data) == 0
        lib.intraPrediction(pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data)
        mvx = C.POINTER(C.POINTER(C.POINTER(C.c_int))).in_dll(lib, "mvL0x")
        mvx[1][0][0] = 1234
        lib.DeriveMVs()
        assert (i4_g == 7).all() and (pL == -5).all() and mvx[1][0][0] == 1234
    finally:
        frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight, frame.L, frame.C[0], frame.C[1] = saved[:7]
        for n, v in zip(names, saved[7]):
            gint(n).value = v
