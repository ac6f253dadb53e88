"""Known-answer tests of the macroblock residual layer in both directions (rows a13 and a19 of SURVEY.md 8a between block
and slice): residual_write() (F/residual.cpp:300) through the encoder's block order and cavlc_nC, residual(0, 15) (:959)
through the decoder's dec_block and dec_nC, with nC DERIVED from arbitrary neighbour states, against the oracle's
fo_residual_write / fo_residual_parse on the same state."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_SKIP = 31
LEVELS = (("lumaLevel", 256), ("dc16", 16), ("ac16", 256), ("cdc", 8), ("cac", 128))


class _BW(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("cap", C.c_size_t), ("nbits", C.c_size_t)]


class _BR(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def _levels(rng, n, maxn):
    """n level vectors as a quantiser leaves them (the kinds of test_cavlc_block_writer_kat's _random_levels, drawn for all
    blocks at once): empty, sparse to full, +-1 only, with an escape-coded level"""
    kind = rng.integers(0, 6, n)[:, None]
    mask = rng.random((n, 16)) < rng.choice([0.1, 0.3, 0.6, 1.0], n)[:, None]
    mag = rng.choice([1, 1, 1, 2, 3, 8, 40, 300, 2000], n)[:, None]
    sign = rng.choice([-1, 1], (n, 16))
    v = np.where(kind == 1, 1, rng.integers(1, mag + 1, (n, 16))) * sign
    esc = (np.arange(16)[None, :] == rng.integers(0, maxn, n)[:, None]) & (kind == 2)
    v = np.where(esc, sign * rng.integers(16, 2040, (n, 1)), v)
    c = np.where((mask | esc) & (kind != 0) & (np.arange(16)[None, :] < maxn), v, 0)
    return c.astype(np.int32)


class _Ctx:
    """an oracle context with its per-macroblock state as writable arrays"""

    def __init__(self, fo, W, H):
        self.o = fo.Oracle(W, H)
        L, c, n = self.o.L, self.o.c, self.o.nmb
        vp, i = C.c_void_p, C.c_int
        L.fo_residual_write.argtypes = [vp, vp]
        L.fo_residual_write.restype = None
        L.fo_residual_parse.argtypes = [vp, vp]
        L.fo_residual_parse.restype = i
        L.fo_setCodedBlockPattern.argtypes = [vp]
        L.fo_setCodedBlockPattern.restype = None
        L.fo_cavlc_nC.argtypes = [vp, i, i, i]
        L.fo_cavlc_nC.restype = i
        self.L, self.c = L, c
        self.mbt = fo._arr(L.fo_dbg_mb_type(c), n, np.int32)
        self.cbp_l, self.cbp_c = fo._arr(L.fo_dbg_cbp(c, 0), n, np.int32), fo._arr(L.fo_dbg_cbp(c, 1), n, np.int32)
        self.tc_l = fo._arr(L.fo_dbg_tc_l(c), n * 16, np.int32).reshape(n, 16)
        self.tc_c = fo._arr(L.fo_dbg_tc_c(c), n * 8, np.int32).reshape(n, 8)

    def write(self):
        buf = np.zeros(4096, np.uint8)
        w = _BW(buf.ctypes.data, buf.size, 0)
        self.L.fo_residual_write(self.c, C.byref(w))
        return buf, int(w.nbits)

    def parse(self, stream, bit_pos):
        r = _BR(stream.ctypes.data, stream.size, bit_pos)
        ok = self.L.fo_residual_parse(self.c, C.byref(r))
        return ok, int(r.pos) - bit_pos


def _mb_type_of(rng, cls, slice_type):
    """an mb_type with MbPartPredMode(mb_type, 0) == cls in that slice type (F/h264_globals.cpp:25-132)"""
    if slice_type == 2:
        assert cls != 2
        return 0 if cls == 0 else int(rng.integers(1, 25))
    return 5 if cls == 0 else int(rng.integers(6, 30)) if cls == 1 else int(rng.integers(0, 5))


def _draw_levels(rng, cls):
    lv = {k: np.zeros(n, np.int32) for k, n in LEVELS}
    live8 = np.repeat(rng.random(4) < 0.65, 4)[:, None]       # whole 8x8 quadrants without levels: every CBP pattern
    if cls == 1:
        lv["dc16"] = _levels(rng, 1, 16)[0]
        lv["ac16"] = np.where(live8 & (rng.random() < 0.7), _levels(rng, 16, 15), 0).reshape(-1)
    else:
        lv["lumaLevel"] = np.where(live8, _levels(rng, 16, 16), 0).reshape(-1)
    chroma = rng.integers(0, 3)                                # none, DC only, DC and AC
    if chroma >= 1:
        lv["cdc"] = _levels(rng, 2, 4)[:, :4].reshape(-1)
    if chroma == 2:
        lv["cac"] = _levels(rng, 8, 15).reshape(-1)
    return lv


def _nb(x, m):
    return dict(p_skip=int(x["mbt"][m] == P_SKIP), cbp_luma=int(x["cbp_l"][m]), cbp_chroma=int(x["cbp_c"][m]), tc_luma=x["tc_l"][m], tc_chroma=x["tc_c"][m])


def test_residual_write_and_parse_kat(pkg, fo):
    W = H = 48                                                 # 3 x 3 macroblocks: every availability pattern by position
    mbw, nmb = 3, 9
    rng = np.random.default_rng(31)
    x = _Ctx(fo, W, H)
    N = 1512
    jobs, refs = [], []
    seen_pairs, seen_nc = set(), set()
    n_skip_nb = n_gated_nb = 0
    for it in range(N):
        cur, cls = it % nmb, (it // nmb) % 3                   # every (position, cls) pair, 56 times
        slice_type = 0 if cls == 2 else int(rng.choice([0, 2]))   # (an inter macroblock lives in a P slice; intra ones in either)
        seen_pairs.add((cur, cls))
        # the neighbours: any macroblock type, any CBP, any counts -- states no encoder need ever have produced together
        x.mbt[:] = rng.choice([P_SKIP, 1, 5 if slice_type == 0 else 0, 12], nmb)
        x.cbp_l[:] = rng.integers(0, 16, nmb)
        x.cbp_c[:] = rng.integers(0, 3, nmb)
        x.tc_l[:] = rng.integers(0, 17, (nmb, 16))
        x.tc_c[:] = rng.integers(0, 17, (nmb, 8))
        x.tc_l[cur], x.tc_c[cur] = 0, 0                        # (residual_write leaves the entries of blocks it does not code as they were)
        lv = _draw_levels(rng, cls)
        x.o.set_mb(cur, _mb_type_of(rng, cls, slice_type), slice_type, 20)
        x.o.set_levels(**lv)
        x.L.fo_setCodedBlockPattern(x.c)                        # -> cbp_l[cur], cbp_c[cur]: blocks inside the macroblock read them
        state = dict(mbt=x.mbt.copy(), cbp_l=x.cbp_l.copy(), cbp_c=x.cbp_c.copy(), tc_l=x.tc_l.copy(), tc_c=x.tc_c.copy())
        cbpL, cbpC = int(x.cbp_l[cur]), int(x.cbp_c[cur])
        availA, availB = cur % mbw != 0, cur >= mbw
        avail = int(availA) | (int(availB) << 1)
        # coverage: nC of the blocks whose neighbours lie outside the macroblock (luma block 0, chroma AC block 0)
        src = {1: "A", 2: "B", 3: "AB"}.get(avail)
        for kind, coded in ((0 if cls == 1 else 2, cls == 1 or cbpL & 1), (4, cbpC & 2)):
            if coded and src:
                nC = x.L.fo_cavlc_nC(x.c, kind, 0, 0)
                seen_nc.add((src, 0 if nC <= 1 else 1 if nC <= 3 else 2 if nC <= 7 else 3))
        for ok, m, blk in ((availA, cur - 1, 5), (availB, cur - mbw, 10)):
            if ok:
                n_skip_nb += int(x.mbt[m] == P_SKIP)
                n_gated_nb += int(x.mbt[m] != P_SKIP and not (x.cbp_l[m] >> (blk // 4)) & 1 and x.tc_l[m, blk] > 0)
        # WRITE on the oracle, then PARSE of its bits at a random bit position on a fresh copy of the same state
        wbits, nbits = x.write()
        assert nbits <= pkg.ferhip.RES_BITS_MAX * 8
        w_tc = (x.tc_l[cur].copy(), x.tc_c[cur].copy())
        for k in state:
            getattr(x, k)[:] = state[k]
        x.o.set_levels(**{k: np.full(n, 77, np.int32) for k, n in LEVELS})   # (parsed or cleared: never read)
        bit_pos = int(rng.integers(0, 32))
        stream = np.packbits(np.concatenate([rng.integers(0, 2, bit_pos).astype(np.uint8), np.unpackbits(wbits)[:nbits]]))
        if stream.size == 0:
            stream = np.zeros(1, np.uint8)                     # (a macroblock without residual: nothing to read, but a stream has a byte)
            bit_pos = 0
        ok, used = x.parse(stream, bit_pos)
        assert ok and used == nbits, (it, ok, used, nbits)
        nb = (_nb(state, cur - 1) if availA else None, _nb(state, cur - mbw) if availB else None)
        common = dict(cls=cls, cbp_luma=cbpL, cbp_chroma=cbpC, avail=avail, nb=nb)
        jobs.append(dict(op=pkg.RES_WRITE, **common, **lv))
        jobs.append(dict(op=pkg.RES_PARSE, **common, bits=stream, bit_pos=bit_pos))
        refs.append(dict(cls=cls, cbpL=cbpL, cbpC=cbpC, nbits=nbits, wbits=wbits[:(nbits + 7) // 8].copy(), w_tc=w_tc, lv=lv, p_lv=x.o.levels(),
                         p_tc=(x.tc_l[cur].copy(), x.tc_c[cur].copy())))
    x.o.close()
    # coverage was reached
    assert seen_pairs == {(p, c) for p in range(nmb) for c in range(3)}
    assert seen_nc == {(s, k) for s in ("A", "B", "AB") for k in range(4)}, sorted(seen_nc)
    assert n_skip_nb > 0 and n_gated_nb > 0
    res = pkg.residual_mbs(jobs)
    for it, ref in enumerate(refs):
        w, p = res[2 * it], res[2 * it + 1]
        tag = (it, ref["cls"], ref["cbpL"], ref["cbpC"])
        assert w["nbits"] == ref["nbits"], tag
        assert w["bits"][:(ref["nbits"] + 7) // 8].tobytes() == ref["wbits"].tobytes(), tag
        assert not w["bits"][(ref["nbits"] + 7) // 8:].any(), tag
        assert np.array_equal(w["tc_luma"], ref["w_tc"][0]) and np.array_equal(w["tc_chroma"], ref["w_tc"][1]), (tag, w["tc_luma"], ref["w_tc"][0])
        assert p["nbits"] == ref["nbits"], tag
        assert np.array_equal(p["tc_luma"], ref["p_tc"][0]) and np.array_equal(p["tc_chroma"], ref["p_tc"][1]), (tag, p["tc_luma"], ref["p_tc"][0])
        want = ref["p_lv"]
        if ref["cls"] == 1:
            assert np.array_equal(p["dc16"], want["dc16"]), tag
            assert np.array_equal(p["ac16"].reshape(16, 16)[:, :15], want["ac16"].reshape(16, 16)[:, :15]), tag
        else:
            assert np.array_equal(p["lumaLevel"], want["lumaLevel"]), tag
        assert np.array_equal(p["cdc"], want["cdc"]), tag
        assert np.array_equal(p["cac"].reshape(8, 16)[:, :15], want["cac"].reshape(8, 16)[:, :15]), tag
        # and the parse gives back what was written
        src = ref["lv"]
        assert np.array_equal(p["lumaLevel"], src["lumaLevel"]) and np.array_equal(p["dc16"], src["dc16"]) and np.array_equal(p["cdc"], src["cdc"]), tag
        assert np.array_equal(p["ac16"].reshape(16, 16)[:, :15], src["ac16"].reshape(16, 16)[:, :15]), tag
        assert np.array_equal(p["cac"].reshape(8, 16)[:, :15], src["cac"].reshape(8, 16)[:, :15]), tag


def test_residual_under_the_reference_names(pkg, fo):
    """residual_write() and residual(0, 15) on the reference's globals for a row of three macroblocks (the second and third
    derive nC from the one before), against the same oracle calls; residual(3, 15) leaves the state alone."""
    lib = pkg.load_library()
    W, H, nmb = 48, 16, 3
    rng = np.random.default_rng(8)

    class Frame(C.Structure):
        _fields_ = [("Lwidth", C.c_int), ("Lheight", C.c_int), ("Cwidth", C.c_int), ("Cheight", C.c_int), ("L", C.c_void_p), ("C", C.c_void_p * 2)]

    def gint(name):
        return C.c_int.in_dll(lib, name)

    def garr(name, n):
        return np.frombuffer((C.c_int * n).in_dll(lib, name), np.int32)

    MAX = 10000                                                # FERHIP_LEGACY_MAX_MBS
    G = dict(lumaLevel=garr("LumaLevel", 256), dc16=garr("Intra16x16DCLevel", 16), ac16=garr("Intra16x16ACLevel", 256), cdc=garr("ChromaDCLevel", 8),
             cac=garr("ChromaACLevel", 128))
    mbt_g, tcl_g, tcc_g = garr("mb_type_array", MAX), garr("totalcoeff_array_luma", MAX * 16).reshape(MAX, 16), garr("totalcoeff_array_chroma", 2 * MAX * 4).reshape(2, MAX, 4)
    nbits_g, pos_g = C.c_uint.in_dll(lib, "ferhip_legacy_nbits"), C.c_uint.in_dll(lib, "ferhip_legacy_bitpos")
    buf = (C.c_ubyte * (1 << 16)).in_dll(lib, "ferhip_legacy_bits")
    frame = Frame.in_dll(lib, "frame")
    saved = (frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight, nbits_g.value, pos_g.value, gint("CurrMbAddr").value, gint("mb_type").value,
             gint("ferhip_legacy_slice_type").value)
    frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight = W, H, W // 2, H // 2
    x = _Ctx(fo, W, H)
    try:
        lib.AllocateMemory()
        cbpl_g = np.ctypeslib.as_array(C.POINTER(C.c_int).in_dll(lib, "CodedBlockPatternLumaArray"), shape=(nmb,))
        cbpc_g = np.ctypeslib.as_array(C.POINTER(C.c_int).in_dll(lib, "CodedBlockPatternChromaArray"), shape=(nmb,))
        mbs = [(2, 1, 3), (0, 2, 1), (2, 0, 0)]               # (slice type, cls, mb_type): Intra16x16, inter, Intra4x4
        lvs, ends = [], []
        obuf = np.zeros(8192, np.uint8)
        ow = _BW(obuf.ctypes.data, obuf.size, 0)
        nbits_g.value = 0
        tcl_g[:nmb], tcc_g[:, :nmb] = 0, 0
        x.tc_l[:], x.tc_c[:] = 0, 0
        for cur, (slice_type, cls, t) in enumerate(mbs):
            lv = _draw_levels(rng, cls)
            while not (lv["cac"].any() and (lv["ac16"].any() or lv["lumaLevel"].any())):   # luma and chroma AC in every one: nC matters
                lv = _draw_levels(rng, cls)
            lvs.append(lv)
            x.o.set_mb(cur, t, slice_type, 20)
            x.o.set_levels(**lv)
            x.L.fo_setCodedBlockPattern(x.c)
            x.L.fo_residual_write(x.c, C.byref(ow))
            ends.append(int(ow.nbits))
            # the same through the reference's names: the caller's part (mb_type_array, setCodedBlockPattern), then residual_write()
            gint("CurrMbAddr").value, gint("mb_type").value, gint("ferhip_legacy_slice_type").value = cur, t, slice_type
            for k in G:
                G[k][:] = lv[k]
            mbt_g[cur] = t
            gint("CodedBlockPatternLuma").value, gint("CodedBlockPatternChroma").value = int(x.cbp_l[cur]), int(x.cbp_c[cur])
            cbpl_g[cur], cbpc_g[cur] = x.cbp_l[cur], x.cbp_c[cur]
            lib.residual_write()
            assert nbits_g.value == ends[-1], cur
            assert bytes(buf[:(ends[-1] + 7) // 8]) == obuf[:(ends[-1] + 7) // 8].tobytes(), cur
            assert np.array_equal(tcl_g[cur], x.tc_l[cur]) and np.array_equal(tcc_g[:, cur].reshape(-1), x.tc_c[cur]), cur
        assert ends[0] > 0 and ends[1] > ends[0] and ends[2] > ends[1]
        # back: residual(0, 15) per macroblock from the cursor, against fo_residual_parse on the same bits
        pos_g.value = 0
        tcl_g[:nmb], tcc_g[:, :nmb] = 0, 0
        x.tc_l[:], x.tc_c[:] = 0, 0
        start = 0
        for cur, (slice_type, cls, t) in enumerate(mbs):
            x.o.set_mb(cur, t, slice_type, 20)
            x.o.set_levels(**lvs[cur])
            x.L.fo_setCodedBlockPattern(x.c)                    # (the macroblock layer's coded_block_pattern)
            x.o.set_levels(**{k: np.full(n, 55, np.int32) for k, n in LEVELS})
            ok, used = x.parse(obuf, start)
            assert ok and start + used == ends[cur]
            want = x.o.levels()
            gint("CurrMbAddr").value, gint("mb_type").value, gint("ferhip_legacy_slice_type").value = cur, t, slice_type
            gint("CodedBlockPatternLuma").value, gint("CodedBlockPatternChroma").value = int(x.cbp_l[cur]), int(x.cbp_c[cur])
            for k in G:
                G[k][:] = 55
            if cur == 1:                                        # only (0, 15) is supported: anything else leaves the state alone
                lib.residual(3, 15)
                assert pos_g.value == start and all((G[k] == 55).all() for k in G) and not tcl_g[cur].any()
            lib.residual(0, 15)
            assert pos_g.value == ends[cur], cur
            if cls == 1:
                assert np.array_equal(G["dc16"], want["dc16"]) and np.array_equal(G["ac16"].reshape(16, 16)[:, :15], want["ac16"].reshape(16, 16)[:, :15]), cur
                assert np.array_equal(G["dc16"], lvs[cur]["dc16"])
            else:
                assert np.array_equal(G["lumaLevel"], want["lumaLevel"]) and np.array_equal(G["lumaLevel"], lvs[cur]["lumaLevel"]), cur
            assert np.array_equal(G["cdc"], want["cdc"]) and np.array_equal(G["cac"].reshape(8, 16)[:, :15], want["cac"].reshape(8, 16)[:, :15]), cur
            assert np.array_equal(tcl_g[cur], x.tc_l[cur]) and np.array_equal(tcc_g[:, cur].reshape(-1), x.tc_c[cur]), cur
            start = ends[cur]
        # CurrMbAddr is checked against the macroblocks AllocateMemory sized: nothing moves
        gint("CurrMbAddr").value = nmb
        lib.residual(0, 15)
        lib.residual_write()
        assert pos_g.value == ends[2] and nbits_g.value == ends[2]
    finally:
        x.o.close()
        (frame.Lwidth, frame.Lheight, frame.Cwidth, frame.Cheight, nbits_g.value, pos_g.value, gint("CurrMbAddr").value, gint("mb_type").value,
         gint("ferhip_legacy_slice_type").value) = saved
