"""Whole Annex-B streams written bit by bit, with real residual data: the decode twin's input chosen to break it.

Test infrastructure (plain Python + numpy, seeded, no GPU).  make_stream() writes SPS, PPS, IDR I slices and P slices
of any size in macroblocks: every macroblock type the decoder supports (I4x4 with all prev / rem combinations, the 24
I16x16 types, P_Skip runs, the five P types with all four sub types, types 5..29 = intra in P), intra modes that only
use neighbours that exist (the reference's decoder does not check; ILLEGAL_PLANS draw the others too), slice_qp_delta / mb_qp_delta over the whole QP
range, and the parameter-set fields dec_parse_sps / dec_parse_pps accept at other values than the encoder's.  The
header pieces (Bits, nal_unit, te_bits, the P slice header) are those of pslice_synth.py.

Residual blocks are random coefficient vectors written by fo_py.cavlc_encode_block (pinned to the reference's leaf
library by test_oracle.py) with the nC of this file's OWN model of the total-coefficient prediction (per-block
TotalCoeff of the left and upper neighbour; P_Skip and a clear cbp bit count 0; picture edges; chroma per plane --
the rules of F/residual.cpp:424-538).  test_slice_synth_host.py proves that model against the oracle's parse: one wrong
nC desynchronises the slice and the macroblock types no longer match the plan.

make_stream() also returns what it wrote (the coverage report, see new_coverage) and mb_type of every macroblock.
"""
import numpy as np

import fo_py
from pslice_synth import INTER_CBP, Bits, nal_unit, p_slice, te_bits

INTRA_CBP = [47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46, 16, 3, 5, 10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1,
             2, 4, 8, 17, 18, 20, 24, 6, 9, 22, 25, 32, 33, 34, 36, 40, 38, 41]  # Table 9-4, intra column
BLK_XY = [(0, 0), (4, 0), (0, 4), (4, 4), (8, 0), (12, 0), (8, 4), (12, 4),
          (0, 8), (4, 8), (0, 12), (4, 12), (8, 8), (12, 8), (8, 12), (12, 12)]  # (x, y) of luma block blk
BLK_AT = {xy: b for b, xy in enumerate(BLK_XY)}
P_SKIP = 31
KINDS = ("unavailable", "skip", "inter", "i4", "i16")
LEVEL_MODES = ("small", "mixed", "escape", "extreme")
TC_CLASSES = [(0, 1), (2, 3), (4, 7), (8, 16)]  # TotalCoeff ranges that put the neighbours into each coeff_token class


def new_coverage():
    return dict(
        coeff_token={c: set() for c in range(5)},  # class 0..2 (nC < 2, < 4, < 8), 3 = nC >= 8, 4 = chroma DC: (TotalCoeff, TrailingOnes)
        level_prefix=set(),           # (level_prefix, suffixLength it was written at)
        max_suffix_length=0,          # the largest suffixLength a level was written at
        start_suffix_1=False,         # a block with TotalCoeff > 10 and TrailingOnes < 3
        total_zeros={16: set(), 15: set(), 4: set()},  # per maxNumCoeff: (TotalCoeff, total_zeros)
        max_run_before=0,
        i4_modes=set(), i16_modes=set(), chroma_modes=set(),  # as derived
        i4_coding=set(),              # (prev_intra4x4_pred_mode_flag, rem_intra4x4_pred_mode or -1)
        intra_in_p=set(),             # (kind of the left, kind of the upper macroblock) of every I4x4 macroblock in a P slice
        mb_types={"I": set(), "P": set()}, sub_types=set(),
        qpy=set(), wrap_up=False, wrap_down=False)


def merge_coverage(a, b):
    for k, v in b.items():
        if isinstance(v, dict):
            for kk, s in v.items():
                a[k][kk] |= s
        elif isinstance(v, set):
            a[k] |= v
        elif isinstance(v, bool):
            a[k] = a[k] or v
        else:
            a[k] = max(a[k], v)
    return a


# ---------------------------------------------------------------------------------------------- coefficient levels

def _level_code_max(sl):
    """largest levelCode level_prefix <= 15 carries at suffixLength sl (escape: 12 suffix bits)"""
    return 30 + 4095 if sl == 0 else (15 << sl) + 4095


def _mag_max(sl, first):
    m = _level_code_max(sl) + (2 if first else 0)  # the first level after < 3 trailing ones is written as levelCode - 2
    return (m + 1) // 2  # negative levels: levelCode = 2 |l| - 1


def _next_sl(sl, mag):
    if sl == 0:
        sl = 1
    if mag > (3 << (sl - 1)) and sl < 6:
        sl += 1
    return sl


_T1_P = dict(small=[.1, .2, .3, .4], mixed=[.25, .25, .25, .25], escape=[.4, .2, .2, .2], extreme=[.5, .2, .2, .1])


def gen_levels(rng, tc, mode, amp):
    """tc levels in coding order (highest frequency first).  amp bounds |level| in the small / mixed modes."""
    t1 = min(int(rng.choice(4, p=_T1_P[mode])), tc)
    lv = [int(rng.choice([-1, 1])) for _ in range(t1)]
    sl = 1 if (tc > 10 and t1 < 3) else 0
    for i in range(t1, tc):
        first = i == t1 and t1 < 3
        lo, hi = (2 if first else 1), _mag_max(sl, first)  # |level| 1 here would be one more trailing one
        r = rng.random()
        if mode == "small":
            m = lo if r < 0.6 else int(rng.integers(lo, 4))
            m = min(m, max(lo, min(3, amp)))
        elif mode == "mixed":
            m = lo if r < 0.5 else int(rng.integers(lo, 4)) if r < 0.8 else int(rng.integers(4, 16)) if r < 0.95 else int(rng.integers(16, 41))
            m = min(m, max(lo, amp))
        elif mode == "escape":
            if i == t1:
                m = int(rng.integers(8, 48))  # level_prefix 14 and 15 at suffixLength 0
            elif sl < 6:
                m = int(rng.integers((3 << (sl - 1)) + 1, 9 << (sl - 1))) if r < 0.75 else int(rng.integers(1, 2000))  # the climb
            else:
                m = int(rng.integers(481, 1500)) if r < 0.3 else int(rng.integers(1, 120))  # level_prefix 15 at suffixLength 6
        else:
            m = hi if r < 0.6 else int(rng.integers(hi // 2, hi + 1))
        m = max(lo, min(m, hi))
        lv.append(m if rng.random() < 0.5 else -m)
        sl = _next_sl(sl, m)
    return lv


def gen_block(rng, n, tc, mode, amp):
    """a coefficient vector of n entries with tc non-zero ones"""
    coef = [0] * n
    if tc:
        pos = sorted((int(p) for p in rng.choice(n, size=tc, replace=False)), reverse=True)
        for p, l in zip(pos, gen_levels(rng, tc, mode, amp)):
            coef[p] = l
    return coef


def analyze_block(coef, n):
    """What residual_block_cavlc writes for coef[0..n): TotalCoeff, TrailingOnes, the (level_prefix, suffixLength) pairs,
    total_zeros and the runs -- for the coverage report only; the bits come from the oracle's writer."""
    nz = [i for i in range(n - 1, -1, -1) if coef[i]]
    tc = len(nz)
    t1 = 0
    for i in nz[:3]:
        if abs(coef[i]) != 1:
            break
        t1 += 1
    out = dict(tc=tc, t1=t1, prefixes=[], tz=None, runs=[])
    if not tc:
        return out
    sl = 1 if (tc > 10 and t1 < 3) else 0
    for k, i in enumerate(nz[t1:]):
        l = coef[i]
        lc = -2 * l - 1 if l < 0 else 2 * l - 2
        if k == 0 and t1 < 3:
            lc -= 2
        if sl == 0:
            prefix = lc if lc < 14 else (14 if lc < 30 else 15)
        else:
            prefix = min(lc >> sl, 15)
        assert lc <= _level_code_max(sl), "level not expressible"
        out["prefixes"].append((prefix, sl))
        sl = _next_sl(sl, abs(l))
    if tc < n:
        out["tz"] = nz[0] + 1 - tc
    runs = [nz[k] - nz[k + 1] - 1 for k in range(tc - 1)]
    zl = out["tz"] if tc < n else 0
    for r in runs:  # run_before is written while zeros are left
        if zl > 0:
            out["runs"].append(r)
        zl -= r
    return out


# ---------------------------------------------------------------------------------------------- parameter sets

CFG_DEFAULT = dict(mbw=11, mbh=9, log2_max_frame_num=9, log2_max_poc_lsb=10, pic_init_qp=26, chroma_qp_index_offset=0,
                   deblocking_control=0, constrained_intra_pred=0)


def sps_rbsp(cfg):
    w = Bits()
    w.put(8, 66)
    w.put(8, 0xC0)
    w.put(8, 41)
    w.ue(0)
    w.ue(cfg["log2_max_frame_num"] - 4)
    w.ue(0)  # pic_order_cnt_type
    w.ue(cfg["log2_max_poc_lsb"] - 4)
    w.ue(1)  # max_num_ref_frames
    w.put(1, 0)
    w.ue(cfg["mbw"] - 1)
    w.ue(cfg["mbh"] - 1)
    w.put(1, 1)  # frame_mbs_only_flag
    w.put(1, 1)
    w.put(1, 0)  # frame_cropping_flag
    w.put(1, 0)
    return w.rbsp(0)


def pps_rbsp(cfg):
    w = Bits()
    w.ue(0)
    w.ue(0)
    w.put(1, 0)  # CAVLC
    w.put(1, 0)
    w.ue(0)  # one slice group
    w.ue(0)  # num_ref_idx_l0_default_active_minus1
    w.ue(0)
    w.put(1, 0)
    w.put(2, 0)
    w.se(cfg["pic_init_qp"] - 26)
    w.se(0)
    w.se(cfg["chroma_qp_index_offset"])
    w.put(1, cfg["deblocking_control"])
    w.put(1, cfg["constrained_intra_pred"])
    w.put(1, 0)
    return w.rbsp(0)


def i_slice_header(rng, cfg, idr_pic_id, slice_qp_delta, deblocking):
    w = Bits()
    w.ue(0)
    w.ue(7 if rng.random() < 0.5 else 2)  # slice_type 2 or 7: both I
    w.ue(0)
    w.put(cfg["log2_max_frame_num"], 0)
    w.ue(idr_pic_id)
    w.put(cfg["log2_max_poc_lsb"], 0)
    w.put(2, 0)  # no_output_of_prior_pics_flag, long_term_reference_flag
    w.se(slice_qp_delta)
    if deblocking is not None:
        w.ue(deblocking[0])
        if deblocking[0] != 1:
            w.se(deblocking[1])
            w.se(deblocking[2])
    return w


# ---------------------------------------------------------------------------------------------- the macroblock layer

class Synth:
    def __init__(self, seed, cfg):
        self.rng = np.random.default_rng(seed)
        self.cfg = dict(CFG_DEFAULT, **cfg)
        self.mbw, self.mbh = self.cfg["mbw"], self.cfg["mbh"]
        self.nmb = self.mbw * self.mbh
        self.cov = new_coverage()
        self.delta = 0  # mb_qp_delta persists when absent, across pictures too (F/rbsp_decoding.cpp:298,322)
        self.active = 0  # num_ref_idx_l0_active_minus1: only an override ever changes it
        self.QPy = 0

    # -- per-picture model of what the decoder knows about the neighbours
    def _new_picture(self):
        n = self.nmb
        self.kind = [None] * n
        self.cbpL, self.cbpC = [0] * n, [0] * n
        self.tcL = [[0] * 16 for _ in range(n)]
        self.tcC = [[[0] * 4 for _ in range(2)] for _ in range(n)]
        self.modes = [[2] * 16 for _ in range(n)]
        self.types = []

    def _count(self, m, luma, b, plane):
        if self.kind[m] == "skip":
            return 0
        if luma:
            return self.tcL[m][b] if (self.cbpL[m] >> (b // 4)) & 1 else 0
        return self.tcC[m][plane][b] if self.cbpC[m] & 2 else 0

    def nC(self, mb, luma, blk, plane=0):
        """total-coefficient prediction of block blk of macroblock mb (all blocks before it are recorded)"""
        mbx, mby = mb % self.mbw, mb // self.mbw
        if luma:
            x0, y0 = BLK_XY[blk]
            at, last = (lambda x, y: BLK_AT[(x, y)]), 12
        else:
            x0, y0 = (blk & 1) * 4, (blk >> 1) * 4
            at, last = (lambda x, y: (y // 4) * 2 + x // 4), 4
        nA = nB = None
        if x0 > 0:
            nA = self._count(mb, luma, at(x0 - 4, y0), plane)
        elif mbx > 0:
            nA = self._count(mb - 1, luma, at(last, y0), plane)
        if y0 > 0:
            nB = self._count(mb, luma, at(x0, y0 - 4), plane)
        elif mby > 0:
            nB = self._count(mb - self.mbw, luma, at(x0, last), plane)
        if nA is not None and nB is not None:
            return (nA + nB + 1) >> 1
        return nA if nA is not None else nB if nB is not None else 0

    def _emit(self, w, coef, n, nC):
        by, nbits, tc = fo_py.cavlc_encode_block(coef, n, nC)
        w.b.extend(np.unpackbits(np.frombuffer(by, np.uint8))[:nbits].tolist())
        a = analyze_block(coef, n)
        assert a["tc"] == tc
        c = self.cov
        c["coeff_token"][4 if nC == -1 else 0 if nC < 2 else 1 if nC < 4 else 2 if nC < 8 else 3].add((tc, a["t1"]))
        c["level_prefix"].update(a["prefixes"])
        if a["prefixes"]:
            c["max_suffix_length"] = max(c["max_suffix_length"], max(s for _, s in a["prefixes"]))
        c["start_suffix_1"] |= tc > 10 and a["t1"] < 3
        if a["tz"] is not None:
            c["total_zeros"][n].add((tc, a["tz"]))
        if a["runs"]:
            c["max_run_before"] = max(c["max_run_before"], max(a["runs"]))
        return tc

    def _step_qp(self, delta=None):
        """QPy of the next macroblock: a coded mb_qp_delta, or the stale one (reference quirk)"""
        if delta is not None:
            self.delta = delta
        q = self.QPy + self.delta
        self.cov["wrap_up"] |= q > 51
        self.cov["wrap_down"] |= q < 0
        self.QPy = (q + 52) % 52
        self.cov["qpy"].add(self.QPy)

    def _residual(self, w, mb, i16, cbpL, cbpC, p):
        """mb_qp_delta + residual(0, 15) of a macroblock whose kind / cbp are already recorded"""
        rng = self.rng
        if p.get("qp_targets"):
            target = p["qp_targets"].pop(0)
            delta = ((target - self.QPy + 26) % 52) - 26
        else:
            dr = p.get("delta_range", 2)
            delta = int(rng.integers(-dr, dr + 1)) if rng.random() < p.get("p_delta", 0.5) else 0
        if p.get("force_delta") and delta == 0:
            delta = p["force_delta"]
        w.se(delta)
        self._step_qp(delta)
        qp = self.QPy
        mode = str(rng.choice(p.get("levels", ["small"])))
        capped = mode in ("small", "mixed")
        amp = max(1, int(p.get("amp", 40) / 2 ** (qp / 6)))
        tcmax = 16 if not capped or qp <= 20 else 5 if qp <= 30 else 2 if qp <= 40 else 1
        lo, hi = TC_CLASSES[int(rng.integers(0, 4))]  # this macroblock's density: decides the class its neighbours see
        nonzero = p.get("nonzero", False)

        def block(n, first_of_kind):
            tc = int(rng.integers(lo, hi + 1)) if rng.random() < 0.65 else int(rng.integers(0, n + 1))
            tc = min(tc, n, tcmax)
            if capped and qp > 30 and rng.random() < 0.7:
                tc = 0
            if nonzero and first_of_kind:
                tc = max(tc, 1)
            return gen_block(rng, n, tc, mode, amp)

        if i16:
            self.tcL[mb][0] = self._emit(w, block(16, False), 16, self.nC(mb, True, 0))
        first = True
        for i8 in range(4):
            if (cbpL >> i8) & 1:
                for i4 in range(4):
                    blk = i8 * 4 + i4
                    n = 15 if i16 else 16
                    self.tcL[mb][blk] = self._emit(w, block(n, first), n, self.nC(mb, True, blk))
                    first = False
        if i16 and cbpL == 0:
            self.tcL[mb][0] = 0
        if cbpC & 3:
            for pl in range(2):
                tc = int(rng.integers(0, 5))
                if capped and qp > 30:
                    tc = min(tc, 1)
                if nonzero and pl == 0:
                    tc = max(tc, 1)
                self._emit(w, gen_block(rng, 4, tc, mode, amp), 4, -1)
        if cbpC & 2:
            for pl in range(2):
                for b in range(4):
                    self.tcC[mb][pl][b] = self._emit(w, block(15, pl == 0 and b == 0), 15, self.nC(mb, False, b, pl))

    def _intra_mb(self, w, mb, kind, slice_type, p):
        rng = self.rng
        mbx, mby = mb % self.mbw, mb // self.mbw
        left, top = mbx > 0, mby > 0
        any_mode = p.get("any_mode", False)  # modes drawn without regard to the neighbours they need (ILLEGAL_PLANS)
        if any_mode:
            chroma = int(rng.integers(0, 4))
        else:
            chroma = int(rng.choice([0] + ([1] if left else []) + ([2] if top else []) + ([3] if left and top else [])))
        self.cov["chroma_modes"].add(chroma)
        base = 5 if slice_type == "P" else 0
        self.kind[mb] = kind
        if kind == "i16":
            if any_mode:
                mode = int(rng.integers(0, 4))
            else:
                mode = int(rng.choice([2] + ([1] if left else []) + ([0] if top else []) + ([3] if left and top else [])))
            cbpC = 2 if p.get("nonzero") else int(rng.integers(0, 3))
            cbpL = 15 if p.get("nonzero") or rng.random() < 0.5 else 0
            t = base + 1 + mode + 4 * cbpC + (12 if cbpL else 0)
            self.cov["i16_modes"].add(mode)
            w.ue(t)
            w.ue(chroma)
        else:
            t = base
            w.ue(t)
            if slice_type == "P":
                self.cov["intra_in_p"].add((self.kind[mb - 1] if left else "unavailable", self.kind[mb - self.mbw] if top else "unavailable"))
            for blk in range(16):
                x0, y0 = BLK_XY[blk]
                okA, okB = mbx * 16 + x0 > 0, mby * 16 + y0 > 0
                pm = 2
                if okA and okB and not self.cfg["constrained_intra_pred"]:
                    mA = self.modes[mb][BLK_AT[(x0 - 4, y0)]] if x0 else (self.modes[mb - 1][BLK_AT[(12, y0)]] if self.kind[mb - 1] == "i4" else 2)
                    mB = self.modes[mb][BLK_AT[(x0, y0 - 4)]] if y0 else (
                        self.modes[mb - self.mbw][BLK_AT[(x0, 12)]] if self.kind[mb - self.mbw] == "i4" else 2)
                    pm = min(mA, mB)
                legal = list(range(9)) if any_mode else [2] + ([0, 3, 7] if okB else []) + ([1, 8] if okA else []) + ([4, 5, 6] if okA and okB else [])
                assert pm in legal
                m = pm if rng.random() < 0.3 else int(rng.choice(legal))
                if m == pm:
                    w.put(1, 1)
                    self.cov["i4_coding"].add((1, -1))
                else:
                    w.put(1, 0)
                    w.put(3, m if m < pm else m - 1)
                    self.cov["i4_coding"].add((0, m if m < pm else m - 1))
                self.modes[mb][blk] = m
                self.cov["i4_modes"].add(m)
            w.ue(chroma)
            if p.get("nonzero"):
                cbp = 47
            else:
                cbp = int(rng.integers(0, 48)) if rng.random() >= p.get("p_cbp0", 0.15) else 0
            w.ue(INTRA_CBP.index(cbp))
            cbpL, cbpC = cbp & 15, cbp >> 4
        self.cbpL[mb], self.cbpC[mb] = cbpL, cbpC
        self.types.append(t)
        self.cov["mb_types"][slice_type].add(t)
        if cbpL or cbpC or kind == "i16":
            self._residual(w, mb, kind == "i16", cbpL, cbpC, p)
        else:
            self._step_qp()

    def _inter_mb(self, w, mb, p, ref_sub, ref_mb, cbp=None):
        rng = self.rng
        r = p.get("mvd_range", 3)
        t = int(rng.choice([0, 1, 2, 3, 3, 4, 4]))
        w.ue(t)

        def mvd():
            w.se(int(rng.integers(-r, r + 1)))
            w.se(int(rng.integers(-r, r + 1)))
        if t >= 3:
            sub = [int(rng.integers(0, 4)) for _ in range(4)]
            self.cov["sub_types"].update(sub)
            for s in sub:
                w.ue(s)
            if ref_sub and t != 4:
                for _ in range(4):
                    te_bits(w, rng)
            for s in sub:
                for _ in range([1, 2, 2, 4][s]):
                    mvd()
        else:
            npart = 1 if t == 0 else 2
            if ref_mb:
                for _ in range(npart):
                    te_bits(w, rng)
            for _ in range(npart):
                mvd()
        if cbp is None:
            if p.get("nonzero"):
                cbp = 47
            else:
                cbp = INTER_CBP[int(rng.integers(1, 48))] if rng.random() >= p.get("p_cbp0", 0.3) else 0
        w.ue(INTER_CBP.index(cbp))
        self.kind[mb] = "inter"
        self.cbpL[mb], self.cbpC[mb] = cbp & 15, cbp >> 4
        self.types.append(t)
        self.cov["mb_types"]["P"].add(t)
        if cbp:
            self._residual(w, mb, False, cbp & 15, cbp >> 4, p)
        else:
            self._step_qp()

    def i_picture(self, idr_pic_id, p):
        cfg, rng = self.cfg, self.rng
        self._new_picture()
        self.QPy = p.get("qp", cfg["pic_init_qp"])
        w = i_slice_header(rng, cfg, idr_pic_id, self.QPy - cfg["pic_init_qp"], p.get("deblocking") if cfg["deblocking_control"] else None)
        for mb in range(self.nmb):
            if p.get("bad_mb") == mb:
                w.ue(25)  # I_PCM: not supported
                self.types.append(25)
                w.put(16, 0xAAAA)
                break
            self._intra_mb(w, mb, "i16" if rng.random() < p.get("p_i16", 0.4) else "i4", "I", p)
        return nal_unit(5, 3, w.rbsp(2))

    def p_picture(self, k, p):
        cfg, rng = self.cfg, self.rng
        self._new_picture()
        self.QPy = p.get("qp", cfg["pic_init_qp"])
        w, override, am1 = p_slice(rng, self.nmb, k, 2 * k, p.get("override", False), p.get("active", 0), p.get("modification"),
                                   log2_max_frame_num=cfg["log2_max_frame_num"], log2_max_poc_lsb=cfg["log2_max_poc_lsb"],
                                   slice_qp_delta=self.QPy - cfg["pic_init_qp"],
                                   deblocking=p.get("deblocking") if cfg["deblocking_control"] else None)
        if override:
            self.active = am1
        ref_sub, ref_mb = bool(override), self.active > 0
        # the kind of every macroblock first: skip runs are written in front of the macroblock that ends them
        pi, ps_ = p.get("p_intra", 0.0), p.get("p_skip", 0.2)
        kinds = []
        head = list(p.get("head", []))
        for mb in range(self.nmb):
            if mb < len(head):
                kinds.append(head[mb])
                continue
            r = rng.random()
            kd = "skip" if r < ps_ else "i4" if r < ps_ + pi * 0.6 else "i16" if r < ps_ + pi else "inter"
            if p.get("steer_pairs"):  # an I4x4 macroblock wherever its (left, upper) kinds were not seen yet
                mbx, mby = mb % self.mbw, mb // self.mbw
                pair = (kinds[mb - 1] if mbx else "unavailable", kinds[mb - self.mbw] if mby else "unavailable")
                pair = tuple("inter" if x == "cbp0" else x for x in pair)
                seen = self.cov["intra_in_p"] | self._planned
                if pair not in seen and rng.random() < 0.9:
                    kd = "i4"
                    self._planned.add(pair)
                elif mbx + 1 < self.mbw:  # ... or the left neighbour the next macroblock still lacks
                    above = kinds[mb + 1 - self.mbw] if mby else "unavailable"
                    want = [a for a in KINDS[1:] if (a, "inter" if above == "cbp0" else above) not in seen]
                    if want and rng.random() < 0.6:
                        kd = want[0]
            kinds.append(kd)
        if p.get("tail_chroma_ac"):
            kinds[-1] = "tail"
        elif kinds[-1] == "skip":
            # No picture ends in a skip run: behind one, the reference's more_rbsp_data() still sees the bytes that follow
            # the stop bit and its loop goes on to parse a macroblock past the picture (F/rbsp_decoding.cpp:115-124 tests no
            # CurrMbAddr there) -- an out-of-range write in the reference, so nothing its decoder could be held to.
            kinds[-1] = "cbp0"
        run = 0
        for mb, kd in enumerate(kinds):
            if kd == "skip":
                self.kind[mb] = "skip"
                self.types.append(P_SKIP)
                self.cov["mb_types"]["P"].add(P_SKIP)
                self._step_qp()
                run += 1
                continue
            w.ue(run)
            run = 0
            if p.get("bad_mb") == mb:
                w.ue(30)  # I_PCM: not supported
                self.types.append(30)
                w.put(16, 0xAAAA)
                break
            if kd in ("i4", "i16"):
                self._intra_mb(w, mb, kd, "P", p)
            elif kd == "cbp0":
                self._inter_mb(w, mb, p, ref_sub, ref_mb, cbp=0)
            elif kd == "tail":  # chroma AC and a non-zero mb_qp_delta left behind for the next picture
                self._inter_mb(w, mb, dict(p, force_delta=p["tail_chroma_ac"], nonzero=True), ref_sub, ref_mb, cbp=47)
            else:
                self._inter_mb(w, mb, p, ref_sub, ref_mb)
        if run:
            w.ue(run)
        return nal_unit(1, 2, w.rbsp(0 if p.get("early_end") else 2))

    _planned = None


def make_stream(seed, cfg, pictures):
    """cfg: the parameter-set fields (CFG_DEFAULT); pictures: one dict per picture, type "I" (an IDR picture) or "P", with
    qp (SliceQPy), levels (the level modes its macroblocks draw from), p_i16, p_intra, p_skip, p_cbp0, delta_range, p_delta,
    qp_targets (QPy of the coded macroblocks, in order), nonzero (every macroblock codes luma, chroma DC and chroma AC),
    head (kinds of the first macroblocks: "skip" / "cbp0"), tail_chroma_ac (mb_qp_delta of a last macroblock with chroma
    AC), steer_pairs, deblocking (idc, alpha, beta), bad_mb (index of an I_PCM macroblock), any_mode (Intra4x4, Intra16x16
    and chroma prediction modes drawn from all of them, whether or not the neighbours they read exist) and the P header options of
    pslice_synth (override, active, modification, mvd_range, early_end).
    -> (Annex-B bytes, coverage report, [mb_type of every macroblock written, per picture])"""
    s = Synth(seed, cfg)
    s._planned = set()
    out = bytearray(nal_unit(7, 3, sps_rbsp(s.cfg)) + nal_unit(8, 3, pps_rbsp(s.cfg)))
    types = []
    assert pictures[0]["type"] == "I"
    k = idr = 0
    for p in pictures:
        p = dict(p)
        if p.get("qp_targets"):
            p["qp_targets"] = list(p["qp_targets"])
        if p["type"] == "I":
            out += s.i_picture(idr, p)
            idr, k = idr + 1, 0
        else:
            k += 1
            out += s.p_picture(k, p)
        types.append(np.array(s.types, np.int32))
    return bytes(out), s.cov, types


# ---------------------------------------------------------------------------------------------- the plans of the tests

def _i(**kw):
    return dict(type="I", **kw)


def _p(**kw):
    return dict(type="P", **kw)


def _qp_walk(nmb):
    """QPy targets that visit 0..51 and wrap both ways (51 -> 0 -> 51), nmb coded macroblocks per picture"""
    seq = list(range(20, 52)) + list(range(0, 20)) + [19, 3, 51, 0, 50, 1, 26, 0, 51, 25, 49, 2]
    seq += [int(x) for x in np.random.default_rng(99).integers(0, 52, 4 * nmb - len(seq))]
    return [seq[i * nmb:(i + 1) * nmb] for i in range(4)]


_SM = ["small", "mixed"]
_I_ONLY = [_i(qp=22, levels=_SM), _i(qp=14, levels=_SM, p_i16=0.6), _i(qp=30, levels=_SM, p_i16=0.2)]
_F4 = [_p(override=True, active=1, modification=[]), _p(modification=[]), _p(modification=[(0, 1)], mvd_range=12),
       _p(override=True, active=0, mvd_range=40, p_skip=0.05)]
_W = _qp_walk(16)

# name -> (cfg, pictures, pictures of the second stream of the batch (None: the same), level cap applies)
PLANS = {
    **{f"i_only_modes_{w}x{h}": (dict(mbw=w, mbh=h), _I_ONLY if w * h > 6 else _I_ONLY * 3, None, True)
       for w, h in ((1, 1), (2, 1), (1, 2), (3, 2), (11, 9))},
    "cavlc_tables": (dict(mbw=5, mbh=3, pic_init_qp=20), [_i(qp=8, levels=["mixed", "escape"], p_cbp0=0.05)] + [
        _p(qp=q, levels=["mixed", "escape"], p_intra=0.3, p_skip=0.1, p_cbp0=0.1) for q in (4, 10, 16)], None, False),
    "intra_in_p": (dict(mbw=5, mbh=4, pic_init_qp=24), [_i(qp=20, levels=_SM)] + [
        _p(qp=q, levels=_SM, p_intra=0.4, p_skip=0.2, steer_pairs=True, p_cbp0=0.3) for q in (18, 22, 16, 24, 20)], None, True),
    "intra_in_p_constrained": (dict(mbw=5, mbh=4, pic_init_qp=24, constrained_intra_pred=1), [_i(qp=20, levels=_SM)] + [
        _p(qp=q, levels=_SM, p_intra=0.4, p_skip=0.2, steer_pairs=True, p_cbp0=0.3) for q in (18, 22, 16, 24, 20)], None, True),
    **{f"qp_walk_c{o}".replace("-", "m"): (dict(mbw=4, mbh=4, pic_init_qp=30, chroma_qp_index_offset=o),
                                            [_i(qp=20, levels=["small"], nonzero=True, qp_targets=_W[0])] + [
                                                _p(qp=q, levels=["small"], nonzero=True, qp_targets=_W[k + 1], p_skip=0.0, p_intra=0.3)
                                                for k, q in enumerate((51, 0, 26))], None, True) for o in (-12, 5, 12)},
    "extreme_levels": (dict(mbw=2, mbh=2, pic_init_qp=26), [
        _i(qp=51, levels=["extreme"], p_delta=0.0), _p(qp=51, levels=["extreme"], p_delta=0.0, p_intra=0.3, p_skip=0.0, p_cbp0=0.0),
        _i(qp=0, levels=["extreme"], p_delta=0.0), _p(qp=0, levels=["extreme"], p_delta=0.0, p_intra=0.3, p_skip=0.0, p_cbp0=0.0)], None, False),
    "carry": (dict(mbw=4, mbh=3, pic_init_qp=28), [
        _i(qp=24, levels=_SM),
        _p(qp=22, levels=_SM, tail_chroma_ac=3),
        _p(qp=26, levels=_SM, head=["skip", "skip", "cbp0", "skip", "cbp0", "cbp0"], tail_chroma_ac=-5),
        _p(qp=20, levels=_SM, head=["cbp0", "skip", "skip", "cbp0"], p_skip=0.4, tail_chroma_ac=2),
        _p(qp=24, levels=_SM, head=["skip"] * 5 + ["cbp0"], p_skip=0.5, p_cbp0=0.6)], 3, True),
    "headers": (dict(mbw=3, mbh=2, log2_max_frame_num=4, log2_max_poc_lsb=16, deblocking_control=1, pic_init_qp=12), [
        _i(qp=18, levels=_SM, deblocking=(1, 0, 0)), _p(qp=20, levels=_SM, deblocking=(0, 3, -2), p_intra=0.2),
        _p(qp=16, levels=_SM, deblocking=(1, 0, 0), p_intra=0.2), _p(qp=22, levels=_SM, deblocking=(2, -6, 6), p_intra=0.2),
        _i(qp=20, levels=_SM, deblocking=(0, -1, 1)), _p(qp=18, levels=_SM, deblocking=(1, 0, 0))], None, True),
    "headers_wide": (dict(mbw=3, mbh=2, log2_max_frame_num=16, log2_max_poc_lsb=4, deblocking_control=0, pic_init_qp=40), [
        _i(qp=18, levels=_SM), _p(qp=20, levels=_SM, p_intra=0.2), _p(qp=16, levels=_SM, p_intra=0.2)], None, True),
    "everything": (dict(mbw=11, mbh=9, pic_init_qp=22, chroma_qp_index_offset=-3), [_i(qp=18, levels=_SM)] + [
        dict(f, qp=q, levels=["small", "mixed", "escape"] if q < 16 else _SM, p_intra=0.25, delta_range=4)
        for f, q in zip(_F4, (20, 14, 24, 12))], None, False),
}
SEEDS = (101, 202)  # the two streams of a plan's batch


def plan_streams(name):
    """-> [(stream, coverage, mb_types)] * 2: the two different streams the plan's batch is made of"""
    cfg, pictures, short, _ = PLANS[name]
    return [make_stream(SEEDS[0], cfg, pictures), make_stream(SEEDS[1], cfg, pictures[:short] if short else pictures)]


# Legal syntax, illegal meaning: streams no conformant encoder writes but whose every field parses.  The reference
# decodes them all (it predicts from its -1 "unavailable" markers and keeps vectors of any size), so the decode twin
# is held to its pictures here too.  Kept apart from PLANS: those streams, their bytes and their recorded md5s stay.
#   any_mode   Intra4x4, Intra16x16 and chroma prediction modes drawn without regard to which neighbours exist
#   mvd_*      vector differences far past what a level allows; mvd_40000 leaves 16 bits, the others stay inside
_ANY = [_i(qp=22, levels=_SM, any_mode=True), _p(qp=20, levels=_SM, p_intra=0.5, any_mode=True),
        _p(qp=18, levels=_SM, p_intra=0.5, p_skip=0.05, any_mode=True), _i(qp=24, levels=_SM, any_mode=True)]
# name -> (cfg, pictures, seeds: one stream each)
ILLEGAL_PLANS = {
    **{f"any_mode_{w}x{h}": (dict(mbw=w, mbh=h), _ANY, (1, 2, 3)) for w, h in ((1, 1), (2, 1), (1, 2), (3, 2), (5, 4))},
    "any_mode_constrained_5x4": (dict(mbw=5, mbh=4, constrained_intra_pred=1), _ANY, (1, 2)),
    **{f"mvd_{r}": (dict(mbw=5, mbh=4), [_i(qp=22, levels=_SM)] + [_p(qp=22, levels=_SM, mvd_range=r, p_skip=0.1)] * 3, (1, 2))
       for r in (300, 3000, 40000)},
}
VECTORS_INSIDE_INT16 = ("mvd_300", "mvd_3000")
VECTORS_PAST_INT16 = ("mvd_40000",)


def illegal_streams(name):
    """-> [(stream, coverage, mb_types)]: one stream per seed of the plan"""
    cfg, pictures, seeds = ILLEGAL_PLANS[name]
    return [make_stream(seed, cfg, pictures) for seed in seeds]


def unsupported_stream(slice_type, seed=5):
    """a 3x2 stream whose last picture holds an I_PCM macroblock (mb_type 25 in an I slice, 30 in a P slice)
    -> (stream, pictures in front of the bad one, the stream up to the bad picture).  Only the last is for the oracle: like
    the reference it has no I_PCM, reads mb_type 30 of a P slice as an Intra16x16 type past its tables and divides by zero"""
    pics = [_i(qp=20, levels=_SM), _p(qp=20, levels=_SM, p_intra=0.2)]
    good = make_stream(seed, dict(mbw=3, mbh=2), pics)[0]
    pics.append(_i(qp=20, levels=_SM, bad_mb=3) if slice_type == "I" else _p(qp=20, levels=_SM, bad_mb=3, p_skip=0.0))
    stream = make_stream(seed, dict(mbw=3, mbh=2), pics)[0]
    assert stream.startswith(good) and len(stream) > len(good)
    return stream, 2, good


def y4m_md5(pictures, W, H):
    """md5 of the Y4M file the reference's decoder writes for these I420 pictures (writeToY4M, F/fileIO.cpp:134)"""
    import hashlib
    h = hashlib.md5()
    h.update(b"YUV4MPEG2 C420jpeg W%d H%d F24:1 Ip A1:1\n" % (W, H))
    for p in pictures:
        h.update(b"FRAME\n")
        h.update(np.ascontiguousarray(p, np.uint8).tobytes())
    return h.hexdigest()
