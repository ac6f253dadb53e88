"""Shared helpers of the neighbourhood-seam tests (ferhip_intra_mbs, ferhip_mv_mbs): seeded job generators and the
oracle-side driver.

A job is a dict with the fields of ferhip_intra_job / ferhip_mv_job (include/ferhip.h): a 3 x 2-macroblock picture, `pos`, the
side information of the macroblocks in front of pos.  NbOracle runs the same job on an Oracle(48, 32) context: it fills the
context through the fo_dbg_* accessors and, for the fields that have none (prev_flag, rem_mode, chroma_mode, mvd,
sub_mb_type, refidx, constrained_intra, chroma_qp_offset), through FoCtx, a ctypes mirror of fo_ctx (oracle/fo.h) that
tests/test_seam_nbhd_host.py pins against the accessors, and calls the exported fo_* functions.

Numbers come from numpy.random.default_rng(seed); pictures are 48 x 32 windows of hard_content.mosaic() and of
synth.gen_frame(), some with a neighbour replaced by a saturated tile.
"""
import ctypes as C

import numpy as np

import hard_content as hc
from conftest import load_pkg

W, H, MBW, NMB = 48, 32, 3, 6
P_SKIP = 31
ENC_QPS = (12, 22, 32, 42, 51)
# neighbours of every pos: A = pos - 1, B = pos - 3, C = pos - 2, D = pos - 4
NB = ({}, {"A": 0}, {"A": 1}, {"B": 0, "C": 1}, {"A": 3, "B": 1, "C": 2, "D": 0}, {"A": 4, "B": 2, "D": 1})
LEVELS = (("lumaLevel", 256), ("dc16", 16), ("ac16", 256), ("cdc", 8), ("cac", 128))
BX = (0, 4, 0, 4, 8, 12, 8, 12, 0, 4, 0, 4, 8, 12, 8, 12)
BY = (0, 0, 4, 4, 0, 0, 4, 4, 8, 8, 12, 12, 8, 8, 12, 12)
NBA = (5, 0, 7, 2, 1, 4, 3, 6, 13, 8, 15, 10, 9, 12, 11, 14)
NBB = (10, 11, 0, 1, 14, 15, 4, 5, 2, 3, 8, 9, 6, 7, 12, 13)
EDGE_A, EDGE_B = (0, 2, 8, 10), (0, 1, 4, 5)


class FoLevels(C.Structure):
    _fields_ = [("Lumalevel", C.c_int * 256), ("DC16", C.c_int * 16), ("AC16", C.c_int * 256), ("CDC", C.c_int * 8), ("CAC", C.c_int * 128)]


class FoCtx(C.Structure):
    """fo_ctx of oracle/fo.h, member for member"""
    _P = C.c_void_p
    _fields_ = [(n, C.c_int) for n in ("W", "H", "Wc", "Hc", "mbw", "mbh", "nmb")] + [
        ("L", _P), ("C", _P * 2), ("dL", _P), ("dC", _P * 2)] + [(n, C.c_int) for n in (
            "have_dpb", "qp", "basic", "window", "maxdiff_set", "intra_every", "chroma_qp_offset", "slice_type", "frame_num", "poc_lsb",
            "idr_pic_id", "first_idr_done", "QPy", "frames_done")] + [
        ("mb_type", _P), ("cbp_l", _P), ("cbp_c", _P), ("tc_l", _P), ("tc_c", _P), ("i4mode", _P), ("mvx", _P), ("mvy", _P), ("refidx", _P),
        ("cur", C.c_int), ("cur_mb_type", C.c_int), ("cbpL", C.c_int), ("cbpC", C.c_int), ("lv", FoLevels),
        ("prev_flag", C.c_int * 16), ("rem_mode", C.c_int * 16), ("chroma_mode", C.c_int), ("mvd", C.c_int * 32), ("sub_mb_type", C.c_int * 4),
        ("mb_qp_delta", C.c_int), ("MAXDIFF", C.c_int), ("interp", _P * 16), ("kar", _P * 80), ("sorted", _P * 5), ("sorted_tmp", _P * 5),
        ("koliko", C.c_int * 16385), ("me_ready", C.c_int), ("type_count", C.c_int * 5), ("num_ref_idx_override", C.c_int),
        ("num_ref_idx_l0_active_minus1", C.c_int), ("log2_max_frame_num", C.c_int), ("log2_max_poc_lsb", C.c_int), ("pic_init_qp", C.c_int),
        ("deblock_ctl", C.c_int), ("nal_ref_idc", C.c_int), ("constrained_intra", C.c_int), ("ref_idx_l0", _P), ("dbg_mvx", _P), ("dbg_mvy", _P),
        ("dbg_mbsize", _P), ("me_rec", _P), ("dbg_max_level", C.c_int), ("chroma_pred_mode", _P), ("undefined", C.c_int),
        ("block_overrun", C.c_int), ("refusals", C.c_int)]


def mirror(oracle):
    """the FoCtx view of an fo_py.Oracle's context"""
    return FoCtx.from_address(oracle.c.value)


# ---------------------------------------------------------------- pictures
_pics = {}


def _sources():
    """the pictures the 48 x 32 windows are cut from: three mosaics and two smooth frames, as (Y, Cb, Cr) planes"""
    if not _pics:
        pw, ph = 176, 144
        gen = load_pkg().gen_frame
        for k, f in enumerate([hc.mosaic(pw, ph, 5), hc.mosaic(pw, ph, 6), hc.mosaic(pw, ph, 7), gen(pw, ph, 0, 1234, 2), gen(pw, ph, 3, 99, 6)]):
            ys = pw * ph
            _pics[k] = (f[:ys].reshape(ph, pw), f[ys:ys + ys // 4].reshape(ph // 2, pw // 2), f[ys + ys // 4:].reshape(ph // 2, pw // 2))
    return _pics


def picture(rng, pos, smooth=None):
    """a 48 x 32 picture: Y [32][48], Cb, Cr [16][24] uint8.  Sometimes a macroblock other than pos is a saturated tile."""
    src = _sources()
    k = int(rng.integers(3, 5)) if smooth or (smooth is None and rng.random() < 0.3) else int(rng.integers(0, 3))
    Ys, Us, Vs = src[k]
    x0, y0 = 16 * int(rng.integers(0, (176 - W) // 16 + 1)), 16 * int(rng.integers(0, (144 - H) // 16 + 1))
    Y = Ys[y0:y0 + H, x0:x0 + W].copy()
    U = Us[y0 // 2:(y0 + H) // 2, x0 // 2:(x0 + W) // 2].copy()
    V = Vs[y0 // 2:(y0 + H) // 2, x0 // 2:(x0 + W) // 2].copy()
    if rng.random() < 0.25:
        m = int(rng.integers(0, NMB))
        if m != pos:
            base = int(rng.choice([0, 2, 253, 255]))
            mx, my = (m % MBW) * 16, (m // MBW) * 16
            Y[my:my + 16, mx:mx + 16] = np.clip(base + rng.integers(-3, 4, (16, 16)), 0, 255)
            U[my // 2:my // 2 + 8, mx // 2:mx // 2 + 8] = np.clip(base + rng.integers(-3, 4, (8, 8)), 0, 255)
            V[my // 2:my // 2 + 8, mx // 2:mx // 2 + 8] = np.clip(255 - base + rng.integers(-3, 4, (8, 8)), 0, 255)
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


# ---------------------------------------------------------------- neighbour states
def _inter_mv(rng, t):
    """vectors of an inter macroblock of type t, one per quadrant: the quadrants of a partition carry its vector"""
    scale = int(rng.choice([0, 0, 4, 40, 300]))
    v = rng.integers(-scale, scale + 1, (4, 2)) if scale else np.zeros((4, 2), np.int64)
    if t in (0, P_SKIP):
        v[:] = v[0]
    elif t == 1:
        v[1], v[3] = v[0], v[2]
    elif t == 2:
        v[2], v[3] = v[0], v[1]
    return v.astype(np.int32)


def nb_state(rng, slice_type, kinds=("i4", "i16", "inter", "skip")):
    """random legal side information of one macroblock in the numbering of slice_type (states no encoder need have produced)"""
    kind = str(rng.choice([k for k in kinds if slice_type == 0 or k != "inter"]))
    off = 5 if slice_type == 0 else 0
    t = {"i4": off, "i16": off + int(rng.integers(1, 25)), "inter": int(rng.integers(0, 5)), "skip": P_SKIP}[kind]
    return dict(mb_type=t, cbp_luma=int(rng.integers(0, 16)), cbp_chroma=int(rng.integers(0, 3)), tc_luma=rng.integers(0, 17, 16).astype(np.int32),
                tc_chroma=rng.integers(0, 17, 8).astype(np.int32), i4mode=rng.integers(0, 9, 16).astype(np.int32),
                mv=_inter_mv(rng, t if kind in ("inter", "skip") else 3).reshape(-1))


def _levels(rng, n, maxn, big):
    """n level vectors as a quantiser leaves them: empty, sparse to full, small or with large entries"""
    kind = rng.integers(0, 4, n)[:, None]
    mask = rng.random((n, 16)) < rng.choice([0.1, 0.3, 0.7], n)[:, None]
    mag = rng.choice([1, 2, 4, big], n)[:, None]
    v = rng.integers(1, mag + 1, (n, 16)) * rng.choice([-1, 1], (n, 16))
    return np.where(mask & (kind != 0) & (np.arange(16)[None, :] < maxn), v, 0).astype(np.int32)


# ---------------------------------------------------------------- intra jobs
def encode_jobs(seed, per_cell):
    """ENCODE jobs: every (pos, qp of ENC_QPS) cell per_cell times; mb[pos].mb_type = the stale entry, P_Skip in a third"""
    rng = np.random.default_rng(seed)
    jobs = []
    for pos in range(NMB):
        for qp in ENC_QPS:
            for k in range(per_cell):
                Y, U, V = picture(rng, pos, smooth=(k % 4 == 3))
                mb = [nb_state(rng, 2, ("i4", "i4", "i16", "i16", "skip")) if m < pos else None for m in range(NMB)]
                mb[pos] = dict(mb_type=int(rng.choice([P_SKIP, 0, int(rng.integers(1, 25))])))
                jobs.append(dict(op=0, pos=pos, slice_type=2, qp=qp, mb=mb, Y=Y, Cb=U, Cr=V))
    return jobs


def i4_modes(job):
    """getIntra4x4PredMode of a DECODE job (the generator's own statement of the rule, used to keep its jobs legal)"""
    pos, st = job["pos"], job["slice_type"]
    i4t = 0 if st == 2 else 5
    nb = NB[pos]
    mode = [0] * 16
    for blk in range(16):
        mA = mB = 2
        if not (blk in EDGE_A and "A" not in nb) and not (blk in EDGE_B and "B" not in nb) and not job["constrained_intra"]:
            if blk in EDGE_A:
                n = job["mb"][pos - 1]
                mA = int(n["i4mode"][NBA[blk]]) if n["mb_type"] == i4t else 2
            else:
                mA = mode[NBA[blk]]
            if blk in EDGE_B:
                n = job["mb"][pos - 3]
                mB = int(n["i4mode"][NBB[blk]]) if n["mb_type"] == i4t else 2
            else:
                mB = mode[NBB[blk]]
        pm, rem = min(mA, mB), int(job["rem_mode"][blk])
        mode[blk] = pm if job["prev_flag"][blk] else (rem if rem < pm else rem + 1)
    return mode


def mode4_legal(pos, blk, m):
    left, top = BX[blk] > 0 or "A" in NB[pos], BY[blk] > 0 or "B" in NB[pos]
    return not ((m in (0, 3, 7) and not top) or (m in (1, 8) and not left) or (m in (4, 5, 6) and not (left and top)))


def decode_jobs(seed, n, slice_types=(0, 0, 2)):
    """DECODE jobs of the generator's own: P and I slices, both constrained_intra values, chroma_qp_offset mostly non-zero, every
    kind of neighbour; legal by construction"""
    rng = np.random.default_rng(seed)
    jobs = []
    for it in range(n):
        pos, st = it % NMB, int(slice_types[(it // NMB) % len(slice_types)])
        nb, off = NB[pos], 5 if st == 0 else 0
        Y, U, V = picture(rng, pos)
        job = dict(op=1, pos=pos, slice_type=st, qp=int(rng.integers(0, 52)), chroma_qp_offset=int(rng.choice([0, -12, 12, int(rng.integers(-12, 13))])),
                   constrained_intra=int(rng.integers(0, 2)), Y=Y, Cb=U, Cr=V)
        job["mb"] = [nb_state(rng, st) if m < pos else None for m in range(NMB)]
        job["chroma_mode"] = int(rng.choice([0] + ([1] if "A" in nb else []) + ([2] if "B" in nb else []) + ([3] if "A" in nb and "B" in nb else [])))
        big = int(rng.choice([3, 20, 200]))
        lv = {k: np.zeros(s, np.int32) for k, s in LEVELS}
        lv["cdc"] = _levels(rng, 2, 4, big)[:, :4].reshape(-1)
        lv["cac"] = _levels(rng, 8, 15, big).reshape(-1)
        if rng.random() < 0.5:
            job["mb"][pos] = dict(mb_type=off)
            job["prev_flag"] = (rng.random(16) < 0.4).astype(np.int32)
            job["rem_mode"] = rng.integers(0, 8, 16).astype(np.int32)
            for blk in range(16):   # a block whose mode reads a missing neighbour draws again (the predicted mode is always legal)
                for attempt in range(9):
                    if mode4_legal(pos, blk, i4_modes(job)[blk]):
                        break
                    job["rem_mode"][blk] = int(rng.integers(0, 8))
                    job["prev_flag"][blk] = int(attempt == 7)
            lv["lumaLevel"] = _levels(rng, 16, 16, big).reshape(-1)
        else:
            m16 = int(rng.choice([2] + ([0] if "B" in nb else []) + ([1] if "A" in nb else []) + ([3] if "A" in nb and "B" in nb else [])))
            job["mb"][pos] = dict(mb_type=off + 1 + m16 + 4 * int(rng.integers(0, 3)) + 12 * int(rng.integers(0, 2)))
            job["prev_flag"], job["rem_mode"] = np.zeros(16, np.int32), np.zeros(16, np.int32)
            lv["dc16"] = _levels(rng, 1, 16, 10 * big)[0]
            lv["ac16"] = _levels(rng, 16, 15, big).reshape(-1)
        job.update(lv)
        jobs.append(job)
    return jobs


def decode_job_of(job, res):
    """the DECODE job that an ENCODE job and its result (oracle's or device's) make: the macroblock as the encoder coded it"""
    d = dict(job, op=1, chroma_qp_offset=0, constrained_intra=0, chroma_mode=int(res["chroma_mode"]))
    d["mb"] = list(job["mb"])
    d["mb"][job["pos"]] = dict(mb_type=int(res["mb_type"]))
    d["prev_flag"] = np.asarray(res["prev_flag"], np.int32)
    d["rem_mode"] = np.where(d["prev_flag"] != 0, 0, np.asarray(res["rem_mode"], np.int32)).astype(np.int32)
    for k, _ in LEVELS:
        d[k] = np.asarray(res[k], np.int32)
    return d


# ---------------------------------------------------------------- vector jobs
def mv_jobs(seed, n):
    """DERIVE jobs over all positions and types (0..4, P_Skip), every kind of neighbour"""
    rng = np.random.default_rng(seed)
    types = (0, 1, 2, 3, 4, P_SKIP)
    jobs = []
    for it in range(n):
        pos, t = it % NMB, types[(it // NMB) % 6]
        mb = [nb_state(rng, 0, ("inter", "inter", "inter", "skip", "i4", "i16")) if m < pos else None for m in range(NMB)]
        s = int(rng.choice([0, 3, 60]))
        jobs.append(dict(op=0, pos=pos, mb_type=t, sub_mb_type=rng.integers(0, 4, 4).astype(np.int32) if rng.random() < 0.8 else np.zeros(4, np.int32),
                         mvd=np.zeros(8, np.int32) if t == P_SKIP else rng.integers(-s, s + 1, 8).astype(np.int32), mb=mb))
    return jobs


def predict_jobs(seed, n):
    """PREDICT jobs: the macroblock's final vectors and type, every neighbour inter"""
    rng = np.random.default_rng(seed)
    jobs = []
    for it in range(n):
        pos, t = it % NMB, (it // NMB) % 5
        mb = [nb_state(rng, 0, ("inter", "inter", "skip")) if m < pos else None for m in range(NMB)]
        jobs.append(dict(op=1, pos=pos, mb_type=t, sub_mb_type=np.zeros(4, np.int32), mv=_inter_mv(rng, t).reshape(-1), mb=mb))
    return jobs


def _flat_nb(t, vx, vy):
    return dict(mb_type=t, mv=np.tile(np.array([vx, vy], np.int32), 4))


# the named jobs whose result leaves 16 bits: (name, job).  Every other component stays in range.
OVERFLOW_JOBS = (
    ("16x16 right of a vector at the top of the range", dict(op=0, pos=1, mb_type=0, sub_mb_type=np.zeros(4, np.int32), mvd=np.array([100, 0] + [0] * 6, np.int32),
                                                             mb=[_flat_nb(0, 32700, 5)] + [None] * 5)),
    ("16x16 below a vector at the bottom of the range (y)", dict(op=0, pos=3, mb_type=0, sub_mb_type=np.zeros(4, np.int32), mvd=np.array([0, -200] + [0] * 6, np.int32),
                                                                mb=[_flat_nb(0, 0, -32700), _flat_nb(5, 0, 0), _flat_nb(0, 7, 7)] + [None] * 3)),
    ("16x8, second partition", dict(op=0, pos=4, mb_type=1, sub_mb_type=np.zeros(4, np.int32), mvd=np.array([0, 0, 65536, 0] + [0] * 4, np.int32),
                                    mb=[_flat_nb(0, 1, 1), _flat_nb(0, 2, 2), _flat_nb(0, 3, 3), _flat_nb(0, 4, 4)] + [None] * 2)),
    ("8x16, first partition, the difference alone", dict(op=0, pos=0, mb_type=2, sub_mb_type=np.zeros(4, np.int32), mvd=np.array([-32769, 0] + [0] * 6, np.int32), mb=[None] * 6)),
    ("8x8, last quadrant", dict(op=0, pos=5, mb_type=3, sub_mb_type=np.array([0, 1, 2, 3], np.int32), mvd=np.array([0] * 6 + [0, 40000], np.int32),
                                mb=[_flat_nb(0, 0, 0), _flat_nb(P_SKIP, 9, 9), _flat_nb(0, -5, 3), _flat_nb(7, 0, 0), _flat_nb(0, 2, 2), None])),
)


# ---------------------------------------------------------------- the oracle side
class NbOracle:
    """one Oracle(48, 32) context and its per-macroblock state as writable arrays"""

    def __init__(self, fo):
        self.fo = fo
        self.o = fo.Oracle(W, H)
        L, c = self.o.L, self.o.c
        vp, i = C.c_void_p, C.c_int
        for name, args, res in (("fo_intraPredictionEncoding", [vp] * 4, i), ("fo_intraPrediction_dec", [vp] * 4, None), ("fo_DeriveMVs", [vp], None),
                                ("fo_setCodedBlockPattern", [vp], None), ("fo_residual_write", [vp, vp], None), ("fo_dbg_tc_l", [vp], vp),
                                ("fo_dbg_tc_c", [vp], vp)):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = res
        self.L, self.c, self.m = L, c, mirror(self.o)
        a = fo._arr
        self.mbt = a(L.fo_dbg_mb_type(c), NMB, np.int32)
        self.cbp_l, self.cbp_c = a(L.fo_dbg_cbp(c, 0), NMB, np.int32), a(L.fo_dbg_cbp(c, 1), NMB, np.int32)
        self.tc_l = a(L.fo_dbg_tc_l(c), NMB * 16, np.int32).reshape(NMB, 16)
        self.tc_c = a(L.fo_dbg_tc_c(c), NMB * 8, np.int32).reshape(NMB, 8)
        self.i4 = a(L.fo_dbg_i4mode(c), NMB * 16, np.int32).reshape(NMB, 16)
        self.mvx = a(L.fo_dbg_dec_mv(c, 0), NMB * 16, np.int32).reshape(NMB, 4, 4)
        self.mvy = a(L.fo_dbg_dec_mv(c, 1), NMB * 16, np.int32).reshape(NMB, 4, 4)
        self.refidx = a(self.m.refidx, NMB, np.int32)
        self.mbsize = a(L.fo_dbg_mbsize(c), NMB * 2, np.int32).reshape(NMB, 2)

    def close(self):
        self.o.close()

    def _load(self, job, slice_type, cur_type, qp):
        for arr in (self.mbt, self.cbp_l, self.cbp_c, self.tc_l, self.tc_c, self.i4, self.mvx, self.mvy, self.refidx):
            arr[:] = 0
        for m in range(job["pos"]):
            n = job["mb"][m]
            self.mbt[m] = n["mb_type"]
            self.cbp_l[m], self.cbp_c[m] = n.get("cbp_luma", 0), n.get("cbp_chroma", 0)
            self.tc_l[m], self.tc_c[m] = n.get("tc_luma", 0), n.get("tc_chroma", 0)
            self.i4[m] = n.get("i4mode", 0)
            v = np.asarray(n["mv"]).reshape(4, 2)
            for q in range(4):
                for j in range(4):
                    self.L.fo_dbg_set_mv(self.c, m, q, j, int(v[q, 0]), int(v[q, 1]))
        if "Y" in job:
            self.o.set_frame(np.concatenate([np.asarray(job[k], np.uint8).ravel() for k in ("Y", "Cb", "Cr")]))
        self.o.set_mb(job["pos"], cur_type, slice_type, qp)
        self.m.chroma_qp_offset = job.get("chroma_qp_offset", 0)
        self.m.constrained_intra = job.get("constrained_intra", 0)

    def _mb_samples(self, pos):
        f = self.o.frame()
        Y, U, V = f[:W * H].reshape(H, W), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)
        x, y = (pos % MBW) * 16, (pos // MBW) * 16
        return (Y[y:y + 16, x:x + 16].astype(np.int32).ravel(), U[y // 2:y // 2 + 8, x // 2:x // 2 + 8].astype(np.int32).ravel(),
                V[y // 2:y // 2 + 8, x // 2:x // 2 + 8].astype(np.int32).ravel())

    def encode(self, job):
        """intraPredictionEncoding and the tail of RBSP_encode for an I macroblock (oracle/fo_encode.c:250-262) -> the fields of
        ferhip_intra_result; tc = the non-zero levels of every block's list, tc_written = the oracle's TotalCoeff arrays after
        residual_write (defined on the blocks the CBP sends through the writer)"""
        pos = job["pos"]
        self._load(job, 2, job["mb"][pos]["mb_type"], job["qp"])
        pL, pCb, pCr = np.zeros((16, 16), np.int32), np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32)
        ret = int(self.L.fo_intraPredictionEncoding(self.c, pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data))
        self.m.cur_mb_type = 0 if ret == -1 else ret + 1
        self.o.quantization_transform(pL, pCb, pCr, True)
        self.L.fo_setCodedBlockPattern(self.c)
        if ret != -1:
            self.m.cur_mb_type += (self.m.cbpC << 2) + (12 if self.m.cbpL == 15 else 0)
        self.mbt[pos] = self.m.cur_mb_type
        r = dict(ret=ret, mb_type=int(self.m.cur_mb_type), cbp_luma=int(self.m.cbpL), cbp_chroma=int(self.m.cbpC), chroma_mode=int(self.m.chroma_mode),
                 mbsize=self.mbsize[pos].copy(), i4mode=self.i4[pos].copy(), prev_flag=np.array(self.m.prev_flag[:], np.int32),
                 rem_mode=np.array(self.m.rem_mode[:], np.int32), predL=pL.ravel().copy(), predCb=pCb.ravel().copy(), predCr=pCr.ravel().copy())
        lv = self.o.levels()
        if ret == -1:
            lv["dc16"][:], lv["ac16"][:] = 0, 0
        else:
            lv["lumaLevel"][:] = 0
        r.update(lv)
        luma = lv["lumaLevel"] if ret == -1 else lv["ac16"]
        r["tc_luma"] = np.count_nonzero(luma.reshape(16, 16)[:, :16 if ret == -1 else 15], axis=1).astype(np.int32)
        r["tc_chroma"] = np.count_nonzero(lv["cac"].reshape(8, 16)[:, :15], axis=1).astype(np.int32)
        r["recY"], r["recCb"], r["recCr"] = self._mb_samples(pos)
        if r["cbp_luma"] or r["cbp_chroma"] or ret != -1:
            buf = np.zeros(8192, np.uint8)
            w = self.fo._BW(buf.ctypes.data, buf.size, 0)
            self.L.fo_residual_write(self.c, C.byref(w))
        r["tc_written"] = np.concatenate([self.tc_l[pos], self.tc_c[pos]]).copy()
        return r

    def block0_cost(self, job, mode):
        """the cost the Intra4x4 search of an ENCODE job sees for block 0 under `mode`: the sum of the |quantised coefficients| of
        source - prediction (F/intra.cpp:819-850).  Block 0 reads no sample of its own macroblock, so this is the search's value."""
        pos = job["pos"]
        self._load(job, 2, 0, job["qp"])
        self.L.fo_intra4x4_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.L.fo_intra4x4_pred.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        p, pr = (C.c_int * 14)(), np.zeros((4, 4), np.int32)
        self.L.fo_intra4x4_fetch(self.c, 0, p)
        self.L.fo_intra4x4_pred(mode, p, pr.ctypes.data)
        x, y = (pos % MBW) * 16, (pos // MBW) * 16
        d = np.asarray(job["Y"])[y:y + 4, x:x + 4].astype(np.int32) - pr
        return int(np.abs(self.fo.forward_residual(job["qp"], d.reshape(1, 16))).sum())

    def decode(self, job):
        """intraPrediction with getIntra4x4PredMode and the reconstruction that follows it in the macroblock loop
        (oracle/fo_decode.c:241-253) -> i4mode, predL / predCb / predCr, recY / recCb / recCr"""
        pos, st = job["pos"], job["slice_type"]
        t = job["mb"][pos]["mb_type"]
        self._load(job, st, t, job["qp"])
        self.m.chroma_mode = job["chroma_mode"]
        self.m.prev_flag[:] = [int(v) for v in job["prev_flag"]]
        self.m.rem_mode[:] = [int(v) for v in job["rem_mode"]]
        self.o.set_levels(**{k: job[k] for k, _ in LEVELS})
        pL, pCb, pCr = np.zeros((16, 16), np.int32), np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32)
        self.L.fo_intraPrediction_dec(self.c, pL.ctypes.data, pCr.ctypes.data, pCb.ctypes.data)
        lvp = self.L.fo_dbg_levels(self.c)
        i4 = t == (0 if st == 2 else 5)
        if not i4:
            self.L.fo_transformDecoding16x16Luma(self.c, lvp + 4 * 256, lvp + 4 * 272, pL.ctypes.data, job["qp"])
        self.L.fo_transformDecodingChroma(self.c, lvp + 4 * 528, lvp + 4 * 536, pCb.ctypes.data, job["qp"], 1)
        self.L.fo_transformDecodingChroma(self.c, lvp + 4 * 532, lvp + 4 * 600, pCr.ctypes.data, job["qp"], 0)
        r = dict(i4mode=self.i4[pos].copy() if i4 else np.zeros(16, np.int32), predL=pL.ravel().copy(), predCb=pCb.ravel().copy(), predCr=pCr.ravel().copy())
        r["recY"], r["recCb"], r["recCr"] = self._mb_samples(pos)
        return r

    def derive(self, job, mvd=None):
        """DeriveMVs -> mv [8] as ints (x, y per quadrant), fits"""
        pos, t = job["pos"], job["mb_type"]
        self._load(job, 0, t, 20)
        d = np.asarray(job["mvd"] if mvd is None else mvd, np.int32).reshape(4, 2)
        full = np.zeros((4, 4, 2), np.int32)
        full[:, 0] = d
        self.m.mvd[:] = [int(v) for v in full.ravel()]
        self.m.sub_mb_type[:] = [int(v) for v in job["sub_mb_type"]]
        self.L.fo_DeriveMVs(self.c)
        mv = np.stack([self.mvx[pos, :, 0], self.mvy[pos, :, 0]], -1).astype(np.int64).ravel()
        return dict(mv=mv, fits=int((mv >= -32768).all() and (mv <= 32767).all()))
