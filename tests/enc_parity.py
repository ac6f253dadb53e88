"""The picture-by-picture comparison of the device encoder with hard_content.oracle_run's record, shared by
test_gpu_hard_content.py and test_gpu_qp_sweep.py.

Where the reference leaves a side array undefined the comparison leaves it out, and only there:
  * I4MODE outside Intra4x4 macroblocks (the device writes the estimate's modes, the oracle keeps what was there);
  * CBP and TC of P_Skip macroblocks (the reference never sets them; the nC rule tests mb_type first, F/residual.cpp:424-538);
  * TC of a block that the macroblock's CBP keeps out of the stream: the oracle holds what the last coded_mb_size estimate left
    there (for Intra16x16 also the DC block's count in slot 0), the nC rule reads such a block as 0 through the CBP.
"""
import numpy as np

import hard_content as hc


def coded_tc_mask(mb_type, cbp):
    """[nmb][24] bool: the blocks whose TotalCoeff the CAVLC writer leaves behind and the nC rule can read (F/residual.cpp:300-372)"""
    m = np.zeros((mb_type.size, 24), bool)
    for i8 in range(4):
        m[:, i8 * 4:i8 * 4 + 4] = ((cbp[:, 0] >> i8) & 1)[:, None] != 0
    m[:, 16:] = ((cbp[:, 1] & 2) != 0)[:, None]
    return m


def device_run(pkg, W, H, seqs, qp, window):
    """seqs [4][S][fsz] through set_frames / encode_picture with explicit types (hard_content.NAL_TYPES) -> dict: pics (per
    picture a dict of what the device produced, [S] leading), stats, status, streams (Annex-B, the context's own SPS and PPS)"""
    S = seqs.shape[1]
    g = pkg.FerHip(W, H, S, qp=qp, window=window, maxdiff=3, intra_every=1000)
    try:
        nmb = g.nmb
        pics = []
        for t, nt in enumerate(hc.NAL_TYPES):
            g.set_frames(seqs[t])
            rbsp, types = g.encode_picture(nal_types=[nt] * S)
            assert types == [nt] * S
            r = dict(rbsp=rbsp, recon=g.get_recon(), mb_type=g.read("MBTYPE").reshape(S, nmb), cbp=g.read("CBP").reshape(S, nmb, 2),
                     tc=g.read("TC").reshape(S, nmb, 24))
            if nt == 5:
                r.update(i4mode=g.read("I4MODE").reshape(S, nmb, 16), mbsize=g.read("MBSIZE").reshape(S, nmb, 2))
            else:
                r.update(mv=g.read("MV").reshape(S, nmb, 4, 2))
            pics.append(r)
        return dict(pics=pics, stats=g.stats(), status=g.status(),
                    streams=[b"".join(g.sps_pps(s)) + b"".join(g.write_nal(nt, p["rbsp"][s]) for nt, p in zip(hc.NAL_TYPES, pics))
                             for s in range(S)])
    finally:
        g.close()


def compare_stream(dev, s, ref, name):
    """stream s of device_run's dict against the oracle's four dicts (hard_content.oracle_run): MBTYPE, CBP, TC, I4MODE, MBSIZE, MV,
    reconstruction, RBSP of every picture, and the counters"""
    for t, (d, o) in enumerate(zip(dev["pics"], ref)):
        tag = f"{name} picture {t}"
        intra = hc.NAL_TYPES[t] == 5
        mt, cbp = o["mb_type"], o["cbp"]
        assert np.array_equal(d["mb_type"][s], mt), f"{tag}: MBTYPE at {np.flatnonzero(d['mb_type'][s] != mt)[:8]}"
        coded = np.ones(mt.size, bool) if intra else mt != 31
        assert np.array_equal(d["cbp"][s][coded], cbp[coded]), f"{tag}: CBP at {np.flatnonzero((d['cbp'][s] != cbp).any(1) & coded)[:8]}"
        m = coded_tc_mask(mt, cbp) & coded[:, None]
        dtc = d["tc"][s].astype(np.int32)
        assert np.array_equal(dtc[m], o["tc"][m]), f"{tag}: TC at macroblocks {np.flatnonzero(((dtc != o['tc']) & m).any(1))[:8]}"
        if intra:
            i4 = mt == 0
            assert np.array_equal(d["i4mode"][s][i4], o["i4mode"][i4]), f"{tag}: I4MODE"
            assert np.array_equal(d["mbsize"][s], o["mbsize"]), f"{tag}: MBSIZE at {np.flatnonzero((d['mbsize'][s] != o['mbsize']).any(1))[:8]}"
        else:
            assert np.array_equal(d["mv"][s].astype(np.int32), o["mv"]), f"{tag}: MV at {np.flatnonzero((d['mv'][s] != o['mv']).any((1, 2)))[:8]}"
        bad = np.flatnonzero(d["recon"][s] != o["recon"])
        assert bad.size == 0, f"{tag}: {bad.size} reconstructed samples differ, first at {bad[:8]}"
        assert d["rbsp"][s] == o["rbsp"], f"{tag}: RBSP {len(d['rbsp'][s])} vs {len(o['rbsp'])} bytes"
    assert list(dev["stats"][s]) == list(ref[-1]["stats"]), f"{name}: brojTipova"
