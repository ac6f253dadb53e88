"""The selection and crowded routes of the motion search that only tests/route_content.py reaches, on the device.

tests/test_route_content_host.py shows on the oracle and the list model alone that each pair reaches what
route_content.REACHES names; here the device has to agree, exactly, at windows 16 and 32:

  lists      check_stream of test_gpu_me_lists.py (ST3, V0, the guessed centres, SPEC_L1 / SPEC_L2 against the model, the
             final vectors against the oracle), MBTYPE, MV and MVD against the oracle.  The partitions the predicates name
             at the oracle's centre were searched by the oracle, so either k_me_spec listed them at that centre or the
             chain searched them itself; both ends are compared, and the test prints which it was.
  walk       ST2N / ST2 against the walk model (walk_compare of test_gpu_walk_dense.py), and slot 41 of every crowded
             partition whose summary the model decides (MeModel.crowded_summary): the fallback bit, nbig and the listed
             count.  Each cause of the bit named for the pair must be seen SET on a compared partition.
  no_spec    TUNE_SPECULATE 0: the chain runs stage2_list (select_topk_ex, resolve_crowded, the re-walk) for every searched
             partition.  MBTYPE, MV, MVD against the oracle, the stage-3 lists against the speculating run.
  streams    IDR, P, P through encode_picture: RBSP and reconstruction against the oracle, the streams through
             decode_streams against the oracle's decoder.
"""
import numpy as np
import pytest

import pan_content as pc
import route_content as rc
from me_model import unpack_xy
from test_gpu_me_lists import check_stream, gpu_state
from test_gpu_walk_dense import walk_compare

pytestmark = pytest.mark.gpu

CASES = [(n, w) for n in sorted(rc.PAIRS) for w in (16, 32)]
_states = {}  # (with rc._analysis: models, recordings and ST2 read-backs of every case stay for the session; fine at QCIF)
# what k_me_spec's lists meet at its OWN guessed centres (the probe of far_below is guessed off centre: nothing there)
SPEC_MEETS = {"far_above": ("mixed_t0",), "far_all": ("general_t0",)}


def _state(pkg, name, window, speculate=True):
    """the read-backs of one inter_encoding() of the pair; run once per argument set and shared"""
    key = (name, window, speculate)
    if key not in _states:
        W, H, _ = rc.PAIRS[name]
        ref, src = rc.pair(name)
        _states[key] = gpu_state(pkg, W, H, window, rc.MAXDIFF, [ref], [src], speculate=speculate, extra=("ST2",))[0]
    return _states[key]


def _against_oracle(tag, st, mbt, omv, mbw):
    assert np.array_equal(st["MBTYPE"], mbt), (tag, "MBTYPE", np.flatnonzero(st["MBTYPE"] != mbt)[:8])
    mv = st["MV"].reshape(-1, 4, 2)
    bad = np.flatnonzero((mv != omv).any((1, 2)))
    assert bad.size == 0, (tag, "MV", bad[:8], mv[bad[0]].tolist(), omv[bad[0]].tolist())
    want = pc.mvd_of(omv.astype(np.int64), mbt, mbw)
    bad = np.flatnonzero((st["MVD"].reshape(-1, 4, 2) != want).any((1, 2)) & (mbt != pc.P_SKIP))
    assert bad.size == 0, (tag, "MVD", bad[:8])


@pytest.mark.parametrize("name,window", CASES)
def test_walk_and_summary(pkg, fo, name, window):
    W, H, _ = rc.PAIRS[name]
    an = rc.analysis(fo, name, window)
    st = _state(pkg, name, window)
    _, src = rc.pair(name)
    walk_compare(name, an["model"].walkm, src[: W * H].reshape(H, W), st["ST2N"], st["ST2"])
    seen = dict(a=0, b=0, c=0, compared=0, undecided=0)
    for p, cs in an["crowded"].items():
        assert st["ST2N"][p] > 384, (name, p)
        assert st["ST2"][p, 40, 0] == cs["J"], (name, p)
        if cs["undecided"]:
            seen["undecided"] += 1
            continue
        w = int(st["ST2"][p, 41, 1])
        seen["compared"] += 1
        assert bool(w & 0x40000000) == cs["fallback"], (name, p, hex(w), cs)
        assert (w >> 16) & 15 == cs["nbig"], (name, p, hex(w), cs)
        if cs["np2"] is not None:
            assert w & 0xffff == min(cs["np2"], 320), (name, p, hex(w), cs)
        for k in "abc":
            seen[k] += cs[k] and bool(w & 0x40000000)
    print("me_routes summary", name, window, seen)
    for k in rc.REACHES[name]:
        if k in "abc":
            assert seen[k] > 0, (name, window, "cause", k, "not seen set")


@pytest.mark.parametrize("name,window", CASES)
def test_lists(pkg, fo, name, window):
    W, H, _ = rc.PAIRS[name]
    an = rc.analysis(fo, name, window)
    _, rec, mbt, omv, _ = an["orc"]
    m = an["model"]
    st = _state(pkg, name, window)
    _against_oracle((name, window), st, mbt, omv, W // 16)
    c = check_stream((name, window), st, rec, omv.reshape(-1, 2), m, W, H)
    # what k_me_spec met at ITS centres, and who ran the partitions named at the oracle's
    hdr = st["SPEC_HDR"]
    spec = dict(general_t0=0, straddle=0, mixed_t0=0)
    by_spec = by_chain = 0
    for p in range(hdr.shape[0]):
        listed = bool((int(hdr[p, 1]) >> 16) & 1)
        gx, gy = (int(v) for v in unpack_xy(hdr[p, 0]))
        if listed and int(st["ST2N"][p]) <= 384:
            r = m.stage2_routes(p, gx, gy)
            for k in spec:
                spec[k] += r[k]
        named = p in an["routes"] and any(an["routes"][p][k] for k in spec)
        cs = an["crowded"].get(p)
        named = named or (bool(rec["searched"][p]) and cs is not None and not cs["undecided"] and cs["fallback"])
        if named:
            # The oracle searched the partition, so the device's chain decided it too (MBTYPE above is not P_Skip there).
            # Its lists are k_me_spec's when bit 16 is set and the guessed centre is the true one (check_stream compared
            # them with the model AT that centre, and the final vector with their first minimum); otherwise the chain ran
            # its own stage2_list at the true centre, and what the device shows of that is the final vector alone, held to
            # the oracle's here once more.
            assert rec["searched"][p] and mbt[p // 4] != pc.P_SKIP, (name, p)
            hit = listed and (gx, gy) == (int(rec["mvp"][p, 0]) >> 2, int(rec["mvp"][p, 1]) >> 2)
            assert st["MV"][p].tolist() == omv.reshape(-1, 2)[p].tolist(), (name, p, "final vector of a named partition", hit)
            by_spec += hit
            by_chain += not hit
    print("me_routes lists", name, window, c, "k_me_spec's own centres:", spec, "named partitions run by k_me_spec / the chain:", by_spec, by_chain)
    assert by_spec + by_chain > 0, (name, window, "no named partition")
    # k_me_spec's own centre follows from V0 by the predictor rules (check_stream), so what it meets there is the model's to say
    for k in SPEC_MEETS.get(name, ()):
        assert spec[k] > 0, (name, window, k, "not met at any of k_me_spec's own centres")


@pytest.mark.parametrize("name,window", CASES)
def test_without_speculation(pkg, fo, name, window):
    W, H, _ = rc.PAIRS[name]
    an = rc.analysis(fo, name, window)
    _, rec, mbt, omv, _ = an["orc"]
    on, off = _state(pkg, name, window), _state(pkg, name, window, speculate=False)
    _against_oracle((name, window, "no speculation"), off, mbt, omv, W // 16)
    for n in ("ST3N", "SUMA", "V0", "ST2N"):
        assert np.array_equal(on[n], off[n]), (name, n)
    for p in range(on["ST3N"].size):
        k = int(on["ST3N"][p])
        assert np.array_equal(on["ST3"][p, :k], off["ST3"][p, :k]), (name, p)


STREAMS = ("far_below", "far_above", "far_all", "many_flats")


@pytest.mark.parametrize("window", [16, 32])
def test_whole_streams(pkg, fo, window):
    """reference, source, reference again coded IDR, P, P at QP 12, four streams in one context"""
    W, H = rc.QCIF
    seqs = np.stack([np.stack([rc.pair(n)[k] for n in STREAMS]) for k in (0, 1, 0)])  # [T][S][fsz]
    types, S = (5, 1, 1), len(STREAMS)
    g = pkg.FerHip(W, H, S, qp=12, window=window, maxdiff=rc.MAXDIFF, intra_every=1000)
    try:
        pics = []
        for t, nt in enumerate(types):
            g.set_frames(seqs[t])
            rbsp, got = g.encode_picture(nal_types=[nt] * S)
            assert got == [nt] * S
            pics.append((rbsp, g.get_recon()))
        assert g.status() == [0] * S
        streams = [b"".join(g.sps_pps(s)) + b"".join(g.write_nal(nt, p[0][s]) for nt, p in zip(types, pics)) for s in range(S)]
    finally:
        g.close()
    for s, name in enumerate(STREAMS):
        o = fo.Oracle(W, H, qp=12, window=window, maxdiff=rc.MAXDIFF, intra_every=1000)
        for t, nt in enumerate(types):
            o.set_frame(seqs[t, s])
            want = o.encode_slice(nt)
            assert pics[t][0][s] == want, (name, t, "RBSP", len(pics[t][0][s]), len(want))
            assert np.array_equal(pics[t][1][s], o.frame()), (name, t, "reconstruction")
        o.close()
    out, n, w, h = pkg.decode_streams(streams, len(types))
    assert n == [len(types)] * S and (w, h) == (W, H)
    for s, name in enumerate(STREAMS):
        k, dec, _ = fo.decode_stream_md5(streams[s])
        assert k == len(types)
        for t in range(k):
            assert np.array_equal(out[t, s], dec[t]), (name, t, "decoded picture")
