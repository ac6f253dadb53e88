"""k_me_resolve asks for the guessed lists of a step one step before it prices them (fer_chain_idx.h, RES_AHEAD).

What can go wrong with that is addressing and bookkeeping, not arithmetic: a request past the end of a short row or of the
arrays, a rotation that is not started afresh for a row (after a ticket, after rows that name nothing, for streams that code
no P picture), lists staged where none exist (speculation off), and a wrong guess whose own search has to leave the
staged operands of the NEXT step intact.  Every case compares every stream with the oracle byte for byte: bitstream,
reconstruction and brojTipova, the way tests/test_gpu_full.py does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDR, SLICE, NONE = 5, 1, -1
QP = 12

_frames_cache = {}
_oracle_cache = {}


def _frames(pkg, W, H, s, times, noise):
    """[T][fsz] of stream s, computed once and never modified"""
    k = (W, H, s, tuple(times), noise)
    if k not in _frames_cache:
        a = np.stack([pkg.gen_frame(W, H, t, 1234 + s, noise) for t in times])
        a.setflags(write=False)
        _frames_cache[k] = a
    return _frames_cache[k]


def _oracle(fo, key, frames, W, H, window):
    k = (key, W, H, window)
    if k not in _oracle_cache:
        o = fo.Oracle(W, H, qp=QP, window=window, maxdiff=3, intra_every=30)
        ref, ref_rec = o.encode_stream(frames)
        cnt = [int(v) for v in o.stats()]
        o.close()
        _oracle_cache[k] = (ref, ref_rec, cnt)
    return _oracle_cache[k]


def _encode_and_compare(pkg, fo, W, H, S, window, times, noise, tune=(), streams=None):
    """encode_streams of S streams under the tuning; the streams listed (all by default) against the oracle.
    -> SPEC_STAT (partitions decided by the chain, guess hits, P_Skip verdicts, of them from the guess)"""
    per = [_frames(pkg, W, H, s, times, noise) for s in range(S)]
    frames = np.stack(per, axis=1)
    g = pkg.FerHip(W, H, S, qp=QP, window=window, maxdiff=3, intra_every=30)
    for k, v in tune:
        g.tune(k, v)
    got, rec = g.encode_streams(frames, want_recon=True)
    assert g.status() == [0] * S, f"status {g.status()} (bit 5 = chain timeout)"
    counts = g.stats()
    st = [int(v) for v in g.read("SPEC_STAT")[:4]]
    g.close()
    for s in (range(S) if streams is None else streams):
        ref, ref_rec, ref_counts = _oracle(fo, (s, tuple(times), noise), per[s], W, H, window)
        assert got[s] == ref, f"bitstream of stream {s}"
        assert np.array_equal(rec[:, s], ref_rec), f"reconstruction of stream {s}"
        assert [int(v) for v in counts[s]] == ref_counts, f"brojTipova of stream {s}"
    return st


@pytest.mark.parametrize("window", [16, 32, 48])
@pytest.mark.parametrize("W,H", [(16, 16), (32, 16), (16, 48), (48, 32), (80, 48)])
def test_rows_shorter_than_the_prefetch_distance_and_the_window(pkg, fo, W, H, window):
    """Rows of 2, 4, 2, 6 and 10 partitions: the step asked for is clamped in most steps of a row, and a row ends before
    the first window over the row above is used up.  I + 2 P, noise 1; one stream (one ticket queue) and 17 (eight);
    1, 3 and 64 workgroups: with one, every row's rotation starts in the workgroup that has just finished another."""
    for S in (1, 17):
        for wgs in (1, 3, 64):
            st = _encode_and_compare(pkg, fo, W, H, S, window, (0, 1, 2), 1, tune=((pkg.TUNE_RESOLVE_WGS, wgs),))
            assert st[2] == S * 2 * (W // 16) * (H // 16), (S, wgs, st)  # one P_Skip verdict per macroblock of a P picture


@pytest.mark.parametrize("S,wgs", [(1, 1), (17, 3)])
def test_speculation_off_stages_nothing(pkg, fo, S, wgs):
    """TUNE_SPECULATE 0: k_me_spec does not run, its lists do not exist, the chain searches every partition itself"""
    st = _encode_and_compare(pkg, fo, 80, 48, S, 16, (0, 1, 2), 1, tune=((pkg.TUNE_SPECULATE, 0), (pkg.TUNE_RESOLVE_WGS, wgs)))
    assert st[0] > 0 and st[1] == 0 and st[3] == 0, st


def test_rows_that_name_nothing_between_rows_that_do(pkg, fo):
    """17 streams of 48x32, picture by picture.  In the second call stream 3 codes an IDR and stream 5 has no picture: the
    tickets of their rows name nothing to do, and the workgroup that draws one goes on to a row of another stream with
    a fresh rotation.  Every stream, after every call, against an oracle of its own that is given the same pictures."""
    W, H, S, T = 48, 32, 17, 3
    per = [_frames(pkg, W, H, s, (0, 1, 2), 1) for s in range(S)]
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    g.tune(pkg.TUNE_RESOLVE_WGS, 3)
    refs = [fo.Oracle(W, H, qp=QP, window=16, maxdiff=3, intra_every=30) for _ in range(S)]
    try:
        for t in range(T):
            req = [0] * S
            if t == 1:
                req[3], req[5] = IDR, NONE
            pics = [None if req[s] == NONE else per[s][t] for s in range(S)]
            rbsp, nt = g.encode_live(pics, req)
            assert g.status() == [0] * S
            rec = g.get_recon()
            counts = g.stats()
            for s in range(S):
                if pics[s] is None:
                    assert nt[s] == NONE and rbsp[s] == b""
                    continue
                o = refs[s]
                o.set_frame(per[s][t])
                want_t = req[s] if req[s] else int(o.L.fo_select_nal_type(o.c))
                want = o.encode_slice(want_t)
                assert nt[s] == want_t, f"call {t} stream {s}: NAL type"
                assert rbsp[s] == want, f"call {t} stream {s}: RBSP"
                assert np.array_equal(rec[s], o.frame()), f"call {t} stream {s}: reconstruction"
                assert [int(v) for v in counts[s]] == [int(v) for v in o.stats()], f"call {t} stream {s}: brojTipova"
            if t == 1:
                assert [nt[s] for s in (2, 3, 4, 5)] == [SLICE, IDR, SLICE, NONE]
    finally:
        g.close()
        for o in refs:
            o.close()


def test_hits_and_misses_in_one_row(pkg, fo):
    """176x144, 17 streams, four pictures whose motion changes from picture to picture (the source at times 0, 1, 3, 2:
    one step forward, two forward, one back), so that the guessed predictor is right for most partitions and wrong for
    some in the same rows: a wrong guess runs the chain's own search between two steps that price staged lists."""
    st = _encode_and_compare(pkg, fo, 176, 144, 17, 16, (0, 1, 3, 2), 2)
    parts, hits, skq, skh = st
    print("SPEC_STAT: partitions %d, guess hits %d, P_Skip verdicts %d, from the guess %d" % (parts, hits, skq, skh))
    assert 0 < hits < parts, st


@pytest.mark.parametrize("W,H", [(16, 16), (208, 112)])
def test_the_last_entries_of_the_arrays(pkg, fo, W, H):
    """The last row of the last stream ends where spec_hdr, spec_l1, spec_l2, st3 and st3n end: its last steps are the
    ones whose clamp matters.  One stream, and the last of 17."""
    _encode_and_compare(pkg, fo, W, H, 1, 16, (0, 1, 2), 1)
    _encode_and_compare(pkg, fo, W, H, 17, 16, (0, 1, 2), 1, streams=(16,))
