"""brojTipova (stats()) is counted once per picture from mb_type (k_type_count) instead of by one atomic per macroblock.

Every case steps the oracle picture by picture next to the GPU and compares the five counters of every stream after EVERY
call, not only at the end: counts accumulate over pictures, a stream that codes an I picture or sits a call out keeps
its counts, ferhip_reset_stream zeroes them, a P_Skip counts twice under BasicInterEncoding, and the staged entry point
(inter_encoding) counts like encode_picture.  Sizes: one macroblock, a few, and 99 (more than one wavefront of the
counting kernel's stride and a ragged last one).  Every comparison is exact equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDR, SLICE, NONE = 5, 1, -1


class Ref:
    """the oracle, one picture at a time (what fo_encode_stream does per picture)"""

    def __init__(self, fo, W, H, **kw):
        self.fo, self.W, self.H, self.kw = fo, W, H, kw
        self.o = fo.Oracle(W, H, **kw)

    def picture(self, frame, nal=None):
        self.o.set_frame(frame)
        t = int(self.o.L.fo_select_nal_type(self.o.c)) if nal is None else nal
        rbsp = self.o.encode_slice(t)
        return t, rbsp

    def stats(self):
        return [int(v) for v in self.o.stats()]

    def reset(self):
        self.o.close()
        self.o = self.fo.Oracle(self.W, self.H, **self.kw)

    def close(self):
        self.o.close()


def _frames(pkg, W, H, T, S, still=()):
    return np.stack([np.stack([pkg.gen_frame(W, H, 0 if s in still else t, 1234 + s, 0 if s in still else 2) for s in range(S)])
                     for t in range(T)])


def _run(pkg, fo, W, H, S, frames, plan=None, reset_at=None, **kw):
    """plan[t][s] = NAL type request of stream s in call t (None = AUTO for all); reset_at = (t, s): stream s is reset before
    call t.  Compares RBSP, NAL types and stats() of every stream after every call; returns the final counts."""
    T = frames.shape[0]
    g = pkg.FerHip(W, H, S, maxdiff=3, **kw)
    refs = [Ref(fo, W, H, maxdiff=3, **kw) for _ in range(S)]
    try:
        for t in range(T):
            if reset_at and reset_at[0] == t:
                g.reset_stream(reset_at[1])
                refs[reset_at[1]].reset()
            req = None if plan is None else plan[t]
            pics = [None if req is not None and req[s] == NONE else frames[t, s] for s in range(S)]
            rbsp, nt = g.encode_live(pics, None if req is None else list(req))
            assert g.status() == [0] * S
            got = g.stats()
            for s in range(S):
                if pics[s] is None:
                    assert nt[s] == NONE and rbsp[s] == b""
                else:
                    want_t, want = refs[s].picture(frames[t, s], None if req is None or req[s] == 0 else req[s])
                    assert nt[s] == want_t, f"call {t} stream {s}: NAL type"
                    assert rbsp[s] == want, f"call {t} stream {s}: RBSP"
                assert [int(v) for v in got[s]] == refs[s].stats(), f"call {t} stream {s}: brojTipova {got[s]} vs {refs[s].stats()}"
        return g.stats()
    finally:
        g.close()
        for r in refs:
            r.close()


@pytest.mark.parametrize("W,H,S", [(16, 16, 1), (48, 32, 1), (176, 144, 3)])
def test_counts_after_every_picture_with_intra_every_3(pkg, fo, W, H, S):
    """six pictures, IntraEvery 3: I P P I P P -- the I pictures leave the counts alone, the P pictures add to them"""
    frames = _frames(pkg, W, H, 6, S)
    st = _run(pkg, fo, W, H, S, frames, qp=12, window=16, intra_every=3)
    assert all(int(st[s].sum()) == 4 * (W // 16) * (H // 16) for s in range(S))  # every macroblock of the four P pictures, once


def test_absent_streams_and_a_reset_in_the_middle(pkg, fo):
    """stream 1 sits out every other call, stream 2 is reset before call 3 (its counts go back to zero, its next picture
    is an IDR); stream 0 runs through"""
    W, H, S, T = 176, 144, 3, 6
    frames = _frames(pkg, W, H, T, S)
    plan = [[0, NONE if t % 2 else 0, 0] for t in range(T)]
    st = _run(pkg, fo, W, H, S, frames, plan=plan, reset_at=(3, 2), qp=12, window=16, intra_every=30)
    nmb = 99
    assert [int(st[s].sum()) for s in range(S)] == [5 * nmb, 2 * nmb, 2 * nmb]


def test_explicit_mixed_types_in_one_call(pkg, fo):
    """I and P pictures side by side in one call, a different stream each time: only the P streams are counted"""
    W, H, S = 176, 144, 3
    plan = [[IDR, IDR, IDR], [SLICE, IDR, SLICE], [IDR, SLICE, SLICE], [SLICE, SLICE, IDR], [SLICE, SLICE, SLICE]]
    frames = _frames(pkg, W, H, len(plan), S)
    st = _run(pkg, fo, W, H, S, frames, plan=plan, qp=12, window=16, intra_every=1000)
    assert [int(st[s].sum()) for s in range(S)] == [3 * 99, 3 * 99, 3 * 99]


@pytest.mark.parametrize("W,H", [(48, 32), (176, 144)])
def test_basic_inter_encoding(pkg, fo, W, H):
    """BasicInterEncoding = 1: the discarded exhaustive pass adds its own 16x16 / 8x8 verdict per non-skipped macroblock
    (k_basic_stat) on top of the final types, and a P_Skip counts twice; stream 1 is a still sequence"""
    S, T = 2, 3
    frames = _frames(pkg, W, H, T, S, still=(1,))
    st = _run(pkg, fo, W, H, S, frames, qp=12, window=16, intra_every=30, basic=1)
    nmb = (W // 16) * (H // 16)
    assert int(st[0].sum()) == 2 * (T - 1) * nmb and int(st[1].sum()) == 2 * (T - 1) * nmb  # two counts per macroblock either way
    assert st[1][0] > 0 and st[1][0] % 2 == 0


@pytest.mark.parametrize("basic", [0, 1])
def test_still_content_is_all_p_skip(pkg, fo, basic):
    """a still sequence without noise: every macroblock of every P picture is a P_Skip, counted once, or twice under
    BasicInterEncoding -- the counts come from k_me_resolve's mb_type alone (k_p_resid merges nothing)"""
    W, H, T = 176, 144, 4
    frames = _frames(pkg, W, H, T, 1, still=(0,))
    st = _run(pkg, fo, W, H, 1, frames, qp=12, window=16, intra_every=30, basic=basic)
    assert [int(v) for v in st[0]] == [(2 if basic else 1) * 99 * (T - 1), 0, 0, 0, 0]


def test_staged_entry_point_counts_like_encode_picture(pkg, fo):
    """inter_encoding() (motion search and residual without entropy coding) on the same reference and source as
    encode_picture: the same counts and the same mb_type"""
    W, H, S = 176, 144, 2
    frames = _frames(pkg, W, H, 2, S, still=(1,))
    a = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    b = pkg.FerHip(W, H, S, qp=12, window=16, maxdiff=3, intra_every=30)
    try:
        a.set_frames(frames[0])
        a.encode_picture()
        rec0 = a.get_recon()
        assert not a.stats().any()
        a.set_frames(frames[1])
        _, nt = a.encode_picture()
        assert nt == [SLICE] * S
        b.set_reference(rec0)
        b.set_frames(frames[1])
        b.inter_encoding()
        assert a.status() == [0] * S and b.status() == [0] * S
        sa, sb = a.stats(), b.stats()
        assert np.array_equal(a.read("MBTYPE"), b.read("MBTYPE"))
        assert np.array_equal(sa, sb), f"{sa} vs {sb}"
        assert int(sa[0].sum()) == 99 and sa[1][0] > 0
        mt = b.read("MBTYPE").reshape(S, 99)
        for s in range(S):  # the counts are the histogram of the types the picture left
            assert [int((mt[s] == v).sum()) for v in (31, 0, 1, 2, 4)] == [int(v) for v in sb[s]]
            r = Ref(fo, W, H, qp=12, window=16, maxdiff=3, intra_every=30)
            r.picture(frames[0, s])
            r.picture(frames[1, s])
            assert r.stats() == [int(v) for v in sb[s]]
            r.close()
    finally:
        a.close()
        b.close()
