"""selectNALUnitType's frame SAD from per-workgroup partials (k_frame_sad, k_frame_sad_sum): exact at the threshold.

Under AUTO a picture whose luma differs from the reference picture by exactly nmb << 12 in total stays a slice, one more
gives an IDR (F/ref_frames.cpp:210-228: strictly greater).  The reference picture is put in place with set_reference after
a first IDR picture, so both sums are known by construction.  Sizes: 16x16 (16 words of 16 bytes: most lanes of the only
workgroup have nothing to read), 208x112 (one workgroup, a ragged last round), 272x256 (two workgroups, 8.5 rounds: the
luma is no multiple of the workgroup's chunk, and the tail launch adds more than one partial).  The difference is
spread over the whole plane (the extra 1 in the first byte), or packed into its last bytes, the extra 1 with it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDR, SLICE, NONE = 5, 1, -1


def _pair(pkg, W, H, seed, where, extra):
    """(reference, current) I420 pictures whose lumas differ by (nmb << 12) + extra in total"""
    ys = W * H
    target = ((W // 16) * (H // 16)) << 12
    ref = pkg.gen_frame(W, H, 0, seed, 2).copy()
    ref[:ys] = np.clip(ref[:ys], 0, 200)
    cur = ref.copy()
    if where == "spread":  # 16 per sample
        cur[:ys] = ref[:ys] + 16
        if extra:
            cur[0] += 1
    else:  # the last bytes of the plane: steps of 255, then the remainder
        n, r = divmod(target, 255)
        assert n + 2 < ys
        ref[ys - n - 2: ys] = 0
        cur[ys - n - 2: ys] = 0
        cur[ys - n: ys] = 255
        cur[ys - n - 1] = r
        if extra:
            cur[ys - n - 2] = 1
    sad = int(np.abs(cur[:ys].astype(np.int64) - ref[:ys].astype(np.int64)).sum())
    assert sad == target + extra
    return ref, cur


def _decisions(pkg, W, H, S, cases, absent=()):
    """cases[k][s] = (where, extra) of stream s in round k -> the NAL types AUTO chose, per round"""
    g = pkg.FerHip(W, H, S, qp=20, window=16, maxdiff=3, intra_every=1000)
    out = []
    try:
        g.set_frames(np.stack([pkg.gen_frame(W, H, 0, 50 + s, 2) for s in range(S)]))
        _, nt = g.encode_picture()
        assert nt == [IDR] * S
        for k, case in enumerate(cases):
            pairs = [_pair(pkg, W, H, 100 + 10 * k + s, *case[s]) for s in range(S)]
            g.set_reference(np.stack([p[0] for p in pairs]))
            _, nt = g.encode_live([None if s in absent else pairs[s][1] for s in range(S)])
            assert g.status() == [0] * S
            out.append(nt)
    finally:
        g.close()
    return out


@pytest.mark.parametrize("W,H", [(16, 16), (208, 112), (272, 256)])
@pytest.mark.parametrize("where", ["spread", "tail"])
def test_exactly_the_threshold_stays_a_slice_one_more_is_an_idr(pkg, W, H, where):
    got = _decisions(pkg, W, H, 1, [[(where, 0)], [(where, 1)], [(where, 0)]])
    assert got == [[SLICE], [IDR], [SLICE]]


def test_three_streams_with_the_middle_one_masked_out(pkg):
    """the absent stream takes no part (its SAD reads 0), its neighbours sit on either side of the threshold and swap"""
    got = _decisions(pkg, 272, 256, 3, [[("tail", 0), ("spread", 1), ("spread", 1)], [("spread", 1), ("tail", 1), ("tail", 0)]], absent=(1,))
    assert got == [[SLICE, NONE, IDR], [IDR, NONE, SLICE]]


def test_every_stream_decides_for_itself(pkg):
    """three present streams in one call: the partials of one stream do not reach another's sum"""
    got = _decisions(pkg, 272, 256, 3, [[("spread", 0), ("tail", 1), ("tail", 0)], [("tail", 1), ("spread", 0), ("spread", 1)]])
    assert got == [[SLICE, IDR, SLICE], [IDR, SLICE, IDR]]
