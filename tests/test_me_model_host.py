"""The list model of me_model.py against the lists the oracle records (no GPU).

One I and one P picture per case through the oracle with Oracle.record_me(); for EVERY partition the oracle searched
the model's stage-3 list, and its stage-1 and stage-2 lists at the oracle's own centre (mvp >> 2), must be the recorded
ones: vectors, order, count, metrics and SADs.  Nothing is left out.  The predictor restatement predict_8x8 (what
k_me_spec's guess is checked with on the GPU) is checked here against the oracle's recorded predictors, and the P_Skip
counts the GPU module's caps rest on are pinned.
"""
import numpy as np
import pytest
from me_model import KINDS, MAXDIFF, model_for, oracle_pair, predict_8x8
from test_gpu_walk_dense import H, W, _content


def assert_list(got, rec, p, st, what):
    """a model list == list `st` of partition p of the oracle's recording"""
    n = int(rec["n"][p, st])
    assert got["n"] == n, (what, p, got["n"], n)
    for key, name in (("vx", "bx"), ("vy", "by"), ("metric", "metric"), ("sad", "sad")):
        assert np.array_equal(got[key], rec[name][p, st, :n]), (what, p, name, got[key].tolist(), rec[name][p, st, :n].tolist())


@pytest.mark.parametrize("kind,window", [(k, w) for k in KINDS for w in (16, 32)] + [("textured", 48)])
def test_model_lists_equal_the_oracle(fo, kind, window):
    f0, f1 = _content(fo, kind, 0), _content(fo, kind, 1)
    rec0, rec, mbt, mv, _ = oracle_pair(fo, f0, f1, W, H, window, MAXDIFF.get(kind, 3))
    m = model_for(fo, rec0, f1, W, H, window)
    searched = np.nonzero(rec["searched"])[0]
    assert searched.size >= 4 * 50, "the case must search most of the picture"
    field = mv.reshape(-1, 2)
    for p in searched:
        p = int(p)
        assert m.sums(p) == rec["suma"][p].tolist(), (kind, p)
        mvpx, mvpy = (int(v) for v in rec["mvp"][p])
        assert predict_8x8(field, W // 16, p) == (mvpx, mvpy), (kind, p)
        assert_list(m.stage3(p), rec, p, 2, "stage 3")
        assert_list(m.stage1(p, mvpx >> 2, mvpy >> 2), rec, p, 0, "stage 1")
        assert_list(m.stage2(p, mvpx >> 2, mvpy >> 2), rec, p, 1, "stage 2")


def test_recording_changes_no_output(fo):
    f0, f1 = _content(fo, "patch", 0), _content(fo, "patch", 1)
    outs = []
    for record in (False, True):
        o = fo.Oracle(W, H, qp=12, window=16, maxdiff=3)
        if record:
            o.record_me()
        o.set_frame(f0)
        b0 = o.encode_slice(5)
        o.set_frame(f1)
        b1 = o.encode_slice(1)
        outs.append((b0, b1, o.frame().tobytes(), o.mv().tobytes(), o.mb_type().tobytes()))
        o.close()
    assert outs[0] == outs[1]


def test_pskip_counts_the_gpu_caps_rest_on(fo):
    """At MAXDIFF 3 the oracle codes this many of the 99 macroblocks as P_Skip (they have no k_me_spec lists to compare)."""
    want = {"textured": 0, "patch": 1, "letterbox": 22, "flat-half": 45, "soft": 99}
    for kind, n in want.items():
        *_, skips = oracle_pair(fo, _content(fo, kind, 0), _content(fo, kind, 1), W, H, 32, 3)
        assert skips == n, (kind, skips)
    *_, skips = oracle_pair(fo, _content(fo, "soft", 0), _content(fo, "soft", 1), W, H, 32, MAXDIFF["soft"])
    assert 2 * skips <= 99, skips
