"""The inputs of tests/test_gpu_sel_routes.py reach every route of the selection at every site where it can be reached
(no GPU): the lane model of sel_model.py names the route of every selection the device has to run on them.

  stage 3 (k_me_pre, behind the pruned wide search)   all three routes on each of the five content kinds, both windows
  stage 3 behind the full evaluation                  runs on each of the five kinds (whenever the pruned route did not deliver)
  stage 2                                             "exact_fits" on ramp21a3, "both_over" on flat-half, both windows
  stage 1                                             "exact_fits" on ramp21a2 (window 32) and ramp31a2 (window 16),
                                                      "both_over" on patch (32) and ramp31a2 (16)
  stage-2 list lengths                                <= 192 everywhere, 193 .. 384 on flat-half and soft, > 384 (crowded)
                                                      on patch, and a winner of arrival index >= 192 on ramp21a2
The model's own statement of the code layout is held to the header's through the figures both must give.
"""
import numpy as np
import pytest

import sel_model as sm
from me_model import KINDS

CASES = [(n, w) for n in sm.INPUTS for w in (16, 32)]


def test_code_layout():
    """code and threshold as fer_sel_thr.h states them (tools/sel_thr_host_check.cpp sweeps the header itself)"""
    assert sm.code_of((1 << 21) - 1) == 151 and sm.thr(151) == (1 << 21) - 1
    prev = -1
    for t in sorted(set(range(0, 5000)) | {(1 << k) + d for k in range(12, 21) for d in (-1, 0, 1)} | {(1 << 21) - 1}):
        c = sm.code_of(t)
        th = sm.thr(c)
        assert t <= th < (1 << 21) and sm.code_of(th) == c and (th == (1 << 21) - 1 or sm.code_of(th + 1) == c + 1), t
        assert th == t if t < 8 else th <= t + (t >> 3) - 1, t
        assert c >= prev, t
        prev = c


def test_route_of_small_sets():
    v = np.full((3, 64), -1)
    assert sm.route(v, 33)[0] is None
    v[0, :40] = np.arange(40) * 8 + 100  # 40 lanes, distinct: need 33 -> exact = 100 + 32 * 8, everything under the coarse bound fits
    assert sm.route(v, 33)[0] == "coarse_fits"
    v[:] = 1000  # 192 equal candidates
    assert sm.route(v, 33)[0] == "both_over"
    v[:] = 1 << 22
    assert sm.route(v, 33)[0] == "general"
    v[:] = -1
    v[0] = 1000 + np.arange(64)  # 33rd smallest minimum 1032 = 0b1000 0001000: its granule is 1024 .. 1151, and the second batch decides
    v[1, :40] = 1040
    r, f = sm.route(v, 33)
    assert (r, f["exact"], f["coarse"], f["under_exact"], f["under_coarse"]) == ("exact_fits", 1032, 1151, 33, 104)


@pytest.mark.parametrize("name,window", CASES)
def test_routes_reached(fo, name, window):
    r = sm.analysis(fo, name, window)["routes"]
    count = lambda site: {k: r[site].count(k) for k in sm.ROUTES + (None, "crowded") if r[site].count(k)}
    n2 = np.asarray(r["n2"])
    print("sel routes", name, window, "st3", count("st3"), "st3 full", count("st3_full"), "st1", count("st1"), "st2", count("st2"),
          "n2 <=192 / 193..384 / >384:", int((n2 <= 192).sum()), int(((n2 > 192) & (n2 <= 384)).sum()), int((n2 > 384).sum()), "late winners", r["late"])
    assert (n2 <= 192).any()
    if name in KINDS:
        assert r["st3_full"], "the full evaluation's selection runs"
        for k in ("coarse_fits", "exact_fits", "both_over"):
            assert k in r["st3"], (name, window, "stage 3", k)
    if name == "ramp21a3":
        assert "exact_fits" in r["st2"]
    if name == "flat-half":
        assert "both_over" in r["st2"]
        assert ((n2 > 192) & (n2 <= 384)).any()
    if name == "soft":
        assert ((n2 > 192) & (n2 <= 384)).any()
    if name == "patch":
        assert "crowded" in r["st2"] and (n2 > 384).any()
    if (name, window) in (("ramp21a2", 32), ("ramp31a2", 16)):
        assert "exact_fits" in r["st1"]
    if (name, window) in (("patch", 32), ("ramp31a2", 16)):
        assert "both_over" in r["st1"]
    if name == "ramp21a2":
        assert r["late"] > 0, "no stage-2 winner of arrival index >= 192"
