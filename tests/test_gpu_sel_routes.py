"""The selection's routes on the device: the inputs of sel_model.py -- tests/test_sel_model_host.py shows on the CPU that
they reach the coarse bound that fits, the coarse bound that overflows with the exact one fitting, and both overflowing,
at every call site, and stage-2 lists of <= 192, 193 .. 384 and > 384 candidates -- at windows 16 and 32.

Every comparison is exact equality, through the harness of test_gpu_me_lists.py: check_stream (SUMA, ST3N, ST3 and V0
against the oracle's recording / the model, the guessed centres, SPEC_L1 / SPEC_L2 against the model and, where the guess
is right, the oracle, the final vectors), ST2N against the walk model, MBTYPE, MV and MVD against the oracle.  Without
speculation the chain runs stage 1 and stage 2 of every searched partition itself, at the oracle's centre -- the
selections the host module names -- and MBTYPE, MV, MVD must be the oracle's again, the stage-3 lists the same.
"""
import numpy as np
import pytest

import sel_model as sm
from test_gpu_me_lists import check_stream, gpu_state
from test_gpu_me_routes import _against_oracle

pytestmark = pytest.mark.gpu

CASES = [(n, w) for n in sm.INPUTS for w in (16, 32)]
W, H = sm.W, sm.H


def _check(tag, st, an):
    _, rec, mbt, omv, _ = an["orc"]
    m = an["model"]
    _against_oracle(tag, st, mbt, omv, W // 16)
    c = check_stream(tag, st, rec, omv.reshape(-1, 2), m, W, H)
    for p in range(st["ST2N"].size):
        n = int(m.stage2_candidates(p)[0].size)
        assert (st["ST2N"][p] == n) if n <= 384 else (st["ST2N"][p] > 384), (tag, p, "st2n", int(st["ST2N"][p]), n)
    return c


@pytest.mark.parametrize("name,window", CASES)
def test_lists_with_and_without_speculation(pkg, fo, name, window):
    an = sm.analysis(fo, name, window)
    rec0, rec, mbt, omv, _ = an["orc"]
    on = gpu_state(pkg, W, H, window, sm.maxdiff_of(name), [rec0], [an["f1"]])[0]
    c = _check((name, window), on, an)
    print("sel_routes", name, window, c)
    assert c["hit"] > 0 and c["nolist"] < c["parts"], c
    off = gpu_state(pkg, W, H, window, sm.maxdiff_of(name), [rec0], [an["f1"]], speculate=False)[0]
    _against_oracle((name, window, "no speculation"), off, mbt, omv, W // 16)
    for n in ("ST3N", "SUMA", "V0", "ST2N"):
        assert np.array_equal(on[n], off[n]), (name, n)
    for p in range(on["ST3N"].size):
        k = int(on["ST3N"][p])
        assert np.array_equal(on["ST3"][p, :k], off["ST3"][p, :k]), (name, p)


@pytest.mark.parametrize("window", [16, 32])
def test_three_streams_mix_the_routes(pkg, fo, window):
    """flat-half, patch and a ramp in one launch: neighbouring wavefronts take different routes"""
    names = ("flat-half", "patch", "ramp21a3")
    ans = [sm.analysis(fo, n, window) for n in names]
    sts = gpu_state(pkg, W, H, window, 0, [a["orc"][0] for a in ans], [a["f1"] for a in ans])
    for name, st, an in zip(names, sts, ans):
        if sm.maxdiff_of(name) == 0:  # (one MAXDIFF per context: the recording of the others was made at 3)
            _check((name, window, "three streams"), st, an)
        else:  # the lists do not depend on MAXDIFF: stage 3 of every partition against the single-stream run's model
            m = an["model"]
            for p in range(st["ST3N"].size):
                mod = m.stage3(p)
                assert st["ST3N"][p] == mod["n"], (name, p)
                assert np.array_equal(st["ST3"][p, :mod["n"]], np.stack([mod["vx"], mod["vy"], mod["sad"]], -1)), (name, p)
