"""What every decoder here has to make of the illegal (slice_synth.ILLEGAL_PLANS) and damaged (damage_corpus) streams.

Test infrastructure shared by test_decode_illegal_host.py and test_gpu_decode_illegal.py.  The reference's verdict is the
record tests/golden/illegal_decode_record.json (make_illegal_record.py); the pictures come from the oracle, which the host
test holds to that record.  expectation() turns both into what the device owes:

    complete   the reference decodes the stream: no fault, the oracle's pictures, all of them
    fatal      the reference stops with its own fatal error in picture `good` (0-based): the pictures in front of it,
               then a fault in the call that carries that picture
    refused    the reference decodes on, the device does not, for a reason include/ferhip.h writes down and this module
               recognises FROM THE ORACLE'S TRACE (never from the device): as `fatal`, at the first such picture
    undefined  the reference died of a signal or its time limit, or the stream is on the OPEN list: nothing is compared
"""
import json
from pathlib import Path

import numpy as np

import damage_corpus as dc
import slice_synth as ss

GOLD = Path(__file__).resolve().parent / "golden"
RECORD = GOLD / "illegal_decode_record.json"
CORPUS_MD5 = "fe680d6626de4f6ad6ce1c340f1a8ce8"
# corpus index -> what was found: damaged streams on which the oracle still differs from the record.  (Three did before
# the oracle followed the reference in two more places -- a macroblock parsed behind a skip run that ends the picture, a
# run_before above zerosLeft that stores a level into the block in front -- none does now.)
OPEN = {}
INT16 = 32767
_REFUSE = {1: "mb_type above 24 in an I slice", 2: "a code no CAVLC table holds"}  # fo.h FO_REFUSE_*

_record = None
_verdicts = {}


def record():
    global _record
    if _record is None:
        _record = json.loads(RECORD.read_text())
    return _record


def tier1():
    """-> [(key "plan[seed]", plan, W, H, stream, record entry)]"""
    out = []
    for name in sorted(ss.ILLEGAL_PLANS):
        cfg, _, seeds = ss.ILLEGAL_PLANS[name]
        for seed, (stream, _, _) in zip(seeds, ss.illegal_streams(name)):
            key = f"{name}[{seed}]"
            out.append((key, name, cfg["mbw"] * 16, cfg["mbh"] * 16, stream, record()["tier1"][key]))
    return out


def tier2():
    """-> [(corpus index, name, golden, stream, record entry)]"""
    return [(i, name, golden, stream, record()["tier2"][i]) for i, (name, golden, stream) in enumerate(dc.corpus())]


def verdict(fo, key, stream):
    """the oracle's decode of the stream (fo_py.decode_stream_verdict), computed once per key"""
    if key not in _verdicts:
        _verdicts[key] = fo.decode_stream_verdict(stream)
    return _verdicts[key]


def refusal(v):
    """-> (picture index, reason) of the first picture the oracle delivered that the device may refuse, or (None, None).
    The reasons are those of include/ferhip.h ("What the decoders refuse"), read off the oracle's trace."""
    for t in range(len(v["frames"])):
        if v["block_overrun"][t] > (v["block_overrun"][t - 1] if t else 0):
            return t, "residual block overrun"
        new = v["refusals"][t] & ~(v["refusals"][t - 1] if t else 0)
        if new:
            return t, _REFUSE[new & -new]
        if v["slice_type"][t] == 0:
            inter = (v["mb_type"][t] <= 4) | (v["mb_type"][t] == ss.P_SKIP)
            if inter.any() and (int(v["mv"][t][inter].min()) < -INT16 - 1 or int(v["mv"][t][inter].max()) > INT16):
                return t, "motion vector past 16 bits"
    new = v["end_refusals"] & ~(v["refusals"][-1] if v["frames"] else 0)
    if new:  # in the picture the oracle ended in (it does not follow the reference past such a code)
        return len(v["frames"]), _REFUSE[new & -new]
    return None, None


def expectation(entry, v, is_open=False):
    """-> dict(kind, good = pictures owed bit for bit, fault = a fault is owed in the call carrying picture `good`, reason)"""
    if entry["class"] == "undefined" or is_open:
        return dict(kind="undefined", good=0, fault=False, reason=entry.get("how", "open"))
    n = len(entry["md5"]) if entry["class"] == "complete" else entry["frame"] - 1
    r, reason = refusal(v)
    if r is not None and r < n:
        return dict(kind="refused", good=r, fault=True, reason=reason)
    return dict(kind=entry["class"], good=n, fault=entry["class"] == "fatal", reason=entry.get("message"))
