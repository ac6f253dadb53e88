"""The three decode paths on streams nobody would write on purpose: legal syntax with illegal meaning (prediction modes
that read neighbours which do not exist, vectors far outside the picture and past 16 bits: slice_synth.ILLEGAL_PLANS) and
the fixed corpus of damaged QCIF streams (damage_corpus).  The rule is no silent divergence: on a stream the reference
decodes the device returns the reference's pictures -- the oracle's, which test_decode_illegal_host.py holds to the
record of the reference's own decoder -- or reports a fault for that stream at that picture, and only for a reason
include/ferhip.h writes down (illegal_cases.refusal reads them off the oracle's trace); where the reference stops with a
fatal error the device reports a fault in the same picture; where the reference itself dies only the status is looked at.
A clean stream beside them stays bit-exact throughout."""
import numpy as np
import pytest

import damage_corpus as dc
import illegal_cases as ic
import slice_synth as ss

pytestmark = pytest.mark.gpu
E_HIP, E_UNSUP, E_DEVICE = -2, -4, -5
FAULTS = (E_DEVICE, E_UNSUP)
FILL = 0xA5


def _cases(fo, W, H):
    """-> [(key, stream, expectation, oracle pictures)] of one picture size, and the clean stream + its pictures"""
    out = []
    if (W, H) == (dc.W, dc.H):
        for i, name, golden, stream, e in ic.tier2():
            v = ic.verdict(fo, i, stream)
            out.append((f"corpus {i} ({name})", stream, ic.expectation(e, v, i in ic.OPEN), v["frames"]))
        clean = (ic.GOLD / "qcif_ippp_4f_qp12_w16.264").read_bytes()
    else:
        for key, name, w, h, stream, e in ic.tier1():
            if (w, h) == (W, H):
                v = ic.verdict(fo, key, stream)
                out.append((key, stream, ic.expectation(e, v), v["frames"]))
        clean = ss.make_stream(77, dict(mbw=W // 16, mbh=H // 16), [dict(type="I", qp=22, levels=["small", "mixed"]),
                                                                    dict(type="P", qp=20, levels=["small", "mixed"], p_intra=0.3),
                                                                    dict(type="P", qp=24, levels=["small", "mixed"], p_intra=0.3),
                                                                    dict(type="I", qp=20, levels=["small", "mixed"])])[0]
    return out, (clean, fo.decode_stream_verdict(clean)["frames"])


SIZES = sorted({(w, h) for _, _, w, h, _, _ in ic.tier1()}) + [(dc.W, dc.H)]


@pytest.mark.parametrize("device_in", [False, True], ids=["host_chunks", "device_chunks"])
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_live_decoder_side_by_side(pkg, fo, W, H, device_in):
    """One context per picture size, every stream of that size side by side and the clean one last, one access unit per
    call.  A stream that has reported its fault gets nothing more."""
    cases, (clean, clean_ref) = _cases(fo, W, H)
    aus = [pkg.access_units(s) for _, s, _, _ in cases] + [pkg.access_units(clean)]
    assert len(aus[-1]) == len(clean_ref)
    S, fsz = len(aus), W * H * 3 // 2
    dec = pkg.LiveDecoder(S, W, H, 1)
    ncall = max(len(a) for a in aus)
    pitch = (max(len(c) for a in aus for c in a) + 79) & ~15
    buf = pkg.DeviceBuffer(S * pitch + 64) if device_in else None
    got, fault, seen = [[] for _ in range(S)], [None] * S, [set() for _ in range(S)]
    for c in range(ncall):
        chunks = [a[c] if c < len(a) and fault[s] is None else None for s, a in enumerate(aus)]
        out = np.full((1, S, fsz), FILL, np.uint8)
        if device_in:
            ptrs, lens = [], []
            for s, ch in enumerate(chunks):
                off = s * pitch + (s & 3)  # addresses of every alignment
                if ch:
                    buf.upload(np.frombuffer(ch, np.uint8), off)
                ptrs.append(buf.ptr + off if ch else None)
                lens.append(len(ch) if ch else 0)
            _, pics, status = dec.decode_dev(ptrs, lens, out)
        else:
            _, pics, status = dec.decode(chunks, out)
        for s in range(S):
            seen[s].add(status[s])
            if pics[s]:
                got[s].append(out[0, s].copy())
            else:
                assert (out[0, s] == FILL).all(), f"stream {s} call {c}: a slot without a picture was written"
            if status[s] != 0 and fault[s] is None:
                fault[s] = (c, status[s], pics[s])
    dec.close()
    if buf:
        buf.free()
    assert fault[-1] is None and len(got[-1]) == len(clean_ref) and all(np.array_equal(a, b) for a, b in zip(got[-1], clean_ref)), "the clean stream"
    wrong = []
    for s, (key, _, x, ref) in enumerate(cases):
        if not seen[s] <= {0, E_DEVICE, E_UNSUP}:
            wrong.append(f"{key}: status {sorted(seen[s])}")
        if x["kind"] == "undefined":
            continue
        n = x["good"]
        if len(got[s]) != n:
            wrong.append(f"{key} [{x['kind']}, {x['reason']}]: {len(got[s])} pictures, {n} owed (fault {fault[s]})")
            continue
        bad = [t for t in range(n) if not np.array_equal(got[s][t], ref[t])]
        if bad:
            wrong.append(f"{key} [{x['kind']}]: picture {bad[0]} differs from the oracle's at byte {int(np.nonzero(got[s][bad[0]] != ref[bad[0]])[0][0])}")
        if x["fault"]:
            if fault[s] is None or fault[s][0] != n or fault[s][1] not in FAULTS or fault[s][2] != 0:
                wrong.append(f"{key} [{x['kind']}, {x['reason']}]: a fault is owed in call {n}, got (call, status, pictures) {fault[s]}")
        elif fault[s] is not None:
            wrong.append(f"{key} [{x['kind']}]: fault {fault[s]} on a stream the reference decodes")
    kinds = [x["kind"] for _, _, x, _ in cases]
    print(f"{W}x{H}: " + ", ".join(f"{kinds.count(k)} {k}" for k in ("complete", "fatal", "refused", "undefined")))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_decode_streams_batches_what_the_reference_decodes(pkg, fo, W, H):
    """ferhip_decode_streams: every stream of a size that the reference decodes and the device does not refuse, in one batch"""
    cases, (clean, clean_ref) = _cases(fo, W, H)
    batch = [(key, s, ref) for key, s, x, ref in cases if x["kind"] == "complete"] + [("clean", clean, clean_ref)]
    assert len(batch) >= 3
    T = max(len(ref) for _, _, ref in batch)
    out, pics, w, h = pkg.decode_streams([s for _, s, _ in batch], T)
    assert (w, h) == (W, H) and pics == [len(ref) for _, _, ref in batch]
    for k, (key, _, ref) in enumerate(batch):
        for t in range(len(ref)):
            assert np.array_equal(out[t, k], ref[t]), f"{key}: picture {t}"


def test_decode_streams_reports_what_the_reference_stops_at(pkg, fo):
    """three streams the reference stops at with a fatal error (in its first, a middle and its last picture), one per
    call: the call fails with the device or the unsupported code, and the library decodes a clean stream right after"""
    cases, (clean, clean_ref) = _cases(fo, dc.W, dc.H)
    fatal = [(key, s, x) for key, s, x, _ in cases if x["kind"] == "fatal"]
    picked = [next(c for c in fatal if c[2]["good"] == 0), next(c for c in fatal if c[2]["good"] in (1, 2)), next(c for c in fatal if c[2]["good"] >= 3)]
    for key, s, x in picked:
        with pytest.raises(pkg.FerHipError, match=f"code ({E_DEVICE}|{E_UNSUP})"):
            pkg.decode_streams([s], 5)
    for key, s, x, _ in [c for c in _cases(fo, 80, 64)[0] if c[2]["kind"] == "refused"]:  # vectors past 16 bits
        with pytest.raises(pkg.FerHipError, match=f"code {E_DEVICE}"):
            pkg.decode_streams([s], 5)
    out, pics, w, h = pkg.decode_streams([clean], len(clean_ref))
    assert pics == [len(clean_ref)] and all(np.array_equal(out[t, 0], clean_ref[t]) for t in range(len(clean_ref)))


@pytest.mark.parametrize("name", sorted(ss.ILLEGAL_PLANS))
def test_streaming_decoder_nal_by_nal(pkg, fo, name):
    """ferhip_dec_nal on the illegal plans: the oracle's pictures; vectors_past_int16: a device fault at the picture whose
    vectors leave 16 bits, the pictures in front of it intact"""
    for key, n, W, H, stream, e in ic.tier1():
        if n != name:
            continue
        v = ic.verdict(fo, key, stream)
        x = ic.expectation(e, v)
        assert x["kind"] == ("refused" if name in ss.VECTORS_PAST_INT16 else "complete"), key
        d = pkg.Decoder()
        got, failed = [], None
        for nal in pkg.split_nals(stream):
            try:
                p = d.nal(*pkg.unescape_nal(nal))
            except pkg.FerHipError as err:
                failed = str(err)
                break
            if p is not None:
                got.append(p)
        d.close()
        assert len(got) == x["good"], f"{key}: {len(got)} pictures, {x['good']} owed ({failed})"
        for t in range(x["good"]):
            assert np.array_equal(got[t], v["frames"][t]), f"{key}: picture {t}"
        if x["fault"]:
            assert failed is not None and f"code {E_DEVICE}" in failed, f"{key}: {failed}"
        else:
            assert failed is None, f"{key}: {failed}"
