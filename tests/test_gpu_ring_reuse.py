"""The pinned rings of an encoder context (slice headers + rate settings, presence masks, parameter sets: PinnedRing,
csrc/fer_ctx.h) under reuse.  A ring has 8 slots; a slot must not be rewritten before the copy that last read it has
run.  Context A is driven through 20 pictures -- more than two laps of every ring -- without any host synchronisation
between the calls, context B through the same calls with a sync() after each.  What A packed must be B's bytes, and B's
bytes must decode, with the oracle's decoder, to B's own reconstructions.

The picture types are requested (IDR / SLICE), never AUTO: the AUTO decision reads a SAD back and so waits for the stream,
which would drain the queue the rings are there for.  A stream's first picture is an IDR in any case (empty DPB)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = 5, 1, -1
W, H, S, T = 64, 48, 3, 20
FILL = 0xA5
REGION = S * 32768   # of the output buffer, per picture: 3 units of at most 5 + 64 + 1.5 * (12 * 1024 + 4096) bytes
# pictures x streams.  No two neighbouring rows are equal; stream 2 joins at picture 11, so that its PPS row is still
# being resent (set_rate below) when the parameter-set ring has gone round once; in the last lap streams 0 and 1 sit out
MASKS = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0],
                  [1, 1, 0], [1, 1, 1], [0, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1], [1, 1, 1], [0, 1, 1]],
                 np.uint8)


def _rate_call(t):
    """(stream, qp) of picture t's set_rate.  Until stream 2 has coded a picture r->qp is its base QP, so its PPS row
    changes with every call: 11 sends of the parameter-set ring before its first IDR needs the last one."""
    return (2, 20 + t) if t <= 10 else (t % S, 16 + t % 7)


def _drive(pkg, frames_dev, sync_each):
    g = pkg.FerHip(W, H, S, qp=24, window=16, maxdiff=3, intra_every=8)
    out = pkg.DeviceBuffer(T * REGION)
    index = pkg.DeviceBuffer(T * 16 * (S + 1))
    out.upload(np.full(T * REGION, FILL, np.uint8))  # the bytes between 16-byte aligned entries are not written
    index.upload(np.zeros(T * 16 * (S + 1), np.uint8))
    count = [0] * S
    types, recs = [], []
    step = g.sync if sync_each else (lambda: None)
    for t in range(T):
        g.set_frames_live(frames_dev.ptr + t * S * g.fsz, MASKS[t])
        step()
        s, qp = _rate_call(t)
        g.set_rate(s, pkg.RC_CQP, qp=qp)
        req = [NONE if not MASKS[t][s] else (IDR if count[s] % 4 == 0 else SLICE) for s in range(S)]
        _, _, _, nt = g.encode_picture_device(req)
        assert nt == req
        step()
        g.pack_nal_device(out.ptr + t * REGION, index.ptr + t * 16 * (S + 1), REGION, pkg.AU_PARAM_SETS)
        step()
        if sync_each:
            recs.append(g.get_recon())
        types.append(nt)
        for s in range(S):
            count[s] += int(MASKS[t][s])
    g.sync()
    assert g.status() == [0] * S
    res = (out.download().reshape(T, REGION), index.download(dtype=pkg.AU).reshape(T, S + 1), types, recs)
    out.free()
    index.free()
    g.close()
    return res


def test_rings_lapped_without_host_sync(pkg, fo):
    assert all((MASKS[t] != MASKS[t - 1]).any() for t in range(1, T))
    assert all((MASKS[lap:lap + 8] == 0).any() for lap in range(0, T, 8)), "a stream is absent somewhere in every lap"
    fsz = W * H * 3 // 2
    frames = np.full((T, S, fsz), FILL, np.uint8)  # the slots of absent streams carry noise that nothing may read
    for t in range(T):
        for s in range(S):
            if MASKS[t][s]:
                frames[t, s] = pkg.gen_frame(W, H, t, 4242 + s, 2)
    dev = pkg.DeviceBuffer(frames.size)
    dev.upload(frames)
    out_a, idx_a, types_a, _ = _drive(pkg, dev, sync_each=False)
    out_b, idx_b, types_b, recs = _drive(pkg, dev, sync_each=True)
    dev.free()
    assert types_a == types_b
    for t in range(T):
        assert idx_a[t].tobytes() == idx_b[t].tobytes(), f"picture {t}: the index differs without host synchronisation"
        assert np.array_equal(out_a[t], out_b[t]), f"picture {t}: the packed bytes differ without host synchronisation"
    # the reference: every stream's units, in order, through the oracle's decoder
    for s in range(S):
        stream, want, kinds = b"", [], []
        for t in range(T):
            e = idx_b[t][s]
            if not MASKS[t][s]:
                assert int(e["bytes"]) == 0 and int(e["nal_type"]) == 0
                continue
            assert int(e["nal_type"]) == types_b[t][s] and int(e["offset"]) + int(e["bytes"]) <= REGION
            stream += bytes(out_b[t][int(e["offset"]): int(e["offset"]) + int(e["bytes"])])
            want.append(recs[t][s])
            kinds.append(types_b[t][s])
        assert IDR in kinds and SLICE in kinds, f"stream {s}: needs an IDR and a P picture, has {kinds}"
        n, dec, _ = fo.decode_stream_md5(stream)
        assert n == len(want), f"stream {s}: the oracle decodes {n} of {len(want)} pictures"
        for k in range(n):
            assert np.array_equal(dec[k], want[k]), f"stream {s} picture {k}: the oracle's decode is not the reconstruction"
