"""RTP packets on the device (ferhip_pack_rtp, ferhip_fetch_rtp, ferhip_rtp_blocks, ferhip_write_sdp_fmtp,
csrc/fer_rtp.hip) against tests/rtp_model.py (pinned on the host by test_rtp_model_host.py) applied to the units that
tests/nal_model.py and ferhip_fetch_nal give; the device depacketiser (ferhip_unrtp_blocks) against the same
model followed by the unit rules of tests/avcc_model.py; and the live decoder on packets in host and in device memory
(ferhip_decs_decode_rtp) against ferhip_decs_decode on the Annex-B form of the same units."""
import ctypes as C

import numpy as np
import pytest

import nal_model
import rtp_model as rm

pytestmark = pytest.mark.gpu
IDR, SLICE, NONE = 5, 1, -1
E_ARG, E_STATE = -1, -3
FILL = 0xA5
PS = (80, 81, 95, 1400)

_cache = {}


def _unit(t, payload):
    """header byte + escaped payload"""
    return nal_model.frame_nal(t, payload)[4:]


def _zeros_reaching(N):
    """the shortest all-zero payload whose unit has at least N bytes"""
    L = 0
    while 1 + L + (max(L - 1, 0) // 2) < N:
        L += 1
    return np.zeros(L, np.uint8)


def _drawn_with(rng, N):
    """a payload over {0, 1, 2, 3, 255} whose unit has exactly N bytes"""
    alphabet = np.array([0, 0, 0, 1, 2, 3, 255], np.uint8)
    p = alphabet[rng.integers(0, alphabet.size, N)]
    L = 0
    while len(_unit(1, p[:L])) < N:
        L += 1
    p = p[:L].copy()
    if len(_unit(1, p)) > N:  # the last byte took an 03 with it: one that takes none
        p[-1] = 255
    assert len(_unit(1, p)) == N
    return p


def _kat_payloads(P):
    k = ("kat", P)
    if k in _cache:
        return _cache[k]
    rng = np.random.default_rng(1000 + P)
    B, F = P - 12, P - 14
    out = [np.zeros(0, np.uint8)]
    for N in (1, 2, B - 1, B, B + 1, F + 1, F + 2, 2 * F + 1, 2 * F + 2):
        out.append(_zeros_reaching(N))
        if N >= 2:
            out.append(_drawn_with(rng, N))
    alphabet = np.array([0, 0, 0, 1, 2, 3, 255], np.uint8)
    for L in (4095, 4096, 4097, 2 * 4096 + 7):
        out.append(np.zeros(L, np.uint8))
        out.append(alphabet[rng.integers(0, alphabet.size, L)])
    # 00 00 0x with its 03 at every escaped position from three before to three behind a fragment seam -- the first and the
    # last of three -- and the pattern at every phase around the edge of a 4096-byte chunk of the payload
    for x in range(4):
        for seam in (F, 2 * F):
            for d in range(-3, 4):
                p = np.full(2 * F + 20, 0xAB, np.uint8)
                at = seam + d - 2
                p[at: at + 3] = (0, 0, x)
                out.append(p)
        for at in range(4096 - 4, 4096 + 2):
            p = np.full(4096 + 100, 0xAB, np.uint8)
            p[at: at + 3] = (0, 0, x)
            out.append(p)
    for p in out:
        p.setflags(write=False)
    _cache[k] = out
    return out


def _hdrs(pkg, n, seq0=65530):
    return pkg.rtp_hdr(n, ssrc=0x11223344 + np.arange(n), timestamp=0x55667788 + 90 * np.arange(n), seq=(seq0 + 7 * np.arange(n)) & 0xFFFF,
                       payload_type=96 + np.arange(n) % 32)


def _hdr_dict(h):
    return dict(ssrc=int(h["ssrc"]), timestamp=int(h["timestamp"]), seq=int(h["seq"]), payload_type=int(h["payload_type"]))


def _check(out, pkts, idx, per_stream, types, cap, pkts_cap, fill=FILL, what=""):
    """the whole buffer, table and index against the model's layout: a stream whose packets or rows do not end within the
    caps is absent, and every byte and row the model does not place holds the fill value"""
    placed, rows, index = rm.layout(per_stream, types)
    want = np.full(out.size, fill, np.uint8)
    want_rows = np.full(pkts.size * pkts.dtype.itemsize, fill, np.uint8).view(pkts.dtype)
    written = 0
    for s, pk in enumerate(per_stream):
        off, nbytes, _, first, npk = index[s]
        assert tuple(int(v) for v in idx[s]) == index[s], f"{what}: index[{s}] = {idx[s]}, expected {index[s]}"
        if not pk or off + nbytes > cap or first + npk > pkts_cap:
            continue
        written += 1
        for o, p in placed[first: first + npk]:
            want[o: o + len(p)] = np.frombuffer(p, np.uint8)
        for r in range(first, first + npk):
            want_rows[r] = rows[r]
    total = index[-1]
    assert tuple(int(v) for v in idx[len(per_stream)]) == (total[0], written, 0, total[3], 0), f"{what}: index[S]"
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])}"
    assert np.array_equal(pkts.view(np.uint8), want_rows.view(np.uint8)), f"{what}: the packet table differs"
    return index


@pytest.mark.parametrize("P", PS)
def test_kat_blocks_equal_the_model(pkg, P):
    payloads = _kat_payloads(P)
    n = len(payloads)
    types = [(1, 5)[k & 1] for k in range(n)]
    hdr = _hdrs(pkg, n)
    per_stream = [rm.packetise([_unit(types[k], payloads[k])], P, _hdr_dict(hdr[k])) for k in range(n)]
    assert len(per_stream[0]) == 1 and len(per_stream[0][0]) == 13, "a zero-length payload is one single-NAL packet of 13 bytes"
    kinds = {(len(pk) > 1) for pk in per_stream}
    assert kinds == {False, True}
    _, rows, index = rm.layout(per_stream, types)
    total, npk = index[-1][0], index[-1][3]
    rc, out, pkts, idx = pkg.rtp_blocks_raw(payloads, types, P, hdr, cap=total + 64, pkts_cap=npk + 3, fill=FILL)
    assert rc == 0
    _check(out, pkts, idx, per_stream, types, total + 64, npk + 3, what=f"P = {P}")
    # one byte, and one row, short: the last stream is absent, nothing beyond is touched, the index is still true
    for cap, pcap in ((total - 1, npk + 3), (total + 64, npk - 1)):
        rc, out, pkts, idx = pkg.rtp_blocks_raw(payloads, types, P, hdr, cap=cap, pkts_cap=pcap, fill=FILL)
        assert rc == 0
        _check(out, pkts, idx, per_stream, types, cap, pcap, what=f"P = {P}, cap {cap}, {pcap} rows")
        assert int(idx[n]["bytes"]) == n - 1


def test_kat_one_payload_per_call_and_refusals(pkg):
    P = 95
    payloads = _kat_payloads(P)
    for k in (0, 5, 9, len(payloads) - 1):
        hdr = _hdrs(pkg, 1, seq0=65535)
        pk = rm.packetise([_unit(5, payloads[k])], P, _hdr_dict(hdr[0]))
        _, _, index = rm.layout([pk], [5])
        rc, out, pkts, idx = pkg.rtp_blocks_raw([payloads[k]], [5], P, hdr, cap=index[-1][0], pkts_cap=len(pk), fill=FILL)
        assert rc == 0
        _check(out, pkts, idx, [pk], [5], index[-1][0], len(pk), what=f"payload {k}")
    hdr = _hdrs(pkg, 1)
    for bad_p in (79, 65536, 0, -5):
        assert pkg.rtp_blocks_raw([payloads[3]], [1], bad_p, hdr, cap=4096, pkts_cap=64)[0] == E_ARG
    h = hdr.copy()
    h["payload_type"] = 128
    assert pkg.rtp_blocks_raw([payloads[3]], [1], P, h)[0] == E_ARG
    h = hdr.copy()
    h["reserved"] = 1
    assert pkg.rtp_blocks_raw([payloads[3]], [1], P, h)[0] == E_ARG
    assert pkg.rtp_blocks_raw([payloads[3]], [1], 65535, hdr)[0] == 0


# ---- pictures

W, H, S, T = 176, 144, 3, 4
QP = 12


def _frames(pkg):
    if "frames" not in _cache:
        # stream 0 stands still: its P slices are a few bytes, single-NAL packets at every P
        a = np.stack([np.stack([pkg.gen_frame(W, H, t if s else 0, 900 + 11 * s, 2) for t in range(T)]) for s in range(S)])
        a.setflags(write=False)
        _cache["frames"] = a
    return _cache["frames"]


def _pictures(t):
    """stream 1 sits out picture 2"""
    return [not (t == 2 and s == 1) for s in range(S)]


def _units_of(entry):
    """an entry of fetch_nal -> its NAL units without their start codes"""
    return rm.access_units_of(entry)[0] if entry else []


def _run(pkg):
    """four pictures of three streams, IPPP; stream 1 sits out picture 2 and slot 2 is reset before picture 3.  Per picture
    and (flags, P): fetch_rtp's and pack_rtp's output against the model on fetch_nal's units; the headers' seq runs on"""
    if "run" in _cache:
        return _cache["run"]
    feeds = _frames(pkg)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    plain = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)  # the same pictures, never packed
    cap, pcap = 1 << 20, 1 << 13
    dst, dpk, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
    seq = {(f, P): np.full(S, 65530, np.int64) for f in (0, pkg.AU_PARAM_SETS) for P in (128, 1400)}
    log = []
    for t in range(T):
        if t == 3:
            g.reset_stream(2)
            plain.reset_stream(2)
        present = _pictures(t)
        pics = [feeds[s][t] if present[s] else None for s in range(S)]
        rbsp, nt = g.encode_live(pics)
        rbsp_plain, nt_plain = plain.encode_live(pics)
        assert rbsp == rbsp_plain and nt == nt_plain, f"picture {t}: packing changed what the encoder reads"
        for (flags, P), sq in seq.items():
            entries, types = g.fetch_nal(flags)
            hdr = pkg.rtp_hdr(S, ssrc=0xCAFE0000 + np.arange(S), timestamp=90000 + 3000 * t, seq=sq & 0xFFFF, payload_type=96)
            per_stream = [rm.packetise(_units_of(entries[s]), P, _hdr_dict(hdr[s])) if entries[s] else [] for s in range(S)]
            what = f"picture {t} flags {flags} P {P}"
            rc, buf, pkts, idx = g.fetch_rtp_raw(hdr, P, cap, pcap, flags, fill=FILL)
            assert rc == 0, what
            _, rows, index = rm.layout(per_stream, types)
            total, npk = index[-1][0], index[-1][3]
            # the host copy takes the bytes between the packets with it: compare what the model places, and the tail
            for s in range(S + 1):
                want = index[s] if s < S else (total, sum(present), 0, npk, 0)
                assert tuple(int(v) for v in idx[s]) == want, f"{what}: index[{s}]"
            assert [tuple(int(v) for v in r) for r in pkts[:npk]] == rows, what
            got = [[bytes(buf[o: o + n]) for o, n, _ in rows[index[s][3]: index[s][3] + index[s][4]]] for s in range(S)]
            assert got == per_stream, f"{what}: ferhip_fetch_rtp"
            assert np.all(buf[total:] == FILL)
            again = g.fetch_rtp_raw(hdr, P, cap, pcap, flags, fill=FILL)
            assert again[0] == 0 and np.array_equal(again[1], buf) and np.array_equal(again[2], pkts), f"{what}: a repeated call"
            # device to device, then copied: the whole buffer and table
            dst.upload(np.full(cap, FILL, np.uint8))
            dpk.upload(np.full(16 * pcap, FILL, np.uint8))
            g.pack_rtp_device(hdr, P, dst.ptr, cap, dpk.ptr, pcap, dix.ptr, flags)
            g.sync()
            _check(dst.download(), dpk.download(dtype=pkg.RTP_PKT), dix.download(dtype=pkg.RTP_AU), per_stream, types, cap, pcap, what=what)
            log.append(dict(t=t, flags=flags, P=P, packets=per_stream, types=types, seq=(sq & 0xFFFF).copy(), nt=nt))
            sq += np.array([len(pk) for pk in per_stream])
    assert g.status() == [0] * S
    _cache["run"] = (g, log)
    return _cache["run"]


def test_pictures_equal_the_model_on_fetch_nal_units(pkg):
    g, log = _run(pkg)
    assert ["".join({5: "I", 1: "P", -1: "."}[r["nt"][s]] for r in log if (r["flags"], r["P"]) == (0, 128)) for s in range(S)] == \
        ["IPPP", "IP.P", "IPPI"]
    kinds = set()
    for r in log:
        for s in range(S):
            pk = r["packets"][s]
            if not pk:
                continue
            # M exactly once per access unit, on its last packet; seq runs on from the header's
            assert [p[1] >> 7 for p in pk] == [0] * (len(pk) - 1) + [1], f"picture {r['t']} stream {s}"
            assert [int.from_bytes(p[2:4], "big") for p in pk] == [(int(r["seq"][s]) + k) & 0xFFFF for k in range(len(pk))]
            kinds |= {p[12] & 31 for p in pk}
            stap = pk[0][12] & 31 == 24
            assert stap == (r["flags"] != 0 and r["types"][s] == IDR)
            units, fault, _ = rm.depacketise(pk, int(r["seq"][s]))
            assert fault == 0 and units[-1][0] & 31 == r["types"][s] and len(units) == (3 if stap else 1)
    assert kinds == {1, 24, 28}, "all three packet kinds (an I picture never fits one packet here)"
    # seq wraps through 65535 in every run
    for key in {(r["flags"], r["P"]) for r in log}:
        for s in range(S):
            seqs = [int.from_bytes(p[2:4], "big") for r in log if (r["flags"], r["P"]) == key for p in r["packets"][s]]
            at = seqs.index(65535)
            assert seqs[0] == 65530 and seqs[at + 1] == 0 and seqs[-1] == (65530 + len(seqs) - 1) & 0xFFFF, key


def test_context_refusals_and_caps(pkg):
    feeds = _frames(pkg)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    lib = g.lib
    cap, pcap = 1 << 19, 1 << 12
    dst, dpk, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
    hdr = pkg.rtp_hdr(S, ssrc=7, timestamp=9, seq=65000, payload_type=127)

    def pack(flags=0, P=1400, h=hdr, d=dst.ptr, c=cap, p=dpk.ptr, pc=pcap, i=dix.ptr):
        return lib.ferhip_pack_rtp(g.ctx, flags, P, h.ctypes.data if h is not None else None, d, c, p, pc, i)

    assert pack() == E_STATE and g.fetch_rtp_raw(hdr, 1400, cap, pcap)[0] == E_STATE
    rbsp, nt = g.encode_live([feeds[s][0] for s in range(S)])
    assert pack() == 0
    for kw in (dict(flags=2), dict(flags=pkg.AU_AVCC), dict(flags=pkg.AU_PARAM_SETS | 8), dict(P=79), dict(P=65536), dict(h=None),
               dict(d=dst.ptr + 8), dict(p=dpk.ptr + 4), dict(i=dix.ptr + 4), dict(i=None), dict(d=None), dict(p=None)):
        assert pack(**kw) == E_ARG, kw
    for field, v in (("payload_type", 128), ("reserved", 1)):
        h = hdr.copy()
        h[field][S - 1] = v
        assert pack(h=h) == E_ARG and g.fetch_rtp_raw(h, 1400, cap, pcap)[0] == E_ARG, field
    assert pack(P=80) == 0 and pack(P=65535) == 0 and pack(d=None, c=0, p=None, pc=0) == 0
    # caps: one byte short and one row short leave the last stream out; fetch fills the index and refuses
    units = [e[4:] for e in g.fetch_nal()[0]]
    P = 128
    per_stream = [rm.packetise([units[s]], P, _hdr_dict(hdr[s])) for s in range(S)]
    _, rows, index = rm.layout(per_stream, nt)
    total, npk = index[-1][0], index[-1][3]
    for c, pc in ((total - 1, npk), (total, npk - 1), (total, npk), (index[1][0] + 5, npk), (0, 0)):
        dst.upload(np.full(cap, FILL, np.uint8))
        dpk.upload(np.full(16 * pcap, FILL, np.uint8))
        assert pack(P=P, c=c, pc=pc) == 0
        g.sync()
        _check(dst.download(), dpk.download(dtype=pkg.RTP_PKT), dix.download(dtype=pkg.RTP_AU), per_stream, nt, c, pc, what=f"caps {c}, {pc}")
    for c, pc in ((total - 1, npk), (total, npk - 1)):
        rc, _, _, idx = g.fetch_rtp_raw(hdr, P, c, pc)
        assert rc == E_ARG and [tuple(int(v) for v in r) for r in idx[:S]] == index[:S] and int(idx[S]["offset"]) == total
    assert g.fetch_rtp_raw(hdr, P, total, npk)[0] == 0
    got, idx = g.fetch_rtp(hdr, P)
    assert got == per_stream
    # a call in which every stream is absent: nothing at all
    g.encode_live([None] * S)
    rc, _, _, idx = g.fetch_rtp_raw(hdr, P, 0, 0, pkg.AU_PARAM_SETS)
    assert rc == 0 and [tuple(int(v) for v in r) for r in idx] == [(0, 0, 0, 0, 0)] * (S + 1)
    assert g.status() == [0] * S
    g.close()


def test_sdp_fmtp(pkg):
    import avcc_model as am
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    g.set_rate(1, qp=20)
    g.set_display_size(170, 140)
    for s in range(S):
        sps, pps = (u[4:] for u in g.sps_pps(s))
        text = g.sdp_fmtp(s)
        assert text == rm.sdp_fmtp(sps, pps)
        assert am.config_record(sps, pps) == g.avcc_config(s), "the units of the configuration record"
        assert text.startswith("profile-level-id=" + g.avcc_config(s)[1:4].hex() + ";packetization-mode=1;sprop-parameter-sets=")
    assert g.sdp_fmtp(1) != g.sdp_fmtp(0)
    n = len(g.sdp_fmtp(0))
    o = C.create_string_buffer(n + 1)
    assert g.lib.ferhip_write_sdp_fmtp(g.ctx, 0, o, n) == 0 and g.lib.ferhip_write_sdp_fmtp(g.ctx, 0, o, n + 1) == n
    assert g.lib.ferhip_write_sdp_fmtp(g.ctx, S, o, n + 1) == 0 and g.lib.ferhip_write_sdp_fmtp(g.ctx, -1, o, n + 1) == 0
    g.close()


# ---- the live decoder, packets in host memory

GOLD_A, GOLD_B = "qcif_ippp_4f_qp12_w16.264", "qcif_skip_5f_qp12.264"


def _gold_aus():
    """three streams (a, b, a) as access units of NAL units without start codes"""
    if "aus" not in _cache:
        from conftest import golden_bytes
        a, b = rm.access_units_of(golden_bytes(GOLD_A)), rm.access_units_of(golden_bytes(GOLD_B))
        _cache["aus"] = [a, b, a]
    return _cache["aus"]


def _annexb(units):
    return b"".join(b"\x00\x00\x00\x01" + u for u in units) if units else None


class _Sender:
    """packetises access units per stream with a running seq, and lays the packets of a call out interleaved, at odd
    offsets, with the table ferhip_decs_decode_rtp takes"""

    def __init__(self, S, P, seq0=65500):
        self.P, self.seq = P, [(seq0 + 1000 * s) & 0xFFFF for s in range(S)]

    def packets(self, s, aus):
        out = []
        for au in aus:
            pk = rm.packetise(au, self.P, dict(ssrc=s, timestamp=0, seq=self.seq[s], payload_type=96))
            self.seq[s] = (self.seq[s] + len(pk)) & 0xFFFF
            out += pk
        return out

    @staticmethod
    def lay(pkg, per_stream):
        buf, rows = bytearray(b"\xEE" * 3), []
        queues = [list(p) for p in per_stream]
        while any(queues):
            for s, q in enumerate(queues):
                for _ in range(2):  # two packets of a stream, then the next stream's
                    if q:
                        p = q.pop(0)
                        rows.append((len(buf), len(p), s))
                        buf += p + b"\xEE" * (1 + len(rows) % 3)
        return bytes(buf), np.array(rows, pkg.RTP_PKT) if rows else np.zeros(0, pkg.RTP_PKT)


def _rtp_call(pkg, dec, base, rows, target, device):
    """decode_rtp with the packets in host memory, or (device) in device memory at an odd address"""
    if not device:
        return dec.decode_rtp(base, rows, target)
    buf = pkg.DeviceBuffer(len(base) + 16)
    buf.upload(np.frombuffer(base, np.uint8), offset=5)
    try:
        return dec.decode_rtp(buf.ptr + 5, rows, target, base_on_device=True)
    finally:
        buf.free()


def _decode_calls(pkg, dec, calls, rtp=None, device=False):
    """calls: per call a list per stream of access units; rtp = a _Sender: through decode_rtp, else Annex-B through decode"""
    out = []
    for call in calls:
        target = np.full((dec.P, dec.S, dec.fsz), FILL, np.uint8)
        if rtp:
            base, rows = rtp.lay(pkg, [rtp.packets(s, aus) for s, aus in enumerate(call)])
            _, pics, st = _rtp_call(pkg, dec, base, rows, target, device)
        else:
            _, pics, st = dec.decode([_annexb([u for au in aus for u in au]) for aus in call], target)
        for s in range(dec.S):
            assert (target[pics[s]:, s] == FILL).all()
        out.append(([target[: pics[s], s].copy() for s in range(dec.S)], pics, st))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for c, ((pa, na, sa), (pb, nb, sb)) in enumerate(zip(a, b)):
        assert na == nb and sa == sb, f"{what} call {c}: pictures {na} / {nb}, status {sa} / {sb}"
        for s in range(len(pa)):
            assert np.array_equal(pa[s], pb[s]), f"{what} call {c} stream {s}"


@pytest.mark.parametrize("P", (95, 1400))
def test_live_decode_rtp_equals_annexb(pkg, P):
    aus = _gold_aus()
    S, n = len(aus), max(len(a) for a in aus)
    schedules = {"one_picture_per_call": ([[a[k: k + 1] for a in aus] for k in range(n)], 1),
                 "everything_in_one_call": ([list(aus)], n),
                 "two_then_the_rest": ([[a[:2] for a in aus], [a[2:] for a in aus]], n)}
    for name, (calls, maxpic) in schedules.items():
        dec = pkg.LiveDecoder(S, W, H, maxpic)
        ref = _decode_calls(pkg, dec, calls)
        dec.close()
        assert sum(sum(npic) for _, npic, _ in ref) == sum(len(a) for a in aus) and all(st == [0] * S for _, _, st in ref)
        for device in (False, True):
            dec = pkg.LiveDecoder(S, W, H, maxpic)
            _same(ref, _decode_calls(pkg, dec, calls, _Sender(S, P), device), f"{name} P={P} device={device}")
            dec.close()
    # mixed with the other decode calls on one decoder: Annex-B, RTP, Annex-B, RTP
    calls = schedules["one_picture_per_call"][0]
    dec = pkg.LiveDecoder(S, W, H, 1)
    ref = _decode_calls(pkg, dec, calls)
    dec.close()
    for device in (False, True):
        dec = pkg.LiveDecoder(S, W, H, 1)
        snd = _Sender(S, P)
        got = []
        for k, call in enumerate(calls):
            got += _decode_calls(pkg, dec, [call], snd if k & 1 else None, device)
        dec.close()
        _same(ref, got, f"alternating device={device}")


@pytest.mark.parametrize("device", (False, True))
def test_live_decode_rtp_faults_are_isolated(pkg, device):
    aus = _gold_aus()
    S, P = len(aus), 95
    v = aus[0]  # I P P P, every slice in many fragments
    # clean: call 0 = the first picture, call 1 = two pictures of streams 0 and 2 and one of stream 1, call 2 = one more
    clean_calls = [[a[:1] for a in aus], [v[1:3], aus[1][1:2], v[1:3]], [v[3:4], aus[1][2:3], v[3:4]]]
    dec = pkg.LiveDecoder(S, W, H, 2)
    clean = _decode_calls(pkg, dec, clean_calls, _Sender(S, P), device)
    dec.close()
    assert [npic for _, npic, _ in clean] == [[1, 1, 1], [2, 1, 2], [1, 1, 1]] and all(st == [0] * S for _, _, st in clean)

    def damage(kind, pk):
        """in the second access unit of call 1 (stream 0): a lost packet, a lost last packet, a packet of version 1"""
        first = len(rm.packetise(v[1], P, rm.HDR))
        assert len(pk) > first + 4 and pk[first + 2][12] & 31 == 28
        if kind == "gap":
            return pk[: first + 2] + pk[first + 3:]
        if kind == "truncated":
            return pk[:-1]
        return pk[: first + 2] + [bytes([0x40 | (pk[first + 2][0] & 0x3F)]) + pk[first + 2][1:]] + pk[first + 3:]

    for kind in ("gap", "truncated", "malformed"):
        dec = pkg.LiveDecoder(S, W, H, 2)
        snd = _Sender(S, P)
        _decode_calls(pkg, dec, clean_calls[:1], snd, device)
        per = [snd.packets(s, aus_s) for s, aus_s in enumerate(clean_calls[1])]
        per[0] = damage(kind, per[0])
        target = np.full((2, S, dec.fsz), FILL, np.uint8)
        _, pics, st = _rtp_call(pkg, dec, *snd.lay(pkg, per), target, device)
        assert (pics, st) == ([1, 1, 2], [E_ARG, 0, 0]), kind
        assert np.array_equal(target[0, 0], clean[1][0][0][0]), f"{kind}: the picture in front of the fault is delivered"
        for s in (1, 2):
            assert np.array_equal(target[: pics[s], s], clean[1][0][s]), f"{kind}: stream {s} is untouched"
        # a P slice behind the fault is refused until the next IDR slice; any seq is taken (the expectation was cleared)
        snd.seq[0] = 77
        nxt = _decode_calls(pkg, dec, [[v[3:4], aus[1][2:3], v[3:4]]], snd, device)[0]
        assert nxt[1] == [0, 1, 1] and nxt[2] == [E_STATE, 0, 0], kind
        assert np.array_equal(nxt[0][1], clean[2][0][1]) and np.array_equal(nxt[0][2], clean[2][0][2])
        # the stream is back at its next IDR slice (seq runs on: the refused slice's packets were walked)
        back = _decode_calls(pkg, dec, [[v[:1], [], []]], snd, device)[0]
        assert back[1] == [1, 0, 0] and back[2] == [0, 0, 0] and np.array_equal(back[0][0], clean[0][0][0]), kind
        dec.close()


def test_live_decode_rtp_arguments_and_the_expectation(pkg):
    aus = _gold_aus()
    S, P = len(aus), 1400
    dec = pkg.LiveDecoder(S, W, H, 1)
    snd = _Sender(S, P)
    first = [a[:1] for a in aus]
    base, rows = snd.lay(pkg, [snd.packets(s, a) for s, a in enumerate(first)])
    bad = rows.copy()
    bad["stream"][3] = S
    with pytest.raises(pkg.FerHipError, match="code -1"):
        dec.decode_rtp(base, bad)
    pics, st = (C.c_int * S)(), (C.c_int * S)()
    assert dec.lib.ferhip_decs_decode_rtp(dec.h, None, 0, rows.ctypes.data, rows.size, None, 0, pics, st) == E_ARG
    assert dec.lib.ferhip_decs_decode_rtp(dec.h, base, 0, rows.ctypes.data, rows.size, None, 0, None, st) == E_ARG
    # more slices than max_pictures: refused as a whole, nothing taken, the expectation stays
    two = _Sender(S, P)
    b2, r2 = two.lay(pkg, [two.packets(s, a[:2]) for s, a in enumerate(aus)])
    with pytest.raises(pkg.FerHipError, match="code -1"):
        dec.decode_rtp(b2, r2)
    _, pics, st = dec.decode_rtp(base, rows)
    assert (pics, st) == ([1] * S, [0] * S)
    # the expectation: the same packets again are a gap for every stream, from device memory too (one expectation for both
    # paths); behind reset_stream any seq is taken
    _, pics, st = _rtp_call(pkg, dec, base, rows, None, True)
    assert (pics, st) == ([0] * S, [E_ARG] * S)
    with pytest.raises(pkg.FerHipError, match="code -1"):
        _rtp_call(pkg, dec, b2, r2, None, True)
    for s in range(S):
        dec.reset_stream(s)
    _, pics, st = dec.decode_rtp(base, rows)
    assert (pics, st) == ([1] * S, [0] * S)
    _, pics, st = dec.decode_rtp(b"", np.zeros(0, pkg.RTP_PKT))
    assert (pics, st) == ([0] * S, [0] * S)
    dec.close()


# ---- the way in, known answers: ferhip_unrtp_blocks against the model

def _check_unrtp(pkg, per_stream, expect, misalign, what, interleave=True):
    """per_stream[s] = the packets of stream s; the whole store, the table, fault[] and seq_next[] against
    rtp_model.depacketise followed by the unit rules and layout of avcc_model"""
    import avcc_model as am
    S = len(per_stream)
    if interleave:
        base, rows = _Sender.lay(pkg, per_stream)
    else:
        base, rows = b"".join(p for pk in per_stream for p in pk), []
        off = 0
        for s, pk in enumerate(per_stream):
            for p in pk:
                rows.append((off, len(p), s))
                off += len(p)
        rows = np.array(rows, pkg.RTP_PKT) if rows else np.zeros(0, pkg.RTP_PKT)
    model = [rm.depacketise(pk, e) for pk, e in zip(per_stream, expect)]
    ranges = [rm.to_avcc(units) for units, _, _ in model]
    want_units, total, overran = am.layout(ranges, 4)
    assert overran == [0] * S
    cap = total + 48
    rc, out, units, count, fault, nxt = pkg.unrtp_blocks_raw(base, rows, S, expect, misalign, cap=cap, units_cap=len(want_units) + 2, fill=FILL)
    assert rc == 0, what
    assert [int(f) for f in fault] == [f for _, f, _ in model], f"{what}: fault[]"
    assert [int(n) for n in nxt] == [n for _, _, n in model], f"{what}: seq_next[]"
    assert count == len(want_units), f"{what}: {count} units, expected {len(want_units)}"
    got = [(int(u["range"]), int(u["nal_type"]), int(u["ref_idc"]), int(u["bytes"]), int(u["offset"])) for u in units[:count]]
    assert got == want_units, what
    want = np.full(out.size, FILL, np.uint8)
    k = 0
    for data in ranges:
        for _, _, _, _, p in am.avcc_split(data, 4)[0]:
            want[want_units[k][4]: want_units[k][4] + len(p)] = np.frombuffer(p, np.uint8)
            k += 1
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])} of {total}"
    return model


def _golden_packets(P):
    from conftest import golden_bytes
    k = ("gold_pk", P)
    if k not in _cache:
        _cache[k] = [rm.packetise_stream(golden_bytes(n), P)[0] for n in
                     ("qcif_ippp_4f_qp12_w16.264", "qcif_ippp_4f_qp28_w32.264", "qcif_i_2f_qp12.264", "qcif_skip_5f_qp12.264")]
    return _cache[k]


@pytest.mark.parametrize("P", (95, 1400))
def test_unrtp_kat_golden_streams(pkg, P):
    per_stream = _golden_packets(P)
    for misalign in (0, 1, 7, 15):
        model = _check_unrtp(pkg, per_stream, [65530, -1, 65530, -1], misalign, f"P = {P}, misalign {misalign}")
        assert all(f == 0 for _, f, _ in model) and sum(len(u) for u, _, _ in model) >= 16
    _check_unrtp(pkg, per_stream, [65530] * 4, 3, f"P = {P}, stream after stream", interleave=False)
    # one stream alone, and a stream without packets between two others
    _check_unrtp(pkg, per_stream[3:], [-1], 0, "one stream")
    _check_unrtp(pkg, [per_stream[0], [], per_stream[3]], [65530, 12, 65530], 9, "an empty stream")


def test_unrtp_kat_dressed_packets_and_fragment_seams(pkg):
    packets = _golden_packets(95)[3]
    dressed = []
    for k, p in enumerate(packets):
        cc, ext, pad = k % 4, (None, 0, 2)[k % 3], (0, 1, 4, 255)[k % 4]
        dressed.append(rm.raw_packet(p[12:], int.from_bytes(p[2:4], "big"), cc=cc, ext=ext, pad=pad, marker=p[1] >> 7))
    plain = _check_unrtp(pkg, [packets], [65530], 0, "plain")
    assert _check_unrtp(pkg, [dressed, packets], [65530, -1], 7, "CSRC, extension, padding")[0] == plain[0]
    # an emulation prevention byte at every place from three before to three behind the first and the second fragment seam
    P, F = 80, 66
    per_stream = []
    for seam in (F, 2 * F):
        for d in range(-3, 4):
            p = np.full(2 * F + 20, 0xAB, np.uint8)
            p[seam + d - 2: seam + d + 1] = (0, 0, 1)
            unit = _unit(5, p)
            assert unit[1 + seam + d] == 3 and unit.count(b"\x00\x00\x03") == 1
            per_stream.append(rm.packetise([unit], P, rm.HDR))
    for misalign in (0, 5):
        model = _check_unrtp(pkg, per_stream, [65530] * len(per_stream), misalign, f"seams, misalign {misalign}")
        assert all(f == 0 and len(u) == 1 for u, f, _ in model)


def test_unrtp_kat_fault_catalogue(pkg):
    cat = rm.catalogue()
    per_stream = [pk for _, pk, _, _, _ in cat]
    expect = [e for _, _, e, _, _ in cat]
    for misalign in (0, 15):
        model = _check_unrtp(pkg, per_stream, expect, misalign, f"catalogue, misalign {misalign}")
        for (name, _, _, fault, front), (units, f, nxt) in zip(cat, model):
            assert f == fault and units == front and (nxt == -1) == (fault != 0), name
    assert {f for _, _, _, f, _ in cat} == {0, 2, 3, 4}
    # every entry alone: a fault's place in the table does not matter
    for name, pk, e, fault, front in cat[::3]:
        _check_unrtp(pkg, [pk], [e], 1, name)


def test_unrtp_arguments_and_capacities(pkg):
    per_stream = _golden_packets(1400)[:2]
    base, rows = _Sender.lay(pkg, per_stream)
    rc, out, units, count, fault, nxt = pkg.unrtp_blocks_raw(base, rows, 2)
    assert rc == 0 and count > 8
    total = int(units[count - 1]["offset"]) + ((int(units[count - 1]["bytes"]) + 15) & ~15)
    # a store one byte short, a table one row short: FERHIP_E_ARG, the true count, nothing at or beyond cap touched
    rc, out2, _, count2, _, _ = pkg.unrtp_blocks_raw(base, rows, 2, cap=total - 1, fill=FILL)
    assert rc == E_ARG and count2 == count
    rc, _, _, count2, _, _ = pkg.unrtp_blocks_raw(base, rows, 2, units_cap=count - 1)
    assert rc == E_ARG and count2 == count
    bad = rows.copy()
    bad["stream"][0] = 2
    assert pkg.unrtp_blocks_raw(base, bad, 2)[0] == E_ARG
    bad = rows.copy()
    bad["offset"][1] = len(base) - 3
    assert pkg.unrtp_blocks_raw(base, bad, 2)[0] == E_ARG
    assert pkg.unrtp_blocks_raw(base, rows, 2, misalign=16)[0] == E_ARG and pkg.unrtp_blocks_raw(base, rows, 0)[0] == E_ARG
    rc, _, _, count, fault, nxt = pkg.unrtp_blocks_raw(b"", np.zeros(0, pkg.RTP_PKT), 3, [5, -1, 7])
    assert rc == 0 and count == 0 and list(fault) == [0, 0, 0] and list(nxt) == [5, -1, 7]


def test_loopback_without_the_bus(pkg):
    """an encoder's packets are decoded where ferhip_pack_rtp left them: only the table crosses the bus"""
    feeds = _frames(pkg)
    g = pkg.FerHip(W, H, S, qp=QP, window=16, maxdiff=3, intra_every=30)
    cap, pcap = 1 << 19, 1 << 11
    dst, dpk, dix = pkg.DeviceBuffer(cap), pkg.DeviceBuffer(16 * pcap), pkg.DeviceBuffer(24 * (S + 1))
    dec, ref = pkg.LiveDecoder(S, W, H, 1), pkg.LiveDecoder(S, W, H, 1)
    seq = np.full(S, 65520, np.int64)
    for t in range(3):
        g.encode_live([feeds[s][t] for s in range(S)])
        entries, _ = g.fetch_nal(pkg.AU_PARAM_SETS)
        hdr = pkg.rtp_hdr(S, ssrc=np.arange(S), timestamp=3000 * t, seq=seq & 0xFFFF)
        g.pack_rtp_device(hdr, 128, dst.ptr, cap, dpk.ptr, pcap, dix.ptr, pkg.AU_PARAM_SETS)
        g.sync()
        idx = dix.download(dtype=pkg.RTP_AU)
        npk = int(idx["first_pkt"][S])
        assert npk <= pcap and int(idx["offset"][S]) <= cap
        rows = dpk.download(16 * npk, dtype=pkg.RTP_PKT)
        got, pics, st = dec.decode_rtp(dst.ptr, rows, base_on_device=True)
        want, wpics, wst = ref.decode(entries)
        assert pics == wpics == [1] * S and st == wst == [0] * S, f"picture {t}"
        assert np.array_equal(got, want), f"picture {t}"
        seq += idx["npkts"][:S]
    assert int(seq[1]) > 65536, "seq wrapped on the way"
    for x in (dec, ref):
        x.close()
    g.close()
