"""SRTP as include/ferhip.h defines it (RFC 3711 with the default transforms: AES-128 counter mode, HMAC-SHA1 with an 80-bit
tag, no MKI, key derivation rate 0), restated for the tests: AES-128 in numpy over any number of blocks at once, the key
derivation, the header rule, the index estimate, and protect / unprotect over a packet list and a state.  HMAC comes from
hmac / hashlib.  test_srtp_model_host.py pins this file to the published vectors and to tests/golden/srtp_kat.json, which
the openssl command line wrote."""
import hashlib
import hmac

import numpy as np

TAG = 10
MAX_PAYLOAD = 1 << 20


def _make_sbox():
    sb = [0] * 256
    p = q = 1
    while True:
        p = (p ^ (p << 1) ^ (0x1B if p & 0x80 else 0)) & 0xFF
        q ^= (q << 1) & 0xFF
        q ^= (q << 2) & 0xFF
        q ^= (q << 4) & 0xFF
        if q & 0x80:
            q ^= 0x09
        r = q ^ ((q << 1 | q >> 7) & 0xFF) ^ ((q << 2 | q >> 6) & 0xFF) ^ ((q << 3 | q >> 5) & 0xFF) ^ ((q << 4 | q >> 4) & 0xFF)
        sb[p] = r ^ 0x63
        if p == 1:
            break
    sb[0] = 0x63
    return np.array(sb, np.uint8)


SBOX = _make_sbox()
# byte i of the state is row i % 4 of column i // 4; ShiftRows takes row r of column c from column c + r
_SHIFT = np.array([(4 * ((i // 4 + i % 4) % 4) + i % 4) for i in range(16)])


def _xtime(a):
    return ((a.astype(np.uint16) << 1) ^ np.where(a & 0x80, 0x1B, 0)).astype(np.uint8)


def expand_key(key):
    """the 11 round keys of a 16-byte key -> uint8 [11][16]"""
    assert len(key) == 16
    w = [list(key[4 * i: 4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [int(SBOX[b]) for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = (rcon << 1) ^ (0x11B if rcon & 0x80 else 0)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return np.array(w, np.uint8).reshape(11, 16)


def aes_ecb(key, data):
    """AES-128 of every 16-byte block of data"""
    rk = expand_key(key)
    s = np.frombuffer(bytes(data), np.uint8).reshape(-1, 16) ^ rk[0]
    for r in range(1, 11):
        s = SBOX[s][:, _SHIFT]
        if r < 10:
            c = s.reshape(-1, 4, 4)
            x = _xtime(c)
            rot = lambda a, n: np.roll(a, -n, axis=2)  # noqa: E731
            # 2 a0 + 3 a1 + a2 + a3 for every row of every column
            c = x ^ rot(x, 1) ^ rot(c, 1) ^ rot(c, 2) ^ rot(c, 3)
            s = c.reshape(-1, 16)
        s = s ^ rk[r]
    return s.tobytes()


def aes_cm(key, iv, n):
    """n bytes of the keystream of RFC 3711 section 4.1.1: block b = AES(key, iv + b), the sum in the last two bytes"""
    assert len(iv) == 16
    nb = (n + 15) // 16
    assert nb <= 65536
    blocks = np.tile(np.frombuffer(bytes(iv), np.uint8), (nb, 1))
    c = (int.from_bytes(iv[14:], "big") + np.arange(nb)) & 0xFFFF
    blocks[:, 14] = c >> 8
    blocks[:, 15] = c & 255
    return aes_ecb(key, blocks.tobytes())[:n]


def derive(master_key, master_salt):
    """the session keys at key derivation rate 0 -> (k_e [16], k_a [20], k_s [14])"""
    assert len(master_key) == 16 and len(master_salt) == 14
    out = []
    for label, n in ((0, 16), (1, 20), (2, 14)):
        x = bytearray(master_salt)
        x[7] ^= label
        out.append(aes_cm(master_key, bytes(x) + b"\0\0", n))
    return tuple(out)


def header_len(p):
    """the header rule: the bytes in front of the payload, 0 = malformed"""
    L = len(p)
    if L < 12 or p[0] >> 6 != 2:
        return 0
    hl = 12 + 4 * (p[0] & 15)
    if p[0] & 0x10:
        if hl + 4 > L:
            return 0
        hl += 4 + 4 * int.from_bytes(p[hl + 2: hl + 4], "big")
    if hl > L or L - hl > MAX_PAYLOAD:
        return 0
    return hl


def estimate(roc, s_l, seq):
    """v of RFC 3711 section 3.3.1, modulo 2^32"""
    if s_l < 32768:
        v = roc - 1 if seq - s_l > 32768 else roc
    else:
        v = roc + 1 if s_l - 32768 > seq else roc
    return v & 0xFFFFFFFF


def keystream(k_e, k_s, ssrc, i, n):
    iv = int.from_bytes(k_s + b"\0\0", "big") ^ (ssrc << 64) ^ (i << 16)
    return aes_cm(k_e, iv.to_bytes(16, "big"), n)


def tag(k_a, packet, v):
    return hmac.new(k_a, bytes(packet) + v.to_bytes(4, "big"), hashlib.sha1).digest()[:TAG]


def sha1_compress(h, block):
    """one SHA-1 compression (FIPS 180): the state h (5 words) over a 64-byte block -> the new state"""
    rotl = lambda x, n: ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF  # noqa: E731
    w = [int.from_bytes(block[4 * t: 4 * t + 4], "big") for t in range(16)]
    for t in range(16, 80):
        w.append(rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = h
    for t in range(80):
        if t < 20:
            f, k = (b & c) | (~b & d), 0x5A827999
        elif t < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif t < 60:
            f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (rotl(a, 5) + f + e + k + w[t]) & 0xFFFFFFFF, a, rotl(b, 30), c, d
    return tuple((x + y) & 0xFFFFFFFF for x, y in zip(h, (a, b, c, d, e)))


SHA1_INIT = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)


def hmac_midstates(k_a):
    """the SHA-1 state after the block k_a ^ 36.. and after the block k_a ^ 5c..: what a session keeps of k_a"""
    pad = lambda x: bytes(b ^ x for b in k_a.ljust(64, b"\0"))  # noqa: E731
    return sha1_compress(SHA1_INIT, pad(0x36)), sha1_compress(SHA1_INIT, pad(0x5C))


def hmac_from_midstates(mid_i, mid_o, msg):
    """HMAC-SHA1 continued from the two midstates (20 bytes)"""
    def finish(h, data, total):
        data += b"\x80" + bytes((55 - len(data)) % 64) + (8 * total).to_bytes(8, "big")
        for at in range(0, len(data), 64):
            h = sha1_compress(h, data[at: at + 64])
        return b"".join(x.to_bytes(4, "big") for x in h)
    return finish(mid_o, finish(mid_i, bytes(msg), 64 + len(msg)), 84)


def _xor(a, b):
    return (np.frombuffer(bytes(a), np.uint8) ^ np.frombuffer(bytes(b), np.uint8)).tobytes()


def _start(rows, states, cut):
    """s_l of every stream for this call: the state's, or with set == 0 the seq of the stream's first well-formed row
    (cut = the tag bytes a row carries)"""
    s_l = {}
    for s, p in rows:
        if s in s_l:
            continue
        roc, sl, st = states[s]
        if st:
            s_l[s] = sl
        elif len(p) >= cut and header_len(p[: len(p) - cut]):
            s_l[s] = int.from_bytes(p[2:4], "big")
    return s_l


def _finish(states, best):
    out = list(states)
    for s, i in best.items():
        roc, sl, st = states[s]
        if not st or i > (roc << 16 | sl):
            out[s] = (i >> 16, i & 0xFFFF, 1)
    return out


def protect(rows, keys, states):
    """rows: [(stream, RTP packet)], keys[s] = (k_e, k_a, k_s), states[s] = (roc, s_l, set) -> ([SRTP packet or None for a
    malformed row], the states afterwards)"""
    s_l = _start(rows, states, 0)
    out, best = [], {}
    for s, p in rows:
        p = bytes(p)
        hl = header_len(p)
        if not hl:
            out.append(None)
            continue
        k_e, k_a, k_s = keys[s]
        seq, ssrc = int.from_bytes(p[2:4], "big"), int.from_bytes(p[8:12], "big")
        v = estimate(states[s][0], s_l[s], seq)
        i = v << 16 | seq
        c = p[:hl] + _xor(p[hl:], keystream(k_e, k_s, ssrc, i, len(p) - hl))
        out.append(c + tag(k_a, c, v))
        best[s] = max(best.get(s, -1), i)
    return out, _finish(states, best)


def unprotect(rows, keys, states):
    """rows: [(stream, SRTP packet)] -> ([RTP packet or None], [status 0 authentic / 1 the tag differs / 2 malformed], the
    states afterwards)"""
    s_l = _start(rows, states, TAG)
    out, status, best = [], [], {}
    for s, p in rows:
        p = bytes(p)
        hl = header_len(p[: len(p) - TAG]) if len(p) >= TAG else 0
        if not hl:
            out.append(None)
            status.append(2)
            continue
        k_e, k_a, k_s = keys[s]
        L = len(p) - TAG
        seq, ssrc = int.from_bytes(p[2:4], "big"), int.from_bytes(p[8:12], "big")
        v = estimate(states[s][0], s_l[s], seq)
        i = v << 16 | seq
        if tag(k_a, p[:L], v) != p[L:]:
            out.append(None)
            status.append(1)
            continue
        out.append(p[:hl] + _xor(p[hl:L], keystream(k_e, k_s, ssrc, i, L - hl)))
        status.append(0)
        best[s] = max(best.get(s, -1), i)
    return out, status, _finish(states, best)


def layout(rows, outs, cap=None):
    """the output table: [(offset, bytes, stream)] + [(total, packets written, 0)], and [(offset, packet)] of the packets
    that end within cap (all of them for cap = None)"""
    table, placed, off, written = [], [], 0, 0
    for (s, _), o in zip(rows, outs):
        n = len(o) if o is not None else 0
        table.append((off, n, s))
        if n and (cap is None or off + n <= cap):
            placed.append((off, o))
            written += 1
        off += (n + 15) & ~15
    return table + [(off, written, 0)], placed


def rtp_packet(payload, seq, ssrc=0x11223344, cc=0, ext=None, pt=96, ts=0x01020304, padding=False):
    """a dressed RTP packet: cc CSRC words, ext = None or the number of extension words"""
    b0 = 0x80 | (0x20 if padding else 0) | (0x10 if ext is not None else 0) | cc
    p = bytes([b0, pt]) + (seq & 0xFFFF).to_bytes(2, "big") + ts.to_bytes(4, "big") + ssrc.to_bytes(4, "big")
    p += bytes((0xC0 + k) & 255 for k in range(4 * cc))
    if ext is not None:
        p += b"\xBE\xDE" + ext.to_bytes(2, "big") + bytes((0xE0 + k) & 255 for k in range(4 * ext))
    return p + bytes(payload)
