"""NumPy model of Annex-B NAL framing (writeNAL, F/nal.cpp:261-299) in closed form, and the corpus that pins it.

writeNAL keeps a counter of zero bytes that only takes the values 0, 1 and 2 and that an insertion resets.  Read as a rule on
the payload alone: inside a maximal run of zero bytes z_0 .. z_{L-1} an 03 is inserted before z_k exactly when k >= 2 and k is
even, and before the non-zero byte b that ends the run exactly when b <= 3, L >= 2 and L is even.  Both cases are one
condition on d = the number of zero bytes directly in front of a byte (its distance to the last non-zero byte, a max-scan):
the byte is <= 3, d >= 2 and d is even.  A byte's output position is its own index plus the prefix sum of the flags.
Nothing here walks the bytes one at a time.
"""
import numpy as np

CHUNK = 4096  # payload bytes one workgroup of the device kernels takes (csrc/fer_nalpack.hip)


def escape_flags(payload):
    """bool [n]: an 03 goes in front of byte i"""
    b = np.asarray(payload, np.uint8)
    n = b.size
    if n == 0:
        return np.zeros(0, bool)
    i = np.arange(n, dtype=np.int64)
    last_nz = np.maximum.accumulate(np.where(b != 0, i, -1))  # index of the last non-zero byte at or before i
    prev = np.concatenate(([-1], last_nz[:-1]))               # ... before i
    d = i - 1 - prev                                          # zero bytes directly in front of i
    return (b <= 3) & (d >= 2) & (d % 2 == 0)


def frame_nal(nal_type, payload, nal_ref_idc=1):
    """start code + header byte + escaped payload, as bytes"""
    b = np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray)) else np.asarray(payload, np.uint8).reshape(-1)
    f = escape_flags(b)
    pos = np.arange(b.size, dtype=np.int64) + np.cumsum(f)  # where byte i lands in the escaped payload
    out = np.empty(5 + b.size + int(f.sum()), np.uint8)
    out[:5] = (0, 0, 0, 1, (nal_ref_idc << 5) | (nal_type & 31))
    out[5 + pos] = b
    out[5 + pos[f] - 1] = 3
    return out.tobytes()


def _lengths():
    ls = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
    for c in (4096, 16384, CHUNK):
        ls += [c - 1, c, c + 1, 2 * c + 5, 3 * c]
    return sorted(set(ls))


_corpus = None


def corpus():
    """-> list of (payload uint8 array, nal_type); built once, never modified by its users"""
    global _corpus
    if _corpus is not None:
        return _corpus
    out = []
    # all-zero payloads and payloads of 00 00 01 of every length
    for n in _lengths():
        out.append(np.zeros(n, np.uint8))
        out.append(np.tile(np.array([0, 0, 1], np.uint8), n // 3 + 1)[:n].copy())
    # zero runs of length 1..7 that end at offsets -3..+3 around every multiple of 16 (so around every multiple of 1024 and
    # of c too) within the first 2c bytes, each followed by a byte of every class; the bytes between the runs are 0xab
    cmax = max(16384, CHUNK)
    for run in range(1, 8):
        for delta in range(-3, 4):
            for follow in (0x01, 0x03, 0x04, 0xFF):
                p = np.full(2 * cmax + 16, 0xAB, np.uint8)
                for m in range(16, 2 * cmax + 1, 16):
                    end = m + delta  # the run is [end - run, end), the follower sits at end
                    p[end - run: end] = 0
                    p[end] = follow
                out.append(p)
            # ... and by the end of the payload: the payload stops where the run does.  Around 16 and 32, and around every
            # multiple of 1024 up to 2 * 4096 and the multiples of 16384: every wavefront boundary of two chunks, both
            # chunk sizes and their doubles
            for m in (16, 32, 1024, 2048, 3072, 4096, 5120, 6144, 7168, 8192, 16384, 32768):
                p = np.full(m + delta, 0xAB, np.uint8)
                p[m + delta - run:] = 0
                out.append(p)
    # the remaining multiples of 1024 within 2 * 16384 (same position in the chunk as one above, another chunk count): the
    # run lengths 2 and 3, the shortest of either parity that reach an insertion
    for m in range(9 * 1024, 2 * cmax, 1024):
        if m == 16384:
            continue
        for run in (2, 3):
            for delta in range(-3, 4):
                p = np.full(m + delta, 0xAB, np.uint8)
                p[m + delta - run:] = 0
                out.append(p)
    # random payloads over an alphabet that makes runs frequent
    rng = np.random.default_rng(20240917)
    alphabet = np.array([0, 0, 0, 1, 2, 3, 4, 0xFF], np.uint8)
    for k in range(200):
        c = (4096, 16384)[k & 1]
        out.append(alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 3 * c + 1)))])
    types = (5, 1, 7, 8)
    _corpus = [(p, types[k % 4]) for k, p in enumerate(out)]
    for p, _ in _corpus:
        p.setflags(write=False)
    return _corpus
