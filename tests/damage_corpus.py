"""A fixed corpus of damaged streams: the three QCIF P goldens with bytes overwritten or one bit flipped.

Test infrastructure (plain Python + numpy, seeded, no GPU).  Per golden 32 streams of the byte recipe of the damage
tests (1..5 bytes inside a 64-byte window overwritten with values 2..255) and 16 streams with one flipped bit; every
change lies behind byte 64 (the parameter sets and the first slice header) and no changed byte becomes 0 or 1, so no
start code is minted.  144 streams, addressed by corpus index.  What the reference's decoder makes of each is recorded
in tests/golden/illegal_decode_record.json (tests/golden/make_illegal_record.py); test_decode_illegal_host.py pins the
bytes, test_gpu_decode_illegal.py runs them on the device.
"""
import hashlib
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden"
GOLDENS = ("qcif_ippp_4f_qp12_w16", "qcif_ippp_4f_qp28_w32", "qcif_skip_5f_qp12")
SEED = 2026
N_BYTES, N_BITS = 32, 16
W, H = 176, 144


def _bytes_recipe(rng, clean):
    bad = bytearray(clean)
    lo = 64 + int(rng.integers(0, len(bad) - 200))
    for _ in range(int(rng.integers(1, 6))):
        bad[min(lo + int(rng.integers(0, 64)), len(bad) - 1)] = int(rng.integers(2, 256))
    return bytes(bad)


def _bit_flip(rng, clean):
    bad = bytearray(clean)
    while True:
        pos, bit = 64 + int(rng.integers(0, len(bad) - 64)), int(rng.integers(0, 8))
        if bad[pos] ^ (1 << bit) >= 2:
            bad[pos] ^= 1 << bit
            return bytes(bad)


_corpus = None


def corpus():
    """-> [(name, golden, damaged stream)], 48 per golden: index i of the list is the corpus index"""
    global _corpus
    if _corpus is None:
        out = []
        for g, golden in enumerate(GOLDENS):
            clean = (GOLD / f"{golden}.264").read_bytes()
            rng = np.random.default_rng([SEED, g])
            for k in range(N_BYTES):
                out.append((f"{golden}/bytes{k:02d}", golden, _bytes_recipe(rng, clean)))
            for k in range(N_BITS):
                out.append((f"{golden}/bit{k:02d}", golden, _bit_flip(rng, clean)))
        _corpus = out
    return _corpus


def corpus_md5():
    h = hashlib.md5()
    for name, _, stream in corpus():
        h.update(name.encode() + b"\0" + hashlib.md5(stream).digest())
    return h.hexdigest()
