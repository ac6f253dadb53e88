"""Known-answer tests of the CAVLC block parser (row a19 of SURVEY.md 8a at block level): residual_block_cavlc
(F/residual.cpp:1069) through ferhip_cavlc_parse_blocks -- the decoder's own dec_block over the decoder's bit reader and
tables -- against the oracle, one block at a time, with nC stated."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMBOS = [(16, nC) for nC in (0, 1, 2, 3, 4, 7, 8, 16)] + [(15, nC) for nC in (0, 1, 2, 3, 4, 7, 8, 16)] + [(4, -1)]


def _random_levels(rng, n, maxn):
    """level vectors the way a quantiser leaves them: mostly zero, a run of +-1 at the tail, now and then large levels (escape codes)
    (the distribution of test_cavlc_block_writer_kat)"""
    c = np.zeros((n, 16), np.int32)
    for i in range(n):
        kind = rng.integers(0, 6)
        if kind == 0:
            continue                                               # empty block
        dens = rng.choice([0.1, 0.3, 0.6, 1.0])
        mask = rng.random(maxn) < dens
        mag = rng.choice([1, 1, 1, 2, 3, 8, 40, 300, 2000])
        v = rng.integers(1, mag + 1, maxn) * rng.choice([-1, 1], maxn)
        if kind == 1:
            v = rng.choice([-1, 1], maxn)                          # trailing ones only
        if kind == 2:
            v[rng.integers(0, maxn)] = rng.choice([-1, 1]) * rng.integers(16, 2040)   # level_prefix 14 / 15 escapes (12-bit suffix: |level| <= 2063)
            mask[:] = mask | (np.arange(maxn) == np.argmax(np.abs(v)))
        c[i, :maxn] = np.where(mask, v, 0)
    return c


def _bits_of(data, nbits):
    """the first nbits bits (MSB first) of bytes / a uint8 array, one per entry"""
    return np.unpackbits(np.frombuffer(data, np.uint8) if isinstance(data, bytes) else np.asarray(data, np.uint8))[:nbits]


def _stream(pieces):
    """bit arrays back to back -> (bytes of the stream, bit position of every piece)"""
    pos = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
    return np.packbits(np.concatenate(pieces)), pos[:-1]


def test_block_parser_kat(pkg, fo):
    rng = np.random.default_rng(2025)
    coef, nCs, maxns, ref_bits, ref_n, ref_tc = [], [], [], [], [], []
    for maxn, nC in COMBOS:
        c = _random_levels(rng, 700, maxn)
        for i in range(700):
            data, n, tc = fo.cavlc_encode_block(c[i], maxn, nC)
            ref_bits.append(_bits_of(data, n))
            ref_n.append(n)
            ref_tc.append(tc)
        coef.append(c)
        nCs += [nC] * 700
        maxns += [maxn] * 700
    coef = np.concatenate(coef)
    N = coef.shape[0]
    assert N == 11900
    # ONE stream, the blocks back to back: they begin at every bit alignment and straddle the reader's 32-bit refills and
    # its 256-byte ring chunks
    stream, pos = _stream(ref_bits)
    assert stream.size > 40 * 256 and len(set(int(p) % 32 for p in pos)) == 32
    got, tc, used = pkg.cavlc_parse_blocks(stream, pos, nCs, maxns)
    ref_n, ref_tc = np.array(ref_n), np.array(ref_tc)
    bad = np.flatnonzero((tc != ref_tc) | (used != ref_n) | (got != coef).any(1))
    assert bad.size == 0, (bad[:5], [(maxns[i], nCs[i], coef[i], got[i], tc[i], ref_tc[i], used[i], ref_n[i]) for i in bad[:3]])
    # the writer on the device followed by the parser on the device is the identity
    dbits, dn, dtc = pkg.cavlc_blocks(coef, nCs, maxns)
    dstream, dpos = _stream([_bits_of(dbits[i], dn[i]) for i in range(N)])
    got2, tc2, used2 = pkg.cavlc_parse_blocks(dstream, dpos, nCs, maxns)
    assert np.array_equal(got2, coef) and np.array_equal(tc2, dtc) and np.array_equal(used2, dn)


def test_block_parser_reports_malformed_blocks(pkg, fo):
    rng = np.random.default_rng(77)

    def enc(c, maxn, nC):
        data, n, tc = fo.cavlc_encode_block(np.asarray(c, np.int32), maxn, nC)
        return _bits_of(data, n), tc

    # coeff_token(TotalCoeff 1, TrailingOnes 0) at nC 0: the block [2] is that token, the level "1" and total_zeros "1"
    one, _ = enc([2] + [0] * 15, 16, 0)
    assert len(one) == 8
    token = one[:6]
    full16, _ = enc(np.arange(1, 17), 16, 0)                  # TotalCoeff 16: too many for maxNumCoeff 15
    five, _ = enc([3, -2, 4, 1, -1] + [0] * 11, 16, 0)        # TotalCoeff 5: too many for maxNumCoeff 4
    long_block, _ = enc(rng.integers(200, 400, 16), 16, 0)    # begins in the last byte of the stream and runs out of it
    assert len(long_block) > 100
    good = _random_levels(rng, 6, 16)
    good[0, :3] = (7, -1, 1)                                   # (no empty one among them)
    pieces, want = [], []                                      # want: (nC, maxn, levels or None = malformed)

    def add(bits, nC, maxn, levels):
        pieces.append(bits)
        want.append((nC, maxn, levels))

    for k, (bits, nC, maxn) in enumerate(((np.concatenate([token, np.zeros(40, np.uint8)]), 0, 16), (full16, 0, 15), (five, 0, 4))):
        add(enc(good[2 * k], 16, 3)[0], 3, 16, good[2 * k])
        add(bits, nC, maxn, None)
        add(enc(good[2 * k + 1], 16, 9)[0], 9, 16, good[2 * k + 1])
    pieces.append(np.zeros(-sum(len(p) for p in pieces) % 8, np.uint8))   # to a byte boundary
    want.append(None)
    add(long_block[:5], 0, 16, None)
    stream, pos = _stream(pieces)
    keep = [i for i, w in enumerate(want) if w is not None]
    pos, want = pos[keep], [want[i] for i in keep]
    assert int(pos[-1]) // 8 == stream.size - 1
    coef, tc, used = pkg.cavlc_parse_blocks(stream, pos, [w[0] for w in want], [w[1] for w in want])
    for i, (nC, maxn, levels) in enumerate(want):
        if levels is None:
            assert tc[i] == -1 and not coef[i].any(), (i, tc[i], coef[i])
        else:
            assert tc[i] == np.count_nonzero(levels) and np.array_equal(coef[i], levels), (i, tc[i], coef[i], levels)
            assert used[i] == len(enc(levels, maxn, nC)[0])
    assert sum(w[2] is None for w in want) == 4


def test_block_parser_under_the_reference_name(pkg, fo):
    """residual_block_cavlc (F/residual.cpp:1069) on ferhip_legacy_bits: a dozen blocks in a row, the cursor advances by each
    block's bits; a malformed block leaves the cursor alone and zeroes the block."""
    lib = pkg.load_library()
    rng = np.random.default_rng(5)
    nbits_g, pos_g, nC_g = (C.c_uint.in_dll(lib, "ferhip_legacy_nbits"), C.c_uint.in_dll(lib, "ferhip_legacy_bitpos"), C.c_int.in_dll(lib, "ferhip_legacy_nC"))
    buf = (C.c_ubyte * (1 << 16)).in_dll(lib, "ferhip_legacy_bits")
    saved = (nbits_g.value, pos_g.value, nC_g.value, bytes(buf[:512]))
    try:
        blocks = []
        for k in range(12):
            maxn, nC = COMBOS[(5 * k) % len(COMBOS)]
            c = _random_levels(rng, 1, maxn)[0]
            if k % 3 == 0 or k == 11:
                c[:2] = (-4, 1)                               # (not empty: block 11 is cut short below)
            data, n, _ = fo.cavlc_encode_block(c, maxn, nC)
            blocks.append((c, maxn, nC, _bits_of(data, n)))
        stream, pos = _stream([b[3] for b in blocks])
        total = sum(len(b[3]) for b in blocks)
        assert stream.size <= 512
        C.memmove(buf, stream.ctypes.data, stream.size)
        nbits_g.value, pos_g.value = total, 0
        for k, (c, maxn, nC, bits) in enumerate(blocks):
            assert pos_g.value == int(pos[k])
            nC_g.value = nC
            out = (C.c_int * 16)(*([99] * 16))
            lib.residual_block_cavlc(out, 0, maxn - 1, maxn)
            assert list(out)[:maxn] == c[:maxn].tolist(), (k, maxn, nC)
            assert list(out)[maxn:] == [99] * (16 - maxn)     # (the caller's array may end at maxNumCoeff: ChromaDCLevel)
        assert pos_g.value == total
        # behind the last block nothing is left: the cursor stays, the block is zeroed
        out = (C.c_int * 16)(*([99] * 16))
        lib.residual_block_cavlc(out, 0, 15, 16)
        assert pos_g.value == total and list(out) == [0] * 16
        # a coeff_token that promises more than the stream holds
        pos_g.value = int(pos[11])
        nbits_g.value = int(pos[11]) + 3
        nC_g.value = blocks[11][2]
        lib.residual_block_cavlc(out, 0, blocks[11][1] - 1, blocks[11][1])
        assert pos_g.value == int(pos[11]) and not any(list(out)[:blocks[11][1]])
    finally:
        nbits_g.value, pos_g.value, nC_g.value = saved[:3]
        C.memmove(buf, saved[3], 512)
