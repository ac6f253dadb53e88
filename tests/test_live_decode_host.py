"""access_units (host only): the chunks a live decoder is fed, one slice NAL unit each, cut so that every NAL unit keeps
exactly the bytes it has inside the whole stream."""
from pathlib import Path

import pytest
from conftest import golden_bytes

GOLD = Path(__file__).resolve().parent / "golden"
GOLDENS = sorted(p.name for p in GOLD.glob("*.264")) + ["drugi.264"]


@pytest.mark.parametrize("name", GOLDENS)
def test_access_units_split_goldens_into_one_slice_each(pkg, name):
    stream = golden_bytes(name)
    chunks = pkg.access_units(stream)
    assert b"".join(chunks) == stream
    nals = pkg.split_nals(stream)
    slices = [n for n in nals if n[4] & 31 in (1, 5)]
    assert len(chunks) == len(slices) > 0
    got = []
    for c in chunks:
        cn = pkg.split_nals(c)
        assert [n[4] & 31 in (1, 5) for n in cn].count(True) == 1
        assert cn[-1][4] & 31 in (1, 5) or c is chunks[-1]
        got += cn
    assert got == nals


def test_access_units_keep_parameter_sets_with_the_next_slice(pkg):
    stream = golden_bytes("qcif_ippp_4f_qp12_w16.264")
    chunks = pkg.access_units(stream)
    assert [n[4] & 31 for n in pkg.split_nals(chunks[0])] == [7, 8, 5]
    assert all([n[4] & 31 for n in pkg.split_nals(c)] == [1] for c in chunks[1:])


def test_access_units_cut_at_the_nal_end_the_decoder_sees(pkg):
    """Zero bytes in front of a start code end the NAL unit before them (00 00 00): they go to the next chunk, so the
    slice's RBSP is the same in the chunk as in the stream."""
    sps, pps = b"\x00\x00\x00\x01\x67\x42", b"\x00\x00\x00\x01\x68\xce"
    s1, s2 = b"\x00\x00\x00\x01\x65\x88\x80", b"\x00\x00\x00\x01\x41\x9a\x80"
    stream = sps + pps + s1 + b"\x00\x00" + s2 + b"\x00\x00\x00\x01\x06\x05"
    chunks = pkg.access_units(stream)
    assert chunks == [sps + pps + s1, b"\x00\x00" + s2 + b"\x00\x00\x00\x01\x06\x05"]
    assert pkg.access_units(b"") == []


def test_live_decoder_create_checks_its_arguments_before_the_device(pkg):
    """Arguments are refused with FERHIP_E_ARG before any device is looked for (so this needs no GPU)."""
    import ctypes as C
    lib = pkg.load_library()
    h = C.c_void_p()
    for args in [(0, 176, 144, 1), (-3, 176, 144, 1), (1, 170, 144, 1), (1, 176, 140, 1), (1, 0, 144, 1), (1, 176, 144, 0),
                 (1, 176, 144, -1)]:
        assert lib.ferhip_decs_create(C.byref(h), *args) == -1, args
        assert not h.value
    assert lib.ferhip_decs_create(None, 1, 176, 144, 1) == -1
    assert lib.ferhip_decs_decode(None, None, None, None, 0, None, None) == -1
    assert lib.ferhip_decs_reset_stream(None, 0) == -1
    lib.ferhip_decs_destroy(None)
