"""Record what the REFERENCE's own decoder makes of every stream of tests/qp_sweep.py (five streams at each QP 0..51, coded
by the oracle: 260 entries): one md5 of its Y4M output per stream, in tests/golden/qp_sweep_md5.json.  Needs oracle/_ref/ref_decode (the
`ref_decode` target of oracle/Makefile links it from the reference's decoder translation units where the reference tree is
present).  test_qp_sweep_host.py holds the oracle decoder to these md5s everywhere, and the binary to them where it exists.

    python tests/golden/make_qp_sweep_md5.py
"""
import importlib.util
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))

_spec = importlib.util.spec_from_file_location("make_synth_md5", HERE / "make_synth_md5.py")
_synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_synth)
REF_DECODE, reference_md5 = _synth.REF_DECODE, _synth.reference_md5


def key(stream, qp):
    return f"{stream}@qp{qp}"


def main():
    import fo_py
    import qp_sweep as qs
    if not REF_DECODE.exists():
        sys.exit(f"{REF_DECODE} missing: make -C oracle ref_decode (needs the reference tree)")
    out = {}
    for stream in qs.STREAMS:
        for qp in qs.QPS:
            out[key(stream, qp)] = reference_md5(qs.run(fo_py, stream, qp)["stream"])
            print(key(stream, qp), out[key(stream, qp)])
    (HERE / "qp_sweep_md5.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
