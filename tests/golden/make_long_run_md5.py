"""Record what the REFERENCE's own decoder makes of the long streams of tests/long_run.py: one md5 of its Y4M output per
stream, in tests/golden/long_run_md5.json -- the two P-run streams the oracle encodes across the frame_num wrap, and every
held and override stream of the synthesized batches.  The mixed family is left out: oracle/_ref/ref_decode dies with
SIGSEGV on it.  Needs oracle/_ref/ref_decode (the `ref` target of oracle/Makefile).  test_long_run_host.py holds the oracle
to these md5s everywhere, and the binary to them where it exists.

    python tests/golden/make_long_run_md5.py
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


def synth_name(key):
    return "%s[offset %d, %d pictures]" % key


def streams():
    """-> [(name, (Annex-B bytes, the oracle's pictures, W, H))] of every stream that carries a record"""
    import long_run as lr
    out = []
    for s, (stream, rec, _) in enumerate(lr.p_run_oracle()):
        out.append((f"p_run[{s}]", (stream, rec, lr.P_RUN["W"], lr.P_RUN["H"])))
    keys = {k for f in lr.RECORDED_FAMILIES for k in lr.SYNTH_BATCHES[f]} | {lr.SYNTH_LONG[f] for f in lr.RECORDED_FAMILIES}
    for key in sorted(keys):
        out.append((synth_name(key), (lr.synth_stream(*key)[0], lr.synth_oracle(*key)[0], lr.SYNTH_W, lr.SYNTH_H)))
    return out


def main():
    if not REF_DECODE.exists():
        sys.exit(f"{REF_DECODE} missing: make -C oracle ref (needs the reference tree)")
    out = {}
    for name, (stream, _, _, _) in streams():
        out[name] = reference_md5(stream)
        print(name, out[name])
    (HERE / "long_run_md5.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
