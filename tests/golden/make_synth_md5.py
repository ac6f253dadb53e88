"""Record what the REFERENCE's own decoder makes of every stream of tests/slice_synth.py: one md5 of its Y4M output per
stream, in tests/golden/synth_decode_md5.json.  Needs oracle/_ref/ref_decode (the `ref` target of oracle/Makefile links it
from the reference's decoder translation units where the reference tree is present).  test_slice_synth_host.py holds the
oracle to these md5s everywhere, and the binary to them where it exists.

    python tests/golden/make_synth_md5.py
"""
import hashlib
import json
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
REF_DECODE = ROOT / "oracle" / "_ref" / "ref_decode"


def reference_md5(stream):
    """md5 of the Y4M file the reference decoder writes for this stream (of an empty file if it writes no picture)"""
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / "in.264", Path(d) / "out.y4m"
        src.write_bytes(stream)
        subprocess.run([str(REF_DECODE), str(src), str(dst)], check=True, timeout=120, stdout=subprocess.DEVNULL, cwd=d)  # (it dumps a picture into its directory when it gives up)
        return hashlib.md5(dst.read_bytes()).hexdigest()


def main():
    import slice_synth as ss
    if not REF_DECODE.exists():
        sys.exit(f"{REF_DECODE} missing: make -C oracle ref (needs the reference tree)")
    out = {}
    for name in sorted(ss.PLANS):
        for k, (stream, _, _) in enumerate(ss.plan_streams(name)):
            out[f"{name}[{k}]"] = reference_md5(stream)
            print(f"{name}[{k}]", out[f"{name}[{k}]"])
    (HERE / "synth_decode_md5.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
