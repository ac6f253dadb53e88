"""Record the verdict of the REFERENCE's own decoder on every illegal and damaged stream of the suite:
tests/golden/illegal_decode_record.json.  Needs oracle/_ref/ref_decode (the `ref` target of oracle/Makefile).

Tier 1 are the streams of slice_synth.ILLEGAL_PLANS (key "name[seed]"), tier 2 the streams of damage_corpus.corpus()
(a list, by corpus index).  Every stream is decoded by a child process with a time limit, and gets one class:

    complete    exit 0: "md5" holds the md5 of every picture (I420 bytes) it wrote, in order
    fatal       exit 1 after its own "Fatal error: ..." / "Frame #k, CurrMbAddr = m" lines: "frame" = k (1-based: k - 1
                pictures were decoded in front of it), "mb" = m, "message" = the text after "Fatal error: "
    undefined   it died of a signal or ran into the time limit ("how"): nothing to hold a decoder to

test_decode_illegal_host.py holds the oracle to this record, test_gpu_decode_illegal.py the device.

    python tests/golden/make_illegal_record.py
"""
import hashlib
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
REF_DECODE = ROOT / "oracle" / "_ref" / "ref_decode"
RECORD = HERE / "illegal_decode_record.json"
TIME_LIMIT = 30


def y4m_picture_md5s(data):
    """md5 of the I420 bytes of every picture of a Y4M file as the reference writes it"""
    if not data:
        return []
    head, _, rest = data.partition(b"\n")
    w, h = (int(re.search(rb" %s(\d+)" % k, head).group(1)) for k in (b"W", b"H"))
    fsz, out = w * h * 3 // 2, []
    while rest:
        assert rest[:6] == b"FRAME\n" and len(rest) >= 6 + fsz, "truncated Y4M file"
        out.append(hashlib.md5(rest[6:6 + fsz]).hexdigest())
        rest = rest[6 + fsz:]
    return out


def reference_verdict(stream, binary=REF_DECODE):
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / "in.264", Path(d) / "out.y4m"
        src.write_bytes(stream)
        try:
            r = subprocess.run([str(binary), str(src), str(dst)], timeout=TIME_LIMIT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, cwd=d)
        except subprocess.TimeoutExpired:
            return {"class": "undefined", "how": "time limit"}
        text = r.stdout.decode("latin-1")
        if r.returncode == 0:
            return {"class": "complete", "md5": y4m_picture_md5s(dst.read_bytes())}
        m = re.search(r"Fatal error: ([^\n]*)\n(?:[^\n]*\n)??Frame #(\d+), CurrMbAddr = (\d+)", text)
        if r.returncode == 1 and m:
            return {"class": "fatal", "frame": int(m.group(2)), "mb": int(m.group(3)), "message": m.group(1).strip()}
        return {"class": "undefined", "how": f"signal {-r.returncode}" if r.returncode < 0 else f"exit {r.returncode}"}


def all_streams():
    """-> ([(key, stream)] of tier 1, [stream] of tier 2)"""
    import damage_corpus as dc
    import slice_synth as ss
    t1 = []
    for name in sorted(ss.ILLEGAL_PLANS):
        for seed, (stream, _, _) in zip(ss.ILLEGAL_PLANS[name][2], ss.illegal_streams(name)):
            t1.append((f"{name}[{seed}]", stream))
    return t1, [s for _, _, s in dc.corpus()]


def main():
    import damage_corpus as dc
    if not REF_DECODE.exists():
        sys.exit(f"{REF_DECODE} missing: make -C oracle ref (needs the reference tree)")
    t1, t2 = all_streams()
    with ThreadPoolExecutor(8) as ex:
        v1 = list(ex.map(reference_verdict, [s for _, s in t1]))
        v2 = list(ex.map(reference_verdict, t2))
    # streams on which an instrumented build of the reference (make -C oracle ref_decode_asan) reads or writes outside its
    # arrays although the plain build exits 0: its output there is whatever lay behind the array
    keep = json.loads(RECORD.read_text()).get("reference_out_of_bounds", {}) if RECORD.exists() else {}
    for idx, why in keep.items():
        v2[int(idx)] = {"class": "undefined", "how": why}
    rec = {"corpus_md5": dc.corpus_md5(), "reference_out_of_bounds": keep, "tier1": {k: v for (k, _), v in zip(t1, v1)}, "tier2": v2}
    RECORD.write_text(json.dumps(rec, indent=0, sort_keys=True) + "\n")
    for tier, vs in (("tier 1", v1), ("tier 2", v2)):
        print(tier, {c: sum(v["class"] == c for v in vs) for c in ("complete", "fatal", "undefined")})


if __name__ == "__main__":
    main()
