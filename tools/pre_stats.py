"""Dev helper (FER_STATS build): how often k_me_pre's lower-bound pruning applies, and which routes the selections take."""
import sys
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import load_pkg
pkg = load_pkg()
W, H, S = 1920, 1072, 4
fr = np.stack([np.stack([pkg.gen_frame(W, H, t, 1234 + s, 2) for s in range(S)]) for t in range(3)])
g = pkg.FerHip(W, H, S, qp=12, window=32, maxdiff=3, intra_every=30)
g.encode_streams(fr)
t = g.read("TIMING")
n = max(int(t[48]), 1)
print("partitions", n, "fallback", t[49] / n, "avg survivors", t[50] / n, "no threshold", t[51] / n, "avg T", t[52] / n)
# slots of d.timing: SEL_SITE_ST1, _ST2, _ST3, _ST3_FULL and SEL_SITE_N2_HI of csrc/fer_me.hip (change both together)
SEL_SITES = (("stage 1", 8), ("stage 2", 11), ("stage 3 pruned", 14), ("stage 3 full", 17))
SEL_N2_HI = 20
for name, k in SEL_SITES:
    m = max(int(t[k]), 1)
    print("%-15s selections %d  coarse bound overflowed %.4f  left the wide route %.4f" % (name, t[k], t[k + 1] / m, t[k + 2] / m))
print("stage 2 selections over all six batches (n2 > 192): %d = %.4f" % (t[SEL_N2_HI], t[SEL_N2_HI] / max(int(t[11]), 1)))
