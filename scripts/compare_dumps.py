"""Compare two directories written by bench.py --dump-outputs or scripts/dump_call_outputs.py file by file with np.array_equal.   usage: compare_dumps.py <dir A> <dir B>
Exit status 0 only if both hold the same .npy files and every one compares equal."""
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
fa, fb = sorted(f for f in os.listdir(a) if f.endswith(".npy")), sorted(f for f in os.listdir(b) if f.endswith(".npy"))
bad = 0 if fa == fb and fa else 1
for f in fa:
    if f not in fb:
        continue
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.dtype == y.dtype and np.array_equal(x, y)
    bad += 0 if same else 1
    print("%-40s %-10s %-20s %s" % (f, x.dtype, x.shape, "equal" if same else "DIFFERENT"))
print("%d files, %s" % (len(fa), "all equal" if not bad else "NOT equal (%d problems; only in one: %s)" % (bad, sorted(set(fa) ^ set(fb)))))
sys.exit(1 if bad else 0)
