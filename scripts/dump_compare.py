"""Compare two `bench.py --dump-outputs` directories bit for bit.
Usage: python scripts/dump_compare.py DIR_A DIR_B   (exit status 1 if any array differs)"""
import os
import sys

import numpy as np


def main(a, b):
    ok = True
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")), (a, b)
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        diff = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape else float("nan")
        print(f"{f[:-4]}: {x.size} elements, bitwise equal {same}, max |difference| {diff:.3e}")
        ok &= same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
