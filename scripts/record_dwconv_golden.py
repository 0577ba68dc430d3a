"""Record tests/golden/dwconv_exact.npz, the fixture of tests/test_gpu_dwconv_exact.py, from the
library that is built in this tree (run it on the commit whose results are to be pinned, before
a change to csrc/dwconv.hip, or from a worktree of that commit).  The cases, the seeded CPU input
generator and the kernel calls are the test's own; only outputs are stored: one SHA-256 per image
row of out / act'(z) / dh / out of the eval entry point, dW and db whole, plus the digest of the
inputs each case was recorded with.
Usage (GPU box): python scripts/record_dwconv_golden.py [OUT.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_dwconv_exact as T  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for dt, shp, act in T.CASES:
        cid = T.case_id(dt, shp, act)
        res, gd = T.run_case(dt, shp, act)
        rec[f"{cid}/inputs"] = T.input_digest(dt, shp, act)
        for k, g in gd.items():
            assert g.guards_intact(), f"{cid}: {k} was written outside its rows"
            assert bool(g.t.float().isfinite().all()), f"{cid}: {k} keeps poison"
            rec[f"{cid}/{k}"] = T.row_digests(res[k], shp[1])
        if act != "none":
            assert np.array_equal(rec[f"{cid}/out"], rec[f"{cid}/out_nosave"]), f"{cid}: fwd != fwd_save"
            rec[f"{cid}/dW"] = res["dW"].cpu().numpy()
            rec[f"{cid}/db"] = res["db"].cpu().numpy()
        print(cid, "recorded")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **rec)
    print(f"{out_path}: {len(rec)} arrays, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
