"""One child process of tests/test_window_sums_gpu.py: the switches of the window null sums that the
library reads once per process (FSCLG_CT_LDS, FSCLG_WIN_DESC, FSCLG_WINDOW_TREE, set by the parent in
the environment), on the cases window_ref.WORKER_CASES.

Prints one line per mismatch and a last line "WORKER <points> points <mismatches> mismatches"; exit
status 0: all equal, 1: mismatches, 3: a device error (nothing more ran on the GPU after it).
"""
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import walk_ref as wr  # noqa: E402
import window_ref as w  # noqa: E402


def main() -> int:
    os.environ["FSCLG_WINDOW_CHUNK"] = "2"
    shim = wr.Shim()
    bad, n = [], 0
    try:
        for name in w.WORKER_CASES:
            c = w.cases()[name]
            os.environ["FSCLG_PROFILE_CHUNK"] = "2" if c.geom.name == "prod" else "16"
            for label, runs in (("dense", c.dense_runs()), ("partial", c.partial_runs())):
                if runs:
                    w.upload_case(shim, c)
                    bad += w.device_mismatches(shim, c, runs, label)
                    n += sum(r.count for r in runs)
    except RuntimeError as e:
        print(f"DEVICE ERROR {e}")
        return 3
    finally:
        shim.close()
    for line in bad[:20]:
        print("MISMATCH", line)
    print(f"WORKER {n} points {len(bad)} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
