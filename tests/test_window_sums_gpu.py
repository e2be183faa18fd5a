"""The window null-sum kernels on crafted null values.

fsclg_profile returns each point's null_logl, which for a chromosome longer than the window is the
device's sum of the window that starts at window_start: a run with one position per site reads every
window start.  Every case of tests/window_ref.py is compared by bit pattern with the sequential sums,
never with another device result: with the chunked kernels (FSCLG_WINDOW_CHUNK=2: chunk_table_lds_kernel,
chunk_tree_kernel, window_chunk_kernel) and with the sequential ones (0: window_null_kernel), over every
window start (the host sums all windows, 256 starts per task) and over three short runs in one call
(on the long chromosome the host sums only their windows: launch_partial_windows).  The switches the
library reads once per process run in child processes (tests/window_worker.py).
tests/test_window_ref.py checks, without a GPU, that every vector is in the regime it is named for.
"""
from __future__ import annotations

import os
import subprocess
import sys
import time

import pytest

import walk_ref as wr
import window_ref as w
from util import ROOT

pytestmark = pytest.mark.gpu

ENV = ("FSCLG_WINDOW_CHUNK", "FSCLG_PROFILE_CHUNK")


@pytest.fixture(scope="module")
def shim(built):
    s = wr.Shim()
    saved = {k: os.environ.get(k) for k in ENV}
    yield s
    s.close()
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("name", list(w.cases()))
def test_window_sums(shim, name):
    c = w.cases()[name]
    g = c.geom
    if not c.on_device:
        # no entry point sums windows this long: the walks' segment table ends at 193 535 sites, and the
        # check comes before any device work (window_ref.MAX_WINDOW; lmax = CT_LMAX needs 262 144)
        w.upload_case(shim, c)
        with pytest.raises(RuntimeError, match="window above the segment table"):
            shim.profile([(0, wr.POS0 + wr.SPACING * g.er, wr.SPACING, 1)], eval_range=g.er)
        return
    os.environ["FSCLG_PROFILE_CHUNK"] = "2" if g.name == "prod" else "16"  # few points over more workgroups
    bad = []
    try:
        for mode in ("2", "0"):
            os.environ["FSCLG_WINDOW_CHUNK"] = mode  # read per call
            for label, runs in (("dense", c.dense_runs()), ("partial", c.partial_runs())):
                if not runs:
                    continue
                w.upload_case(shim, c)
                t0 = time.perf_counter()
                bad += w.device_mismatches(shim, c, runs, f"mode {mode} {label}")
                print(f"TIME {name} mode {mode} {label}: {sum(r.count for r in runs)} points "
                      f"{time.perf_counter() - t0:.2f} s")
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("switch", ["FSCLG_CT_LDS", "FSCLG_WIN_DESC", "FSCLG_WINDOW_TREE"])
def test_process_wide_switches(built, switch):
    """chunk_table_kernel with every tree level by chunk_tree_kernel; the halving search one level per
    round trip; no block maps (groups of 16 chunks): each in one fresh process."""
    env = dict(os.environ, **{switch: "0"})
    try:
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "window_worker.py")], env=env, capture_output=True,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{switch}=0: the worker did not finish", returncode=3)
    print(r.stdout[-3000:], r.stderr[-2000:])
    if r.returncode in (3, 124, 134, 137, 139) or r.returncode < 0:
        pytest.exit(f"{switch}=0: worker ended with {r.returncode}: {r.stdout[-500:]} {r.stderr[-500:]}", returncode=3)
    assert r.returncode == 0 and "WORKER" in r.stdout and " 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
