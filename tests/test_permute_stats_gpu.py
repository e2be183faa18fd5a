"""The pipelined permutation test's schedule-determined counters, pinned to the values recorded from
the commit named in tests/golden/permute_stats.json: which points went to the blocking batch, how
many were merged, how many cells were evaluated.  A change of a stage boundary that leaves the
results right but sends other points to the blocking batch shows here."""
from __future__ import annotations

import json

import pytest

from util import GOLD
import fscl_amd
from fscl_amd import synth

pytestmark = pytest.mark.gpu


def test_schedule_counters_match_the_recorded_commit(built, tmp):
    gold = json.loads((GOLD / "permute_stats.json").read_text())
    g = gold["genome"]
    snp = tmp / "pipe.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=g["n_chr"], chr_len=g["chr_len"], snps_per_chr=g["snps_per_chr"],
                                                  n=g["n"], seed=g["seed"], sweeps_per_chr=g["sweeps_per_chr"]))
    fscl_amd.reset_stats()
    fscl_amd.run(snp, tmp / "g.txt", large_grid_sp=g["large_grid_sp"], n_permute=g["n_permute"])
    st = fscl_amd.get_stats()
    got = {k: int(st[k]) for k in gold["counters"]}
    print(got)
    assert set(gold["counters"]) == {"trials", "gp_evals", "n_crit", "n_merged", "n_drain", "negj", "plan_mode",
                                     "plan_fallback"} - set(gold["dropped"])
    assert got == gold["counters"]
