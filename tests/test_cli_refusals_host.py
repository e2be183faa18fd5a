"""What the `fscl` command line answers to arguments it refuses (no GPU): the exit code and the message lines, in
their order, of every option check, of the refusals between the data load and the first device call, and of the
argument loop, against tests/golden/cli_refusals.json (recorded by tests/golden/make_cli_refusals.py); and no file
named in the arguments is left behind by a refusal.  And tools/cli_host_check.c under the sanitizers: the
argument loop and the resolved option record, default by default."""
from __future__ import annotations

import json

import pytest

from util import GOLD, cli_answer, run_host_check

CASES = json.loads((GOLD / "cli_refusals.json").read_text())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_answers_as_recorded(built, tmp_path, case):
    code, lines = cli_answer(case, tmp_path)
    assert (code, lines) == (case["exit"], case["lines"])
    if code != 0:
        assert list(tmp_path.iterdir()) == []   # (every file the arguments name lies under @TMP@)


def test_the_fixture_covers_what_it_claims():
    text = "\n".join(ln for c in CASES for ln in c["lines"])
    for opt in ("surface", "conditional", "expect", "jackknife"):
        assert f"--{opt}-alphas must be LO:HI:N" in text
    for what in ("--scan-mode=grid", "--bootstrap-file", "--tail-file", "--familywise-file"):
        assert f"{what} runs in one process" in text
    for opt in ("simulate", "bootstrap", "given", "expect"):
        assert f"fscl: --{opt}-sweep=" in text and "unknown chromosome name" in text
    for cap in ("FSCL_AMD_COND_CAP", "FSCL_AMD_FWER_CAP", "a position past the int range"):
        assert cap in text
    assert sum(len(c["lines"]) > 3 for c in CASES) >= 4
    by = {c["name"]: c for c in CASES}
    assert by["lenient_sites_top_word"]["exit"] == 0 == by["lenient_surface_step_minus_one"]["exit"]
    assert by["help"]["exit"] == 0 and by["missing_value_long"]["exit"] == 255
    assert [ln[:30] for ln in by["surface_halfwidth_negative"]["lines"]] == ["Error: --surface-halfwidth mus", "Error: --jackknife-halfwidth m"]


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/cli_host_check.c: the argument loop and the check-and-resolve pass on a table of argument vectors, the
    resolved record asserted field by field, under ASan and UBSan, as a stand-alone program (no device library,
    nothing loaded into Python)."""
    run_host_check("cli_host_check", ["cli_options.c", "surface.c", "util.c"], tmp_path)
