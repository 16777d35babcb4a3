"""The cases of tests/test_gpu_update_tile_stages.py against the host-only
planner export (sac_debug_plan_host, include/sac_engine_testing.h; no GPU):
every case is planned on the kernel path, phase-B block size and slot count
that tests/golden/make_update_tile_parent_digests.py's table claims, so a
planner change cannot silently move a case off the instance of the update tile
it is there to reach."""
import json
import os
import sys

import pytest

from test_plan_cpu import _plan_text

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_update_tile_parent_digests as G  # noqa: E402


@pytest.mark.parametrize("case", list(G.CASES))
def test_the_case_is_planned_on_its_instance(case):
    c, precision, path, upd_threads_b, upd_slots = G.CASES[case]
    rc, text = _plan_text(c, precision, **c.get("layout", {}))
    assert rc == 0, text
    plan = json.loads(text)
    got = {k: plan[k] for k in ("path", "upd_threads_b", "upd_slots")}
    assert got == dict(path=path, upd_threads_b=upd_threads_b, upd_slots=upd_slots), case
    # the block sizes the launches use: phase D's tiles are always 1024 threads
    assert (plan["launch"]["B"]["threads"], plan["launch"]["D"]["threads"]) == (upd_threads_b, 1024), case


def test_the_cases_reach_both_block_sizes_and_slot_counts():
    rows = [v[3:] for v in G.CASES.values()]
    assert {r[0] for r in rows} == {512, 1024} and {r[1] for r in rows} == {1, 2}
    assert {v[1] for v in G.CASES.values()} == {"fp32", "bf16"}
