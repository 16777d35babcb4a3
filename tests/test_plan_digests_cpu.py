"""The engine's whole launch plan on the CPU (no GPU needed): the kernel path,
workspace and LDS sizes, every phase's grid and the bytes of every descriptor
the planner builds (sac_debug_plan_host, include/sac_engine_testing.h), for the
matrix of tests/golden/make_plan_digests.py, against the committed
tests/golden/plan_digests.json.  A planner edit that is meant to leave the
plan alone is proved here to do so, down to the padding bytes of a tile."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "soft-actor-critic_amd"))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import make_plan_digests as G  # noqa: E402
from sac import _engine as E  # noqa: E402

CASES = G.cases()
with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    return G.bind(E.load_library())


def test_the_committed_file_holds_exactly_the_matrix():
    assert sorted(GOLDEN) == sorted(CASES)
    with open(G.OUT) as f:
        assert f.read() == G.render(GOLDEN), "plan_digests.json: sorted, one case per line (make_plan_digests.render)"


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_matches_the_committed_digest(lib, case):
    assert G.digest(lib, CASES[case]) == GOLDEN[case]


def test_plan_dump_is_deterministic(lib):
    """Two calls on one config give the same text: the hashed structs' padding is
    zeroed, and nothing of an earlier call is left in the planner."""
    for case in ("bench/c2/fp32/default", "bench/c3/bf16/default", "past_lds/obs24_act4_512x512/fp32"):
        first = G.plan_text(lib, CASES[case])
        G.plan_text(lib, CASES["bench/c1/fp32/default"])
        assert first[0] == 0 and G.plan_text(lib, CASES[case]) == first, case


def test_plan_dump_refuses_a_short_buffer(lib):
    rc, msg = G.plan_text(lib, CASES["bench/c2/fp32/default"], cap=64)
    assert rc == -1 and "plan dump needs" in msg, (rc, msg)


# The kernels phases A and C run for each bench config, as the engine picks them
# (no override), read off plan_digests.json: "split" the hidden-split role
# kernels (sac_split.h), "roles" the per-network role kernels and "rows" one
# workgroup per row tile (sac_phases.h), "pairs" the pair-tile kernels
# (sac_pairs.h), "wide" the layer-synchronous stage path (sac_wide.h).
BENCH_PATHS = {
    ("c1", "fp32"): "roles", ("c1", "bf16"): "roles",    # [64, 64] nets, B = 64
    ("c2", "fp32"): "split", ("c2", "bf16"): "split",    # [256, 256], B = 256: the headline
    ("c3", "fp32"): "pairs", ("c3", "bf16"): "pairs",    # B = 4096: 256 row tiles, too many role workgroups
    ("c4", "fp32"): "split", ("c4", "bf16"): "split",
    ("c4w", "fp32"): "split", ("c4w", "bf16"): "split",  # obs 216: only the role kernels' R-row layout fits
}


def test_bench_configs_run_the_kernels_the_table_names(lib):
    assert sorted(BENCH_PATHS) == sorted((n, p) for n in bench.CONFIGS for p in G.PRECISIONS)
    for (name, prec), path in BENCH_PATHS.items():
        case = f"bench/{name}/{prec}/default"
        assert GOLDEN[case]["path"] == path, case
        assert G.digest(lib, CASES[case])["path"] == path, case
