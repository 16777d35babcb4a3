"""The ReLU masks of the hidden-split kernels' dX epilogues (csrc/sac_split.h,
gemm_hf's masked form): pi's layer-2 and layer-1 dX in phase C and the critic
roles' unit-seed dX in phases A and C zero dX where !(p > 0), with the lane's
pre-activations read into registers ahead of the GEMM chain instead of one by
one between the epilogue's stores.

What a hoisted read can get wrong is WHICH element it reads, and p == 0.  So
the cases kill hidden units (tests/_dead_units.py: zero weight row and bias,
the pre-activation is +0.0 in every row) in every 16-column tile, at columns
0, 15, 16 and 255, over one whole tile, over a whole hidden layer, at Kp0 = 32
and 64, with 2A = 8, 16 and 24 (pi's layer-2 dX over one and two fp32 chunks
of dOut), at batch 20 (a full row tile and one with 4 valid rows):

  * every case is held to the CPU oracle by
    tests/test_gpu_parity.py::_check_config_against_oracle at its own bounds,
    two steps with injected indices and eps, on the split layout;
  * after each step the dead rows of W and b of all five networks and of
    Adam's m and v are exactly zero: a dead unit whose mask was read from
    another element gets a gradient, and its bias moves;
  * identity and tanh / elu nets, which read no mask (no derivative to apply,
    or act_pass_bwd applies it), are held to the oracle the same way;
  * every case is bit-identical to the parent commit's build:
    tests/golden/epilogue_parent_digests.json holds the SHA-256 of every
    array of state_tensors() and of the stats buffer after two steps, made
    from that build by tests/golden/make_epilogue_parent_digests.py.

tests/test_epilogue_masks_oracle.py shows on the CPU that the oracle alone
keeps the dead rows at zero, i.e. that these inputs do put p == 0 to the test.
"""
import json
import os
import sys

import pytest

import _dead_units as D
from test_gpu_parity import _check_config_against_oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_epilogue_parent_digests as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(D.CASES))
def test_dead_units_stay_dead_and_the_rest_matches_the_oracle(case):
    """fp32, 2 steps on the split layout."""
    c, sp = D.CASES[case]
    seen = []

    def on_step(k, hp, bt, pi_pre, post_loc, eng):
        D.assert_engine_rows_zero(eng, sp, (case, k))
        seen.append(k)

    with D.dead_nets(sp):
        _check_config_against_oracle(dict(c, name="epimask_" + case), "fp32", 2, expect="split", on_step=on_step)
    assert seen == [1, 2]


def test_bf16_dead_units_stay_dead():
    """bf16, with the bf16 mode's own bounds: the masks are the same LDS floats."""
    c, sp = D.CASES["dead_units"]
    seen = []

    def on_step(k, hp, bt, pi_pre, post_loc, eng):
        D.assert_engine_rows_zero(eng, sp, ("bf16", k))
        seen.append(k)

    with D.dead_nets(sp):
        _check_config_against_oracle(dict(c, name="epimask_bf16_dead_units"), "bf16", 2, expect="split",
                                     on_step=on_step)
    assert seen == [1, 2]


@pytest.mark.parametrize("acts", [("identity", "identity"), ("tanh", "elu")])
def test_paths_without_a_mask_match_the_oracle(acts):
    """Identity hidden layers (no mask) and tanh / elu (act_pass_bwd): nothing is read early."""
    c = D._shape(24, 4, 20, q_act=acts[0], pi_act=acts[1])
    _check_config_against_oracle(dict(c, name="epimask_" + "_".join(acts)), "fp32", 2, expect="split")


with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


def test_the_committed_digests_cover_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(G.CASES) and GOLDEN["steps"] == G.STEPS
    with open(G.OUT) as f:
        assert f.read() == G.render(GOLDEN)


@pytest.mark.parametrize("case", list(G.CASES))
def test_state_is_bit_identical_to_the_parent_build(case):
    """Two injected steps: every state array and the stats buffer hash to the
    parent build's digests (and the dead rows are zero: checked in digests())."""
    got = G.digests(case)
    want = GOLDEN["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (case, differ)
