"""The transposed stashes of the hidden-split kernels (csrc/sac_split.h): in
fp32, with a ReLU / identity hidden activation, the X^T stashes of phase A
(H0^T, H1^T of the critics and pi(s)), the critics' unit-seed dY^T (U1^T, the U0
partial and layer 2's valid-row indicator) and pi's dY1^T / dY0^T of phase C are
stored from the GEMM epilogues' registers (store_acc_T: the lane's four rows of
a column are 16 contiguous bytes of the [k][Bp] stash) instead of by store_T's
pass over LDS.  No float operation moves and every element receives the value
store_T gave it, so

  * every case is bit-identical to the parent commit's build:
    tests/golden/stash_store_parent_digests.json holds the SHA-256 of every
    array of state_tensors() and of the stats buffer after two injected
    steps, made from that build by
    tests/golden/make_stash_store_parent_digests.py; the digests are
    recomputed here;
  * every case is held to the CPU oracle by
    tests/test_gpu_parity.py::_check_config_against_oracle at its own bounds,
    two steps with injected indices and eps, on the split layout.

What a register store can get wrong is which rows it masks (rows >= nvalid and
padded columns are written as +0, not skipped: the dW reductions sum over
them) and where a lane's four rows land.  A row tile is 16 batch rows and a
lane holds 4, so the cases are batch 32 (two full tiles), 21 (the second tile
has 5 valid rows: one lane group holds 1 valid row of 4), 1, Kp0 = 64, 2A = 24,
a tanh / elu net (every stash stays on store_T), a net with dead hidden units
(tests/_dead_units.py: the ReLU masks zero whole k-rows) and one bf16 case
(bf16 keeps store_T).  Every case has hidden [256, 256] and a capacity of 1024.
"""
import contextlib
import json
import os
import sys

import pytest

import _dead_units as D
from test_gpu_parity import _check_config_against_oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_stash_store_parent_digests as G  # noqa: E402

pytestmark = pytest.mark.gpu

with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


def test_the_committed_digests_cover_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(G.CASES) and GOLDEN["steps"] == G.STEPS
    with open(G.OUT) as f:
        assert f.read() == G.render(GOLDEN)


@pytest.mark.parametrize("case", list(G.CASES))
def test_state_is_bit_identical_to_the_parent_build(case):
    """Two injected steps: every state array and the stats buffer hash to the
    parent build's digests."""
    got = G.digests(case)
    want = GOLDEN["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (case, differ)


@pytest.mark.parametrize("case", list(G.CASES))
def test_two_steps_match_the_oracle(case):
    """2 steps on the split layout against the CPU oracle (a dead-unit net: its dead rows stay zero)."""
    c, sp, precision = G.CASES[case]
    seen = []

    def on_step(k, hp, bt, pi_pre, post_loc, eng):
        if sp:
            D.assert_engine_rows_zero(eng, sp, (case, k))
        seen.append(k)

    with D.dead_nets(sp) if sp else contextlib.nullcontext():
        _check_config_against_oracle(dict(c, name="stashstore_" + case), precision, 2, expect="split", on_step=on_step)
    assert seen == [1, 2]
