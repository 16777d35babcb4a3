"""Gradient steps at network depths 1..5 and at unequal depths on every kernel
layout, against the CPU oracle.

sac_engine_create takes one to five hidden layers per network (SAC_DEV_LAYERS
= 6 Linear layers), the critics' depth independent of the policy's; every
other parity test trains two or three.  What depends on the depth:

* mlp_forward<HELD> (csrc/sac_phases.h) starts layers 0 and 1 on register-held
  fragments; with one hidden layer "layer 1" is the output layer (16 or 32
  padded columns, so held_issue returns early on most waves) and runs with the
  output activation and the output stride;
* mlp_backward<HELD> holds the l == Lh - 1 step, which at Lh = 1 never runs
  while phase C still issues the held load of pi.l[pi.L - 2], then layer 0;
  critic_unit_backward's loop l = Lh - 1 .. 1 is empty at one hidden layer;
* lds_layout (csrc/sac_plan.h) sizes the P1 buffers over max(Lhq, Lhp) with
  per-net guards and the P2 buffers over Lhq only: unequal depths are the only
  inputs that separate the two;
* every per-layer array has SAC_DEV_LAYERS slots, and only depth 5 reaches the
  last one;
* the pair tiles (csrc/sac_pairs.h) keep a ReLU bit mask per pi hidden layer
  and branch on l == q.L - 1 / l == pi.L - 1;
* the stage path (csrc/sac_wide.h) adds stages per layer and applies only
  where both nets have two hidden layers or more;
* the update tiles' tables grow with the depth.

The cases are tests/_depth.py::CASES: depth 1 and depth 5 on every family that
takes them, depth 4, and the critics and the policy at 1|3, 5|1, 2|5 and 5|2
layers, at widths that pad and differ between the nets; [256] (the hidden
split refused by depth) and [256] * 5 (the stage path by default); B = 1100
(69 row tiles, the last ragged, the update tiles in two batch parts) at depth
1 and 5.  Per case three tests, each asserting its kernel family
(tests/_gpu.py::assert_layout), with the checks and tolerances of the functions
they call, unchanged:

* fp32, default hyper-parameters: test_gpu_parity.py::
  _check_config_against_oracle, 3 steps (2 at B = 1100), traj_tol 2e-3;
* fp32, the rl+adam set of test_gpu_hyper.py (adam_eps 1e-3: a mis-scaled
  gradient of one layer shows in the post-step parameters) with that file's
  per-step conditions and Polyak check;
* bf16: test_gpu_parity.py::_bf16_one_step_from_the_engine_state with its
  bounds.

That a dropped or stale dW of any layer would show is asserted on the oracle
alone in tests/test_depth_cpu.py: on step 1 of every case at least half of
every weight matrix moves by more than the element bound.

Device RNG (indices=None, eps=None) at depth 1 and 5, three eager steps and
three replayed from one hipGraph, with the checks of test_gpu_action_width.py::
test_device_rng_steps_match_oracle_at_wide_actions.  Device draws cannot be
redrawn, so each case first asserts on the CPU that tests/_ties.py finds no
tie on the oracle's six steps at engine seed RNG_SEED."""
import numpy as np
import pytest
import torch

import _depth
from oracle import sac_oracle as O
from test_gpu_action_width import oracle_walk
from test_gpu_device_rng import _check_losses, _check_params, _rows
from test_gpu_hyper import _conditions
from test_gpu_parity import _bf16_one_step_from_the_engine_state, _check_config_against_oracle, _engine_mlp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = _depth.CASES


def _steps(shape):
    return 2 if shape["batch"] > 1024 else 3


@pytest.mark.parametrize("case", sorted(CASES))
def test_depths_match_oracle(case):
    shape, lay, family = CASES[case]
    _check_config_against_oracle(_depth.config(case, "default"), "fp32", _steps(shape), traj_tol=2e-3, layout=lay,
                                 expect=family)


@pytest.mark.parametrize("case", sorted(CASES))
def test_depths_both_hyper_sets_match_oracle(case):
    shape, lay, family = CASES[case]
    c = _depth.config(case, "rl+adam")
    _check_config_against_oracle(c, "fp32", _steps(shape), traj_tol=2e-3, layout=lay, expect=family,
                                 on_step=_conditions(f"{c['name']}/fp32", True))


# bf16 rounding compounds per layer: the five-layer nets at B = 1100 (f = 1: no small-batch allowance, while
# B = 40 has f = 2.53) exceed two of _bf16_one_step_from_the_engine_state's bounds by rounding alone.  The same
# steps on the CPU with bf16 products (tests/_bf16_emulation.py: every matmul's operands rounded to bf16, float64
# sums) against the fp32 oracle, from the fresh state on the same rows, next to the engine (pairs; the stage path
# agrees to three digits) and the bound that results, twice the emulation's missing share:
#   step 1, share within 0.01 lr (standing bound 0.985), pi q1 q2 q1t q2t:
#     emulation 0.9767 0.9834 0.9849 0.9837 0.9850 (just under); engine 0.9769 0.9837 0.9850 0.9840 0.9850
#     -> asked 0.9535 0.9668 0.9698 0.9674 0.9700
#   step 2, share within 0.05 lr (standing bound 0.92):
#     emulation 0.9247 0.8826 0.9032 0.8892 0.9100; engine 0.9240 0.8829 0.9037 0.8891 0.9097
#     -> asked 0.92 0.7652 0.8063 0.7784 0.8200
#   step 2, share within 0.25 lr (standing bound 0.985): emulation q1 0.9845 q1t 0.9847; engine q1 0.9846
#     -> asked 0.9689 0.9693
#   step 3 (stage path only; pairs meets 0.92): q1 within 0.05 lr, emulation 0.9187 -> asked 0.8374
# Steps 2 and 3 start from the engine's own state, so the test runs the emulation there itself, from that state,
# and takes each bound from it (emulated=True); the 2 lr cap, y, log pi, the medians and every bound the emulation
# meets stay as they are.  profiles/depth_gputest.txt has every figure ([bf16-emu] next to [bf16-local]).
BF16_EMULATED = {"h5_b1100_pairs", "h5_b1100_stage"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_depths_bf16_one_step_from_the_engine_state(case):
    shape, lay, family = CASES[case]
    _bf16_one_step_from_the_engine_state(case, dict(shape), lay, expect=family, emulated=case in BF16_EMULATED)


# ---------------------------------------------------------------- the device RNG at depth 1 and 5
RNG_SEED = 0
RNG_CASES = ("h1_roles", "h1_rows", "h1_pairs", "h5_roles", "h5_pairs", "h5_stage")


@pytest.mark.parametrize("case", RNG_CASES)
def test_device_rng_steps_match_oracle_at_depths(case):
    from _gpu import assert_layout, build_engine, oracle_hyper

    shape, lay, family = CASES[case]
    eng, rb, c = build_engine(dict(shape, done_p=0.01), "fp32", RNG_SEED, DEV, layout=lay)
    assert_layout(eng, family)
    assert int(eng.cfg.seed) == RNG_SEED and int(eng.rng_step.item()) == 0
    B, A = c["batch"], c["act"]
    hp = oracle_hyper(c)
    st = O.SacState.fresh(_engine_mlp(eng, "pi"), _engine_mlp(eng, "q1"), _engine_mlp(eng, "q2"), hp, A)
    walk = oracle_walk(st, hp, _rows(rb), len(rb), B, A, RNG_SEED, 0, 6)
    ties = [t for t, _, _ in walk]
    print(f"[ties] device_rng_{case}: seed {RNG_SEED}, steps 0..5, ties {ties}")
    assert not any(ties), (case, ties)
    for k in range(1, 4):
        _, ref, post = walk[k - 1]
        eng.train(rb, 1)  # device sampler + device eps
        torch.cuda.synchronize()
        _check_losses(eng.losses(), ref, post, (case, k))
        np.testing.assert_allclose(eng.last_targets().cpu().numpy(), ref["y"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(eng.last_log_pi().cpu().numpy(), ref["log_pi"], rtol=1e-4, atol=1e-4)
        _check_params(eng, post, hp, k, (case, k))
    assert int(eng.rng_step.item()) == 3
    eng.train_graph(rb, 3, chunk=3)
    torch.cuda.synchronize()
    eng.check()
    assert int(eng.rng_step.item()) == 6
    _check_losses(eng.losses(), walk[5][1], walk[5][2], (case, "graph"))
    _check_params(eng, walk[5][2], hp, 6, (case, "graph"))
