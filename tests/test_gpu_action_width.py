"""Gradient steps at action widths 7..32 on every kernel layout, against the
CPU oracle.

sac_engine_create takes 1 <= act_dim <= 32; every other parity test trains at
act <= 6.  The squashed-Gaussian head, its backward pass and the hand-offs of
the action gradient exist once per kernel family (csrc/sac_split.h,
sac_pairs.h, sac_phases.h, sac_wide.h), and their action-width arithmetic
starts above 6:

* AP = next_pow2(A) lanes per row with an AP-lane shuffle sum of log pi: dead
  lanes at A = 9 and 17; at A = 32 a row fills half a wave and 32 rows of a
  pair tile take two passes of the 512 threads;
* the 2A output columns against the 32-column pad, NOp = 32 ceil(2A / 32),
  the pad zeroed before pi's backward: 16 of 32 (A = 8), 18 of 32 (9), exactly
  32 (16), 34 of 64 (17), exactly 64 (32);
* buffers sized by A: head_st [Br][4A], the granules' stride 16 (A + 1), the
  split's 16 max(2A, A + 1), the 576-float hand-off payload (528 used at
  A = 32), the critics' layer-0 Kp = pad32(obs + act);
* the planner's two action bounds: 2A <= 32 for the hidden split (split_a16 on
  the bound, roles256_a17 past it) and 2A <= 16 for the stage path (stage_a8 on
  the bound; past it stage_path = 1 is ignored, tests/test_plan_cpu.py).

Per case three tests, each asserting its kernel family (tests/_gpu.py::
assert_layout), with the checks and tolerances of the functions they call,
unchanged:

* fp32, default hyper-parameters: test_gpu_parity.py::
  _check_config_against_oracle, 3 steps, traj_tol 2e-3 as for every B = 40
  shape;
* fp32, the rl+adam set of test_gpu_hyper.py (adam_eps 1e-3, so a mis-scaled
  gradient of one action column shows in the post-step parameters; the narrow
  clamp, action_scale 2.5, 30 % terminals) with that file's per-step
  conditions and Polyak check;
* bf16: test_gpu_parity.py::_bf16_one_step_from_the_engine_state with its
  bounds.

Device RNG (indices=None, eps=None) on every family at a wide action: the
in-step samplers of the role, row-tile and pair-tile kernels and the stage
path's eps selection against oracle/sampler_oracle.py, three eager steps and
three replayed from one hipGraph, with the checks of
test_gpu_device_rng.py::test_device_rng_steps_match_oracle.  Device draws
cannot be redrawn, so each case first asserts (on the CPU, from the engine's
initial state) that tests/_ties.py finds no tie on the oracle's six steps:
engine seed 0, rng_step 0 and the replay rows of seed 0 are tie-free at all
five shapes.

Measured on an MI355X (profiles/action_width_gputest.txt): every case inside
the unchanged bounds, so no bf16 bound is set here; at most 1 row redrawn per
step; 7..15 terminal rows of 40."""
import numpy as np
import pytest
import torch

import _ties
from oracle import sac_oracle as O
from oracle import sampler_oracle as S
from test_gpu_device_rng import _batch, _check_losses, _check_params, _rows
from test_gpu_hyper import _conditions, hyper
from test_gpu_parity import _bf16_one_step_from_the_engine_state, _check_config_against_oracle, _engine_mlp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PADH = dict(q_hidden=[72, 40], pi_hidden=[40, 72])  # widths that pad (72 -> 96, 40 -> 64) and differ between the nets


def _pad(act):
    return dict(obs=5, act=act, batch=40, capacity=512, **PADH)


def _w256(act, batch):
    return dict(obs=24, act=act, hidden=[256, 256], batch=batch, capacity=512)


# name -> (shape, layout override, the kernel family phases A and C must run)
CASES = {
    "split_a8": (_w256(8, 40), None, "split"),
    "split_a16": (_w256(16, 64), None, "split"),  # 2A = 32: the hidden split's bound
    "roles256_a17": (_w256(17, 64), None, "roles"),  # the split refused by the action width
    "roles_a17": (_pad(17), {"layout": "roles"}, "roles"),
    "rows_a17": (_pad(17), {"layout": "rows"}, "rows"),
    "pairs_a17": (_pad(17), {"layout": "pairs"}, "pairs"),
    "roles_a32": (_pad(32), {"layout": "roles"}, "roles"),  # the API's maximum
    "rows_a32": (_pad(32), {"layout": "rows"}, "rows"),
    "pairs_a32": (_pad(32), {"layout": "pairs"}, "pairs"),
    "rows_a9": (_pad(9), {"layout": "rows"}, "rows"),
    "pairs_a9": (_pad(9), {"layout": "pairs"}, "pairs"),
    "stage_a8": (_pad(8), {"stage_path": 1}, "stage"),  # 2A = 16: the stage path's bound
    "stage_deep_a8": (dict(obs=5, act=8, q_hidden=[96, 160, 64], pi_hidden=[64, 96, 160], batch=72, capacity=512),
                      {"stage_path": 1}, "stage"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_actions_match_oracle(case):
    shape, lay, family = CASES[case]
    _check_config_against_oracle(dict(shape, name=case), "fp32", 3, traj_tol=2e-3, layout=lay, expect=family)


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_actions_both_hyper_sets_match_oracle(case):
    shape, lay, family = CASES[case]
    name = f"{case}_rl+adam"
    c = dict(shape, name=name, **hyper("rl+adam", shape["act"]))
    _check_config_against_oracle(c, "fp32", 3, traj_tol=2e-3, layout=lay, expect=family,
                                 on_step=_conditions(f"{name}/fp32", True))


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_actions_bf16_one_step_from_the_engine_state(case):
    shape, lay, family = CASES[case]
    _bf16_one_step_from_the_engine_state(case, dict(shape), lay, expect=family)


# ---------------------------------------------------------------- the device RNG on every family
RNG_SEED = 0
RNG_CASES = {
    "roles": (_pad(17), {"layout": "roles"}, "roles"),
    "rows": (_pad(17), {"layout": "rows"}, "rows"),
    "pairs": (_pad(17), {"layout": "pairs"}, "pairs"),
    "stage": (_pad(7), {"stage_path": 1}, "stage"),  # an odd act: the last Box-Muller pair half used
    "roles256_a17": (_w256(17, 64), None, "roles"),
}


def oracle_walk(st, hp, rows, n_rows, B, A, seed, t0, steps):
    """`steps` oracle steps from `st` (not mutated) on the device RNG's draws
    for (seed, t0 ..): per step (rows tied per pass, tests/_ties.py::step_ties;
    the step's result; the post-step state).  No GPU needed."""
    out = []
    for t in range(t0, t0 + steps):
        idx = np.asarray(S.sample_indices(n_rows, B, seed, t), np.int64)
        e = S.eps_draws(seed, t, B, A)
        ties, ref, st = _ties.step_ties(st, hp, _batch(rows, idx), e[0], e[1])
        out.append(({k: int(v.sum()) for k, v in ties.items()}, ref, st))
    return out


@pytest.mark.parametrize("case", sorted(RNG_CASES))
def test_device_rng_steps_match_oracle_at_wide_actions(case):
    from _gpu import assert_layout, build_engine, oracle_hyper

    shape, lay, family = RNG_CASES[case]
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

