"""The single-round path of the update tiles (csrc/sac_phases.h, dw_adam_tile),
against the CPU oracle.

A 1024-thread update tile whose whole batch fits the slots of one round
(bp <= slots x 128 columns in fp32, slots x 256 in bf16) stages every slot
behind one barrier, reads all MFMA fragments of its (sub-tile, K-quarter) pair
up front, writes the K-quarter partials to an LDS area of their own and keeps
the summed dW of an element in the register of the thread that runs its Adam
step: 3 block barriers per tile where the multi-round path takes 7.  No float
operation moves, so the checks and tolerances are those of
tests/test_gpu_parity.py::_check_config_against_oracle and
::_bf16_one_step_from_the_engine_state as they stand.  traj_tol (y and log pi
against the oracle's own trajectory from step 2 on) is the existing files'
value where they run the batch size: 2e-3 at 16, 40 and 64, 1e-4 at 256.  The
batch sizes no earlier test runs (48, 144, 272) take twice the deviation of the
parent build on the same case, the larger of the two hyper-parameter sets
(profiles/update_single_round_gputest.txt: 7.5e-7, 1.62e-6 and 1.17e-6, all
fp32 rounding, no Adam sign flip); the margin is for the fp32 summation order,
which this path does not alter.

fp32 runs 3 steps with the default hyper-parameters and 3 steps with
test_gpu_hyper.hyper("rl+adam", act) and that file's per-step conditions: with
adam_eps 1e-3 a wrong dW magnitude shows in the parameters.  bf16 runs one
engine-state comparison (3 single steps, each from the engine's own state).
Every case asserts its kernel layout.

Shapes (obs 24, act 4, hidden [256, 256], capacity 1024 unless stated; Bp is
the batch padded to whole 32-column K-steps):

  b16   Bp 32   one partial slot of two chunks: K-quarters 2 and 3 own no
                chunk; summed dY parts (gsum) but no batch parts
  b40   Bp 64   the smallest batch with layer-0 batch-part halves (kpart), 32
                columns each; ragged last row tile
  b144  Bp 160  slot 0 full, slot 1 partial; unequal halves (96 and 64 columns)
  b256  Bp 256  both slots full: the compile-time trip counts; halves of one slot
  b272  Bp 288  fp32: the first size whose full-batch tiles stay on the
                multi-round path (its halves still take the new one); bf16:
                still single-round (two slots of 256)
  b528  Bp 544  bf16 only: past two bf16 slots, on the layout the planner picks
  small48       obs 5, act 3, q [72, 40], pi [40, 72], batch 48: masked N and K
                edges of the tiles, no summed parts
  c1            obs 4, act 1, [64, 64], batch 64 (bench.py's c1)"""
import pytest

from test_gpu_hyper import _conditions, hyper
from test_gpu_parity import _bf16_one_step_from_the_engine_state, _check_config_against_oracle

pytestmark = pytest.mark.gpu


def _split(batch):
    return dict(obs=24, act=4, hidden=[256, 256], batch=batch, capacity=1024)


# name -> (config dict, the layout it must run, traj_tol)
SHAPES = {
    "b16": (_split(16), "split", 2e-3),
    "b40": (_split(40), "split", 2e-3),
    "b144": (_split(144), "split", 2 * 1.62e-6),
    "b256": (_split(256), "split", 1e-4),
    "b272": (_split(272), "split", 2 * 1.17e-6),
    "small48": (dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=48, capacity=1024), "roles",
                2 * 7.5e-7),
    "c1": (dict(obs=4, act=1, hidden=[64, 64], batch=64, capacity=1024), "roles", 2e-3),
}
BF16_SHAPES = dict(SHAPES, b528=(_split(528), "roles", None))
# rl+adam: the replay seeds at which test_gpu_hyper._conditions holds on every step (16 rows with >= 4 terminal
# and >= 4 other rows; act 1: 64 log sigma entries with >= 5 % on each side of the narrow clamp)
HYPER_REPLAY_SEED = {"b16": 2, "c1": 6}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_default_hyper_matches_oracle(shape):
    c, layout, tol = SHAPES[shape]
    _check_config_against_oracle(dict(c, name="upd1r_" + shape), "fp32", 3, traj_tol=tol, expect=layout)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_rl_adam_hyper_matches_oracle(shape):
    c, layout, tol = SHAPES[shape]
    name = "upd1r_hyper_" + shape
    if shape in HYPER_REPLAY_SEED:
        c = dict(c, replay_seed=HYPER_REPLAY_SEED[shape])
    _check_config_against_oracle(dict(c, name=name, **hyper("rl+adam", c["act"])), "fp32", 3, traj_tol=tol,
                                 expect=layout, on_step=_conditions(name + "/fp32", True))


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_bf16_one_step_from_the_engine_state(shape):
    c, layout, _ = BF16_SHAPES[shape]
    _bf16_one_step_from_the_engine_state("upd1r_" + shape, c, expect=layout)
