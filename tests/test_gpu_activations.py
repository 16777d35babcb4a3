"""Non-ReLU hidden activations, output activations and a fixed alpha on every
kernel layout, against the CPU oracle.

Each kernel family has a branch of its own for a net that is not ReLU, apart
from the ReLU fast path the other parity tests run: the hidden-split kernels
stash pi's pre-activations instead of rebuilding ReLU masks (csrc/sac_split.h),
the pair and row tiles read that stash instead of mask words (csrc/sac_pairs.h,
csrc/sac_phases.h), the stage path transforms its A operand in LDS instead of
applying ReLU as the fragment is read (csrc/sac_wide.h, HR = false), and every
family branches on an output activation at the critics' seed, the min-Q
backward and the policy head.  The golden fixtures reach those activations on
the plain role kernels only (B <= 128, never [256, 256] x 2).

Shapes: the smallest at which each layout runs with a ragged last row tile
(B = 40: three row tiles of 16, so the last pair of the pair tiles holds one),
widths that pad (72 -> 96, 40 -> 64) and differ between the critics and the
policy.  Checks and tolerances are those of tests/test_gpu_parity.py, unchanged
(fp32: _check_config_against_oracle with tie-free draws, traj_tol 2e-3 as for
the edge shapes; bf16: the same function's bf16 bounds and the per-element
form of test_bf16_one_step_from_the_engine_state).  Every case asserts the
layout it ran (tests/_gpu.py::assert_layout)."""
import pytest

from test_gpu_parity import _bf16_one_step_from_the_engine_state, _check_config_against_oracle

pytestmark = pytest.mark.gpu

SMALL = dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=40, capacity=512)
# layout -> (shape, layout overrides); "split" is the planner's own choice at [256, 256] x 2
LAYOUTS = {
    "split": (dict(obs=24, act=4, hidden=[256, 256], batch=40, capacity=512), None),
    "roles": (SMALL, {"layout": "roles"}),
    "rows": (SMALL, {"layout": "rows"}),
    "pairs": (SMALL, {"layout": "pairs"}),
    "stage": (SMALL, {"stage_path": 1}),
}
# (q_act, pi_act).  The two pairings with one ReLU net: the pair tiles' choice
# between mask words and the stash keys on pi alone, the stage path's HR on both nets.
PAIRINGS = [("elu", "elu"), ("leaky_relu", "selu"), ("gelu", "tanh"), ("tanh", "gelu"), ("selu", "leaky_relu"),
            ("relu", "tanh"), ("elu", "relu"), ("identity", "identity")]
# derivative at most ~1.13: the bf16 bounds of test_gpu_parity.py were measured on ReLU and ELU nets
BF16_PAIRINGS = [("elu", "elu"), ("gelu", "tanh"), ("tanh", "gelu")]
# (q_out_act, pi_out_act): smooth (tanh keeps log sigma in [-1, 1]: with the clamp
# at +-0.5 both edges are active and the clamp's mask meets tanh's backward) and kinked
OUT_ACTS = {"smooth": dict(q_out_act="elu", pi_out_act="tanh", log_std_min=-0.5, log_std_max=0.5),
            "kink": dict(q_out_act="leaky_relu", pi_out_act="selu")}
# More shapes of the stage path: three hidden layers with ragged column blocks,
# and a hidden layer past 256 (288: a second column block of 32), both forced.
# The planner takes the stage path on its own only where the phase kernels' LDS
# layout does not fit a CU, and at 16 rows per role workgroup [288, 40] fits (it
# runs the role kernels: W288 below, the only shape here that does so with a
# hidden layer wider than 256); the smallest critics that do not fit are
# [384, 384]: w384, with no override.
W288 = dict(obs=5, act=3, q_hidden=[288, 40], pi_hidden=[40, 288], batch=40, capacity=512)
STAGE_SHAPES = {
    "deep": (dict(obs=5, act=3, q_hidden=[96, 160, 64], pi_hidden=[64, 96, 160], batch=72, capacity=512),
             {"stage_path": 1}),
    "w288": (W288, {"stage_path": 1}),
    "w384": (dict(obs=5, act=3, q_hidden=[384, 384], pi_hidden=[40, 72], batch=40, capacity=512), None),
}


def _ids(pairs):
    return [f"{q}-{p}" for q, p in pairs]


def _fp32(name, shape, lay, expect, **acts):
    _check_config_against_oracle(dict(shape, name=name, **acts), "fp32", 3, traj_tol=2e-3, layout=lay, expect=expect)


@pytest.mark.parametrize("acts", PAIRINGS, ids=_ids(PAIRINGS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_hidden_activations_match_oracle(layout, acts):
    shape, lay = LAYOUTS[layout]
    _fp32(f"{layout}_{acts[0]}_{acts[1]}", shape, lay, layout, q_act=acts[0], pi_act=acts[1])


@pytest.mark.parametrize("acts", [("elu", "elu"), ("gelu", "tanh")], ids=_ids([("elu", "elu"), ("gelu", "tanh")]))
@pytest.mark.parametrize("shape", sorted(STAGE_SHAPES))
def test_stage_path_shapes_hidden_activations_match_oracle(shape, acts):
    c, lay = STAGE_SHAPES[shape]
    _fp32(f"stage_{shape}_{acts[0]}_{acts[1]}", c, lay, "stage", q_act=acts[0], pi_act=acts[1])


@pytest.mark.parametrize("acts", [("elu", "elu"), ("gelu", "tanh")], ids=_ids([("elu", "elu"), ("gelu", "tanh")]))
def test_width_288_without_override_runs_the_role_kernels(acts):
    """q [288, 40], pi [40, 288] at B = 40 with no layout override: the
    planner keeps the role kernels (their LDS layout fits), with a hidden layer
    wider than 256 and a non-ReLU net."""
    _fp32(f"roles_w288_{acts[0]}_{acts[1]}", W288, None, "roles", q_act=acts[0], pi_act=acts[1])


OUT_HIDDEN = {"split": [("relu", "relu"), ("elu", "elu")], "roles256": [("relu", "relu"), ("elu", "elu")],
              "rows": [("relu", "relu"), ("tanh", "gelu")], "pairs": [("relu", "relu"), ("tanh", "gelu")],
              "stage": [("relu", "relu"), ("tanh", "gelu")]}
OUT_CASES = [(lay, out, acts) for lay in sorted(OUT_HIDDEN) for out in sorted(OUT_ACTS) for acts in OUT_HIDDEN[lay]]


@pytest.mark.parametrize("layout,out,acts", OUT_CASES, ids=[f"{lay}-{o}-{a[0]}-{a[1]}" for lay, o, a in OUT_CASES])
def test_output_activations_match_oracle(layout, out, acts):
    """Output activations on the critics and the policy.  split: on the
    critics only (a policy output activation turns the hidden split off);
    roles256: the same [256, 256] nets with the policy's too, which must run
    the role kernels without the split."""
    o = dict(OUT_ACTS[out])
    if layout == "split":
        o["pi_out_act"] = "identity"
    shape, lay = LAYOUTS["split" if layout == "roles256" else layout]
    _fp32(f"{layout}_out_{out}_{acts[0]}_{acts[1]}", shape, lay, "roles" if layout == "roles256" else layout,
          q_act=acts[0], pi_act=acts[1], **o)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fixed_alpha_matches_oracle(layout):
    """auto_entropy_tuning off: L_alpha is NaN on both sides and [log alpha,
    alpha] stay as created (_check_config_against_oracle asserts both)."""
    shape, lay = LAYOUTS[layout]
    _fp32(f"{layout}_fixed_alpha", shape, lay, layout, q_act="elu", pi_act="elu", auto=False)


@pytest.mark.parametrize("acts", BF16_PAIRINGS, ids=_ids(BF16_PAIRINGS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bf16_hidden_activations_match_oracle(layout, acts):
    """bf16 products with _check_config_against_oracle's bf16 tolerances
    (test_engine_matches_oracle applies the same numbers to the non-ReLU
    fixtures on the role kernels)."""
    shape, lay = LAYOUTS[layout]
    c = dict(shape, name=f"{layout}_{acts[0]}_{acts[1]}", q_act=acts[0], pi_act=acts[1])
    _check_config_against_oracle(c, "bf16", 3, traj_tol=2e-3, layout=lay, expect=layout)


@pytest.mark.parametrize("acts", BF16_PAIRINGS, ids=_ids(BF16_PAIRINGS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bf16_one_step_hidden_activations(layout, acts):
    """The per-element bf16 bounds of test_bf16_one_step_from_the_engine_state
    (f = sqrt(256 / 40) at these batches) on non-ReLU nets; roles and pairs at
    the padded widths 96 / 64 are also the regression of the row-tile kernels'
    bf16 fault at hidden widths other than 256."""
    shape, lay = LAYOUTS[layout]
    _bf16_one_step_from_the_engine_state(f"{layout}_{acts[0]}_{acts[1]}", dict(shape, q_act=acts[0], pi_act=acts[1]),
                                         lay, expect=layout)
