"""The narrow steps of the hidden-split kernels' fp32 critic chains, against the
CPU oracle.

In fp32 phase C's critic roles (csrc/sac_split.h) form layer 2 (N = 1) in the
epilogue of layer 1 instead of as a k-split MFMA step: lanes are summed in a
fixed order, then waves in wave order; a non-ReLU / non-identity hidden
activation keeps the k-split path.  The same roles load s and a~ straight into
the layer-0 input (one thread per element when 16 Kp0 <= 512), and pi computes
the da-independent terms of its head backward before it polls the critics.
The shapes also cover what a fused dX0 of the action columns would have to get
right (measured slower and not kept: profiles/ab_narrow_items.txt): action
columns across a 16-column boundary, A = 1, A > 8, R A > 64.

Shapes: every case has hidden [256, 256] (what selects the split kernels) and a
capacity of 1024; the table below says what each one is for.  Checks and
tolerances are tests/test_gpu_parity.py::_check_config_against_oracle's own,
as it stands (tie-free draws; the local oracle loaded with the engine's full
state: >= 99.9% of post-step elements within 1e-6, losses to 1e-5 relative,
log alpha to 1e-7).  Every case asserts that it ran the split layout."""
import pytest

from test_gpu_parity import _check_config_against_oracle

pytestmark = pytest.mark.gpu


def _shape(obs, act, batch, **extra):
    return dict(obs=obs, act=act, hidden=[256, 256], batch=batch, capacity=1024, **extra)


SHAPES = {
    # one full row tile
    "b16": _shape(24, 4, 16),
    # ragged last tile (8 valid rows): padded rows must add nothing to the lane and wave sums
    "b40_ragged": _shape(24, 4, 40),
    # action columns 30..33 straddle the 16-column boundary of the padded layer-0 input
    "obs30_straddle": _shape(30, 4, 32),
    # A = 1: the action column sits inside the first tile, next to s
    "act1": _shape(3, 1, 32),
    # R A > 64: pi's two-poll branch behind the early head-backward terms
    "act6_two_polls": _shape(17, 6, 32),
    # A > 8: two 16-column tiles of W0^T for the action columns' dX0, with the fused layer 2 on
    "act12_dx0_fallback": _shape(11, 12, 32),
    # non-ReLU hidden activations: layer 2 on the k-split path
    "tanh_elu_fallbacks": _shape(24, 4, 32, q_act="tanh", pi_act="elu"),
    # critic output activation on the fused partial q
    "q_out_tanh": _shape(24, 4, 32, q_out_act="tanh"),
}
# the last shape of each kind (ReLU fused path / wide action space / activation fallback / output activation)
BF16_SHAPES = ["act6_two_polls", "act12_dx0_fallback", "tanh_elu_fallbacks", "q_out_tanh"]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_narrow_steps_match_oracle(shape):
    """fp32, 3 steps: the fused layer 2 (or its fallback) on the split layout."""
    _check_config_against_oracle(dict(SHAPES[shape], name="narrow_" + shape), "fp32", 3, expect="split")


@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_bf16_keeps_its_path_and_bounds(shape):
    """bf16, 2 steps: the bf16 instantiation keeps the k-split steps and passes its own bounds."""
    _check_config_against_oracle(dict(SHAPES[shape], name="narrow_bf16_" + shape), "bf16", 2, expect="split")
