"""The fixed-shape GEMM steps of the hidden-split kernels (csrc/sac_split.h,
gemm_hf): layer 0 with every chunk held (Kp0 = 32 and 64, two instantiations),
layer 1 forward, both layer-1 dX steps and pi's layer-2 dX run with compile-time
chunk counts and the tile ownership tested once per chain, and the k-split
steps (gemm_ksplit_epi) with a compile-time tile count.  Each accumulator takes
the same products in the same order as before, and the k-split partials are
summed in the same slice order, so

  * every case is held to the CPU oracle by
    tests/test_gpu_parity.py::_check_config_against_oracle as it stands (fp32:
    elements within 1e-6; bf16: its bounds in units of the learning rate), two
    steps with injected indices and eps, and asserts the split layout;
  * three fp32 shapes and one bf16 shape are bit-identical to the parent
    commit's build: tests/golden/split_gemm_parent_digests.json holds the
    SHA-256 of every array of state_tensors() and of the stats buffer after
    two steps, made from that build by
    tests/golden/make_split_gemm_parent_digests.py; the digests are recomputed
    here.

Every case has hidden [256, 256] (what selects the split kernels) and a
capacity of 1024; Kp0 is obs + act padded to 32."""
import json
import os
import sys

import pytest

from test_gpu_parity import _check_config_against_oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_split_gemm_parent_digests as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _shape(obs, act, batch, **extra):
    return dict(obs=obs, act=act, hidden=[256, 256], batch=batch, capacity=1024, **extra)


SHAPES = {
    # Kp0 = 32: layer 0 in 2 held fp32 chunks (1 bf16); two full row tiles
    "kp32_b32": _shape(24, 4, 32),
    # a partial row tile: nvalid = 4 < 16 in the second one
    "kp32_b20": _shape(24, 4, 20),
    # Kp0 = 64: 4 held fp32 chunks (2 bf16), the other instantiation; act 8: 2A = 16, pi's layer-2 dX
    # over exactly one full fp32 chunk of dOut
    "kp64_act8": _shape(40, 8, 32),
    # Kp0 = 64 with a partial tile
    "kp64_b20": _shape(56, 8, 20),
    # Kp0 = 96 > 64: layer 0's held chunks, then the streamed remainder (the general path)
    "kp96_stream": _shape(80, 4, 32),
    # act 1: 2A = 2, one chunk of dOut that is almost all padding
    "act1": _shape(3, 1, 32),
    # 2A = 24: two fp32 chunks of dOut hold data (the two-chunk instantiation of pi's layer-2 dX)
    "act12_two_chunks": _shape(11, 12, 20),
    # other hidden activations: P1 kept and U1 from the loop, layer 2 k-split in phase C, the activation passes
    "tanh_elu": _shape(24, 4, 32, q_act="tanh", pi_act="elu"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_fixed_shape_steps_match_oracle(shape):
    """fp32, 2 steps on the split layout."""
    _check_config_against_oracle(dict(SHAPES[shape], name="splitgemm_" + shape), "fp32", 2, expect="split")


@pytest.mark.parametrize("shape", ["kp32_b32", "kp32_b20", "kp64_act8"])
def test_bf16_fixed_shape_steps_match_oracle(shape):
    """bf16, 2 steps on the split layout, with the bf16 mode's own bounds."""
    _check_config_against_oracle(dict(SHAPES[shape], name="splitgemm_bf16_" + shape), "bf16", 2, expect="split")


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
