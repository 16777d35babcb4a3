"""The barriers and LDS passes taken off the hidden-split kernels' chains
(csrc/sac_split.h), against the CPU oracle and against the in-step gather.

Phase A writes the staged record from registers straight into the layer-0 input
(every role; pad columns zeroed by the same threads), publishes pi(s')'s layer-2
partial and the partial q of the target critics and critics from the threads
that sum the k-split partials, and writes the critics' unit seed U1 in layer 1's
epilogue (ReLU / identity).  Phase C writes U1 the same way, publishes the
action columns' dX0 from its reducers, keeps d(-min Q)/d a~ in the lane that
runs the head backward (R A <= 64) and multiplies only the chunks of dOut that
hold pi's 2A output columns.  None of it moves a float operation.

Shapes: every case has hidden [256, 256] (what selects the split kernels) and a
capacity of 1024; the table says what each one is for.  Checks and tolerances
are tests/test_gpu_parity.py::_check_config_against_oracle's own, as it stands.
Every case asserts that it ran the split layout.  That helper injects indices,
so phase A gathers there; the record -> X path has its own test below."""
import ctypes

import pytest
import torch

from test_gpu_parity import _check_config_against_oracle

pytestmark = pytest.mark.gpu


def _shape(obs, act, batch, **extra):
    return dict(obs=obs, act=act, hidden=[256, 256], batch=batch, capacity=1024, **extra)


SHAPES = {
    # one full row tile
    "b16": _shape(24, 4, 16),
    # ragged last tile (8 valid rows)
    "b40_ragged": _shape(24, 4, 40),
    # action columns 30..33 straddle a 16-column tile of the layer-0 input: dX0 over two tiles, pad zeroing
    "obs30_straddle": _shape(30, 4, 32),
    # A = 1, Kp0 - O large: almost every column of X is padding
    "obs3_act1": _shape(3, 1, 32),
    # R A > 64: pi's two-poll branch, which still goes through LDS
    "act6_two_polls": _shape(17, 6, 32),
    # 2A = 24: two output tiles publish from the k-split reducers; two chunks of dOut hold data
    "act12_two_tiles": _shape(11, 12, 32),
    # O == 32: the widest observation whose record goes straight into X
    "obs32": _shape(32, 2, 32),
    # O > 32: the record goes through LDS as before
    "obs40_fallback": _shape(40, 4, 32),
    # identity hidden activation on both nets: U1 is W2's row itself
    "identity_hidden": _shape(24, 4, 32, q_act="identity", pi_act="identity"),
    # other hidden activations: U1 from the loop over the stored pre-activations
    "tanh_elu_fallbacks": _shape(24, 4, 32, q_act="tanh", pi_act="elu"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_chain_trims_match_oracle(shape):
    """fp32, 3 steps on the split layout."""
    _check_config_against_oracle(dict(SHAPES[shape], name="trims_" + shape), "fp32", 3, expect="split")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bf16_chain_trims_match_oracle(shape):
    """bf16, 2 steps on the split layout, with the bf16 mode's own bounds."""
    _check_config_against_oracle(dict(SHAPES[shape], name="trims_bf16_" + shape), "bf16", 2, expect="split")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_record_to_x_equals_gather(precision):
    """B = 40, obs 24 / act 4, two engines from one seed, 4 device-sampled steps
    each.  The first trains them in one call, so phase A takes every staged
    record (registers -> X).  The second has a replay push between the steps:
    each record is stale when phase A reads it, so phase A gathers and builds X
    from LDS.  The push rewrites the full ring with its own rows (_touch), so
    both engines sample the same rows.  All state tensors are equal, and the
    first engine did use a staged record."""
    from _gpu import assert_layout, build_engine
    from sac import _engine as E

    c = _shape(24, 4, 40)
    out = {}
    for mode in ("staged", "gathered"):
        eng, rb, cc = build_engine(dict(c, name="trims_record_" + mode), precision, 3, torch.device("cuda", 0))
        assert_layout(eng, "split")
        if mode == "staged":
            eng.train(rb, 4)
            lib = eng.lib
            lib.sac_engine_debug_staged_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            got = ctypes.c_uint64(0)
            E.check(lib.sac_engine_debug_staged_step(eng.handle, ctypes.byref(got), eng._stream()))
            assert got.value > 0, "phase A never used a staged record"
        else:
            for _ in range(4):
                eng.train(rb, 1)
                _touch(rb)
        eng.check()
        out[mode] = {k: v.clone() for k, v in eng.state_tensors().items()}
        out[mode]["stats"] = eng.stats.clone()
    for k in out["staged"]:
        assert torch.equal(out["staged"][k], out["gathered"][k]), k


def _touch(rb):
    """A push that makes the staged record stale and changes nothing a step
    samples: the full ring's own rows, oldest first, so size, cursor and every
    slot's contents come back as they were and only the push generation moves."""
    assert len(rb) == rb.capacity
    pos = int(rb.state[1].item())
    cols = [torch.roll(getattr(rb, k).clone(), -pos, 0) for k in ("obs", "act", "rew", "next_obs", "done")]
    rb.push_batch(*cols)
    assert int(rb.state[1].item()) == pos and len(rb) == rb.capacity
