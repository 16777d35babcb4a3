"""Generate tests/golden/epilogue_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on the hidden-split kernels with dead
hidden units (tests/_dead_units.py), taken from a build of the commit BEFORE
the dX epilogues' ReLU masks were read ahead of their GEMM chains
(csrc/sac_split.h, gemm_hf's masked form).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_epilogue_parent_digests.py --parent <commit>

How the file is made and what a digest covers: tests/golden/_parent_digests.py
(the engine of a case is built with the case's dead units).  The change moves
no float operation, so tests/test_gpu_epilogue_masks.py recomputes every
digest on the build under test and asks for equality.
"""
from __future__ import annotations

import os

import _parent_digests as P
from _parent_digests import STEPS, render  # noqa: F401  (the test reads them from here)

import _dead_units as D  # noqa: E402  (tests/ is on the path once _parent_digests is imported)

OUT = os.path.join(P.HERE, "epilogue_parent_digests.json")

# name -> (tests/_dead_units.py case or None, config dict when there is no case, precision)
CASES = {
    "dead_units_fp32": ("dead_units", None, "fp32"),
    "dead_layer0_fp32": ("dead_layer0", None, "fp32"),
    "dead_layer1_fp32": ("dead_layer1", None, "fp32"),
    "dead_units_kp64_act8_fp32": ("dead_units_kp64_act8", None, "fp32"),
    "dead_units_act12_fp32": ("dead_units_act12", None, "fp32"),
    "dead_units_bf16": ("dead_units", None, "bf16"),
    # no mask is read: identity, and the activations act_pass_bwd applies
    "identity_fp32": (None, D._shape(24, 4, 20, q_act="identity", pi_act="identity"), "fp32"),
    "tanh_elu_fp32": (None, D._shape(24, 4, 20, q_act="tanh", pi_act="elu"), "fp32"),
}


def digests(name):
    """{array name: sha256 hex} of case `name` on the loaded engine library."""
    case, c, precision = CASES[name]
    sp = None
    if case is not None:
        c, sp = D.CASES[case]
    return P.state_digests(dict(c, name="epilogue_" + name), precision, "split",
                           nets=D.dead_nets(sp) if sp else None,
                           check=(lambda eng: D.assert_engine_rows_zero(eng, sp, name)) if sp else None)


if __name__ == "__main__":
    P.main(OUT, CASES, digests)
