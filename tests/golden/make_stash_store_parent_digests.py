"""Generate tests/golden/stash_store_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on the hidden-split kernels, taken from a
build of the commit BEFORE the transposed stashes (X^T / dY^T) were stored from
the GEMM epilogues' registers (csrc/sac_split.h, store_acc_T).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_stash_store_parent_digests.py --parent <commit>

How the file is made and what a digest covers: tests/golden/_parent_digests.py.
The change moves no float operation and every stash element receives the value
store_T gave it, so tests/test_gpu_stash_stores.py recomputes every digest on
the build under test and asks for equality.
"""
from __future__ import annotations

import os

import _parent_digests as P
from _parent_digests import STEPS, render  # noqa: F401  (the test reads them from here)

import _dead_units as D  # noqa: E402  (tests/ is on the path once _parent_digests is imported)

OUT = os.path.join(P.HERE, "stash_store_parent_digests.json")


def _shape(obs, act, batch, **extra):
    return dict(obs=obs, act=act, hidden=[256, 256], batch=batch, capacity=1024, **extra)


# name -> (config dict, tests/_dead_units.py spec or None, precision).  A row tile is 16 batch rows and a
# lane of an epilogue holds 4 of them.
CASES = {
    "kp32_b32_fp32": (_shape(24, 4, 32), None, "fp32"),   # two full row tiles
    "kp32_b21_fp32": (_shape(24, 4, 21), None, "fp32"),   # second tile: 5 valid rows, a lane with 1 valid row of 4
    "kp32_b1_fp32": (_shape(24, 4, 1), None, "fp32"),     # one valid row
    "kp64_b32_fp32": (_shape(40, 8, 32), None, "fp32"),   # Kp0 = 64
    "act12_b21_fp32": (_shape(11, 12, 21), None, "fp32"),  # 2A = 24: two fp32 chunks of dOut
    # neither ReLU nor identity: every stash stays on the LDS + store_T path
    "tanh_elu_b32_fp32": (_shape(24, 4, 32, q_act="tanh", pi_act="elu"), None, "fp32"),
    # ReLU masks zero whole k-rows of the stashes
    "dead_units_b32_fp32": (_shape(24, 4, 32), D.spec(D.DEAD, D.DEAD), "fp32"),
    "kp32_b32_bf16": (_shape(24, 4, 32), None, "bf16"),   # bf16 keeps store_T
}


def digests(name):
    """{array name: sha256 hex} of case `name` on the loaded engine library."""
    c, sp, precision = CASES[name]
    return P.state_digests(dict(c, name="stash_store_" + name), precision, "split",
                           nets=D.dead_nets(sp) if sp else None,
                           check=(lambda eng: D.assert_engine_rows_zero(eng, sp, name)) if sp else None)


if __name__ == "__main__":
    P.main(OUT, CASES, digests)
