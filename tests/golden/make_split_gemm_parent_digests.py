"""Generate tests/golden/split_gemm_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on the hidden-split kernels, taken from a
build of the commit BEFORE the split kernels' fixed-shape GEMM steps
(csrc/sac_split.h, gemm_hf).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_split_gemm_parent_digests.py --parent <commit>

How the file is made and what a digest covers: tests/golden/_parent_digests.py.
The change moves no float operation, so tests/test_gpu_split_gemm_shapes.py
recomputes every digest on the build under test and asks for equality.
"""
from __future__ import annotations

import os

import _parent_digests as P
from _parent_digests import STEPS, render  # noqa: F401  (the test reads them from here)

OUT = os.path.join(P.HERE, "split_gemm_parent_digests.json")


def _shape(obs, act, batch):
    return dict(obs=obs, act=act, hidden=[256, 256], batch=batch, capacity=1024)


# name -> (config dict, precision); Kp0 = obs + act padded to 32
CASES = {
    "kp32_b32_fp32": (_shape(24, 4, 32), "fp32"),   # layer 0 held in 2 fp32 chunks, two full row tiles
    "kp64_b32_fp32": (_shape(40, 8, 32), "fp32"),   # 4 held chunks; 2A = 16: one full chunk of dOut
    "kp32_b20_fp32": (_shape(24, 4, 20), "fp32"),   # a partial row tile (4 valid rows)
    "kp32_b32_bf16": (_shape(24, 4, 32), "bf16"),
}


def digests(name):
    """{array name: sha256 hex} of case `name` on the loaded engine library."""
    c, precision = CASES[name]
    return P.state_digests(dict(c, name="split_gemm_" + name), precision, "split")


if __name__ == "__main__":
    P.main(OUT, CASES, digests)
