"""Generate tests/golden/stash_store_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on the hidden-split kernels, taken from a
build of the commit BEFORE the transposed stashes (X^T / dY^T) were stored from
the GEMM epilogues' registers (csrc/sac_split.h, store_acc_T).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_stash_store_parent_digests.py --parent <commit>

Needs the MI355X.  SAC_ENGINE_LIB must name a library built from the parent
commit (tools/build_rev.sh; the script refuses to run without it, so that the
file is never made from the tree's own build); --parent is recorded in the
file.  The change moves no float operation and every stash element receives
the value store_T gave it, so tests/test_gpu_stash_stores.py recomputes every
digest on the build under test and asks for equality.

Each case builds tests/_gpu.py::build_engine's engine and synthetic replay
(seed 3), draws indices and eps for two steps from numpy's default_rng(17), runs
them one by one and hashes the bytes of every array of state_tensors() and of
the stats buffer (losses, y, log pi).
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "soft-actor-critic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _dead_units as D  # noqa: E402

OUT = os.path.join(HERE, "stash_store_parent_digests.json")
STEPS = 2


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
    import numpy as np
    import torch
    from _gpu import assert_layout, build_engine

    c, sp, precision = CASES[name]
    with D.dead_nets(sp) if sp else contextlib.nullcontext():
        eng, rb, cc = build_engine(dict(c, name="stash_store_" + name), precision, 3, torch.device("cuda", 0))
    assert_layout(eng, "split")
    B, A = cc["batch"], cc["act"]
    g = np.random.default_rng(17)
    idx = g.integers(0, cc["capacity"], (STEPS, B)).astype(np.int32)
    eps = g.standard_normal((STEPS, 2, B, A)).astype(np.float32)
    for k in range(STEPS):
        eng.train(rb, 1, indices=torch.from_numpy(idx[k:k + 1]), eps=torch.from_numpy(eps[k:k + 1]))
    torch.cuda.synchronize()
    eng.check()
    if sp:
        D.assert_engine_rows_zero(eng, sp, name)
    arrays = dict(eng.state_tensors(), stats=eng.stats)
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            for k, v in sorted(arrays.items())}


def render(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit the library named by SAC_ENGINE_LIB was built from")
    args = ap.parse_args()
    if not os.environ.get("SAC_ENGINE_LIB"):
        sys.exit("SAC_ENGINE_LIB must name a library built from the parent commit")
    doc = {"parent": args.parent, "steps": STEPS, "cases": {name: digests(name) for name in CASES}}
    with open(OUT, "w") as f:
        f.write(render(doc))
    print(f"wrote {OUT}: {len(CASES)} cases, {sum(len(v) for v in doc['cases'].values())} digests")


if __name__ == "__main__":
    main()
