"""Generate tests/golden/epilogue_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on the hidden-split kernels with dead
hidden units (tests/_dead_units.py), taken from a build of the commit BEFORE
the dX epilogues' ReLU masks were read ahead of their GEMM chains
(csrc/sac_split.h, gemm_hf's masked form).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_epilogue_parent_digests.py --parent <commit>

Needs the MI355X.  SAC_ENGINE_LIB must name a library built from the parent
commit (the script refuses to run without it, so that the file is never made
from the tree's own build); --parent is recorded in the file.  The change moves
no float operation, so tests/test_gpu_epilogue_masks.py recomputes every
digest on the build under test and asks for equality.

Each case builds tests/_gpu.py::build_engine's engine (with the case's dead
units) and synthetic replay (seed 3), draws indices and eps for two steps from
numpy's default_rng(17), runs them one by one and hashes the bytes of every
array of state_tensors() and of the stats buffer (losses, y, log pi).
"""
from __future__ import annotations

import argparse
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

OUT = os.path.join(HERE, "epilogue_parent_digests.json")
STEPS = 2

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
    import contextlib

    import numpy as np
    import torch
    from _gpu import assert_layout, build_engine

    case, c, precision = CASES[name]
    sp = None
    if case is not None:
        c, sp = D.CASES[case]
    with D.dead_nets(sp) if sp else contextlib.nullcontext():
        eng, rb, cc = build_engine(dict(c, name="epilogue_" + name), precision, 3, torch.device("cuda", 0))
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
