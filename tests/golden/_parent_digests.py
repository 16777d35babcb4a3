"""What the make_*_parent_digests.py scripts of this directory share: SHA-256
digests of the engine state after STEPS injected steps, written to a JSON file
from a build of a change's PARENT commit and recomputed by the change's GPU
test on the build under test, which asks for equality (the change moves no
float operation).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_<name>_parent_digests.py --parent <commit>

Needs the MI355X.  SAC_ENGINE_LIB must name a library built from the parent
commit (tools/build_rev.sh; main refuses to run without it, so that a file is
never made from the tree's own build); --parent is recorded in the file.

A case builds tests/_gpu.py::build_engine's engine and synthetic replay (seed
3), draws indices and eps for STEPS steps from numpy's default_rng(17), runs
them one by one and hashes the bytes of every array of state_tensors() and of
the stats buffer (losses, y, log pi).  A script is its case table, a digests(name)
that hands one case to state_digests, and whatever else it truly adds.
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

STEPS = 2


def state_digests(c, precision, layout, nets=None, check=None):
    """{array name: sha256 hex} of config dict c (with its engine name) on the
    loaded engine library, which must plan it on `layout` (_gpu.assert_layout).
    nets: a context manager the engine is built under; check(eng) runs after
    the steps."""
    import numpy as np
    import torch
    from _gpu import assert_layout, build_engine

    with nets or contextlib.nullcontext():
        eng, rb, cc = build_engine(c, precision, 3, torch.device("cuda", 0))
    assert_layout(eng, layout)
    B, A = cc["batch"], cc["act"]
    g = np.random.default_rng(17)
    idx = g.integers(0, cc["capacity"], (STEPS, B)).astype(np.int32)
    eps = g.standard_normal((STEPS, 2, B, A)).astype(np.float32)
    for k in range(STEPS):
        eng.train(rb, 1, indices=torch.from_numpy(idx[k:k + 1]), eps=torch.from_numpy(eps[k:k + 1]))
    torch.cuda.synchronize()
    eng.check()
    if check:
        check(eng)
    arrays = dict(eng.state_tensors(), stats=eng.stats)
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            for k, v in sorted(arrays.items())}


def render(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


def main(out, cases, digests):
    """Write `out` from digests(name) of every case, on the library SAC_ENGINE_LIB names."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit the library named by SAC_ENGINE_LIB was built from")
    args = ap.parse_args()
    if not os.environ.get("SAC_ENGINE_LIB"):
        sys.exit("SAC_ENGINE_LIB must name a library built from the parent commit")
    doc = {"parent": args.parent, "steps": STEPS, "cases": {name: digests(name) for name in cases}}
    with open(out, "w") as f:
        f.write(render(doc))
    print(f"wrote {out}: {len(cases)} cases, {sum(len(v) for v in doc['cases'].values())} digests")
