"""What bf16 products alone cost a fixture's losses, on the CPU (no GPU, no engine):
the fp32 oracle's step against the same step with every forward matmul's
operands (activations and weights) rounded to bf16 and accumulated in fp32, one
step from the same state.  The reference for a bf16 loss bound that is not the
engine's own output (tests/test_gpu_parity.py::BF16_LOSS_RTOL).

    python tools/debug/bf16_loss_emulation.py out_smooth out_kink gelu_tanh
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "soft-actor-critic_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _fixtures import CONFIGS, batch, eps, oracle_state  # noqa: E402
from oracle import sac_oracle as O  # noqa: E402


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


def forward_bf16(self, x):
    """O.MLP.forward with bf16 operands in every matmul."""
    cache = []
    h = x.astype(np.float32)
    n = len(self.W)
    for i in range(n):
        p = (bf(h) @ bf(self.W[i]).T + self.b[i]).astype(np.float32)
        o = O.act_fwd(self.hidden_act if i < n - 1 else self.out_act, p)
        cache.append((h, p, o))
        h = o
    return h, cache


def main(names):
    fwd = O.MLP.forward
    for name in names:
        st, hp, fx, meta = oracle_state(name)
        for k in range(1, meta["steps"] + 1):
            et, ea = eps(fx, k)
            st16 = copy.deepcopy(st)
            ref = O.training_step(st, hp, batch(fx, k), et, ea)
            O.MLP.forward = forward_bf16
            try:
                em = O.training_step(st16, hp, batch(fx, k), et, ea)
            finally:
                O.MLP.forward = fwd
            rel = [abs(a - b) / max(abs(b), 1e-3) for a, b in zip(em["losses"][:2], ref["losses"][:2])]
            print(f"{name} (B {meta['batch']}) step {k}: L_Q1 {rel[0]:.2e} L_Q2 {rel[1]:.2e} rel")


if __name__ == "__main__":
    main(sys.argv[1:] or CONFIGS)
