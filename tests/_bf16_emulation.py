"""The oracle's training step with bf16 products, on the CPU (no GPU, no
engine): every matmul of every network -- the forward's x W^T, the backward's
dY W and dY^T x -- with both operands rounded to bf16 and the products summed
in float64, the bias gradient summed from the rounded dY; everything else
(activations, the head, the losses, Adam, Polyak) as the fp32 oracle has it.
This is the arithmetic of the engine's bf16 mode up to its fp32 summation
order, so its deviation from the fp32 oracle on the same state and rows is
what bf16 rounding alone costs there: the reference for a bf16 bound that is
not taken from the engine's output (tools/debug/bf16_loss_emulation.py does
the same for the forward's losses)."""
import contextlib
import copy

import numpy as np
import torch

from oracle import sac_oracle as O

F32 = np.float32


def bf(x):
    """x rounded to bf16 (round to nearest even), as float64."""
    return torch.from_numpy(np.ascontiguousarray(x, F32)).bfloat16().double().numpy()


def _forward(self, x):
    cache = []
    h = x.astype(F32)
    n = len(self.W)
    for i in range(n):
        p = (bf(h) @ bf(self.W[i]).T + self.b[i].astype(np.float64)).astype(F32)
        o = O.act_fwd(self.hidden_act if i < n - 1 else self.out_act, p)
        cache.append((h, p, o))
        h = o
    return h, cache


def _backward(self, cache, g_out, need_dx=False):
    n = len(self.W)
    gW, gb = [None] * n, [None] * n
    g = g_out.astype(F32)
    dx = None
    for i in reversed(range(n)):
        h_in, p, o = cache[i]
        gp = bf(O.act_bwd(self.hidden_act if i < n - 1 else self.out_act, p, o, g))
        gW[i] = (gp.T @ bf(h_in)).astype(F32)
        gb[i] = gp.sum(0).astype(F32)
        if i > 0 or need_dx:
            g = (gp @ bf(self.W[i])).astype(F32)
    if need_dx:
        dx = g
    return gW, gb, dx


@contextlib.contextmanager
def bf16_products():
    """oracle.sac_oracle.MLP with bf16 products inside the block."""
    fwd, bwd = O.MLP.forward, O.MLP.backward
    O.MLP.forward, O.MLP.backward = _forward, _backward
    try:
        yield
    finally:
        O.MLP.forward, O.MLP.backward = fwd, bwd


def step(st, hp, bt, et, ea):
    """One emulated step from `st` (not mutated): (the step's result, the post-step state)."""
    post = copy.deepcopy(st)
    with bf16_products():
        out = O.training_step(post, hp, bt, et, ea)
    return out, post
