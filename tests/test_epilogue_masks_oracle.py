"""The dead-unit inputs of tests/test_gpu_epilogue_masks.py on the CPU oracle
alone (no GPU): for every case of tests/_dead_units.py the dead units'
pre-activations are exactly +0.0 on the passes whose backward runs, and after
two oracle steps the dead rows of W and b (targets included) and of Adam's m
and v are exactly zero.  So the GPU cases do test the mask at p == 0, and
"the dead rows stay zero" is what a correct implementation gives."""
import numpy as np
import pytest

import _dead_units as D
from _gpu import oracle_fresh_state, synthetic_rows
from oracle import sac_oracle as O

STEPS = 2


@pytest.mark.parametrize("case", list(D.CASES))
def test_the_oracle_keeps_dead_rows_at_zero(case):
    c, sp = D.CASES[case]
    with D.dead_nets(sp):
        st, hp = oracle_fresh_state(c)
    B, A = c["batch"], c["act"]
    rows = synthetic_rows(c["capacity"], c["obs"], A, 3, 0.01)
    g = np.random.default_rng(17)
    D.assert_oracle_rows_zero(st, sp, (case, 0))
    for k in range(1, STEPS + 1):
        idx = g.choice(c["capacity"], size=B, replace=False)
        et = g.standard_normal((B, A)).astype(np.float32)
        ea = g.standard_normal((B, A)).astype(np.float32)
        bt = O.Batch(rows["obs"][idx], rows["act"][idx], rows["rew"][idx], rows["next_obs"][idx], rows["done"][idx])
        # the passes with a backward: pi on s, the critics on (s, a)
        for net, x in ((st.pi, bt.s), (st.q1, np.concatenate([bt.s, bt.a], 1)), (st.q2, np.concatenate([bt.s, bt.a], 1))):
            _, cache = net.forward(np.asarray(x, np.float32))
            for layer, units in D.dead_rows(sp):
                p = cache[layer][1][:, units]
                assert p.dtype == np.float32 and not np.any(p) and not np.any(np.signbit(p)), (case, k, layer)
        O.training_step(st, hp, bt, et, ea)
        D.assert_oracle_rows_zero(st, sp, (case, k))
    # the live part did train: some live row of every trained net's layer 0 or 1 has a non-zero first moment
    for opt in (st.opt_pi, st.opt_q1, st.opt_q2):
        assert any(np.any(m) for m in opt.m)
