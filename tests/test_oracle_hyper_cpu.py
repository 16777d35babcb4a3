"""The oracle's Adam settings and target entropy, on the CPU.

The reference cannot set betas, eps or the target entropy, so no golden fixture
pins oracle.sac_oracle.SacHyper's beta1 / beta2 / adam_eps / target_entropy
(the fixtures pin the defaults: tests/test_oracle_golden.py).  torch.optim.Adam
is the yardstick for the first three; the alpha loss of the reference
(sac/agent.py:263-280) with another target entropy, written in torch, for the
last.  The last test keeps the reason for adam_eps = 1e-3 in
tests/test_gpu_hyper.py executable: at 1e-8 a constant factor on a gradient is
invisible in the post-step parameters."""
import copy

import numpy as np
import pytest
import torch

from oracle import sac_oracle as O

ADAMS = [dict(beta1=0.9, beta2=0.999, eps=1e-8), dict(beta1=0.8, beta2=0.99, eps=1e-3),
         dict(beta1=0.5, beta2=0.9, eps=1e-5)]


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("kw", ADAMS, ids=lambda kw: f"b{kw['beta1']}-{kw['beta2']}-eps{kw['eps']}")
def test_adam_update_matches_torch_adam(kw):
    """fp32 tensors of a net and one fp64 scalar through the same three
    gradients: adam_update within 1 ulp of torch.optim.Adam's parameters,
    adam_update_scalar within 1e-15 relative."""
    g = np.random.default_rng(0)
    shapes = [(40, 8), (40,), (6, 40), (6,)]
    lr = 1e-3
    params = [g.standard_normal(s).astype(np.float32) for s in shapes]
    # gradient magnitudes on both sides of every eps here
    grads = [[(g.standard_normal(s) * 10.0 ** g.uniform(-6, -1, s)).astype(np.float32) for s in shapes]
             for _ in range(3)]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = torch.optim.Adam(tp, lr=lr, betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"], foreach=False)
    st = O.AdamState.zeros_like(params)
    la, la_g = -1.2, [0.37, -0.011, 2.5e-4]
    tla = torch.nn.Parameter(torch.tensor(la, dtype=torch.float64))
    opt_a = torch.optim.Adam([tla], lr=lr, betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"], foreach=False)
    m = v = step = 0.0
    for k in range(3):
        for t, gr in zip(tp, grads[k]):
            t.grad = torch.from_numpy(gr.copy())
        opt.step()
        O.adam_update(params, grads[k], st, lr, kw["beta1"], kw["beta2"], kw["eps"])
        for p, t in zip(params, tp):
            u = _ulps(p, t.detach().numpy())
            assert u.max() <= 1.0, (k, p.shape, u.max())
        tla.grad = torch.tensor(la_g[k], dtype=torch.float64)
        opt_a.step()
        la, m, v, step = O.adam_update_scalar(la, la_g[k], m, v, step, lr, kw["beta1"], kw["beta2"], kw["eps"])
        assert abs(la - tla.item()) <= 1e-15 * abs(tla.item()), (k, la, tla.item())
    assert st.step == 3.0 and step == 3.0


def _small_case(**over):
    from _gpu import config_rows, oracle_fresh_state
    from test_gpu_activations import SMALL
    from test_gpu_hyper import hyper

    c = dict(SMALL, **hyper("adam", SMALL["act"]))
    c.update(over)
    st, hp = oracle_fresh_state(c)
    return c, st, hp, config_rows(c)


def _draws(c, rows, steps):
    g = np.random.default_rng(11)
    B, A = c["batch"], c["act"]
    for _ in range(steps):
        idx = g.choice(c["capacity"], size=B, replace=False)
        et, ea = g.standard_normal((2, B, A)).astype(np.float32)
        yield O.Batch(*(rows[k][idx] for k in ("obs", "act", "rew", "next_obs", "done"))), et, ea


def test_training_step_passes_the_hyper_fields_on():
    """SacHyper's Adam fields and target entropy reach all four optimizers and
    the alpha loss: the defaults spelled out equal the defaults; each changed
    Adam field moves every trained network and log alpha; the target entropy
    moves L_alpha and log alpha alone, and both equal the reference's alpha
    loss written in torch with that target entropy."""
    c, st0, hp0, rows = _small_case()
    assert hp0.auto_entropy_tuning
    (bt, et, ea), = _draws(c, rows, 1)

    def step(**kw):
        hp = copy.deepcopy(hp0)
        for k, v in kw.items():
            setattr(hp, k, v)
        st = copy.deepcopy(st0)
        return st, O.training_step(st, hp, bt, et, ea), hp

    dflt = dict(beta1=0.9, beta2=0.999, adam_eps=1e-8, target_entropy=None)
    a, ra, _ = step(**dflt)
    b, rb, _ = step(**dict(dflt, target_entropy=-float(c["act"])))
    assert ra["losses"] == rb["losses"] and a.log_alpha == b.log_alpha
    plain = O.SacHyper(alpha=hp0.alpha, auto_entropy_tuning=True)
    assert (plain.beta1, plain.beta2, plain.adam_eps, plain.target_entropy) == (0.9, 0.999, 1e-8, None)
    for field in ("beta1", "beta2", "adam_eps"):
        # (step 1 from zero moments: beta1 and beta2 cancel in m^ / sqrt(v^); later steps show them)
        outs = []
        for kw in (dflt, dict(dflt, **{field: {"beta1": 0.8, "beta2": 0.99, "adam_eps": 1e-3}[field]})):
            hp = copy.deepcopy(hp0)
            for k, v in kw.items():
                setattr(hp, k, v)
            st = copy.deepcopy(st0)
            for bt2, et2, ea2 in _draws(c, rows, 3):
                O.training_step(st, hp, bt2, et2, ea2)
            outs.append(st)
        for net in ("pi", "q1", "q2"):
            d = max(np.abs(x - y).max() for x, y in zip(getattr(outs[0], net).params(), getattr(outs[1], net).params()))
            assert d > 1e-7, (field, net, d)
        assert abs(outs[0].log_alpha - outs[1].log_alpha) > 1e-7, field
    # target entropy: the networks' step does not read it
    H = -0.5 * c["act"]
    t, rt, hp = step(**dict(dflt, target_entropy=H))
    assert rt["losses"][:3] == ra["losses"][:3]
    for net in ("pi", "q1", "q2", "q1t", "q2t"):
        for x, y in zip(getattr(t, net).params(), getattr(a, net).params()):
            assert np.array_equal(x, y)
    la = torch.tensor(float(np.log(hp.alpha)), dtype=torch.float64, requires_grad=True)
    lp = torch.from_numpy(rt["log_pi"])
    loss = -(la * (lp + H).detach()).mean()
    opt = torch.optim.Adam([la], lr=hp.alpha_lr)
    loss.backward()
    opt.step()
    assert abs(rt["losses"][3] - loss.item()) <= 1e-5 * abs(loss.item())
    assert abs(t.log_alpha - la.item()) <= 1e-12
    assert rt["losses"][3] != ra["losses"][3]


def _within(a, b):
    """Share of elements within 1e-6, per tensor: {(net, tensor index): share}."""
    return {(n, i): float(np.mean(np.abs(x - y) <= 1e-6)) for n in ("pi", "q1", "q2", "q1t", "q2t")
            for i, (x, y) in enumerate(zip(getattr(a, n).params(), getattr(b, n).params()))}


@pytest.mark.parametrize("adam_eps", [1e-8, 1e-3])
def test_adam_eps_decides_whether_a_scaled_gradient_shows(adam_eps, monkeypatch):
    """The oracle against itself with every bias gradient doubled (what a bias
    sum over padded rows with a wrong factor, or a wrong 2/B seed on one path,
    would give), shape SMALL, 3 steps, through the parity tests' element check
    (>= 99.5 % of every tensor within 1e-6).  adam_eps = 1e-8: the check passes
    on every step, and the losses agree to 1e-6: the blind spot.  adam_eps =
    1e-3: it fails on step 1, on biases of all three trained networks."""
    c, st, hp, rows = _small_case(adam_eps=adam_eps)
    mut = copy.deepcopy(st)
    backward = O.MLP.backward

    def doubled(self, cache, g_out, need_dx=False):
        gW, gb, dx = backward(self, cache, g_out, need_dx)
        return gW, [np.float32(2) * x for x in gb], dx

    for k, (bt, et, ea) in enumerate(_draws(c, rows, 3), 1):
        ref = O.training_step(st, hp, bt, et, ea)
        monkeypatch.setattr(O.MLP, "backward", doubled)
        got = O.training_step(mut, hp, bt, et, ea)
        monkeypatch.setattr(O.MLP, "backward", backward)
        share = _within(mut, st)
        if adam_eps == 1e-8:
            assert min(share.values()) >= 0.995, (k, share)
            for a, b in zip(got["losses"], ref["losses"]):
                assert abs(a - b) <= 1e-6 * max(abs(b), 1e-3), (k, got["losses"], ref["losses"])
        elif k == 1:
            for n in ("pi", "q1", "q2"):
                biases = [v for (net, i), v in share.items() if net == n and i % 2 == 1]
                assert min(biases) < 0.995, (n, biases)  # (a critic's output bias, |g| >> eps, may still agree)
            return
