"""What the balancing cart-pole (sac.control_envs.CartPoleEnv) is worth: the
episode lengths (= returns, +1 per step) of the scripted policies of
tests/test_cartpole_cpu.py on the host class, one default 500-step episode per
seed.  No GPU.  Writes profiles/cartpole_baselines.txt:

    python tools/cartpole_baselines.py [--out profiles/cartpole_baselines.txt]
"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "soft-actor-critic_amd"), os.path.join(R, "tests")]
import numpy as np  # noqa: E402


def main():
    from test_cartpole_cpu import BASELINE_SEEDS, linear_feedback, scripted_lengths, zero_force

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "cartpole_baselines.txt"))
    args = ap.parse_args()
    rngs = {}

    def uniform_random(env):
        return rngs.setdefault(id(env), np.random.default_rng(len(rngs))).uniform(-1.0, 1.0, size=1).astype(np.float32)

    seeds = list(BASELINE_SEEDS)
    lines = ["Returns (= episode lengths: +1 per step) of scripted policies on sac.control_envs.CartPoleEnv (the host",
             f"class; max_steps 500, dt 0.02, max_action 1.0), one episode per seed, seeds {seeds[0]}..{seeds[-1]} "
             "(env.reset(seed=s)).", "tools/cartpole_baselines.py.", "",
             "policy            mean return   shortest    longest   ended by failure"]
    means = {}
    for name, policy in (("zero force", zero_force), ("uniform random", uniform_random),
                         ("linear feedback", linear_feedback)):
        length, term = scripted_lengths(policy, seeds)
        means[name] = float(length.mean())
        lines.append(f"{name:<16} {length.mean():>12.2f} {length.min():>10d} {length.max():>10d}   "
                     f"{int(term.sum()):>4d} of {len(seeds)}")
    zero, fb = means["zero force"], means["linear feedback"]
    lines += ["",
              "uniform random: U(-1, 1) per step, numpy default_rng(episode index).",
              "linear feedback: u = clip(0.1 x + 0.3 xdot + 4 th + 0.6 thdot, +-1).  tests/test_cartpole_cpu.py asserts on",
              "the first 20 of these seeds that zero force fails before 200 steps and the feedback reaches 500 every time.",
              "",
              f"The learning bar of tests/test_gpu_cartpole.py: the midpoint ({zero:.2f} + {fb:.2f}) / 2 = "
              f"{(zero + fb) / 2:.2f};",
              f"a tenth of the zero-to-feedback gap is {(fb - zero) / 10:.2f}, so the worst seed has to reach "
              f"{(zero + fb) / 2 + (fb - zero) / 10:.2f}",
              "when the step count of the test is chosen (profiles/cartpole_learning.txt)."]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
