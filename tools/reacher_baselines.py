"""What the two-link reacher (sac.control_envs.ReacherEnv) is worth: the returns
of the scripted policies of tests/test_reacher_cpu.py on the host class, one
default 100-step episode per seed.  No GPU.  Writes profiles/reacher_baselines.txt:

    python tools/reacher_baselines.py [--out profiles/reacher_baselines.txt]
"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "soft-actor-critic_amd"), os.path.join(R, "tests")]
import numpy as np  # noqa: E402


def main():
    from test_reacher_cpu import BASELINE_SEEDS, pd_controller, scripted_returns, zero_torque

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "reacher_baselines.txt"))
    args = ap.parse_args()
    rngs = {}

    def uniform_random(env):
        return rngs.setdefault(id(env), np.random.default_rng(len(rngs))).uniform(-1.0, 1.0, size=2).astype(np.float32)

    seeds = list(BASELINE_SEEDS)
    lines = ["Returns of scripted policies on sac.control_envs.ReacherEnv (the host class; max_steps 100, dt 0.05,",
             f"max_torque 1.0), one episode per seed, seeds {seeds[0]}..{seeds[-1]} (env.reset(seed=s)).  "
             "tools/reacher_baselines.py.", "",
             "policy           mean return      worst       best   final distance (max)"]
    means = {}
    for name, policy in (("zero torque", zero_torque), ("uniform random", uniform_random),
                         ("PD controller", pd_controller)):
        ret, dist = scripted_returns(policy, seeds)
        means[name] = float(ret.mean())
        lines.append(f"{name:<16} {ret.mean():>11.3f} {ret.min():>10.3f} {ret.max():>10.3f}   {dist.max():.2e}")
    zero, pd = means["zero torque"], means["PD controller"]
    lines += ["",
              "uniform random: each component U(-1, 1) per step, numpy default_rng(episode index).",
              "PD controller: u = clip(2 wrap(q* - th) - 0.4 w, +-1) toward the inverse-kinematics solution q* nearer in",
              "joint space.  tests/test_reacher_cpu.py asserts zero torque <= -12 and PD >= -6 on these seeds.",
              "",
              f"The learning bar of tests/test_gpu_reacher.py: the midpoint ({zero:.3f} + {pd:.3f}) / 2 = "
              f"{(zero + pd) / 2:.3f};",
              f"a tenth of the zero-to-PD gap is {(pd - zero) / 10:.3f}, so the worst seed has to reach "
              f"{(zero + pd) / 2 + (pd - zero) / 10:.3f}."]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
