"""Whether train.random_steps helps on the two learning tasks of the suite, on one MI355X: the pendulum at
tests/test_gpu_pendulum.py's configuration and the cart-pole at tests/test_gpu_cartpole.py's, seeds 0..2, with
K = 0 and K = warming_steps, all in one process.  Prints one line per run (the deterministic policy's evaluation
before and after training, as the tests measure it) and appends them to --out.

    python tools/random_steps_learning.py [--tasks pendulum cartpole] [--seeds 0 1 2] [--out FILE]
"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "soft-actor-critic_amd"), os.path.join(R, "tests")]


def run(task, seed, random_steps):
    import torch

    import _control
    from sac.agent import SAC
    from sac.device_envs import DeviceVectorEnv

    if task == "pendulum":
        from test_gpu_pendulum import LEARNING as c

        cfg = _control.cfg("pendulum", hidden=c["hidden"], precision=c["precision"], capacity=c["capacity"],
                           batch=c["batch"], warming=c["warming"], seed=seed, action_scale=c["action_scale"])
        dv = DeviceVectorEnv("pendulum", c["num_envs"], device="cuda")
        evaluate = lambda agent: agent.evaluate_device(c["eval_episodes"], dv)  # noqa: E731
    else:
        from sac.control_envs import CartPoleEnv
        from test_gpu_cartpole import LEARNING as c

        cfg = _control.cfg("cartpole", hidden=c["hidden"], precision=c["precision"], capacity=c["capacity"],
                           batch=c["batch"], warming=c["warming"], seed=seed, alpha=c["alpha"], alpha_lr=c["alpha_lr"])
        dv = DeviceVectorEnv(CartPoleEnv, c["num_envs"], device="cuda")
        evaluate = lambda agent: agent.evaluate_device(episodes_per_env=c["episodes_per_env"], vec_env=dv)  # noqa: E731
    cfg["train"]["random_steps"] = random_steps
    agent = SAC(dv, cfg)
    untrained = evaluate(agent)
    vec_steps = (c["gradient_steps"] + c["warming"] - 1) // c["num_envs"]
    t0 = time.perf_counter()
    m = agent.run_device_training_loop(vec_steps * c["num_envs"], seed=seed, graph_steps=c["graph_steps"])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    trained = evaluate(agent)
    agent.engine.close()
    return (f"{task:<9} seed {seed}  random_steps {random_steps:>5}  untrained {untrained:>9.2f}  trained "
            f"{trained:>9.2f}  gradient_steps {m['gradient_steps']}  train_s {dt:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", nargs="+", default=["pendulum", "cartpole"], choices=["pendulum", "cartpole"])
    ap.add_argument("--seeds", nargs="+", type=int, default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("random_steps_learning: no HIP device visible")
    from test_gpu_cartpole import LEARNING as cart
    from test_gpu_pendulum import LEARNING as pend

    warming = {"pendulum": pend["warming"], "cartpole": cart["warming"]}
    for task in args.tasks:
        for seed in args.seeds:
            for k in (0, warming[task]):
                line = run(task, seed, k)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
