#!/usr/bin/env python3
"""What the PPO learner's loop costs per step around its step (profiles/ppo_replay).

N = 256, A = 15, a replay of 20 000 transitions, fp32 and bf16.  Per dtype, host wall time and
device event time per step over --steps steps after --warmup, for
  (a) PPOLearner.train_step over the host ReplayBuffer  (sample, collate_transitions: torch.cat
      of 256 items, pin_memory, H2D; then the step)
  (b) PPOLearner.train_step over a DeviceTransitionBuffer  (sample_rows; the step reads the ring
      in place)
  (c) Engine.train_step alone on a fixed device batch
in --runs alternating runs a, b, c, a, b, c, ...  Prints one JSON line per dtype with each run's
figures, the means, the loop's cost (a) - (c) and (b) - (c), each path's run-to-run spread, and
whether (a) - (b) exceeds three times the larger spread; then one line with the time of one
extend_rollout at L = 129 (events around --ingests calls on device inputs).

usage: python tools/ppo_replay_time.py [--steps 200] [--warmup 20] [--runs 4] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from impala_amd.engine import Engine  # noqa: E402
from impala_amd.learner import ImpalaAdam  # noqa: E402
from impala_amd.model import AtariPPOModel  # noqa: E402
from impala_amd.ppo import PPOLearner  # noqa: E402
from impala_amd.replay import DeviceTransitionBuffer, ReplayBuffer  # noqa: E402

N, A = 256, 15


def timed(step, steps, warmup):
    """-> (host wall ms per step, device event ms per step) of `steps` back-to-back calls."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return wall, e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--cap", type=int, default=20_000)
    ap.add_argument("--ingests", type=int, default=200)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cap = args.cap
    g = torch.Generator().manual_seed(7)
    host = ReplayBuffer(cap, seed=1)
    ring = DeviceTransitionBuffer(cap, A, device=dev, seed=1)
    for i0 in range(0, cap, 2000):  # the same transitions into both replays
        n = min(2000, cap - i0)
        s = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, generator=g)
        a = torch.randint(0, A, (n,), generator=g)
        t = torch.randn(n, generator=g)
        mu = 0.3 * torch.randn(n, A, generator=g)
        host.extend([[s[i:i + 1].clone(), a[i:i + 1].clone(), t[i:i + 1].clone(), mu[i:i + 1].clone()]
                     for i in range(n)])
        ring.extend((s, a, t, mu))
    torch.cuda.synchronize()
    lines = []
    for dtype in args.dtypes:
        def learner(rb):
            m = AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
            ln = PPOLearner(m, rb, ImpalaAdam(lr=1e-4, eps=1e-5), batch_size=N, dtype=dtype,
                            model_push_period=1 << 30)
            ln.prepare()
            return ln

        la, lb = learner(host), learner(ring)
        mc = AtariPPOModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
        ec = Engine(mc, batch_size=N, algo="ppo", dtype=dtype)
        mc._train_engine = ec
        fixed = tuple(f[:N].clone() for f in ring.fields)

        def step_c():
            ec.train_step(*fixed)

        runs = {"a": [], "b": [], "c": []}
        for _ in range(args.runs):
            for name, fn in (("a", la.train_step), ("b", lb.train_step), ("c", step_c)):
                runs[name].append(timed(fn, args.steps, args.warmup))
        assert lb._rows, "the device path fell back to gathers"
        out = {"capacity": cap, "dtype": dtype, "N": N, "steps": args.steps, "warmup": args.warmup}
        for kind, col in (("wall_ms", 0), ("event_ms", 1)):
            v = {k: [round(r[col], 5) for r in rs] for k, rs in runs.items()}
            mean = {k: float(np.mean(x)) for k, x in v.items()}
            spread = {k: round(max(x) - min(x), 5) for k, x in v.items()}
            larger = max(spread["a"], spread["b"])
            out[kind] = {
                "runs": v, "mean": {k: round(x, 5) for k, x in mean.items()}, "spread": spread,
                "host_loop_cost_a_minus_c": round(mean["a"] - mean["c"], 5),
                "device_loop_cost_b_minus_c": round(mean["b"] - mean["c"], 5),
                "a_minus_b": round(mean["a"] - mean["b"], 5),
                "b_below_a_by_more_than_3_spreads": bool(mean["a"] - mean["b"] > 3 * larger),
            }
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        for e in (la.engine, lb.engine, ec):
            e.close()
    # one extend_rollout at L = 129 on device inputs: events around --ingests calls
    L = 129
    ro = (torch.randint(0, 256, (L, 3, 64, 64), dtype=torch.uint8, device=dev),
          torch.randint(0, A, (L,), device=dev), torch.randn(L, device=dev),
          (torch.rand(L, device=dev) < 0.05).to(torch.uint8), torch.randn(L, A, device=dev),
          torch.randn(L, device=dev))
    wall, ev = timed(lambda: ring.extend_rollout(*ro), args.ingests, 10)
    line = json.dumps({"extend_rollout": {"L": L, "calls": args.ingests, "wall_ms": round(wall, 5),
                                          "event_ms": round(ev, 5)}})
    print(line, flush=True)
    lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
