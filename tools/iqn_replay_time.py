#!/usr/bin/env python3
"""What the distributional (IQN) Ape-X learner's replay costs per step (DESIGN.md §14;
profiles/iqn_replay).

Shapes (N = 512, W = 8) and (N = 128, W = 32), A = 15, fp32 and bf16, a ring of 100 000 transitions
filled with random priorities.  Per cell, host wall time and device event time per step over
--steps steps after --warmup, for
  (a) PrioritizedReplay(target_width=W).sample + IqnEngine.train_step + update  (the torch replay)
  (b) iqn_train_step_replay                                                      (one call)
  (c) iqn_train_step alone on a fixed batch
in --runs alternating runs a, b, c, a, b, c, ...  Prints one JSON line per cell with each run's
figures, the means, the replay's cost (b) - (c) beside (a) - (c), and whether (a) - (b) exceeds
three times the larger run-to-run spread of the two.  Per W it also times one rollout of --rollout
steps into the ring: NativeQuantileReplay.extend_rollout beside iqn_nstep_targets + the torch
replay's extend (device inputs, events around --steps calls).

usage: python tools/iqn_replay_time.py [--steps 200] [--warmup 20] [--runs 4] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dqn_replay_time import timed  # noqa: E402
from impala_amd.dqn import PrioritizedReplay  # noqa: E402
from impala_amd.iqn import (DistributionalAtariDQN, IqnEngine, NativeQuantileReplay,  # noqa: E402
                            iqn_nstep_targets)

A = 15
SHAPES = ((512, 8), (128, 32))


def fill(rb, cap, W, seed, chunk=50_000):
    """The same transitions and priorities into either replay (obs bytes random per chunk)."""
    g = torch.Generator(device=rb.device).manual_seed(seed)
    for i0 in range(0, cap, chunk):
        n = min(chunk, cap - i0)
        s = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, device=rb.device, generator=g)
        a = torch.randint(0, A, (n,), device=rb.device, generator=g)
        t = torch.randn(n, W, device=rb.device, generator=g)
        p = torch.rand(n, device=rb.device, generator=g) * 2 + 0.01
        rb.extend((s, a, t), priorities=p)
        del s
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--cap", type=int, default=100_000)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--rollout", type=int, default=100, help="L of the timed ingest (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cap = args.cap
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    for N, W in SHAPES:
        plain = PrioritizedReplay(cap, device=dev, seed=1, target_width=W)
        fill(plain, cap, W, seed=7)
        native = NativeQuantileReplay(cap, W, device=dev, seed=1)
        native.extend((plain.s, plain.a, plain.target), priorities=plain.priorities)
        torch.cuda.synchronize()
        if args.rollout >= 2:
            L = args.rollout
            g = torch.Generator(device=dev).manual_seed(3)
            s = torch.randint(0, 256, (L, 3, 64, 64), dtype=torch.uint8, device=dev, generator=g)
            a = torch.randint(0, A, (L,), device=dev, generator=g)
            r, q_pi = torch.randn(L, device=dev, generator=g), torch.randn(L, device=dev, generator=g)
            d = torch.zeros(L, dtype=torch.uint8, device=dev)
            q_star = torch.randn(L, W, device=dev, generator=g)

            def ingest_native():
                native.extend_rollout(s, a, r, d, q_pi, q_star, n_step=3, gamma=0.99)

            def ingest_torch():
                tg, prio = iqn_nstep_targets(r, d, q_pi, q_star, 3, 0.99)
                plain.extend((s[:-1], a[:-1], tg), prio)

            runs = {"extend_rollout": [], "nstep_targets_plus_torch_extend": []}
            for _ in range(args.runs):
                runs["extend_rollout"].append(timed(ingest_native, args.steps, args.warmup))
                runs["nstep_targets_plus_torch_extend"].append(timed(ingest_torch, args.steps, args.warmup))
            out = {"capacity": cap, "W": W, "rollout_L": L, "calls": args.steps}
            for k, rs in runs.items():
                out[k] = {"wall_ms": [round(x[0], 5) for x in rs], "event_ms": [round(x[1], 5) for x in rs],
                          "mean_wall_ms": round(float(np.mean([x[0] for x in rs])), 5),
                          "mean_event_ms": round(float(np.mean([x[1] for x in rs])), 5)}
            emit(out)
        for dtype in args.dtypes:
            engines = []
            for _ in range(3):
                m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
                e = IqnEngine(m, batch_size=N, train=True)
                m._train_engine = e
                engines.append(e)
            ea, eb, ec = engines
            _, fixed, probs = plain.sample(N)
            fixed = tuple(x.clone() for x in fixed)
            probs = probs.clone()
            counter = [0]

            def step_a():
                counter[0] += 1
                k, batch, p = plain.sample(N)
                plain.update(k, ea.train_step(*batch, p, seed=2, counter=counter[0])[0])

            def step_b():
                counter[0] += 1
                eb.train_step_replay(native, 1, counter[0], tau_seed=2, tau_counter=counter[0])

            def step_c():
                counter[0] += 1
                ec.train_step(*fixed, probs, seed=2, counter=counter[0])

            steps = (("a", step_a), ("b", step_b), ("c", step_c))
            runs = {k: [] for k, _ in steps}
            for _ in range(args.runs):
                for name, fn in steps:
                    runs[name].append(timed(fn, args.steps, args.warmup))
            out = {"capacity": cap, "dtype": dtype, "N": N, "W": W, "steps": args.steps, "warmup": args.warmup}
            for kind, col in (("wall_ms", 0), ("event_ms", 1)):
                v = {k: [round(r[col], 5) for r in rs] for k, rs in runs.items()}
                mean = {k: float(np.mean(x)) for k, x in v.items()}
                sp = {k: max(x) - min(x) for k, x in v.items()}
                s3 = max(sp["a"], sp["b"])
                out[kind] = {"runs": v, "mean": {k: round(x, 5) for k, x in mean.items()},
                             "spread": {k: round(x, 5) for k, x in sp.items()},
                             "replay_cost_b_minus_c": round(mean["b"] - mean["c"], 5),
                             "torch_replay_cost_a_minus_c": round(mean["a"] - mean["c"], 5),
                             "a_minus_b": round(mean["a"] - mean["b"], 5),
                             "larger_spread_of_a_b": round(s3, 5),
                             "b_below_a_by_more_than_3_spreads": bool(mean["a"] - mean["b"] > 3 * s3)}
            emit(out)
            for e in engines:
                e.close()
        native.close()
        del plain, native
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
