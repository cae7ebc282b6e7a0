#!/usr/bin/env python3
"""What the distributional learner's step costs beside the dueling one's (DESIGN.md §14;
profiles/iqn_step).

A = 15.  Per dtype (fp32, bf16): host wall time and device event time per call over --steps
back-to-back calls after --warmup, for
  iqn_train_step at N = 512, W = 8 and at N = 128, W = 32  (R = 4096 quantile rows each,
                                                            library-drawn taus, probabilities)
  dqn_train_step at N = 512 and at N = 128
in --runs alternating runs iqn512x8, dqn512, iqn128x32, dqn128, iqn512x8, ...  Prints one JSON line
per dtype with each run's figures, the means and the run-to-run spreads.  With --once NAME it runs
that path alone, --steps calls after the warm-up, for a kernel trace of its own.

usage: python tools/iqn_step_time.py [--steps 100] [--warmup 10] [--runs 3] [--dtypes fp32 bf16]
                                     [--once iqn512x8|iqn128x32|dqn512|dqn128] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from impala_amd.dqn import AtariDQNModel, DqnEngine  # noqa: E402
from impala_amd.iqn import DistributionalAtariDQN, IqnEngine  # noqa: E402
from tools.iqn_time import timed  # noqa: E402

A = 15


def paths(dev, dtype):
    g = torch.Generator(device=dev).manual_seed(3)
    counter = [0]
    out, keep = {}, []
    for N, W in ((512, 8), (128, 32)):
        obs = torch.randint(0, 256, (N, 3, 64, 64), dtype=torch.uint8, device=dev, generator=g)
        act = torch.randint(0, A, (N,), device=dev, generator=g)
        prob = torch.rand(N, device=dev, generator=g) * 1e-2 + 1e-4
        m = DistributionalAtariDQN((3, 64, 64), A, W, device=dev, dtype=dtype, seed=0)
        e = IqnEngine(m, batch_size=N, train=True)
        tgt = torch.randn(N, W, device=dev, generator=g)

        def step(e=e, obs=obs, act=act, tgt=tgt, prob=prob):
            counter[0] += 1
            e.train_step(obs, act, tgt, prob, seed=1, counter=counter[0])
        out[f"iqn{N}x{W}"] = step
        md = AtariDQNModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
        ed = DqnEngine(md, batch_size=N)
        tgt1 = torch.randn(N, device=dev, generator=g)

        def step_d(e=ed, obs=obs, act=act, tgt=tgt1, prob=prob):
            e.train_step(obs, act, tgt, prob)
        out[f"dqn{N}"] = step_d
        keep += [(m, e), (md, ed)]
    return out, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--once", default=None, help="run this path alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for dtype in args.dtypes:
        steps, keep = paths(dev, dtype)
        if args.once:
            wall, ev = timed(steps[args.once], args.steps, args.warmup)
            line = json.dumps({"dtype": dtype, "path": args.once, "calls": args.steps,
                               "wall_ms": round(wall, 5), "event_ms": round(ev, 5)})
        else:
            runs = {k: [] for k in steps}
            for _ in range(args.runs):
                for name, fn in steps.items():
                    runs[name].append(timed(fn, args.steps, args.warmup))
            out = {"dtype": dtype, "A": A, "steps": args.steps, "warmup": args.warmup}
            for kind, col in (("wall_ms", 0), ("event_ms", 1)):
                v = {k: [round(r[col], 5) for r in rs] for k, rs in runs.items()}
                out[kind] = {"runs": v, "mean": {k: round(float(np.mean(x)), 5) for k, x in v.items()},
                             "spread": {k: round(max(x) - min(x), 5) for k, x in v.items()}}
            line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        for _, e in keep:
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
