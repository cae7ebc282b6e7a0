#!/usr/bin/env python3
"""What the Ape-X learner's replay costs per step (profiles/dqn_replay).

N = 512, A = 15, fp32 and bf16, rings of 100 000 and 1 000 000 transitions filled with random
priorities.  Per configuration, host wall time and device event time per step over --steps steps
after --warmup, for
  (a) PrioritizedReplay.sample + DqnEngine.train_step + update  (the torch replay path)
  (b) dqn_train_step_replay                                      (one call)
  (c) dqn_train_step alone on a fixed batch
  (d) dqn_train_step_replay_rows                                 (one call, the ring read in place)
in --runs alternating runs a, b, c, d, a, b, c, d, ...  Prints one JSON line per configuration with
each run's figures, the means, the replay's cost (b) - (c) and (d) - (c) beside (a) - (c), and
whether (a) - (b) and (b) - (d) exceed three times the larger run-to-run spread of the two (the
method of README's wgloop note).  (b) and (d) share the native ring.  Per ring it also times one
extend_rollout of --rollout steps (device inputs, events around --steps calls).

usage: python tools/dqn_replay_time.py [--steps 200] [--warmup 20] [--runs 4] [--paths abcd]
                                       [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from impala_amd.dqn import (AtariDQNModel, DqnEngine, NativePrioritizedReplay,  # noqa: E402
                            PrioritizedReplay)

N, A = 512, 15


def fill(rb, cap, seed, chunk=50_000):
    """The same transitions and priorities into either replay (obs bytes random per chunk)."""
    g = torch.Generator(device=rb.device).manual_seed(seed)
    for i0 in range(0, cap, chunk):
        n = min(chunk, cap - i0)
        s = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, device=rb.device, generator=g)
        a = torch.randint(0, A, (n,), device=rb.device, generator=g)
        t = torch.randn(n, device=rb.device, generator=g)
        p = torch.rand(n, device=rb.device, generator=g) * 2 + 0.01
        rb.extend((s, a, t), priorities=p)
        del s
    torch.cuda.synchronize()


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
    ap.add_argument("--caps", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--paths", default="abcd", help="which of the paths a, b, c, d to run")
    ap.add_argument("--rollout", type=int, default=100, help="L of the timed extend_rollout (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for cap in args.caps:
        plain = PrioritizedReplay(cap, device=dev, seed=1)
        fill(plain, cap, seed=7)
        native = NativePrioritizedReplay(cap, device=dev, seed=1)
        # the plain ring's rows, so both replays hold the same transitions
        native.extend((plain.s, plain.a, plain.target), priorities=plain.priorities)
        torch.cuda.synchronize()
        if args.rollout >= 2:
            L = args.rollout
            g = torch.Generator(device=dev).manual_seed(3)
            ro = (torch.randint(0, 256, (L, 3, 64, 64), dtype=torch.uint8, device=dev, generator=g),
                  torch.randint(0, A, (L,), device=dev, generator=g), torch.randn(L, device=dev, generator=g),
                  torch.zeros(L, dtype=torch.uint8, device=dev), torch.randn(L, device=dev, generator=g),
                  torch.randn(L, device=dev, generator=g))
            wall, ev = timed(lambda: native.extend_rollout(*ro, n_step=3, gamma=0.99), args.steps, args.warmup)
            line = json.dumps({"capacity": cap, "extend_rollout_L": L, "calls": args.steps,
                               "wall_ms": round(wall, 5), "event_ms": round(ev, 5)})
            print(line, flush=True)
            lines.append(line)
        for dtype in args.dtypes:
            engines = []
            for _ in range(4):
                m = AtariDQNModel((3, 64, 64), A, device=dev, dtype=dtype, seed=0)
                e = DqnEngine(m, batch_size=N)
                m._train_engine = e
                engines.append(e)
            ea, eb, ec, ed = engines
            keys, fixed, probs = plain.sample(N)
            fixed = tuple(x.clone() for x in fixed)
            probs = probs.clone()
            counter = [0]

            def step_a():
                k, batch, p = plain.sample(N)
                plain.update(k, ea.train_step(*batch, p))

            def step_b():
                counter[0] += 1
                eb.train_step_replay(native, 1, counter[0])

            def step_c():
                ec.train_step(*fixed, probs)

            def step_d():
                counter[0] += 1
                ed.train_step_replay_rows(native, 1, counter[0])

            steps = [(k, f) for k, f in (("a", step_a), ("b", step_b), ("c", step_c), ("d", step_d))
                     if k in args.paths]
            runs = {k: [] for k, _ in steps}
            for _ in range(args.runs):
                for name, fn in steps:
                    runs[name].append(timed(fn, args.steps, args.warmup))
            out = {"capacity": cap, "dtype": dtype, "N": N, "steps": args.steps, "warmup": args.warmup}
            for kind, col in (("wall_ms", 0), ("event_ms", 1)):
                v = {k: [round(r[col], 5) for r in rs] for k, rs in runs.items()}
                mean = {k: float(np.mean(x)) for k, x in v.items()}
                sp = {k: max(x) - min(x) for k, x in v.items()}
                o = {"runs": v, "mean": {k: round(x, 5) for k, x in mean.items()},
                     "spread": {k: round(x, 5) for k, x in sp.items()}}

                def gap(hi, lo):  # is `lo` below `hi` by more than three times the larger spread
                    if hi in mean and lo in mean:
                        s3 = max(sp[hi], sp[lo])
                        o[f"{hi}_minus_{lo}"] = round(mean[hi] - mean[lo], 5)
                        o[f"larger_spread_of_{hi}_{lo}"] = round(s3, 5)
                        o[f"{lo}_below_{hi}_by_more_than_3_spreads"] = bool(mean[hi] - mean[lo] > 3 * s3)
                        o[f"{hi}_below_{lo}_by_more_than_3_spreads"] = bool(mean[lo] - mean[hi] > 3 * s3)

                for k, name in (("b", "replay_cost_b_minus_c"), ("d", "in_place_cost_d_minus_c"),
                                ("a", "torch_replay_cost_a_minus_c")):
                    if k in mean and "c" in mean:
                        o[name] = round(mean[k] - mean["c"], 5)
                gap("a", "b")
                gap("b", "d")
                out[kind] = o
            line = json.dumps(out)
            print(line, flush=True)
            lines.append(line)
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
