"""Episodes of 510 fp32 steps from the same start on the same batch: every episode must end with
finite, bitwise identical parameters and metrics.  usage: IMPALA_HIP_LIB=<lib> python tools/repro_episodes.py <episodes>"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from impala_amd.engine import Engine  # noqa: E402
from impala_amd.model import AtariPPOModel  # noqa: E402

dev = torch.device("cuda:0")
n_ep = int(sys.argv[1])
m = AtariPPOModel((3, 64, 64), 15, device=dev, dtype="fp32", seed=0)
flat0 = m.flat.clone()
batch = bench.synthetic_batch(64, 20, 15, 1234, dev)
ref = None
bad = 0
for ep in range(n_ep):
    m2 = AtariPPOModel((3, 64, 64), 15, device=dev, dtype="fp32", seed=0)
    e = Engine(m2, batch_size=64, rollout_length=20)
    snaps = []
    for s in range(510):
        e.train_step(*batch)
        if s % 51 == 50:
            snaps.append(torch.cat([m2.flat.clone(), e.metrics[:7].clone()]))
    torch.cuda.synchronize()
    snaps = torch.stack(snaps).cpu().numpy()
    e.close()
    fin = np.isfinite(snaps).all(axis=1)
    if ref is None:
        ref = snaps
    same = [bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))) for a, b in zip(snaps, ref)]
    if not fin.all() or not all(same):
        bad += 1
        print(f"episode {ep}: finite {fin.tolist()} same-as-episode-0 {same}", flush=True)
print(f"{os.environ.get('IMPALA_HIP_LIB', 'tree')}: {bad} bad of {n_ep} episodes", flush=True)
sys.exit(1 if bad else 0)
