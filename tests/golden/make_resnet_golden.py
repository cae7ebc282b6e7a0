"""Generate tests/golden/resnet_body.npz FROM THE REFERENCE ITSELF (data only).

Run where the reference checkout is (see make_golden.py, whose stubs this goes through):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_resnet_golden.py

The reference's own ``ImpalaCNNLarge`` (models/common.py:64-83), constructed under torch seed 0,
runs on 2 random u8 frames divided by 255 as ``AtariActorCritic.forward`` divides them
(models/models.py:73): the fixture holds the body's state_dict (keys, and the values as one flat
fp32 vector in its order), the frames and the [2, 2048] fp32 output.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (the stubs and the reference import)


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    mg._import_reference()
    import models.common as mc  # (reference)
    torch.manual_seed(0)
    net = mc.ImpalaCNNLarge((3, 64, 64))
    sd = net.state_dict()
    obs = np.random.default_rng(0).integers(0, 256, size=(2, 3, 64, 64), dtype=np.uint8)
    with torch.no_grad():
        out = net(torch.from_numpy(obs).float() / 255.)
    assert tuple(out.shape) == (2, net.output_dim)
    np.savez_compressed(
        os.path.join(HERE, "resnet_body.npz"), obs=obs, out=out.numpy(),
        flat=torch.cat([v.reshape(-1) for v in sd.values()]).numpy(),
        state_dict_keys=np.array(list(sd.keys())),
        state_dict_shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]))
    print("resnet_body.npz written to", HERE)


if __name__ == "__main__":
    main()
