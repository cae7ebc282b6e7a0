"""tests/resnet_oracle.py's body against the reference's own ImpalaCNNLarge
(tests/golden/resnet_body.npz, written by tests/golden/make_resnet_golden.py): the pool's padding,
the ReLU placement, the flatten order and the key names come from the reference's code."""
import os

import numpy as np

import resnet_oracle as orc
from impala_amd import resnet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_body.npz")


def test_body_matches_reference():
    g = np.load(GOLDEN)
    body = [(k, s) for k, s in resnet.param_specs(15) if ".body." in k]
    assert [k for k, _ in body] == ["model.body." + k for k in g["state_dict_keys"]]
    assert [",".join(map(str, s)) for _, s in body] == list(g["state_dict_shapes"])
    assert g["flat"].size == 97600 and resnet.param_count(15) == 630352
    flat = np.concatenate([g["flat"], np.zeros(resnet.param_count(15) - 97600, np.float32)])
    got = orc.body(orc.params(flat, 15), g["obs"]).numpy()
    rel = np.linalg.norm(got - g["out"]) / np.linalg.norm(g["out"])
    print(f"float64 oracle against the reference's fp32 output: rel-L2 {rel:.2e}")
    assert rel <= 1e-6
