"""The IMPALA ResNet actor-critic (include/resnet_hip.h) restated in torch float64, one function per
stage, so that a stage can be evaluated on given inputs (tests/test_gpu_resnet.py feeds each the
kernel's own exported tensors).  Activations are NCHW.  With ``quant`` the operands the kernels
keep in bf16 -- the convolutions' and the projection's weights -- are rounded as they round them.
"""
import numpy as np
import torch
import torch.nn.functional as F

from impala_amd.resnet import param_specs
from oracle.ref_stages import rne_bf16

# the body's 15 convolutions in flat order; 5 per stage: the pooled one, then conv0, conv1 of two blocks
CONV_KEYS = [k[:-len(".weight")] for k, s in param_specs(1) if len(s) == 4]


def params(flat, A, quant=False):
    """The flat fp32 buffer -> {state_dict key: float64 tensor}."""
    P, off = {}, 0
    for k, s in param_specs(A):
        n = int(np.prod(s))
        v = torch.from_numpy(np.asarray(flat[off:off + n], np.float64)).reshape(s)
        P[k] = rne_bf16(v) if quant and (len(s) == 4 or k == "model.projection.1.weight") else v
        off += n
    assert off == len(flat)
    return P


def conv(x, P, i):
    return F.conv2d(x, P[CONV_KEYS[i] + ".weight"], P[CONV_KEYS[i] + ".bias"], padding=1)


def pooled(x, P, i):
    """A stage's first convolution and its max-pool (padding -inf, as torch pads)."""
    return F.max_pool2d(conv(x, P, i), kernel_size=3, stride=2, padding=1)


def res_t(x, P, i):
    return conv(F.relu(x), P, i)


def res_x(x, t, P, i):
    return x + conv(F.relu(t), P, i)


def features(x):
    return F.relu(x).flatten(1)  # index c*64 + y*8 + x


def layer_norm(f, P):
    return F.layer_norm(f, (f.shape[1],), P["model.projection.0.weight"], P["model.projection.0.bias"], 1e-5)


def fc(y, P):
    return F.gelu(F.linear(y, P["model.projection.1.weight"], P["model.projection.1.bias"]))


def heads(h, P):
    """-> (logits [n, A], values [n])."""
    return (F.linear(h, P["model.actor.weight"], P["model.actor.bias"]),
            F.linear(h, P["model.critic.weight"], P["model.critic.bias"])[:, 0])


def body(P, obs):
    """obs u8 [n,3,64,64] -> the 2048 features, float64."""
    x = torch.as_tensor(obs).to(torch.float64) / 255
    for s in range(3):
        x = pooled(x, P, 5 * s)
        for b in (1, 3):
            x = res_x(x, res_t(x, P, 5 * s + b), P, 5 * s + b + 1)
    return features(x)


def forward(P, obs):
    return heads(fc(layer_norm(body(P, obs), P), P), P)
