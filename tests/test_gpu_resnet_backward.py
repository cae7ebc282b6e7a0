"""The IMPALA ResNet backward pass on the GPU (include/resnet_hip.h: resnet_forward_train,
resnet_backward) against float64 autograd through tests/resnet_oracle.py.

Shapes: n = 1 a lone frame; n = 3 an odd count below the workgroup count; n = 17 one full 16-row
projection tile and a one-row tail; batch_size 17.  Parameters as test_gpu_resnet.py's; frame 0 is
made of 8 x 8 blocks of one colour each, so that pool windows hold equal values and ReLU inputs
repeat.  Each of the 38 parameter tensors is held by rel-L2 to max(1e-4, 4 s): 1e-4 is
stage_checks.BLOCK_RL2, s that tensor's distance between the same oracle run in torch float32 on the
CPU and the float64 one (the stem's weight gradient sums 17 x 4096 rows, more than BLOCK_RL2 was set
for).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resnet_oracle as orc
from impala_amd import _lib
from oracle import ref_stages as rs
from stage_checks import BLOCK_RL2
from test_gpu_resnet import _inputs

pytestmark = pytest.mark.gpu
BATCH = 17
CASES = [(1, 15), (3, 2), (17, 6)]


@functools.lru_cache(maxsize=None)
def _case(n, A):
    """(obs u8 [n,3,64,64] on the device, dlogits [n,A], dvalues [n])."""
    obs = _inputs(A)[2][:n].clone()
    rng = np.random.default_rng(11)
    blocks = torch.from_numpy(rng.integers(0, 256, size=(3, 8, 8), dtype=np.uint8))
    obs[0] = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2).cuda()
    g = torch.Generator().manual_seed(5)
    return obs, torch.randn(n, A, generator=g), torch.randn(n, generator=g)


def _oracle(A, obs, dl, dv):
    """{key: (float64 gradient, bound, s)} from autograd through the oracle in float64 and float32."""
    from impala_amd.resnet import param_specs
    flat = _inputs(A)[1]
    grads = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.to(dt).requires_grad_() for k, v in orc.params(flat, A).items()}
        x = obs.cpu().to(dt) / 255
        for s in range(3):
            x = orc.pooled(x, P, 5 * s)
            for b in (1, 3):
                x = orc.res_x(x, orc.res_t(x, P, 5 * s + b), P, 5 * s + b + 1)
        lg, v = orc.heads(orc.fc(orc.layer_norm(orc.features(x), P), P), P)
        ((lg * dl.to(dt)).sum() + (v * dv.to(dt)).sum()).backward()
        grads[dt] = {k: P[k].grad.to(torch.float64).numpy() for k, _ in param_specs(A)}
    out = {}
    for k, _ in param_specs(A):
        s = rs.rel_l2(grads[torch.float32][k], grads[torch.float64][k])
        out[k] = (grads[torch.float64][k], max(BLOCK_RL2, 4 * s), s)
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, A):
    return _oracle(A, *_case(n, A))


def _hold(flat_grad, ref, A):
    from impala_amd.resnet import param_specs
    off, bad = 0, []
    g = np.asarray(flat_grad, np.float64)
    for k, shape in param_specs(A):
        r, bound, s = ref[k]
        d = rs.rel_l2(g[off:off + r.size].reshape(shape), r)
        print(f"{k:44s} rel-L2 {d:.2e} = {d / bound:.3f} of the bound (float32 stand-in {s / bound:.3f})")
        if not d <= bound:
            bad.append(f"{k}: {d:.2e} > {bound:.1e}")
        off += r.size
    assert off == g.size and not bad, bad


@functools.lru_cache(maxsize=None)
def _run(n, A):
    from impala_amd.resnet import ResnetEngine
    model = _inputs(A)[0]
    obs, dl, dv = _case(n, A)
    eng = ResnetEngine(model, BATCH, "fp32", train=True)
    o = dict(fwd=[t.cpu().numpy() for t in ResnetEngine(model, BATCH, "fp32").forward(obs)])
    o["train"] = [t.cpu().numpy() for t in eng.forward_train(obs)]
    o["grad"] = eng.backward(dl, dv).cpu().numpy()
    eng.forward_train(obs)
    o["again"] = eng.backward(dl, dv).cpu().numpy()
    preset = torch.randn(model.flat.numel(), generator=torch.Generator().manual_seed(9))
    buf = preset.cuda()
    o["acc"] = eng.backward(dl, dv, out=buf, accumulate=True).cpu().numpy()
    o["sum"] = (preset + torch.from_numpy(o["grad"])).numpy()
    return o


@pytest.mark.parametrize("n,A", CASES)
def test_gradient_against_float64(n, A):
    _hold(_run(n, A)["grad"], _reference(n, A), A)


@pytest.mark.parametrize("n,A", CASES)
def test_bits(n, A):
    o = _run(n, A)
    assert np.array_equal(o["train"][0], o["fwd"][0]) and np.array_equal(o["train"][1], o["fwd"][1])
    assert np.array_equal(o["grad"], o["again"])
    assert np.array_equal(o["acc"], o["sum"])


def test_public_interface():
    from impala_amd.resnet import ImpalaResNetModel
    A = 6
    model = ImpalaResNetModel((3, 64, 64), A, "cuda", seed=0, train_batch=BATCH)
    model.flat.copy_(_inputs(A)[0].flat)
    model.params_changed()
    obs17, dl17, dv17 = _case(17, A)
    obs = torch.cat([obs17, obs17[:3]])
    dl, dv = torch.cat([dl17, dl17[:3]]), torch.cat([dv17, dv17[:3]])
    ref = _oracle(A, obs, dl, dv)
    dl, dv = dl.cuda(), dv.cuda()

    def step():
        logits, values = model.forward_train(obs)
        ((logits * dl).sum() + (values[:, 0] * dv).sum()).backward()
        return torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    model.flat_grad.zero_()
    g1 = step()
    _hold(g1, ref, A)
    assert np.array_equal(g1, model.flat_grad.cpu().numpy())
    assert np.array_equal(step(), g1 + g1)
    assert not any(t.requires_grad for t in model.forward(obs[:3]))


def test_refusals():
    from impala_amd.resnet import ResnetEngine, default_config
    model = _inputs(6)[0]
    obs, dl, dv = _case(3, 6)
    L, sp = _lib.lib(), _lib.stream_ptr(None)
    dl, dv, g = dl.cuda(), dv.cuda(), torch.zeros(model.flat.numel(), device="cuda")
    bwd = lambda e, n: L.resnet_backward(e._h, _lib.ptr(obs), n, _lib.ptr(dl), _lib.ptr(dv), _lib.ptr(g), 0, sp)  # noqa: E731
    e = ResnetEngine(model, BATCH, "fp32", train=True)
    e._fresh()
    assert bwd(e, 3) == 1001  # no resnet_forward_train yet
    e.forward_train(obs)
    assert bwd(e, 2) == 1001  # another n
    plain = ResnetEngine(model, BATCH, "fp32")
    plain.forward(obs)
    assert bwd(plain, 3) == 1001  # a train = 0 handle
    torch.cuda.synchronize()
    assert not g.any()  # nothing was launched
    cfg, h = default_config(), C.c_void_p()
    cfg.train, cfg.dtype = 1, 1
    assert L.resnet_create(C.byref(cfg), 0, C.byref(h)) == 1001 and not h
