"""The IMPALA ResNet learner step on the GPU (include/resnet_hip.h: resnet_loss_head, resnet_compute_grads,
resnet_apply_update, resnet_train_step) against float64: tests/resnet_oracle.py's network,
oracle/ref_cpu.py's loss and torch's clip_grad_norm_ and Adam.

Shapes (B, T, A): (1, 2, 15) L = 1 and one live wave of four; (3, 5, 2) a partial workgroup and an Adam
tail of 3 floats; (5, 4, 6) a second workgroup, tail of 3; (1, 64, 15) a full wave, 63 sweeps; (2, 20, 15)
the product's T.  The case builder asserts what the inputs must contain: a discount of 0 among the
T - 1 frames the V-trace reads, rho on both sides of the clip thresholds (all 1) -- among those frames
where there is more than one of them, else (L = 1, B = 1) among the trajectory's two -- and a
piecewise constant frame 0.

Bounds.  Loss head: stage_checks' F32_NORMWISE on (dlogits | dvalues) and hold_metrics, from the
kernel's own heads.  Pre-clip gradient: test_gpu_resnet_backward.py's max(1e-4, 4 s).  Three steps: the
parameters max |d| <= max(2e-6, 4 x the distance of the same steps in torch float32 on the CPU from
float64); the grad norm, a metric, relative max(stage_checks.MET_RTOL, 4 x that stand-in's).

The reference's near-ties.  A max-pool's and a ReLU's derivative jump where two values of a window change
order or a value changes sign, and the fp32 forward is F32_NORMWISE from float64: at 64 frames one pool
window of 1.7 million has its two largest values 2.8e-8 apart, and the float64 and the fp32 network route
its gradient to different pixels (the eleven tensors below it then differ by 3e-4 .. 1e-3, the CPU float32
stand-in's too).  The float64 (and stand-in) network therefore takes the kernel's pool winner where that
tap's value is within F32_NORMWISE of the window's maximum, and the kernel's ReLU mask where |x| is within
F32_NORMWISE of 0 (_pool, _relu, from the step's own amax and saved tensors), and asserts that everywhere
else the kernel's winners and masks are torch's.  With that the stand-in's s is below 1e-6 for every
tensor, so the gradient bound is 1e-4 throughout.  Measured on an MI355X: every gradient tensor within 0.04
of its bound; three steps 1.6e-7 .. 2.4e-7 (stand-in 1.6e-7 .. 2.4e-7), grad norm 1.5e-8 .. 2.4e-7 relative.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_oracle as orc
import stage_checks as sc
from oracle import ref_cpu
from oracle import ref_stages as rs
from oracle.vtrace import GRAD_MODES, mode_kwargs

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, 15), (3, 5, 2), (5, 4, 6), (1, 64, 15), (2, 20, 15)]
STEP3 = [SHAPES[1], SHAPES[4]]
DTYPES = ["fp32", "bf16"]
NO_CLIP = 1e6
F64, F32 = torch.float64, torch.float32


def _pool(c, win):
    """max_pool2d(3, 2, 1) of c [n,C,H,H] -> (the pooled tensor, the windows whose kernel winner is no maximum).
    A max-pool's derivative jumps where two values of a window change order, and the fp32 forward's values are
    F32_NORMWISE from float64's: where the tap the kernel took (win u8 [n,H/2,H/2,C], 0..8 row-major) holds a
    value within that bound of the window's maximum, the gradient goes where the kernel sent it; anywhere
    else the kernel's winner must be torch's."""
    out, idx = F.max_pool2d(c, 3, 2, 1, return_indices=True)
    if win is None:
        return out, 0
    H, w = c.shape[2], torch.from_numpy(win.astype(np.int64)).permute(0, 3, 1, 2)
    o = torch.arange(H // 2)
    ky, kx = 2 * o[:, None] + w // 3 - 1, 2 * o[None, :] + w % 3 - 1
    kidx = ky.clamp(min=0) * H + kx.clamp(min=0)
    cd = c.detach()
    kval = cd.flatten(2).gather(2, kidx.flatten(2)).reshape(out.shape)
    near = (ky >= 0) & (kx >= 0) & (out.detach() - kval <= sc.F32_NORMWISE * (kval.abs() + cd.pow(2).mean().sqrt()))
    idx = torch.where(near, kidx, idx)
    return c.flatten(2).gather(2, idx.flatten(2)).reshape(out.shape), int((idx != kidx).sum())


def _relu(x, sav):
    """relu(x) -> (it, the elements where the kernel's mask is wrong).  As _pool: where |x| is within
    F32_NORMWISE of 0 the mask is the kernel's, [its saved tensor sav [n,H,H,C] > 0]; elsewhere they must agree."""
    m = x.detach() > 0
    if sav is None:
        return x * m, 0
    k, xd = torch.from_numpy(sav).permute(0, 3, 1, 2) > 0, x.detach()
    m = torch.where(xd.abs() <= sc.F32_NORMWISE * xd.pow(2).mean().sqrt(), k, m)
    return x * m, int((m != k).sum())


def _net(P, obs, dt, kern=None, off=None):
    """-> (logits, values); kern: the kernel's (pool winners, saved stage tensors) of the same step, which
    decide the pools' and the ReLUs' near-ties; off: a list that takes the counts of disagreements elsewhere."""
    wins, sav = kern or (None, [None] * 15)
    off = [] if off is None else off

    def conv(x, i):  # conv i of relu(stage tensor i - 1)
        r, bad = _relu(x, sav[i - 1])
        off.append(bad)
        return orc.conv(r, P, i)
    x = obs.to(dt) / 255
    for s in range(3):
        x, bad = _pool(orc.conv(x, P, 5 * s), None if wins is None else wins[s])
        off.append(bad)
        for b in (1, 3):
            x = x + conv(conv(x, 5 * s + b), 5 * s + b + 1)
    f, bad = _relu(x, sav[14])
    off.append(bad)
    return orc.heads(orc.fc(orc.layer_norm(f.flatten(1), P), P), P)


def _loss(lg, v, batch, dt):
    """learning.py:144-159 on logits [B,T,A], values [B,T] -> (loss, rho)."""
    _, a, r, g, mu = batch
    pi, pim = (torch.distributions.Categorical(logits=x) for x in (lg, mu.to(dt)))
    rho = torch.exp(pi.log_prob(a) - pim.log_prob(a))
    adv, err, _ = ref_cpu.batched_vtrace(v[:, :-1], v[:, 1:], r.to(dt)[:, :-1], g.to(dt)[:, :-1], rho[:, :-1],
                                         **mode_kwargs("sg_advantage"))
    return -(pi.log_prob(a)[:, :-1] * adv).mean() + err.pow(2).mean() - 0.01 * pi.entropy().mean(), rho


@functools.lru_cache(maxsize=None)
def _case(B, T, A):
    """(flat fp32 parameters as test_gpu_resnet.py makes them, the batch as CPU tensors)."""
    from impala_amd.resnet import param_specs, resnet_init_flat
    torch.manual_seed(0)
    flat, off = resnet_init_flat(A).numpy().copy(), 0
    rng = np.random.default_rng(3)
    for _, s in param_specs(A):
        k = int(np.prod(s))
        if len(s) == 1:
            flat[off:off + k] += (0.05 * rng.standard_normal(k)).astype(np.float32)
        off += k
    obs = rng.integers(0, 256, size=(B, T, 3, 64, 64), dtype=np.uint8)
    obs[0, 0] = np.kron(rng.integers(0, 256, size=(3, 8, 8), dtype=np.uint8), np.ones((8, 8), np.uint8))
    act = rng.integers(0, A, size=(B, T), dtype=np.int64)
    rew = rng.standard_normal((B, T)).astype(np.float32)
    disc = np.full((B, T), 0.99, np.float32)
    disc[:, (T - 1) // 2] = 0
    with torch.no_grad():
        lg = _net(orc.params(flat, A), torch.from_numpy(obs).flatten(0, 1), F64)[0].reshape(B, T, A)
    # behaviour logits: the policy's, a little off, and at the action taken 0.7 down (rho > 1) or up by turns
    mu = (lg.numpy() + 0.1 * rng.standard_normal((B, T, A))).astype(np.float32)
    turn = np.where(np.arange(B * T).reshape(B, T) % 2 == 0, -0.7, 0.7).astype(np.float32)
    np.put_along_axis(mu, act[..., None], np.take_along_axis(mu, act[..., None], -1) + turn[..., None], -1)
    batch = tuple(torch.from_numpy(x) for x in (obs, act, rew, disc, mu))
    rho = _loss(lg, torch.zeros(B, T, dtype=F64), batch, F64)[1]
    seen = rho[:, :-1] if B * (T - 1) > 1 else rho
    assert (disc[:, :-1] == 0).any() and bool((seen > 1).any() and (seen < 1).any())
    assert (obs[0, 0].reshape(3, 8, 8, 8, 8) == obs[0, 0][:, ::8, ::8][:, :, None, :, None]).all()
    return flat, batch


@functools.lru_cache(maxsize=None)
def _ref(case, dt, max_norm, steps):
    """The steps in torch on the CPU, every step's near-ties decided as _pool and _relu say by the same step
    of _steps -> (parameters after them, the first step's pre-clip gradient per key, every step's
    gradient norm)."""
    from impala_amd.resnet import param_specs
    B, T, A = case
    flat, batch = _case(*case)
    kern, off = _steps(case, max_norm, steps)["kern"], []
    P = {k: v.to(dt).requires_grad_() for k, v in orc.params(flat, A).items()}
    opt, norms, g1 = torch.optim.Adam(P.values(), lr=1e-4, eps=1e-5), [], None
    for i in range(steps):
        opt.zero_grad()
        lg, v = _net(P, batch[0].flatten(0, 1), dt, kern[i], off)
        _loss(lg.reshape(B, T, A), v.reshape(B, T), batch, dt)[0].backward()
        g1 = g1 or {k: P[k].grad.to(F64).numpy().copy() for k, _ in param_specs(A)}
        norms.append(float(torch.nn.utils.clip_grad_norm_(P.values(), max_norm)))
        opt.step()
    assert not any(off), off  # away from the near-ties every pool winner and ReLU mask of the kernel's is torch's
    return torch.cat([P[k].detach().reshape(-1) for k, _ in param_specs(A)]).to(F64).numpy(), g1, norms


def _engine(case, dtype, **kw):
    from impala_amd.resnet import ImpalaResNetModel
    B, T, A = case
    model = ImpalaResNetModel((3, 64, 64), A, "cuda", seed=0, train_batch=B * T, train_dtype=dtype)
    model.flat.copy_(torch.from_numpy(_case(*case)[0]))
    model.params_changed()
    eng = model.train_engine()
    eng.step_init(B, T, **kw)
    return eng, [t.cuda() for t in _case(*case)[1]]


@functools.lru_cache(maxsize=None)
def _steps(case, max_norm, steps):
    """`steps` fp32 steps as resnet_compute_grads + resnet_apply_update (bitwise resnet_train_step:
    test_one_call_is_its_parts) -> the first step's pre-clip gradient, every step's pool winners (u8
    [n,HO,HO,C] per pool) and saved stage tensors, the parameters and the metrics after the last."""
    eng, dev = _engine(case, "fp32", max_grad_norm=max_norm)
    n, o = case[0] * case[1], dict(kern=[], pre=None)
    for _ in range(steps):
        eng.compute_grads(*dev)
        o["pre"] = eng.model.flat_grad.cpu().numpy().copy() if o["pre"] is None else o["pre"]
        a = eng.debug_tensor("amax", n).view(np.uint8).reshape(n, -1)
        o["kern"].append(([a[:, lo:hi].reshape(n, h, h, c) for lo, hi, h, c in
                           ((0, 16384, 32, 16), (16384, 24576, 16, 32), (24576, 26624, 8, 32))],
                          [eng.debug_tensor(f"s{i}", n) for i in range(15)]))
        eng.apply_update()
    return dict(o, params=eng.model.flat.cpu().numpy().astype(np.float64), met=eng.metrics.cpu().numpy())


def _state(eng):
    return {k: t.cpu().numpy().copy() for k, t in dict(
        params=eng.model.flat, grads=eng.model.flat_grad, m=eng.exp_avg, v=eng.exp_avg_sq, met=eng.metrics).items()}


@functools.lru_cache(maxsize=None)
def _runs(case, dtype, mode="sg_advantage"):
    """One step from the same state three ways: resnet_train_step; resnet_compute_grads then
    resnet_apply_update; forward_train, loss_head, backward on the exported cotangents, apply_update."""
    from impala_amd.resnet import ResnetEngine
    B, T, A = case
    n, o = B * T, {}
    eng, dev = _engine(case, dtype, vtrace_grad_mode=mode)
    eng.train_step(*dev)
    o["one"] = _state(eng)
    o["after"] = [[t.cpu().numpy() for t in e.forward(dev[0].flatten(0, 1))]
                  for e in (eng, ResnetEngine(eng.model, n, dtype))]
    eng, dev = _engine(case, dtype, vtrace_grad_mode=mode)
    eng.compute_grads(*dev)
    o["pre"] = eng.model.flat_grad.cpu().numpy().copy()
    eng.apply_update()
    o["two"] = _state(eng)
    eng, dev = _engine(case, dtype, vtrace_grad_mode=mode)
    o["vt"] = eng.debug_vtrace()
    eng.forward_train(dev[0].flatten(0, 1))
    eng.loss_head(*dev)
    o.update(heads=eng.debug_tensor("heads", n), dl=eng.debug_tensor("dlogits", n), dv=eng.debug_tensor("dvalues", n))
    eng.backward(torch.from_numpy(o["dl"]), torch.from_numpy(o["dv"]), out=eng.model.flat_grad)
    eng.apply_update()
    o["parts"] = _state(eng)
    return o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,mode", [(c, GRAD_MODES[0]) for c in SHAPES] + [(SHAPES[2], m) for m in GRAD_MODES[1:]])
def test_loss_head_against_float64(case, mode, dtype):
    from impala_amd.engine import vtrace
    (B, T, A), o, batch = case, _runs(case, dtype, mode), _case(*case)[1]
    hd = o["heads"].reshape(B, T, 16)
    r = ref_cpu.loss_from_outputs(hd[..., :A], hd[..., 15], *[x.numpy() for x in batch[1:]], grad_mode=mode, dtype=F64)
    logpa = torch.log_softmax(torch.from_numpy(hd[..., :A]).double(), -1).gather(-1, batch[1][..., None])[..., 0]
    r["pg_abs"] = float((logpa[:, :-1] * torch.from_numpy(r["adv"])).abs().mean())
    d = rs.f32_figures(np.concatenate([o["dl"], o["dv"][:, None]], 1),
                       np.concatenate([r["dlogits"].reshape(-1, A), r["dvalues"].reshape(-1, 1)], 1))
    print(f"{case} {dtype} {mode}: dlogits | dvalues normwise {d:.2e}")
    bad = sc.hold_metrics(o["parts"]["met"][:6], {"met": r}, f"{case} {dtype} {mode}")
    assert d <= sc.F32_NORMWISE and not bad, (d, bad)
    # the V-trace outputs: bitwise impala_vtrace on the exported values and rho
    L, vt = T - 1, o["vt"]
    adv, err, q = vt[:3 * B * L].reshape(3, B, L)
    rho, v = vt[3 * B * L:].reshape(B, T), torch.from_numpy(hd[..., 15]).cuda()
    rew, disc = batch[2].cuda(), batch[3].cuda()
    want = vtrace(v[:, :-1], v[:, 1:], rew[:, :-1], disc[:, :-1], rho[:, :-1])
    assert all(torch.equal(a, b) for a, b in zip((adv, err, q), want))
    assert np.allclose(rho.cpu().numpy(), r["rho"], rtol=1e-5)


@pytest.mark.parametrize("case", SHAPES)
def test_gradient_against_float64(case):
    from impala_amd.resnet import param_specs
    steps = 3 if case in STEP3 else 1
    g, off, bad = np.asarray(_steps(case, 0.5, steps)["pre"], np.float64), 0, []
    assert np.array_equal(g, _runs(case, "fp32")["pre"])
    g64, g32 = _ref(case, F64, 0.5, steps)[1], _ref(case, F32, 0.5, steps)[1]
    for k, shape in param_specs(case[2]):
        s = rs.rel_l2(g32[k], g64[k])
        bound, d = max(sc.BLOCK_RL2, 4 * s), rs.rel_l2(g[off:off + g64[k].size].reshape(shape), g64[k])
        print(f"{k:44s} rel-L2 {d:.2e} = {d / bound:.3f} of the bound (float32 stand-in {s / bound:.3f})")
        if not d <= bound:
            bad.append(f"{k}: {d:.2e} > {bound:.1e}")
        off += g64[k].size
    assert off == g.size and not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SHAPES)
def test_one_call_is_its_parts(case, dtype):
    o = _runs(case, dtype)
    for k, x in o["one"].items():
        assert np.array_equal(x, o["two"][k]) and np.array_equal(x, o["parts"][k]), k
    assert o["one"]["met"][7] == 1 and o["one"]["met"][8] == 0
    assert not np.array_equal(o["one"]["params"], _case(*case)[0])
    (lg, v), (lg_fresh, v_fresh) = o["after"]  # the step re-packed the weights it updated
    assert np.array_equal(lg, lg_fresh) and np.array_equal(v, v_fresh)


@pytest.mark.parametrize("max_norm", [0.5, NO_CLIP])
@pytest.mark.parametrize("case", STEP3)
def test_three_steps_against_float64(case, max_norm):
    p64, _, n64 = _ref(case, F64, max_norm, 3)
    p32, _, n32 = _ref(case, F32, max_norm, 3)
    assert all(n > 0.5 + 1e-3 for n in n64) if max_norm == 0.5 else all(n < NO_CLIP for n in n64)
    o = _steps(case, max_norm, 3)
    got, norm = o["params"], float(o["met"][6])
    d, s = np.abs(got - p64).max(), np.abs(p32 - p64).max()
    dn, sn = abs(norm - n64[2]) / n64[2], abs(n32[2] - n64[2]) / n64[2]
    print(f"{case} max_norm {max_norm}: params max |d| {d:.2e} (float32 stand-in {s:.2e}), "
          f"grad norm rel {dn:.2e} (stand-in {sn:.2e}); float64 norms {n64}")
    assert o["met"][7] == 3
    assert d <= max(2e-6, 4 * s) and dn <= max(sc.MET_RTOL, 4 * sn)


def test_builder_learner_interface():
    from impala_amd import _lib
    from impala_amd.builder import ImpalaResNetBuilder
    from impala_amd.config import load_config
    B, T, A = 2, 3, 15
    traj = ref_cpu.to_trajectories(*[x.numpy() for x in _case(B, T, A)[1]])

    class Replay:
        warm_up = staticmethod(lambda n: None)
        sample = staticmethod(lambda b: (None, traj, None))

    def learner():
        b = ImpalaResNetBuilder(load_config({"agent": {"batch_size": B, "rollout_length": T},
                                             "learner": {"dtype": "fp32"}}, agent="impala_resnet"))
        torch.manual_seed(0)
        return b.make_learner(b.make_network(None), Replay())

    one, two = learner(), learner()
    met = one.train_step()
    assert set(_lib.METRIC_NAMES) <= set(met) and all(np.isfinite(float(met[k])) for k in _lib.METRIC_NAMES)
    two._model.flat.zero_()
    two.load_state_dict(one.state_dict())
    m1, m2 = one.train_step(), two.train_step()
    assert all(float(m1[k]) == float(m2[k]) for k in _lib.METRIC_NAMES)
    assert float(one.engine.metrics[7]) == 2 == float(two.engine.metrics[7])
    assert torch.equal(one._model.flat, two._model.flat) and torch.equal(one.engine.exp_avg_sq, two.engine.exp_avg_sq)


def test_refusals():
    import ctypes as C
    from impala_amd import _lib
    from impala_amd.resnet import ResnetEngine
    eng, dev = _engine(SHAPES[1], "fp32")
    eng._fresh()
    L, sp = _lib.lib(), _lib.stream_ptr(None)
    b = C.byref(eng._batch(*dev))
    fresh = ResnetEngine(eng.model, 15, "fp32", train=True)
    fresh._fresh()
    assert L.resnet_train_step(fresh._h, b, sp) == 1002  # no resnet_step_init
    cfg = _lib.ResnetStepConfig()
    L.resnet_step_config_default(C.byref(cfg))
    cfg.batch_size, cfg.rollout_length = 4, 4
    assert L.resnet_step_init(fresh._h, C.byref(cfg)) == 1001  # B T > batch_size
    cfg.batch_size, cfg.rollout_length = 3, 5
    assert L.resnet_step_init(fresh._h, C.byref(cfg)) == 0
    assert L.resnet_train_step(fresh._h, b, sp) == 1002 and L.resnet_apply_update(fresh._h, sp) == 1002  # unbound
    assert L.resnet_step_init(ResnetEngine(eng.model, 15, "fp32")._h, C.byref(cfg)) == 1001  # train = 0
    assert L.resnet_loss_head(eng._h, b, sp) == 1002  # no resnet_forward_train
    torch.cuda.synchronize()
    assert not eng.model.flat_grad.any() and float(eng.metrics.abs().sum()) == 0  # nothing was launched
