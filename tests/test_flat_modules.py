"""The four flat-buffer modules (impala_amd/flat.py FlatModule) on the CPU: parameters and grads
are views of the flat buffers at their specs' offsets, and stay so through pickling, deepcopy,
clone_to and load_state_dict.  The expected layout is written out here, per class, from the spec
tables -- not read back from the module's own segment list."""
import copy
import io

import numpy as np
import pytest
import torch

from impala_amd import dqn, model, sac
from impala_amd.dqn import AtariDQNModel
from impala_amd.model import AtariPPOModel
from impala_amd.sac import SoftActor, SoftCritic

TRUNK = 77984  # three convs + LayerNorm(1024): 6176 + 32832 + 36928 + 2048 parameters

# name -> (constructor(seed), [(root attribute or None, specs, flat, grad)], has clone_to)
CASES = {
    "ppo1": (lambda s: AtariPPOModel(action_dim=1, device="cpu", seed=s),
             [(None, model.param_specs(1), "flat", "flat_grad")], True),
    "ppo15": (lambda s: AtariPPOModel(action_dim=15, device="cpu", seed=s),
              [(None, model.param_specs(15), "flat", "flat_grad")], True),
    "dqn1": (lambda s: AtariDQNModel(action_dim=1, device="cpu", seed=s),
             [("online_net", dqn.net_specs(1), "flat", "flat_grad"),
              ("target_net", dqn.net_specs(1), "target_flat", None)], True),
    "dqn15": (lambda s: AtariDQNModel(action_dim=15, device="cpu", seed=s),
              [("online_net", dqn.net_specs(15), "flat", "flat_grad"),
               ("target_net", dqn.net_specs(15), "target_flat", None)], True),
    "actor": (lambda s: (torch.manual_seed(s), SoftActor((1,), (1,), device="cpu"))[1],
              [(None, sac.actor_specs(1, 1), "flat", "flat_grad")], True),
    "critic": (lambda s: (torch.manual_seed(s), SoftCritic((1,), (1,), device="cpu"))[1],
               [(None, sac.critic_specs("critic", 1, 1), "flat", "flat_grad"),
                (None, sac.critic_specs("target_critic", 1, 1), "target_flat", None)], False),
}
ENGINES = ("_train_engine", "_infer_engine", "_engine")


def _buffers(m, segs):
    names = [f for _, _, f, _ in segs] + (["la_buf"] if isinstance(m, SoftCritic) else [])
    return {n: getattr(m, n) for n in names}


def _first_param(m, segs):
    root, specs, _, _ = segs[0]
    return (m if root is None else getattr(m, root)).get_parameter(specs[0][0])


def check_views(m, segs, requires_grad=None):
    """Item 1.  ``requires_grad``: what trainable segments must say (None: True, as built)."""
    seen = 0
    for root, specs, flat, grad in segs:
        node = m if root is None else getattr(m, root)
        buf, gbuf, off = getattr(m, flat), None if grad is None else getattr(m, grad), 0
        for name, shape in specs:
            p = node.get_parameter(name)
            assert tuple(p.shape) == tuple(shape), name
            assert p.data_ptr() == buf.data_ptr() + 4 * off, name
            if grad is None:  # a target segment
                assert not p.requires_grad and p.grad is None, name
            else:
                assert p.grad.data_ptr() == gbuf.data_ptr() + 4 * off, name
                assert tuple(p.grad.shape) == tuple(shape), name
                assert p.requires_grad == (True if requires_grad is None else requires_grad), name
            off += int(np.prod(shape))
            seen += 1
        assert off == buf.numel() and (gbuf is None or gbuf.numel() == off)
    if isinstance(m, SoftCritic):
        assert m.log_alpha.data_ptr() == m.la_buf.data_ptr()
        assert m.log_alpha.grad.data_ptr() == m.la_buf.data_ptr() + 4
        seen += 1
    assert seen == len(list(m.parameters()))  # no parameter outside the flat buffers


def check_copy(src, cp, segs, requires_grad=None):
    """Item 2: equal buffers on storage of their own, still views, writes seen through them."""
    for name, b in _buffers(src, segs).items():
        c = getattr(cp, name)
        assert torch.equal(c, b) and c.data_ptr() != b.data_ptr(), name
    check_views(cp, segs, requires_grad)
    cp.flat[0] = 7.0
    assert float(_first_param(cp, segs).detach().reshape(-1)[0]) == 7.0
    assert float(src.flat[0]) != 7.0


@pytest.mark.parametrize("case", CASES)
def test_views_alias_the_buffers(case):
    make, segs, _ = CASES[case]
    check_views(make(0), segs)


@pytest.mark.parametrize("case", CASES)
def test_pickle_deepcopy_clone_round_trips(case):
    make, segs, has_clone = CASES[case]
    m = make(0)
    if "target_flat" in _buffers(m, segs):
        m.target_flat.add_(1.0)  # (so a copy that took target from flat shows)
    for attr in ENGINES:  # a native handle's stand-in: dropped by pickling
        if hasattr(m, attr) and not callable(getattr(m, attr)):
            setattr(m, attr, object())
    f = io.BytesIO()
    torch.save(m, f)
    f.seek(0)
    m2 = torch.load(f, weights_only=False)
    check_copy(m, m2, segs)
    for attr in ENGINES:
        assert not hasattr(m2, attr) or callable(getattr(m2, attr)) or getattr(m2, attr) is None
    for attr in ENGINES:
        if hasattr(m, attr) and not callable(getattr(m, attr)):
            setattr(m, attr, None)
    d = copy.deepcopy(m)
    check_copy(m, d, segs)
    if isinstance(m, SoftActor):  # learning.py:134: the target actor's copy trains
        assert all(p.requires_grad for p in d.parameters())
    if has_clone:
        c = m.clone_to("cpu")
        assert not any(p.requires_grad for p in c.parameters())
        check_copy(m, c, segs, requires_grad=False)


@pytest.mark.parametrize("case", CASES)
def test_state_saved_before_flatmodule_restores(case):
    """A whole-model checkpoint written before FlatModule existed carries none of its own
    attributes (``_segments`` of an intermediate layout, ``downstream`` on a critic) and names
    ``_Node`` in the module that defined it then: the layout comes from the class, so such a
    state restores as views, and ``push`` / ``load_flat_from`` work on the result."""
    make, segs, _ = CASES[case]
    m = make(0)
    if isinstance(m, SoftCritic):
        with torch.no_grad():
            m.la_buf[0] = 0.5
    state = copy.deepcopy(m.__getstate__())
    for k in ("_segments", "downstream"):
        state.pop(k, None)
    old = type(m).__new__(type(m))
    old.__setstate__(state)
    check_views(old, segs)
    for name, b in _buffers(m, segs).items():
        assert torch.equal(getattr(old, name), b), name
    old.push()  # no downstream: nothing to publish
    fresh = make(1)
    fresh.load_flat_from(old)
    for name, b in _buffers(m, segs).items():
        n = 1 if name == "la_buf" else b.numel()
        assert torch.equal(getattr(fresh, name)[:n], b[:n]), name
    assert sac._Node is model._Node  # where older pickles look the class up


@pytest.mark.parametrize("case", CASES)
def test_load_state_dict_writes_through_and_bumps_version(case):
    make, segs, _ = CASES[case]
    m, m2 = make(0), make(1)
    if isinstance(m, SoftCritic):
        with torch.no_grad():
            m.la_buf[0] = 0.5
    assert not torch.equal(m.flat, m2.flat)
    before = m2._version
    m2.load_state_dict(m.state_dict())
    assert m2._version == before + 1
    for name, b in _buffers(m, segs).items():
        got = getattr(m2, name)
        n = 1 if name == "la_buf" else b.numel()  # (la_buf[1:] is grad and Adam state)
        assert torch.equal(got[:n], b[:n]) and got.data_ptr() != b.data_ptr(), name
    check_views(m2, segs)
    # an object unpickled from before the counter existed: the count restarts (from
    # nn.Module's class-level ``_version``, which the lookup then finds) and goes on counting
    del m2._version
    m2.params_changed()
    restarted = m2.__dict__["_version"]
    m2.params_changed()
    assert m2._version == restarted + 1


@pytest.mark.parametrize("seed", [0, 7])
def test_trunk_init_is_shared(seed):
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for A in (1, 15):
        p = AtariPPOModel(action_dim=A, device="cpu", seed=seed)
        q = AtariDQNModel(action_dim=A, device="cpu", seed=seed)
        assert torch.equal(bits(p.flat[:TRUNK]), bits(q.flat[:TRUNK]))
        assert torch.equal(bits(q.target_flat), bits(q.flat))
        assert q.target_flat.data_ptr() != q.flat.data_ptr()
