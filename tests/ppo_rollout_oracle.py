"""numpy restatement of the PPO actor's target computation (include/impala_hip.h,
impala_ppo_extend_rollout) and a float64 transcription of rlax's ``lambda_returns`` scan.

``agents/ppo/learning.py:68`` reads ``rlego.lambda_returns(r[:-1], discount_t[:-1], values[1:],
lambda)`` with ``discount_t = logical_not(d) * gamma`` and ``values`` undefined; rlego is absent,
so the line is restated on the actor's ``v`` (parity unpinned)."""
import numpy as np

F = np.float32


def lambda_returns_f32(r, done, v, gamma, lam):
    """The fp32 recurrence in the header's order, one rounding per operation -> targets [L-1]."""
    r, v = np.asarray(r, F).reshape(-1), np.asarray(v, F).reshape(-1)
    done = np.asarray(done).reshape(-1).astype(bool)
    L = r.size
    K = L - 1
    gamma, lam = F(gamma), F(lam)
    oml = F(F(1.0) - lam)
    out = np.empty(K, F)
    acc = v[K]
    for t in range(K - 1, -1, -1):
        d = F(0.0) if done[t] else gamma
        p = F(oml * v[t + 1])
        q = F(lam * acc)
        s = F(p + q)
        m = F(d * s)
        acc = F(r[t] + m)
        out[t] = acc
    return out


def rlax_lambda_returns_f64(r_t, discount_t, v_t, lam):
    """rlax.lambda_returns's reversed scan, ``acc = r + discount * ((1 - lambda) * v + lambda *
    acc)`` from ``acc = v_t[-1]``, in float64."""
    r_t, discount_t, v_t = (np.asarray(x, np.float64) for x in (r_t, discount_t, v_t))
    lam = np.ones_like(discount_t) * np.float64(lam)
    acc = v_t[-1]
    out = np.empty_like(r_t)
    for t in range(r_t.size - 1, -1, -1):
        acc = r_t[t] + discount_t[t] * ((1.0 - lam[t]) * v_t[t] + lam[t] * acc)
        out[t] = acc
    return out


def reference_f64(r, done, v, gamma, lam):
    """The reference line on fp32-valued inputs (gamma and lambda as the fp32 values the kernel
    receives), evaluated in float64 -> targets [L-1]."""
    r, v = np.asarray(r, F).astype(np.float64), np.asarray(v, F).astype(np.float64)
    disc = np.logical_not(np.asarray(done).astype(bool)) * np.float64(F(gamma))
    return rlax_lambda_returns_f64(r[:-1], disc[:-1], v[1:], np.float64(F(lam)))


def magnitude_f64(r, done, v, gamma, lam):
    """M_t: the same recurrence in float64 on |r|, |v| and |acc|."""
    return reference_f64(np.abs(np.asarray(r, F)), done, np.abs(np.asarray(v, F)), gamma, lam)


def error_bound(r, done, v, gamma, lam):
    """|fp32 - float64| <= 6 * 2^-24 * (K - t) * M_t: at most 6 roundings per step (1 - lambda,
    p, q, s, m, acc), each relative to a magnitude <= M_t, and the error carried from step t + 1
    is scaled by d * lambda <= 1."""
    M = magnitude_f64(r, done, v, gamma, lam)
    K = M.size
    return 6.0 * 2.0 ** -24 * (K - np.arange(K)) * M


def draw(rng, L, scale, done_rate):
    r = (scale * rng.standard_normal(L)).astype(F)
    v = (scale * rng.standard_normal(L)).astype(F)
    done = rng.random(L) < done_rate
    return r, done, v
