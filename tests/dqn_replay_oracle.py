"""numpy float64 restatement of the dqn_replay contract (include/dqn_hip.h): the counter-based
draw, prefix-sum sampling, and the actor's n-step targets -- the latter both as the header's nested
form and as a transcription of rlax's ``n_step_bootstrapped_returns`` loop (lambda = 1)."""
import numpy as np

M64 = (1 << 64) - 1


def mix(z: int) -> int:
    """The header's mix(z) on Python ints, mod 2^64."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniforms(seed: int, counter: int, n: int) -> np.ndarray:
    """u_j = (mix(mix(seed ^ mix(counter)) + j) >> 11) * 2^-53, j < n."""
    base = mix((seed & M64) ^ mix(counter & M64))
    return np.array([(mix((base + j) & M64) >> 11) * 2.0 ** -53 for j in range(n)], dtype=np.float64)


def weights(priorities, alpha: float) -> np.ndarray:
    return np.power(np.asarray(priorities, dtype=np.float32).astype(np.float64), np.float64(alpha))


def sample(w, size: int, seed: int, counter: int, n: int):
    """-> (keys [n] i64, probabilities [n] f32, margin): the contract on weights w[0..size).
    margin is min_j |u_j * total - nearest prefix boundary| / total (inf when the total is 0): the
    distance of the inputs from the cases where summation order decides the key."""
    w = np.asarray(w, dtype=np.float64)[:size]
    u = uniforms(seed, counter, n)
    C = np.cumsum(w)
    total = C[-1]
    if not total > 0:
        keys = np.minimum(np.floor(u * size).astype(np.int64), size - 1)
        return keys, np.full(n, 1.0 / size, dtype=np.float64).astype(np.float32), np.inf
    x = u * total
    keys = np.minimum(np.searchsorted(C, x, side="right"), size - 1).astype(np.int64)
    edges = np.concatenate([[0.0], C])
    margin = float(np.min(np.abs(x[:, None] - edges[None, :]))) / total if n * size <= 4_000_000 else \
        float(min(np.min(np.abs(xi - edges)) for xi in x)) / total
    return keys, (w[keys] / total).astype(np.float32), margin


def nstep_targets(rewards, done, q_star, n_step: int, gamma: float) -> np.ndarray:
    """The header's form in float64: K = L - 1 targets; d_t = gamma (1 - done_t), v_t = q_star[t+1],
    m = min(n_step, K - t); target_t = r_t + d_t (r_{t+1} + ... d_{t+m-1} v_{t+m-1})."""
    r = np.asarray(rewards, dtype=np.float64)
    d = np.float64(gamma) * (1.0 - np.asarray(done, dtype=np.float64))
    q = np.asarray(q_star, dtype=np.float64)
    K = len(r) - 1
    out = np.empty(K, dtype=np.float64)
    for t in range(K):
        m = min(n_step, K - t)
        acc = q[t + m]
        for k in range(t + m - 1, t - 1, -1):
            acc = r[k] + d[k] * acc
        out[t] = acc
    return out


def rlax_nstep(r_t, discount_t, v_t, n: int) -> np.ndarray:
    """rlax.n_step_bootstrapped_returns(r_t, discount_t, v_t, n, lambda_t=1.) transcribed:
    bootstrap values v_t[n-1:] padded with v_t[-1], rewards padded with 0 and discounts with 1,
    then n reversed accumulation steps."""
    r_t, discount_t, v_t = (np.asarray(x, dtype=np.float64) for x in (r_t, discount_t, v_t))
    seq_len = len(r_t)
    pad = min(n - 1, seq_len)
    targets = np.concatenate([v_t[n - 1:], np.full(pad, v_t[-1])])
    r_p = np.concatenate([r_t, np.zeros(n - 1)])
    d_p = np.concatenate([discount_t, np.ones(n - 1)])
    v_p = np.concatenate([v_t, np.full(n - 1, v_t[-1])])
    lam = 1.0
    for i in reversed(range(n)):
        r_, d_, v_ = r_p[i:i + seq_len], d_p[i:i + seq_len], v_p[i:i + seq_len]
        targets = r_ + d_ * ((1.0 - lam) * v_ + lam * targets)
    return targets


def rlax_targets(rewards, done, q_star, n_step: int, gamma: float) -> np.ndarray:
    """ApexActor._async_make_replay's call: the first K steps' rewards and discounts, values
    q_star[1:]."""
    r = np.asarray(rewards, dtype=np.float64)[:-1]
    d = np.float64(gamma) * (1.0 - np.asarray(done, dtype=np.float64)[:-1])
    return rlax_nstep(r, d, np.asarray(q_star, dtype=np.float64)[1:], n_step)
