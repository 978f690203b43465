"""NumPy float32 restatement of DeviceRolloutStorage's four kernels (csrc/segment.hip; the rule of include/trajopt_grpo_hip.h,
tg_segment), and the fp64 per-row definition of GAE with the terminated / truncated split that the recurrence must equal.
g = float32(gamma), c = float32(gamma * lam) with the product formed in float64; every float32 operation is rounded on its own."""
import numpy as np

from philox_fp64 import draw_np

f32 = np.float32
U = 2.0 ** -24                          # unit roundoff of float32


def push(rew, flags, reward, terminated, truncated, final_value, gamma):
    """Row t of `rew` / `flags` for one step: a select on the flags, never a product with them."""
    with np.errstate(invalid="ignore"):
        eff = (reward + (f32(gamma) * final_value.astype(f32)).astype(f32)).astype(f32)
    rew[:] = np.where(truncated & ~terminated, eff, reward)
    flags[:] = terminated.astype(np.uint8) | (truncated.astype(np.uint8) << 1)


def gae(rew, val, flags, last_value, gamma, lam):
    """-> (adv, ret) [L][n] from [L][n] inputs and last_value [n]."""
    g, c = f32(gamma), f32(float(gamma) * float(lam))
    adv, ret = np.empty_like(rew), np.empty_like(rew)
    nxt, last = last_value.astype(f32), np.zeros_like(last_value, dtype=f32)
    for t in range(rew.shape[0] - 1, -1, -1):
        live = (flags[t] == 0).astype(f32)
        delta = ((rew[t] + ((g * nxt).astype(f32) * live).astype(f32)).astype(f32) - val[t]).astype(f32)
        last = (delta + ((c * live).astype(f32) * last).astype(f32)).astype(f32)
        adv[t], ret[t], nxt = last, (last + val[t]).astype(f32), val[t]
    return adv, ret


def gae_fp64(reward, terminated, truncated, final_value, val, last_value, gamma, lam):
    """The definition, row by row: with e the first step >= t of column i that ends an episode (or L - 1) and V[L] = last_value,
        delta_k = r_k + gamma * fv_k [truncated_k and not terminated_k] + gamma * V[k + 1] [k did not end] - V[k]
        adv[t]  = sum_{k = t .. e} (gamma lam)^(k - t) delta_k,   ret[t] = adv[t] + V[t]
    -> (adv, ret, mag, ops): mag[t] = the same sum over the magnitudes of every term, ops[t] = float32 roundings on the longest path
    from an input to adv[t] in the recurrence (6 to form a delta and its coefficients, 3 per step it is carried)."""
    L, n = reward.shape
    adv, mag, ops = np.zeros((L, n)), np.zeros((L, n)), np.zeros((L, n))
    V = np.concatenate([val.astype(np.float64), last_value.astype(np.float64)[None]])
    done = terminated | truncated
    for i in range(n):
        for t in range(L):
            w, k = 1.0, t
            while True:
                boot = gamma * float(final_value[k, i]) if truncated[k, i] and not terminated[k, i] else 0.0
                nxt = 0.0 if done[k, i] else gamma * V[k + 1, i]
                adv[t, i] += w * (float(reward[k, i]) + boot + nxt - V[k, i])
                mag[t, i] += w * (abs(float(reward[k, i])) + abs(boot) + abs(nxt) + abs(V[k, i]))
                if done[k, i] or k == L - 1:
                    break
                w, k = w * gamma * lam, k + 1
            ops[t, i] = 6 + 3 * (k - t + 1)
    return adv, adv + V[:L], mag, ops


def gae_bound(mag, ops, val):
    """|float32 result - definition| <= gamma_K * (sum of magnitudes), K = ops roundings (Higham's gamma_K = K u / (1 - K u)): every
    term reaches adv[t] through at most K float32 operations, each with relative error <= u.  ret adds one rounding and |V[t]|."""
    bound = lambda K, m: K * U / (1.0 - K * U) * m
    return bound(ops, mag), bound(ops + 1, mag + np.abs(val.astype(np.float64)))


def permute_bits(rows):
    bits = 2
    while (1 << bits) < rows:
        bits += 2
    return bits


def permutation(rows, seed, ordinal):
    """-> (idx int64 [rows], the longest cycle walk).  Four Feistel rounds on permute_bits(rows) bits, round function = word 0 of
    Philox(key seed, counter (half, round, ordinal lo, ordinal hi)) masked to half the bits; walk until the value is < rows."""
    half = permute_bits(rows) // 2
    mask = np.uint64((1 << half) - 1)
    y = np.arange(rows, dtype=np.uint64)
    todo, walks = np.ones(rows, bool), 0
    while todo.any():
        l, r = y[todo] >> np.uint64(half), y[todo] & mask
        for rnd in range(4):
            w = draw_np(seed, (np.uint64(rnd) << np.uint64(32)) | r, ordinal & 0xFFFFFFFF, (ordinal >> 32) & 0xFFFFFFFF)[0]
            l, r = r, l ^ (np.asarray(w, dtype=np.uint64) & mask)
        y[todo] = (l << np.uint64(half)) | r
        todo, walks = y >= np.uint64(rows), walks + 1
    return y.astype(np.int64), walks
