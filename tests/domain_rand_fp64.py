"""Plain restatement of the per-env parameter draw of tg_env_randomize (csrc/env_kernels.hip), for the tests.

Column i of the table f64 [12][n] is the nominal p[] of the env; the k-th randomised parameter (parameters in p[] order) is
multiplied by

    lo_k + (hi_k - lo_k) * u01d(w[2 (k & 1)], w[2 (k & 1) + 1]),
    w = Philox::draw(seed ^ (randomize_seed * 0x9E3779B97F4A7C15 mod 2^64), (key_offset + i) // key_div, 0xFFFFFFFE - k // 2, stream)

-- the key of the rollout's reset, with sub values counted down from 0xFFFFFFFE.  Every operation is one IEEE double operation
(numpy float64 rounds each of them), so the kernel's table equals this one bit for bit.  Nothing here calls the library."""
import numpy as np

import philox_fp64 as PX

GOLDEN64 = 0x9E3779B97F4A7C15
SUB_FIRST = 0xFFFFFFFE
M64 = (1 << 64) - 1


def combined_seed(seed, randomize_seed):
    return (int(seed) ^ ((int(randomize_seed) * GOLDEN64) & M64)) & M64


def factors(spec, seed, stream, n, key_offset=0, key_div=1, randomize_seed=0):
    """spec: list of (p index, lo, hi) in p[] order -> fp64 factors [len(spec)][n] of env slots 0..n-1."""
    i = np.arange(n, dtype=np.uint64)
    idx = (np.uint64(key_offset) + i) // np.uint64(key_div)
    out = np.ones((len(spec), n))
    s = combined_seed(seed, randomize_seed)
    for d in range((len(spec) + 1) // 2):
        w = PX.draw_np(s, idx, SUB_FIRST - d, stream & PX.MASK)
        for half in range(2):
            k = 2 * d + half
            if k < len(spec):
                _, lo, hi = spec[k]
                lo, hi = np.float64(lo), np.float64(hi)
                out[k] = lo + (hi - lo) * PX.u01d(w[2 * half], w[2 * half + 1])
    return out


def table(nominal, spec, seed, stream, n, key_offset=0, key_div=1, randomize_seed=0):
    """nominal: the 12 p[] values -> fp64 [12][n]: rows of un-randomised parameters hold the nominal value."""
    nominal = np.asarray(nominal, dtype=np.float64)
    tab = np.repeat(nominal[:, None], n, axis=1)
    f = factors(spec, seed, stream, n, key_offset, key_div, randomize_seed)
    for k, (r, _, _) in enumerate(spec):
        tab[r] = nominal[r] * f[k]
    return tab


def spec_of(env):
    """[(p index, lo, hi)] of an env's randomize() ranges, in p[] order."""
    rng = env.randomization or {}
    return sorted(((env.RANDOMIZABLE[k], lo, hi) for k, (lo, hi) in rng.items()), key=lambda e: e[0])
