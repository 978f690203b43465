"""NumPy restatement of the privileged critic's row contract (tg_privileged_rows, include/trajopt_grpo_hip.h), operation by operation.

A feature of a multiplicative factor f on [lo, hi] is x = (f - c) * s with c = 0.5 * (lo + hi), s = 2 / (hi - lo) (0 for hi == lo), both
Python floats computed once.  The kernel reads the table value t = nominal * f and forms ((t / nominal) - c) * s: an IEEE f64 divide, a
subtract and a multiply, each rounded on its own (NumPy float64 arrays round every operation), then ONE rounding to f32 and, on bf16
rows, one more to bf16 with round-to-nearest-even.  Row r: columns [0, S) keep the BITS of the source row, column S + k is feature k of
env e = idx[r] % n (e = r without idx), every other column is 0 except a 1 in ones_col (-1: none)."""
import numpy as np


def center_scale(ranges):
    """([c_k], [s_k]) of {name: (lo, hi)} in the mapping's order, in Python floats."""
    c = [0.5 * (float(lo) + float(hi)) for lo, hi in ranges.values()]
    s = [2.0 / (float(hi) - float(lo)) if float(hi) > float(lo) else 0.0 for lo, hi in ranges.values()]
    return c, s


def features_of_factors(factors, center, scale):
    """f32 [..., P] of factors [..., P]: (f - c) * s in f64, two roundings, then one to f32 (policy.value / forward's host path)."""
    f = np.asarray(factors, dtype=np.float64)
    d = f - np.asarray(center, dtype=np.float64)
    return (d * np.asarray(scale, dtype=np.float64)).astype(np.float32)


def features_of_table(ptab, env, index, nominal, center, scale):
    """f32 [rows][P] of the f64 [12][n] table for the env of each row: ((t / nominal) - c) * s, three f64 roundings, one to f32."""
    ptab = np.asarray(ptab, dtype=np.float64)
    t = ptab[np.asarray(index, dtype=np.int64)][:, np.asarray(env, dtype=np.int64)].T          # [rows][P]
    q = t / np.asarray(nominal, dtype=np.float64)
    d = q - np.asarray(center, dtype=np.float64)
    return (d * np.asarray(scale, dtype=np.float64)).astype(np.float32)


def bf16_bits(x):
    """uint16 bf16 bit patterns of f32 values, round to nearest even (NaN is not expected here)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_round(x):
    """f32 values rounded to the nearest bf16 (ties to even), as f32."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def rows(src_bits, S, idx, n, ptab, index, nominal, center, scale, dst_pad, bf16, ones_col):
    """The destination rows as BIT patterns: uint32 [rows][dst_pad] for f32 rows, uint16 for bf16 rows.  src_bits: the source rows'
    bit patterns [rows][src_pad] of the same width; idx int64 [rows] (flat t * n + e) or None (row r is env r)."""
    src_bits = np.asarray(src_bits)
    R, P = src_bits.shape[0], len(index)
    assert src_bits.dtype == (np.uint16 if bf16 else np.uint32) and S + P <= dst_pad and S <= src_bits.shape[1]
    assert ones_col == -1 or S + P <= ones_col < dst_pad
    env = np.arange(R, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64) % int(n)
    x = features_of_table(ptab, env, index, nominal, center, scale)
    out = np.zeros((R, dst_pad), dtype=src_bits.dtype)                                          # +0.0 in either format
    out[:, :S] = src_bits[:, :S]
    out[:, S:S + P] = bf16_bits(x) if bf16 else x.view(np.uint32)
    if ones_col >= 0:
        out[:, ones_col] = 0x3F80 if bf16 else 0x3F800000
    return out
