"""NumPy restatement of the prioritised replay tree (csrc/replay_prio.hip; include/trajopt_grpo_hip.h, tg_replay_prio): the level
layout, the butterfly node sum, the Kogge-Stone scan and the descent, every float32 add in the kernels' order.  Nothing here calls
the library."""
import numpy as np

import philox_fp64 as P

F32 = np.float32


def levels(rows):
    """[(offset, size)] of every level, leaves first, and the floats of the allocation: every level padded to a multiple of 64."""
    out, n, off = [], int(rows), 0
    while True:
        out.append((off, n))
        off += -(-n // 64) * 64
        if n == 1 and len(out) > 1:
            return out, off
        n = -(-n // 64)


def node_sum(children):
    """float32 [.., 64] -> [..]: s[i] += s[i + 32], then strides 16, 8, 4, 2, 1."""
    s = np.asarray(children, dtype=F32)
    for d in (32, 16, 8, 4, 2, 1):
        s = (s[..., :d] + s[..., d:2 * d]).astype(F32)
    return s[..., 0]


def scan(children):
    """float32 [.., 64] -> the inclusive prefix by Kogge-Stone: for d = 1, 2, .., 32: x[i] += x[i - d] for i >= d."""
    x = np.array(children, dtype=F32)
    for d in (1, 2, 4, 8, 16, 32):
        x[..., d:] = (x[..., d:] + x[..., :-d].copy()).astype(F32)
    return x


def build(leaves):
    """Every level of the tree over `leaves`, each zero-padded to a multiple of 64: [leaves, level 1, .., root]."""
    tree, cur = [], np.asarray(leaves, dtype=F32)
    for l, (_, n) in enumerate(levels(len(leaves))[0]):
        cur = node_sum(tree[-1].reshape(-1, 64)) if l else cur
        tree.append(np.concatenate([cur, np.zeros(-n % 64, F32)]))
    return tree


def descend(tree, seed, ordinal, B):
    """The rows tg_replay_prio_sample draws from `tree` (build()'s, or the device's own levels): int64 [B]."""
    b = np.arange(B, dtype=np.uint64)
    w = P.draw_np(seed, b, (ordinal >> 32) & P.MASK, ordinal & P.MASK)
    t = (b.astype(np.float64) + P.u01d(w[0], w[1])) / np.float64(B) * np.float64(tree[-1][0])
    node = np.zeros(B, np.int64)
    for level in tree[-2::-1]:
        child = level.reshape(-1, 64)[node]
        prefix, pos = scan(child), child > 0
        over = pos & (prefix.astype(np.float64) > t[:, None])
        last = np.where(pos.any(1), 63 - np.argmax(pos[:, ::-1], axis=1), 0)
        chosen = np.where(over.any(1), np.argmax(over, axis=1), last)
        t = t - np.where(chosen > 0, prefix[np.arange(B), np.maximum(chosen - 1, 0)].astype(np.float64), 0.0)
        node = node * 64 + chosen
    return node
