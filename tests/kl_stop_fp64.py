"""NumPy restatement of tg_kl_control (csrc/policy_shift.hip), bit for bit: IEEE double `/`, `*`, `+` and comparisons, one operation
each, on the device control block
    ctl f64 [8] = {stopped, lr, stop_update, kl_at_stop, last_kl, last_clip_fraction, checks, 0}.
No GPU, no native library.  The lr rule is tests/kl_control_fp64.py::lr_rule's (tg_lr_adapt's), applied to ctl[1]."""
import numpy as np

from kl_control_fp64 import bits, lr_rule

NAN = float("nan")
STOPPED, LR, STOP_UPDATE, KL_AT_STOP, LAST_KL, LAST_CLIP, CHECKS, PAD = range(8)


def init_block(lr):
    """The block as the host writes it at the entry of learn()."""
    return np.array([0.0, lr, 0.0, 0.0, NAN, NAN, 0.0, 0.0], dtype=np.float64)


def kl_control(ctl, sums, target_kl, stop_factor, desired_kl, factor, lr_min, lr_max, update):
    """-> the block after one check (a new array)."""
    ctl = np.array(ctl, dtype=np.float64)
    if ctl[STOPPED] != 0.0:                     # 1. latched: byte for byte
        return ctl
    s = np.asarray(sums, dtype=np.float64)
    kl, cf, _, lr_out = lr_rule(s, desired_kl, factor, lr_min, lr_max, ctl[LR])        # 2., 3.
    ctl[LR], ctl[LAST_KL], ctl[LAST_CLIP], ctl[CHECKS], ctl[PAD] = lr_out, kl, cf, ctl[CHECKS] + np.float64(1.0), 0.0
    target_kl, stop_factor = np.float64(target_kl), np.float64(stop_factor)
    if target_kl > 0.0 and s[0] > 0.0 and kl > stop_factor * target_kl:                # 4.
        ctl[STOPPED], ctl[STOP_UPDATE], ctl[KL_AT_STOP] = 1.0, np.float64(update), kl
    return ctl


def same_bits(a, b):
    """Two blocks agree bit for bit (a NaN equals a NaN of the same payload; the device's 0 / 0 and NumPy's may differ in sign and
    payload, so NaNs are compared as NaNs)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))


# kl = sums[1] / sums[0] with sums[0] = 128 is exact: kl == sums[1] / 128.  stop_factor * target_kl = 1.5 * 0.25 = 0.375 exactly.
_AT = 0.375 * 128.0
_ABOVE = float(np.nextafter(np.float64(0.375), np.float64(1.0))) * 128.0
# name -> (block before, sums, target_kl, stop_factor, desired_kl, factor, lr_min, lr_max, update)
CASES = {
    "at_threshold_does_not_stop": (init_block(1e-3), (128.0, _AT, 3.0, 0.5), 0.25, 1.5, 0.0, 1.5, 1e-5, 1e-2, 3),
    "next_double_above_stops": (init_block(1e-3), (128.0, _ABOVE, 3.0, 0.5), 0.25, 1.5, 0.0, 1.5, 1e-5, 1e-2, 3),
    "nan_sum": (init_block(1e-3), (128.0, NAN, 3.0, 0.5), 0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2, 2),
    "nan_rows": (init_block(1e-3), (NAN, 1.0, 3.0, 0.5), 0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2, 2),
    "no_rows": (init_block(1e-3), (0.0, 0.0, 0.0, 0.0), 0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2, 1),
    "latched_stays": (np.array([1.0, 2e-3, 4.0, 0.7, 0.7, 0.125, 4.0, 0.0]), (128.0, 1e6, 3.0, 0.5), 0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2, 9),
    "lr_clamp_min": (init_block(1.2e-5), (100.0, 3.0, 10.0, -1.0), 0.0, 1.5, 0.01, 1.5, 1e-5, 1e-2, 1),
    "lr_clamp_max": (init_block(9e-3), (100.0, 0.1, 0.0, 0.2), 0.0, 1.5, 0.01, 1.5, 1e-5, 1e-2, 1),
    "stop_and_adapt": (init_block(1e-3), (100.0, 300.0, 10.0, -1.0), 0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2, 7),
    "target_off": (init_block(1e-3), (100.0, 300.0, 10.0, -1.0), 0.0, 1.5, 0.0, 1.5, 1e-5, 1e-2, 7),
}

# five checks through one block: adapt (down), adapt (up), latch (adapting down once more), two no-ops
SEQUENCE_ARGS = (0.25, 1.5, 0.01, 1.5, 1e-5, 1e-2)          # target_kl, stop_factor, desired_kl, factor, lr_min, lr_max
SEQUENCE_SUMS = [(128.0, 6.4, 2.0, 0.1), (128.0, 0.32, 0.0, 0.0), (128.0, 64.0, 40.0, -3.0), (128.0, 0.32, 0.0, 0.0), (128.0, 900.0, 9.0, 1.0)]


def run_sequence(lr=1e-3):
    """-> the block after each of the five checks (check j follows update j + 1)."""
    ctl, out = init_block(lr), []
    for j, sums in enumerate(SEQUENCE_SUMS):
        ctl = kl_control(ctl, sums, *SEQUENCE_ARGS, j + 1)
        out.append(ctl)
    return out
