"""Tensor-level wrappers over the C ABI for the returns / advantage / loss kernels.

Every function takes CUDA (ROCm) tensors and enqueues on torch's current stream; none has a
CPU fallback.  Layouts are the time-major SoA of the device trajectory: `[T][n]`, env fastest.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N


def _st(t):
    return N.stream_ptr(t.device)


def suffixed(base: str, suffix: str, extra):
    """One optional feature of an entry point: its arguments `extra` (None: off) -> (entry name, those arguments as a tuple)."""
    return (base, ()) if extra is None else (base + suffix, tuple(extra))


def rtg_scan(rew: torch.Tensor, mask: torch.Tensor, gamma: float) -> torch.Tensor:
    """Reward-to-go (algorithms/grpo.py:66-74 == algorithms/ppo.py:100-111).  rew f32 [T][n], mask u8 [T][n]."""
    N.require_cuda(rew, mask)
    assert rew.dtype == torch.float32 and mask.dtype == torch.uint8 and rew.is_contiguous() and mask.is_contiguous()
    T, n = rew.shape
    out = torch.empty_like(rew)
    N.check(N.load().tg_rtg_scan(rew.data_ptr(), mask.data_ptr(), float(gamma), out.data_ptr(), n, T, _st(rew)), "tg_rtg_scan")
    return out


def gae_scan(rew, values, mask, gamma: float, lam: float):
    """GAE advantages and returns (algorithms/ppo.py:112-124)."""
    N.require_cuda(rew, values, mask)
    assert rew.dtype == values.dtype == torch.float32 and mask.dtype == torch.uint8
    assert rew.is_contiguous() and values.is_contiguous() and mask.is_contiguous()
    T, n = rew.shape
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    N.check(N.load().tg_gae_scan(rew.data_ptr(), values.data_ptr(), mask.data_ptr(), float(gamma), float(lam),
                                 adv.data_ptr(), ret.data_ptr(), n, T, _st(rew)), "tg_gae_scan")
    return adv, ret


def masked_moments(x: torch.Tensor, mask: torch.Tensor, group_size: int) -> torch.Tensor:
    """f64 [n/group_size][3] = (count, sum, sum of squares) over the valid entries of each group."""
    N.require_cuda(x, mask)
    assert x.dtype == torch.float32 and mask.dtype == torch.uint8 and x.is_contiguous() and mask.is_contiguous()
    T, n = x.shape
    out = torch.empty(n // group_size, 3, dtype=torch.float64, device=x.device)
    work = torch.empty(3 * n, dtype=torch.float64, device=x.device)
    N.check(N.load().tg_masked_moments(x.data_ptr(), mask.data_ptr(), n, T, int(group_size), out.data_ptr(),
                                       work.data_ptr(), _st(x)), "tg_masked_moments")
    return out


def group_normalize(x, mask, moments, mode: int, group_size: int) -> torch.Tensor:
    """mode 0: (x-mean_g)/std_g (GRPO, grpo.py:115); mode 1: /(std_g+1e-8) (PPO, ppo.py:138-139)."""
    N.require_cuda(x, mask, moments)
    assert moments.dtype == torch.float64 and moments.is_contiguous()
    T, n = x.shape
    out = torch.empty_like(x)
    N.check(N.load().tg_group_normalize(x.data_ptr(), mask.data_ptr(), moments.data_ptr(), int(mode), out.data_ptr(),
                                        n, T, int(group_size), _st(x)), "tg_group_normalize")
    return out


def grpo_step_advantage(rtg: torch.Tensor, mask: torch.Tensor, group_size: int, scale: bool = True, out=None, work=None, group=None):
    """tg_grpo_step_advantage: (adv f32 [T][n], group f64 [n / group_size][3] = {Q, C, K}) -- every valid return-to-go minus the mean of
    its group's valid entries at its time step; scale: divided by the group's pooled within-step std + 1e-8.  Invalid entries +0.
    out / work (f64, 3 * (n / group_size) * T) / group: reused buffers."""
    N.require_cuda(rtg, mask, out, work, group)
    assert rtg.dtype == torch.float32 and mask.dtype == torch.uint8 and rtg.is_contiguous() and mask.is_contiguous() and rtg.shape == mask.shape
    T, n = rtg.shape
    G = n // int(group_size) if group_size >= 1 else 0
    if out is None:
        out = torch.empty_like(rtg)
    if work is None:
        work = torch.empty(max(3 * G * T, 1), dtype=torch.float64, device=rtg.device)
    if group is None:
        group = torch.empty(G, 3, dtype=torch.float64, device=rtg.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == rtg.shape and out.data_ptr() != rtg.data_ptr()
    assert work.dtype == group.dtype == torch.float64 and work.numel() >= 3 * G * T and group.is_contiguous() and group.numel() == 3 * G
    if n == 0:                                                             # (an empty tensor has no address to pass)
        return out, group
    N.check(N.load().tg_grpo_step_advantage(rtg.data_ptr(), mask.data_ptr(), n, T, int(group_size), 1 if scale else 0, work.data_ptr(),
                                            out.data_ptr(), group.data_ptr(), _st(rtg)), "tg_grpo_step_advantage")
    return out, group


def returns_moments(rew: torch.Tensor, mask: torch.Tensor, gamma: float, group_size: int):
    """(rtg, moments) = (rtg_scan(rew, mask, gamma), masked_moments(rtg, mask, group_size)), bit-identical, in two launches built for
    rollouts of a few thousand envs (tg_returns_moments: LDS-staged strips, one lane per env on the recurrence)."""
    N.require_cuda(rew, mask)
    assert rew.dtype == torch.float32 and mask.dtype == torch.uint8 and rew.is_contiguous() and mask.is_contiguous()
    T, n = rew.shape
    rtg = torch.empty_like(rew)
    moments = torch.empty(n // group_size, 3, dtype=torch.float64, device=rew.device)
    work = torch.empty(3 * n, dtype=torch.float64, device=rew.device)
    N.check(N.load().tg_returns_moments(rew.data_ptr(), mask.data_ptr(), float(gamma), rtg.data_ptr(), n, T, int(group_size),
                                        moments.data_ptr(), work.data_ptr(), _st(rew)), "tg_returns_moments")
    return rtg, moments


def returns_moments_max_horizon() -> int:
    return int(N.load().tg_returns_moments_max_horizon())


def learn_count(mask: torch.Tensor, expected_rows: int, work: torch.Tensor, total: torch.Tensor) -> None:
    """tg_learn_count: per-chunk counts of the flat mask and their exclusive prefix into `work` (int32 buffer of
    learn_count_workspace(mask.numel()) bytes); total int64 [2] = (valid entries, 1 if != expected_rows >= 0)."""
    N.require_cuda(mask, work, total)
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and total.dtype == torch.int64 and total.numel() >= 2
    N.check(N.load().tg_learn_count(mask.data_ptr(), mask.numel(), int(expected_rows), work.data_ptr(), work.numel() * work.element_size(),
                                    total.data_ptr(), _st(mask)), "tg_learn_count")


def learn_count_workspace(entries: int) -> int:
    return int(N.load().tg_learn_count_workspace(int(entries)))


def learn_compact(traj, offsets, rows_cap: int, xin: torch.Tensor, ones_col: int, act_rows, idx, src0=None, dst0=None, src1=None, dst1=None,
                  moments=None, norm_mode: int = 0, group_size: int = 0, obs_norm=None) -> None:
    """tg_learn_compact on a DeviceTrajectory: the valid rows' flat indices, padded input rows, action rows and up to two per-row
    scalars (src0 optionally normalised with `moments`), in time-major order, in one launch.  obs_norm (a policy's ObsNorm):
    tg_learn_compact_on -- the input rows hold the normalised observation."""
    N.require_cuda(traj.mask, traj.obs, traj.act, xin, act_rows, idx, src0, dst0, src1, dst1, moments)
    assert xin.dim() == 2 and xin.is_contiguous() and xin.dtype in (torch.bfloat16, torch.float32) and xin.shape[0] >= rows_cap
    assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() >= rows_cap
    assert traj.obs.is_contiguous() and traj.act.is_contiguous() and traj.mask.is_contiguous()
    a = N.CompactArgs()
    a.d_mask, a.d_offsets, a.n, a.T, a.S, a.A = traj.mask.data_ptr(), offsets.data_ptr(), traj.n, traj.T, traj.S, traj.A
    a.obs_dtype, a.d_obs, a.obs_feat_stride, a.d_act = N.dtype_code(traj.obs.dtype), traj.obs.data_ptr(), (traj.T + 1) * traj.n, traj.act.data_ptr()
    a.d_xin, a.in_pad, a.xin_bf16, a.ones_col, a.norm_mode = xin.data_ptr(), xin.shape[1], int(xin.dtype == torch.bfloat16), int(ones_col), int(norm_mode)
    if act_rows is not None:
        assert act_rows.dtype == torch.float32 and act_rows.is_contiguous() and act_rows.shape[0] >= rows_cap and act_rows.shape[1] == traj.A
    a.d_act_rows, a.d_idx = N.ptr(act_rows), idx.data_ptr()
    for s_, d_ in ((src0, dst0), (src1, dst1)):
        assert (s_ is None) == (d_ is None)
        if s_ is not None:
            assert s_.dtype == d_.dtype == torch.float32 and s_.is_contiguous() and d_.is_contiguous() and s_.numel() == traj.T * traj.n and d_.numel() >= rows_cap
    a.d_src0, a.d_dst0, a.d_src1, a.d_dst1 = N.ptr(src0), N.ptr(dst0), N.ptr(src1), N.ptr(dst1)
    if moments is not None:
        assert moments.dtype == torch.float64 and moments.is_contiguous() and moments.numel() == 3 * (traj.n // group_size)
    a.d_moments, a.group_size, a.rows_cap = N.ptr(moments), int(group_size), int(rows_cap)
    assert obs_norm is None or (obs_norm.table.numel() == 2 * traj.S and obs_norm.table.device == xin.device)
    name, tail = suffixed("tg_learn_compact", "_on", None if obs_norm is None else (obs_norm.table.data_ptr(), obs_norm.clip_value))
    N.check(getattr(N.load(), name)(C.byref(a), *tail, _st(xin)), name)


def obs_moments(traj, center: torch.Tensor, out: torch.Tensor = None, work: torch.Tensor = None) -> torch.Tensor:
    """tg_obs_moments on a DeviceTrajectory: f64 [S][3] = {count, sum (x - center[s]), sum (x - center[s])^2} over the valid (t, e)
    entries, per feature, in a fixed order.  center f64 [S]; work: f64 scratch of obs_moments_workspace(T * n, S) bytes."""
    N.require_cuda(traj.obs, traj.mask, center, out, work)
    assert center.dtype == torch.float64 and center.is_contiguous() and center.numel() == traj.S
    assert traj.obs.is_contiguous() and traj.mask.is_contiguous()
    need = int(N.load().tg_obs_moments_workspace(traj.T * traj.n, traj.S))
    if work is None:
        work = torch.empty(need // 8, dtype=torch.float64, device=center.device)
    if out is None:
        out = torch.empty(traj.S, 3, dtype=torch.float64, device=center.device)
    assert work.dtype == torch.float64 and work.numel() * 8 >= need and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 3 * traj.S
    tr = traj.native()
    N.check(N.load().tg_obs_moments(C.byref(tr), traj.S, center.data_ptr(), work.data_ptr(), work.numel() * 8, out.data_ptr(), _st(center)),
            "tg_obs_moments")
    return out


def obs_moments_workspace(entries: int, S: int) -> int:
    return int(N.load().tg_obs_moments_workspace(int(entries), int(S)))


def obs_norm_merge(batch, eps: float, count: torch.Tensor, mean: torch.Tensor, m2: torch.Tensor, table: torch.Tensor) -> None:
    """tg_obs_norm_merge: Chan's merge of batch f64 [S][3] (None: nothing to merge) into count / mean / m2, and the f32 table [2][S]
    rewritten in place."""
    N.require_cuda(batch, count, mean, m2, table)
    S = mean.numel()
    for t in (count, mean, m2) + ((batch,) if batch is not None else ()):
        assert t.dtype == torch.float64 and t.is_contiguous()
    assert count.numel() == 1 and m2.numel() == S and table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 2 * S
    assert batch is None or batch.numel() == 3 * S
    N.check(N.load().tg_obs_norm_merge(N.ptr(batch), S, float(eps), count.data_ptr(), mean.data_ptr(), m2.data_ptr(), table.data_ptr(),
                                       _st(table)), "tg_obs_norm_merge")


def obs_normalize_rows(x: torch.Tensor, obs_norm, xin: torch.Tensor, ones_col: int = -1) -> torch.Tensor:
    """tg_obs_normalize_rows: x [M][S] f32 / f64 with any two strides (an SoA slot's transposed view, row-major rows) -> xin
    [M][in_pad] bf16 / f32: the normalised observation, zero padding, 1 in column ones_col (or -1)."""
    N.require_cuda(x, xin, obs_norm.table)
    M, S = x.shape
    assert xin.dim() == 2 and xin.is_contiguous() and xin.shape[0] >= M and xin.dtype in (torch.bfloat16, torch.float32)
    assert obs_norm.table.numel() == 2 * S and xin.data_ptr() % 16 == 0
    N.check(N.load().tg_obs_normalize_rows(x.data_ptr(), N.dtype_code(x.dtype), max(x.stride(0), 1), max(x.stride(1), 1), M, S,
                                           obs_norm.table.data_ptr(), obs_norm.clip_value, xin.data_ptr(), xin.shape[1],
                                           int(xin.dtype == torch.bfloat16), int(ones_col), _st(xin)), "tg_obs_normalize_rows")
    return xin


def scatter_rows(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor, table: torch.Tensor = None) -> None:
    """dst.view(-1)[idx[r]] = src[r][0] (tg_scatter_rows): src f32 [rows][>= 1] with any row stride, idx int64 [rows], dst f32.
    table (a ValueNorm's f32 [4]): tg_scatter_rows_affine -- the value written is src[r][0] * table[1] + table[0], two roundings."""
    N.require_cuda(src, idx, dst, table)
    rows = idx.numel()
    assert src.dtype == dst.dtype == torch.float32 and idx.dtype == torch.int64 and idx.is_contiguous() and dst.is_contiguous()
    assert src.dim() == 2 and src.shape[0] >= rows
    assert table is None or (table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 4 and table.device == dst.device)
    name, tab = suffixed("tg_scatter_rows", "_affine", None if table is None else (table.data_ptr(),))
    # (max: an empty src may carry a row stride of 0, which the entry points refuse before they see rows == 0)
    N.check(getattr(N.load(), name)(src.data_ptr(), max(src.stride(0), 1), idx.data_ptr(), rows, *tab, dst.data_ptr(), _st(dst)), name)


def boot_values_affine(v: torch.Tensor, timeout: torch.Tensor, table: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """tg_boot_values_affine: out[i] = (v[i] * table[1] + table[0]) * timeout[i], each fp32 operation rounded on its own.  v f32 [n]
    with any stride, timeout u8 [n], table a ValueNorm's f32 [4]."""
    N.require_cuda(v, timeout, table, out)
    n = timeout.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=v.device)
    assert v.dtype == out.dtype == torch.float32 and v.dim() == 1 and v.numel() == n and out.is_contiguous() and out.numel() == n
    assert timeout.dtype == torch.uint8 and timeout.is_contiguous()
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 4
    N.check(N.load().tg_boot_values_affine(v.data_ptr(), max(v.stride(0), 1), timeout.data_ptr(), n, table.data_ptr(), out.data_ptr(), _st(out)),
            "tg_boot_values_affine")
    return out


def value_norm_merge(moments3, eps: float, count: torch.Tensor, mean: torch.Tensor, m2: torch.Tensor, table: torch.Tensor,
                     norm8: torch.Tensor = None) -> None:
    """tg_value_norm_merge: Chan's merge of moments3 f64 [3] = {n, sum, sum of squares} of a batch of returns (None: nothing to
    merge) into count / mean / m2 f64 [1], the f32 table [4] rewritten in place, and -- norm8 given -- entries 2 and 3 of tg_ppo_norm's
    f32 [8] overwritten with table[0] and table[2]."""
    N.require_cuda(moments3, count, mean, m2, table, norm8)
    for t in (count, mean, m2):
        assert t.dtype == torch.float64 and t.numel() == 1
    assert moments3 is None or (moments3.dtype == torch.float64 and moments3.is_contiguous() and moments3.numel() == 3)
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 4
    assert norm8 is None or (norm8.dtype == torch.float32 and norm8.is_contiguous() and norm8.numel() == 8)
    N.check(N.load().tg_value_norm_merge(N.ptr(moments3), float(eps), count.data_ptr(), mean.data_ptr(), m2.data_ptr(), table.data_ptr(),
                                         N.ptr(norm8), _st(table)), "tg_value_norm_merge")


def value_norm_merge_popart(moments3, eps: float, count: torch.Tensor, mean: torch.Tensor, m2: torch.Tensor, table: torch.Tensor,
                            norm8, head_w: torch.Tensor, head_b: torch.Tensor) -> None:
    """tg_value_norm_merge_popart: value_norm_merge and, in the same launch, PopArt's rescale of the critic's last layer -- head_w f32
    [1][H] and head_b f32 [1], the fp32 MASTERS, written in place by raw pointer (torch's version counters do not move: the caller
    bumps N.RAW_PARAM_WRITES and marks the layouts derived from them stale)."""
    N.require_cuda(moments3, count, mean, m2, table, norm8, head_w, head_b)
    for t in (count, mean, m2):
        assert t.dtype == torch.float64 and t.numel() == 1
    assert moments3 is None or (moments3.dtype == torch.float64 and moments3.is_contiguous() and moments3.numel() == 3)
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() == 4
    assert norm8 is None or (norm8.dtype == torch.float32 and norm8.is_contiguous() and norm8.numel() == 8)
    assert head_w.dtype == head_b.dtype == torch.float32 and head_w.is_contiguous() and head_b.is_contiguous()
    assert head_w.dim() == 2 and head_w.shape[0] == 1 and head_w.shape[1] >= 1 and tuple(head_b.shape) == (1,)
    assert head_w.device == head_b.device == count.device
    N.check(N.load().tg_value_norm_merge_popart(N.ptr(moments3), float(eps), count.data_ptr(), mean.data_ptr(), m2.data_ptr(),
                                                table.data_ptr(), N.ptr(norm8), head_w.data_ptr(), int(head_w.shape[1]),
                                                head_b.data_ptr(), _st(table)), "tg_value_norm_merge_popart")


def privileged_rows(src: torch.Tensor, S: int, idx, n: int, env_params: torch.Tensor, spec: "N.PrivilegedSpec", out: torch.Tensor,
                    ones_col: int = -1) -> torch.Tensor:
    """tg_privileged_rows: the privileged critic's input rows.  src [rows][src_pad] bf16 / f32 (the actor's prepared rows), out
    [>= rows][dst_pad] of the same dtype: columns [0, S) of a row are src's bits, column S + k is env e's parameter spec.index[k] as a
    feature on [-1, 1], the rest 0 with 1 in ones_col (or -1).  idx int64 [rows] holds the rows' flat t * n + e (e = idx % n), or None:
    row r is env r.  env_params: DeviceRollout.env_params, f64 [12][n]."""
    N.require_cuda(src, idx, env_params, out)
    rows = src.shape[0]
    assert src.dim() == 2 and out.dim() == 2 and src.is_contiguous() and out.is_contiguous() and out.shape[0] >= rows
    assert src.dtype == out.dtype and src.dtype in (torch.bfloat16, torch.float32)
    assert idx is None or (idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == rows)
    assert env_params.dtype == torch.float64 and env_params.is_contiguous() and tuple(env_params.shape) == (12, int(n))
    N.check(N.load().tg_privileged_rows(src.data_ptr(), src.shape[1], int(S), N.ptr(idx), rows, int(n), env_params.data_ptr(), C.byref(spec),
                                        out.data_ptr(), out.shape[1], int(src.dtype == torch.bfloat16), int(ones_col), _st(out)),
            "tg_privileged_rows")
    return out[:rows]


def ppo_returns(rew, values, mask, gamma: float, lam: float, monte_carlo: bool, adv: torch.Tensor, ret: torch.Tensor,
                work: torch.Tensor = None) -> torch.Tensor:
    """tg_ppo_returns: fills adv / ret f32 [T][n] (ppo.py:100-124) and returns the f64 [2][3] masked moments {count, sum, sum of
    squares} of the advantages and of the returns -- bit-identical to rtg_scan / `rtg - values` / gae_scan + masked_moments(group = n)."""
    return ppo_returns_boot(rew, values, mask, None, None, gamma, lam, monte_carlo, adv, ret, work)


def rollout_final_state(params, traj, s_final: torch.Tensor = None, timeout: torch.Tensor = None, env_params: torch.Tensor = None,
                        substeps: int = 1, motor: torch.Tensor = None):
    """tg_rollout_final_state on a DeviceTrajectory: (s_final f32 [n][S], timeout u8 [n]) -- the state each episode's last step
    produced (Env.step on obs[:, len-1], act[:, len-1]: tg_env_step's bits) and whether the clock, not a failure, ended the episode.
    params: the env's tg_env_params (DeviceRollout.params / Env.native_params()).  A swarm env is refused: ValueError.
    env_params: the per-env parameter table of a randomised rollout (DeviceRollout.env_params, f64 [12][n]): every slot is re-stepped
    with its own vehicle (tg_rollout_final_state_dr).
    substeps != 1 (DeviceRollout.substeps; params are then those of the physics clock): the last CONTROL step is re-run, up to
    `substeps` calls that stop at the first truncation (tg_rollout_final_state_sub, which takes the table or NULL).
    motor: the motor record of a rollout with an actuator lag (DeviceTrajectory.motor, f32 [A][T+1][n]; params then carry the time
    constant in p[10]): the re-step filters the last commanded action from slot len-1 (tg_rollout_final_state_lag)."""
    N.require_cuda(traj.obs, traj.act, traj.len, s_final, timeout)
    assert traj.obs.is_contiguous() and traj.act.is_contiguous() and traj.len.is_contiguous() and traj.len.dtype == torch.int32
    dev = traj.obs.device
    if s_final is None:
        s_final = torch.empty(traj.n, traj.S, dtype=torch.float32, device=dev)
    if timeout is None:
        timeout = torch.empty(traj.n, dtype=torch.uint8, device=dev)
    assert s_final.dtype == torch.float32 and s_final.is_contiguous() and s_final.numel() == traj.n * traj.S
    assert timeout.dtype == torch.uint8 and timeout.is_contiguous() and timeout.numel() == traj.n
    tr = traj.native()
    if env_params is not None:
        N.require_cuda(env_params)
        assert env_params.dtype == torch.float64 and env_params.is_contiguous() and tuple(env_params.shape) == (12, traj.n)
    ptab = None if env_params is None else env_params.data_ptr()
    if motor is not None:
        N.require_cuda(motor)
        assert motor.dtype == torch.float32 and motor.is_contiguous() and tuple(motor.shape) == (traj.A, traj.T + 1, traj.n)
        name, table, tail = "tg_rollout_final_state_lag", (ptab,), (int(substeps), motor.data_ptr())
    elif substeps != 1:
        name, table, tail = "tg_rollout_final_state_sub", (ptab,), (int(substeps),)
    else:
        name, table = suffixed("tg_rollout_final_state", "_dr", None if ptab is None else (ptab,))
        tail = ()
    rc = getattr(N.load(), name)(C.byref(params), *table, C.byref(tr), s_final.data_ptr(), timeout.data_ptr(), *tail, _st(traj.obs))
    if rc == N.TG_ERR_UNSUPPORTED:
        raise ValueError(N.load().tg_last_error().decode("utf-8", "replace"))
    N.check(rc, name)
    return s_final, timeout


def param_grid(indices, levels, values: torch.Tensor, episodes_per_cell: int) -> "N.ParamGrid":
    """tg_param_grid: the swept p[] indices, the number of factors of each, the device f64 array of the concatenated factor lists
    (kept alive by the caller) and the episodes of a cell."""
    N.require_cuda(values)
    assert values.dtype == torch.float64 and values.is_contiguous() and values.numel() == sum(int(v) for v in levels)
    assert len(indices) == len(levels) <= 12
    g = N.ParamGrid()
    g.count, g.d_values, g.episodes_per_cell = len(indices), values.data_ptr(), int(episodes_per_cell)
    for k, (i, l) in enumerate(zip(indices, levels)):
        g.index[k], g.levels[k] = int(i), int(l)
    g._values = values                                   # (the struct holds a raw address: keep the factors alive with it)
    return g


def env_param_grid(params, grid: "N.ParamGrid", out: torch.Tensor, env_offset: int = 0) -> torch.Tensor:
    """tg_env_param_grid: the per-env parameter table f64 [12][n] of a sweep -- env slot i steps the vehicle of cell
    (env_offset + i) / episodes_per_cell, the cell decoded row-major over the swept parameters in p[] order."""
    N.require_cuda(out)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == 12
    N.check(N.load().tg_env_param_grid(C.byref(params), C.byref(grid), out.data_ptr(), out.shape[1], int(env_offset), _st(out)),
            "tg_env_param_grid")
    return out


def eval_tile_states(traj, episodes_per_cell: int) -> None:
    """tg_eval_tile_states: slot 0 of obs of the first `episodes_per_cell` envs copied to every other cell, in place."""
    N.require_cuda(traj.obs)
    assert traj.obs.is_contiguous()
    tr = traj.native()
    N.check(N.load().tg_eval_tile_states(C.byref(tr), traj.S, int(episodes_per_cell), _st(traj.obs)), "tg_eval_tile_states")


def eval_cells(traj, timeout: torch.Tensor, episodes_per_cell: int, returns: torch.Tensor = None, cells: torch.Tensor = None):
    """tg_eval_cells on a DeviceTrajectory: (returns f64 [n], cells f64 [n / E][8]) -- per episode the f64 sum of its rewards, per cell
    {episodes, sum of returns, sum of squared returns, min, max, sum of lengths, clock-ended, ended early} in the fixed summation
    order of the header.  timeout: u8 [n] from rollout_final_state."""
    N.require_cuda(traj.rew, traj.len, timeout, returns, cells)
    E = int(episodes_per_cell)
    assert traj.rew.is_contiguous() and traj.len.is_contiguous() and traj.len.dtype == torch.int32
    assert timeout.dtype == torch.uint8 and timeout.is_contiguous() and timeout.numel() == traj.n
    dev = traj.rew.device
    if returns is None:
        returns = torch.empty(traj.n, dtype=torch.float64, device=dev)
    if cells is None:
        cells = torch.empty(max(traj.n // max(E, 1), 1), 8, dtype=torch.float64, device=dev)
    assert returns.dtype == torch.float64 and returns.is_contiguous() and returns.numel() == traj.n
    assert cells.dtype == torch.float64 and cells.is_contiguous() and cells.numel() >= 8 * (traj.n // max(E, 1))
    tr = traj.native()
    N.check(N.load().tg_eval_cells(C.byref(tr), timeout.data_ptr(), E, returns.data_ptr(), cells.data_ptr(), _st(traj.rew)), "tg_eval_cells")
    return returns, cells


def ppo_returns_boot(rew, values, mask, length, boot, gamma: float, lam: float, monte_carlo: bool, adv: torch.Tensor, ret: torch.Tensor,
                     work: torch.Tensor = None) -> torch.Tensor:
    """tg_ppo_returns_boot: ppo_returns() on the rewards with gamma * boot[i] added to the reward of env i's last step
    (t == length[i] - 1; fp32, each operation rounded on its own) -- `rew` is read, not written.  length i32 [n], boot f32 [n].
    (ppo_returns()'s body too: it passes None for both and runs tg_ppo_returns.)"""
    N.require_cuda(rew, values, mask, length, boot, adv, ret, work)
    T, n = rew.shape
    for t in (rew, values, adv, ret):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == T * n
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == T * n
    assert (length is None) == (boot is None)
    if boot is not None:
        assert length.dtype == torch.int32 and length.is_contiguous() and length.numel() == n
        assert boot.dtype == torch.float32 and boot.is_contiguous() and boot.numel() == n
    if work is None:
        work = torch.empty(6 * n, dtype=torch.float64, device=rew.device)
    assert work.dtype == torch.float64 and work.numel() >= 6 * n
    moments = torch.empty(2, 3, dtype=torch.float64, device=rew.device)
    name, lb = suffixed("tg_ppo_returns", "_boot", None if boot is None else (length.data_ptr(), boot.data_ptr()))
    N.check(getattr(N.load(), name)(rew.data_ptr(), values.data_ptr(), mask.data_ptr(), *lb, float(gamma), float(lam), 1 if monte_carlo else 0,
                                    adv.data_ptr(), ret.data_ptr(), n, T, moments.data_ptr(), work.data_ptr(), _st(rew)), name)
    return moments


def ppo_norm(moments: torch.Tensor, c1: float, kl_coeff: float, out: torch.Tensor = None) -> torch.Tensor:
    """tg_ppo_norm: f32 [8] = {adv mean, 1 / (adv std + 1e-8), ret mean, 1 / (ret std + 1e-8), -1 / n, c1 / n, kl_coeff / n, n} on the
    device (what the loss heads read through `norm8=`)."""
    N.require_cuda(moments, out)
    assert moments.dtype == torch.float64 and moments.is_contiguous() and moments.numel() == 6
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=moments.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 8
    N.check(N.load().tg_ppo_norm(moments.data_ptr(), float(c1), float(kl_coeff), out.data_ptr(), _st(moments)), "tg_ppo_norm")
    return out


def gather_rows2(idx: torch.Tensor, src0: torch.Tensor, dst0: torch.Tensor, src1: torch.Tensor = None, dst1: torch.Tensor = None) -> None:
    """dst0[r] = src0.view(-1)[idx[r]] (and dst1 / src1): tg_gather_rows2."""
    N.require_cuda(idx, src0, dst0, src1, dst1)
    rows = idx.numel()
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    for s_, d_ in ((src0, dst0), (src1, dst1)):
        assert (s_ is None) == (d_ is None)
        if s_ is not None:
            assert s_.dtype == d_.dtype == torch.float32 and s_.is_contiguous() and d_.is_contiguous() and d_.numel() >= rows
    N.check(N.load().tg_gather_rows2(idx.data_ptr(), rows, src0.data_ptr(), dst0.data_ptr(), N.ptr(src1), N.ptr(dst1), _st(idx)),
            "tg_gather_rows2")


def _var_array(var):
    v = [float(x) for x in var]
    return (C.c_float * len(v))(*v), len(v)


def gaussian_logp(mean: torch.Tensor, act: torch.Tensor, var, out: torch.Tensor = None) -> torch.Tensor:
    """log N(act; mean, diag(var)) per row (actor_critic.py:159-160).  mean [M][A] f32 (row stride free),
    act any 2-D strided [M][A] f32.  out: a contiguous f32 [M] to write into (e.g. a slice of a larger result)."""
    N.require_cuda(mean, act, out)
    assert mean.dtype == act.dtype == torch.float32 and mean.dim() == 2 and mean.stride(1) == 1
    M, A = mean.shape
    va, k = _var_array(var)
    assert k == A
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=mean.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M
    N.check(N.load().tg_gaussian_logp(mean.data_ptr(), mean.stride(0), act.data_ptr(), act.stride(0), act.stride(1),
                                      va, A, out.data_ptr(), M, _st(mean)), "tg_gaussian_logp")
    return out


def policy_shift_blocks(rows: int) -> int:
    """How many f64 [4] partials tg_policy_shift leaves for a chunk of `rows` rows (host arithmetic of the library)."""
    return int(N.load().tg_policy_shift_blocks(int(rows)))


def policy_shift(mean: torch.Tensor, act: torch.Tensor, logp_old: torch.Tensor, var, log_lo: float, log_hi: float, partials: torch.Tensor,
                 slot: int = 0, log_std: torch.Tensor = None) -> int:
    """tg_policy_shift on one chunk of rows: per row d = logp(act; mean) - logp_old in float64, and the workgroups' partials
    {rows, sum expm1(d) - d, rows with d outside [log_lo, log_hi], sum d} into partials[slot:slot + blocks] (f64 [*][4]).  mean, act as
    gaussian_logp() takes them; `var` a host sequence [A <= 8], or log_std a DEVICE f32 [A <= 4] (then `var` is not looked at: no host
    read of a learned std).  Returns the number of partials written."""
    N.require_cuda(mean, act, logp_old, partials, log_std)
    assert mean.dtype == act.dtype == logp_old.dtype == torch.float32 and mean.dim() == 2 and (mean.shape[0] == 0 or mean.stride(1) == 1)
    rows, A = mean.shape
    assert act.dim() == 2 and tuple(act.shape) == (rows, A) and logp_old.is_contiguous() and logp_old.numel() == rows
    blocks = policy_shift_blocks(rows)
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.dim() == 2 and partials.shape[1] == 4
    assert slot >= 0 and slot + blocks <= partials.shape[0]
    if log_std is not None:
        assert log_std.dtype == torch.float32 and log_std.is_contiguous() and log_std.numel() == A
        va = None
    else:
        va, k = _var_array(var)
        assert k == A
    N.check(N.load().tg_policy_shift(mean.data_ptr(), mean.stride(0), act.data_ptr(), act.stride(0), act.stride(1), logp_old.data_ptr(),
                                     va, N.ptr(log_std), A, float(log_lo), float(log_hi), rows, partials.data_ptr(), int(slot), _st(mean)),
            "tg_policy_shift")
    return blocks


def policy_shift_finish(partials: torch.Tensor, n_partials: int, sums: torch.Tensor) -> torch.Tensor:
    """tg_policy_shift_finish: sums f64 [4] <- the first n_partials rows of `partials`, added in index order."""
    N.require_cuda(partials, sums)
    assert partials.dtype == sums.dtype == torch.float64 and partials.is_contiguous() and sums.is_contiguous() and sums.numel() == 4
    assert 0 <= n_partials <= partials.shape[0] and partials.dim() == 2 and partials.shape[1] == 4
    N.check(N.load().tg_policy_shift_finish(partials.data_ptr(), int(n_partials), sums.data_ptr(), _st(sums)), "tg_policy_shift_finish")
    return sums


def lr_adapt(sums: torch.Tensor, desired_kl: float, factor: float, lr_min: float, lr_max: float, lr: float, out: torch.Tensor) -> torch.Tensor:
    """tg_lr_adapt: out f64 [4] = {kl, clip_fraction, lr_in, lr_out} from the (all-reduced) sums of policy_shift_finish(); desired_kl
    <= 0 measures only (lr_out = lr_in)."""
    N.require_cuda(sums, out)
    assert sums.dtype == out.dtype == torch.float64 and sums.is_contiguous() and out.is_contiguous() and sums.numel() == 4 and out.numel() == 4
    N.check(N.load().tg_lr_adapt(sums.data_ptr(), float(desired_kl), float(factor), float(lr_min), float(lr_max), float(lr), out.data_ptr(),
                                 _st(sums)), "tg_lr_adapt")
    return out


def kl_control(sums: torch.Tensor, target_kl: float, stop_factor: float, desired_kl: float, factor: float, lr_min: float, lr_max: float,
               update: int, ctl: torch.Tensor) -> torch.Tensor:
    """tg_kl_control: one check between the optimizer steps of a learn() on the device control block ctl f64 [8] = {stopped, lr,
    stop_update, kl_at_stop, last_kl, last_clip_fraction, checks, 0} from the (all-reduced) sums of policy_shift_finish().  target_kl
    <= 0 never stops, desired_kl <= 0 leaves the rate; a latched block is left as it is."""
    N.require_cuda(sums, ctl)
    assert sums.dtype == ctl.dtype == torch.float64 and sums.is_contiguous() and ctl.is_contiguous() and sums.numel() == 4 and ctl.numel() == 8
    N.check(N.load().tg_kl_control(sums.data_ptr(), float(target_kl), float(stop_factor), float(desired_kl), float(factor), float(lr_min),
                                   float(lr_max), int(update), ctl.data_ptr(), _st(sums)), "tg_kl_control")
    return ctl


def surrogate_loss(mean, value, act, logp_old, adv, ret, mask, norm, var, epsilon, surr_coef, critic_coef, kl_coef,
                   want_total: bool = True, coef: torch.Tensor = None, logp_ref: torch.Tensor = None, ref_coef: float = 0.0,
                   log_std: torch.Tensor = None, std_out: torch.Tensor = None):
    """One launch of tg_surrogate_loss: returns (total f32 scalar, sums f64[4], d total/d mean, d total/d value|None).
    want_total=False skips the handful of scalar launches that combine the sums (the learners only use the sums).
    coef: device f32 [3] {surr_coef, critic_coef, kl_coef} used instead of the three host numbers (PPO: tg_ppo_norm's output [4:7]).
    logp_ref f32 [M] with ref_coef != 0 (tg_surrogate_loss_ref): GRPO's KL penalty to a frozen reference policy, x = logp_ref - logp,
    D = exp(x) - x - 1 in sums[2] (kl_coef must be 0; no value head), total -= ref_coef * sum D.
    log_std (device f32 [A], A <= 4) with std_out (f32 [M][4]) (tg_surrogate_loss_std): the head reads the policy's learned log-std on
    the device (`var` is ignored) and writes each row's contribution to d total / d log_std into std_out (log_std_grad() sums it)."""
    N.require_cuda(mean, act, logp_old, adv, coef)
    assert mean.dtype == torch.float32 and mean.dim() == 2 and mean.stride(1) == 1
    M, A = mean.shape
    a = N.LossArgs()
    a.d_mean, a.mean_row_stride = mean.data_ptr(), mean.stride(0)
    a.d_act, a.act_row_stride, a.act_col_stride = act.data_ptr(), act.stride(0), act.stride(1)
    a.d_logp_old, a.d_adv = logp_old.data_ptr(), adv.data_ptr()
    grad_value = None
    if value is not None:
        assert value.dtype == torch.float32 and value.is_contiguous() and ret is not None and ret.is_contiguous()
        grad_value = torch.empty_like(value)
        a.d_value, a.d_ret, a.d_grad_value = value.data_ptr(), ret.data_ptr(), grad_value.data_ptr()
    a.d_mask, a.d_norm = N.ptr(mask), N.ptr(norm)
    if coef is not None:
        assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() >= 3 and not want_total
        a.d_coef = coef.data_ptr()
    if log_std is None:
        va, k = _var_array(var)
        assert k == A
        for i in range(A):
            a.var[i] = va[i]
    a.act_dim, a.epsilon = A, float(epsilon)
    a.surr_coef, a.critic_coef, a.kl_coef = float(surr_coef), float(critic_coef), float(kl_coef)
    grad_mean = torch.empty(M, A, dtype=torch.float32, device=mean.device)
    sums = torch.empty(4, dtype=torch.float64, device=mean.device)
    work = torch.empty(4 * N.load().tg_loss_work_blocks(), dtype=torch.float64, device=mean.device)
    a.d_grad_mean, a.d_sums, a.d_work, a.M = grad_mean.data_ptr(), sums.data_ptr(), work.data_ptr(), M
    ref = ref_penalty(logp_ref, ref_coef, M)
    sd = learned_std(log_std, std_out, M, A) if log_std is not None else None
    name, tail = head_entry("tg_surrogate_loss", ref, sd)
    N.check(getattr(N.load(), name)(C.byref(a), *tail, _st(mean)), name)
    total = ((surr_coef * sums[0] + critic_coef * sums[1] + (kl_coef if ref is None else -float(ref_coef)) * sums[2]).float()
             if want_total else None)
    return total, sums, grad_mean, grad_value


def ref_penalty(logp_ref: torch.Tensor, coef: float, rows: int) -> "N.RefPenalty":
    """N.RefPenalty for the `_ref` entry points (logp_ref device f32 [rows]), or None: no reference policy, or a zero coefficient."""
    if logp_ref is None or float(coef) == 0.0:
        return None
    N.require_cuda(logp_ref)
    assert logp_ref.dtype == torch.float32 and logp_ref.is_contiguous() and logp_ref.numel() == rows
    r = N.RefPenalty()
    r.d_logp_ref, r.coef = logp_ref.data_ptr(), float(coef)
    return r


def head_entry(base: str, ref, std, act=None):
    """(entry name, tail arguments) of a loss head, stand-alone or inside an MLP chain.  ref / std: N.RefPenalty / N.LearnedStd or None;
    act: the hidden activation (TG_ACT_*) of a family whose kernels take one (the fp32 chain learner), else None.
        std          -> base_std, or base_act_std   (ref or NULL, std[, act])
        act != ReLU  -> base_act                    (ref or NULL, act)
        ref          -> base_ref                    (ref,)
        none of them -> base                        ()"""
    rp = None if ref is None else C.byref(ref)
    if std is not None:
        return (base + "_std", (rp, C.byref(std))) if act is None else (base + "_act_std", (rp, C.byref(std), act))
    if act not in (None, N.TG_ACT_RELU):
        return base + "_act", (rp, act)
    return suffixed(base, "_ref", None if ref is None else (rp,))


def learned_std(log_std: torch.Tensor, out: torch.Tensor, rows: int, act_dim: int) -> "N.LearnedStd":
    """N.LearnedStd for the `_std` entry points: log_std device f32 [act_dim <= 4], out device f32 [rows][4]."""
    N.require_cuda(log_std, out)
    assert log_std.dtype == torch.float32 and log_std.is_contiguous() and log_std.numel() == act_dim <= 4
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (rows, 4) and out.data_ptr() % 16 == 0
    sd = N.LearnedStd()
    sd.d_log_std, sd.d_out = log_std.data_ptr(), out.data_ptr()
    return sd


def log_std_grad(rows4: torch.Tensor, act_dim: int, grad: torch.Tensor, add: float = 0.0, work: torch.Tensor = None) -> torch.Tensor:
    """tg_log_std_grad: grad[k] += sum over rows of rows4[:, k] (f64, fixed order) + add, k < act_dim.  rows4 f32 [rows][4] (the
    heads' side output), grad f32 [act_dim] (log_std's window of the gradient bucket)."""
    N.require_cuda(rows4, grad)
    assert rows4.dtype == torch.float32 and rows4.is_contiguous() and rows4.dim() == 2 and rows4.shape[1] == 4
    assert grad.dtype == torch.float32 and grad.is_contiguous() and grad.numel() == act_dim
    lib = N.load()
    if work is None:
        work = torch.empty(4 * lib.tg_log_std_grad_blocks(), dtype=torch.float64, device=rows4.device)
    assert work.dtype == torch.float64 and work.numel() >= 4 * lib.tg_log_std_grad_blocks()
    N.check(lib.tg_log_std_grad(rows4.data_ptr(), rows4.shape[0], act_dim, float(add), grad.data_ptr(), work.data_ptr(), _st(rows4)),
            "tg_log_std_grad")
    return grad


class SurrogateLoss(torch.autograd.Function):
    """Fused clipped-surrogate (+ value MSE + KL-ish penalty) head: one kernel computes the loss sums
    AND d(total)/d(mean), d(total)/d(value); backward just hands those to autograd so the MLP
    forward/backward stay on PyTorch-ROCm.

        total = surr_coef * sum_i min(rho_i A_i, clip(rho_i) A_i)
              + critic_coef * sum_i (V_i - R_i)^2 + kl_coef * sum_i exp(lp_old_i)(lp_old_i - lp_i)

    GRPO (grpo.py:137-145): surr_coef=+1/G, descent on J as the reference writes it.
    PPO  (ppo.py:159-179): surr_coef=-1/n, critic_coef=c1/n, kl_coef=kl_coeff/n.
    Returns (total f32 scalar, sums f64[4] = [sum surrogate, sum sq err, sum kl, #valid]).
    """

    @staticmethod
    def forward(ctx, mean, value, act, logp_old, adv, ret, mask, norm, var, epsilon, surr_coef, critic_coef, kl_coef):
        total, sums, grad_mean, grad_value = surrogate_loss(mean, value, act, logp_old, adv, ret, mask, norm, var,
                                                            epsilon, surr_coef, critic_coef, kl_coef)
        ctx.save_for_backward(grad_mean, grad_value)
        ctx.has_value = value is not None
        ctx.mark_non_differentiable(sums)
        return total, sums

    @staticmethod
    def backward(ctx, g_total, g_sums):
        grad_mean, grad_value = ctx.saved_tensors
        gm = grad_mean * g_total
        gv = grad_value * g_total if ctx.has_value else None
        return (gm, gv) + (None,) * 11
