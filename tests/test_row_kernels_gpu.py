"""The kernels between a rollout and the learner's first forward pass on the MI355X, bit for bit against tests/row_kernels_ref.py
(run with `-m gpu`).  They decide WHICH rows the learner sees, in which order and with what padding: a mistake here is a plausible
gradient on the wrong rows, which no fp64 learner test can see.

  1. tg_learn_count / tg_learn_compact[_on]: every shape and mask pattern of row_kernels_ref (1 to 1,053,443 mask entries: M % 4 of
     1 and 3, one chunk exactly, one chunk and one entry, a thread's 4 entries wrapping over a time step, 33 chunks, 1,029 chunks
     = the scan's second trip; empty, full and trailing chunks; mask bytes 2, 128, 255) on a bf16 and an f32 row format, and every
     row format (in_pad 8 to 64, S == in_pad, ones column in the first / a second 8-column group / absent on bf16 rows) on two
     shapes; f32 and f64 observations, A in {1, 4, 16, none}, zero to two per-row scalars, both normalisation modes, group sizes n
     and a divisor that is no multiple of 4.  Each case runs with rows_cap = M, count, count - 1 and 0 and with the mask 1, 2 and 3
     bytes past an aligned address (load_mask4's byte path), the bytes around the mask being non-zero.
  2. tg_scatter_rows[_affine], tg_gather_rows2, tg_boot_values_affine at 0, 1, 255, 256, 257 and 4,096 x 256 + 3 rows (the last:
     the grid-stride loop), source strides 1 and 4.
  3. tg_rollout_begin on six regions carved out of one arena: region sizes with 8-, 12- and 15-byte tails, and the shape whose
     16-byte units exceed the launch's grid; tg_rollout_finish_stats / tg_rollout_finish on zero and negative lengths, M around the
     2,048-entry block and past the 256-block cap; tg_params_differ on 1, 3 and 64 tensors whose boundaries fall inside a block.

Every output buffer is allocated with every byte 0xA5 and with guard rows (bytes); what a kernel must not touch is asserted to be
0xA5 still.  Every launch stays inside its allocations: the row buffers hold M + GUARD rows, whatever the kernel counts."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import row_kernels_ref as R

pytestmark = pytest.mark.gpu

CASES = R.compact_cases()
ON_CASES = R.on_cases()
GUARD = 5


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _filled(shape, dtype, dev):
    """A tensor whose every byte is 0xA5."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((nbytes,), R.SENTINEL_BYTE, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)


_INT = {torch.bfloat16: (torch.int16, np.uint16), torch.float32: (torch.int32, np.uint32), torch.int32: (torch.int32, np.uint32),
        torch.int64: (torch.int64, np.int64), torch.uint8: (torch.uint8, np.uint8), torch.float64: (torch.int64, np.uint64)}


def _bits(t):
    ti, ni = _INT[t.dtype]
    return t.detach().contiguous().view(ti).cpu().numpy().view(ni)


def _untouched(t):
    return bool((t.detach().contiguous().view(-1).view(torch.uint8) == R.SENTINEL_BYTE).all())


def _to(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. count and compaction
# --------------------------------------------------------------------------------------------------------------------------------
def _mask_at(mask, k, dev):
    """The [T][n] mask k bytes into an allocation whose other bytes are 255: a read before or past the mask would count them."""
    M = mask.size
    buf = torch.full((M + 16,), 255, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[k:k + M] = torch.from_numpy(np.array(mask)).reshape(-1).to(dev)
    view = buf[k:k + M].view(mask.shape)
    assert view.data_ptr() % 4 == k % 4 and view.is_contiguous()
    return view


def _device_inputs(c, x, dev):
    d = SimpleNamespace(obs=_to(x.obs, dev), act=_to(x.act, dev), src0=_to(x.src0, dev), src1=_to(x.src1, dev), moments=_to(x.moments, dev))
    if d.act is None:
        d.act = torch.zeros(1, dtype=torch.float32, device=dev)     # (never read: no act_rows)
    return d


def _compact(K, c, d, mask_t, rows_cap, expected_rows, obs_norm=None):
    """One tg_learn_count + tg_learn_compact[_on] into fresh 0xA5 buffers of M + GUARD rows -> row_kernels_ref.compact_image's layout."""
    dev = mask_t.device
    M = c.T * c.n
    alloc = M + GUARD
    wbytes = K.learn_count_workspace(M)
    assert wbytes == (R.chunks(M) + 4) * 4
    work, total = _filled(wbytes // 4, torch.int32, dev), _filled(2, torch.int64, dev)
    K.learn_count(mask_t, expected_rows, work, total)
    idx = _filled(alloc, torch.int64, dev)
    xin = _filled((alloc, c.in_pad), torch.bfloat16 if c.bf16 else torch.float32, dev)
    act_rows = None if c.A is None else _filled((alloc, c.A), torch.float32, dev)
    dst0 = None if d.src0 is None else _filled(alloc, torch.float32, dev)
    dst1 = None if d.src1 is None else _filled(alloc, torch.float32, dev)
    traj = SimpleNamespace(mask=mask_t, obs=d.obs, act=d.act, n=c.n, T=c.T, S=c.S, A=c.A or 1)
    K.learn_compact(traj, work, rows_cap, xin, c.ones_col, act_rows, idx, src0=d.src0, dst0=dst0, src1=d.src1, dst1=dst1,
                    moments=d.moments, norm_mode=c.norm_mode or 0, group_size=c.group_size if d.moments is not None else 0, obs_norm=obs_norm)
    torch.cuda.synchronize()
    tot = total.cpu().numpy()
    got = {"offsets": _bits(work), "total": int(tot[0]), "idx": _bits(idx), "xin": _bits(xin)}
    for name, t in (("act_rows", act_rows), ("dst0", dst0), ("dst1", dst1)):
        if t is not None:
            got[name] = _bits(t)
    return got, int(tot[1]), SimpleNamespace(idx=idx, dst0=dst0)


def _sweep(K, c, x, d, ref, dev, obs_norm=None):
    M, count = c.T * c.n, ref.total
    alloc = M + GUARD
    caps = sorted({M, count, max(count - 1, 0), 0}, reverse=True)
    mask0 = _mask_at(x.mask, 0, dev)
    for cap in caps:
        for expected, flag in ((-1, 0), (count, 0), (count + 1, 1), (count - 1, 1 if count >= 1 else 0)):
            if cap != M and expected != -1:
                continue
            got, mismatch, bufs = _compact(K, c, d, mask0, cap, expected, obs_norm)
            assert mismatch == flag, (c.id, cap, expected, mismatch)
            R.check_compact(got, R.capped(ref, cap), alloc, tag=f"{c.id} cap {cap}")
            if cap == M and expected == -1 and d.moments is not None and count:
                # the stand-alone normalisation kernel (tied to fp64 by test_returns_loss_fp64.py), gathered: the same bits
                gn = K.group_normalize(d.src0, mask0, d.moments, c.norm_mode, c.group_size).reshape(-1)[bufs.idx[:count]]
                assert torch.equal(gn.view(torch.int32), bufs.dst0[:count].view(torch.int32)), c.id
    for k in (1, 2, 3):                                            # the unaligned branch of load_mask4
        got, mismatch, _ = _compact(K, c, d, _mask_at(x.mask, k, dev), M, count, obs_norm)
        assert mismatch == 0
        R.check_compact(got, ref, alloc, tag=f"{c.id} mask offset {k}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_count_and_compact_match_the_restatement(tg, dev, c):
    K = tg.hip_ops
    if (c.T, c.n) == R.BIG:
        R.check_shape_table(torch.cuda.get_device_properties(dev).multi_processor_count)
    x = R.case_inputs(c)
    R.check_pattern(x.mask, c.pattern)
    _sweep(K, c, x, _device_inputs(c, x, dev), R.case_ref(c, x), dev)


@pytest.mark.parametrize("c", ON_CASES, ids=[c.id for c in ON_CASES])
def test_compact_on_normalises_and_clamps_the_observation(tg, dev, c):
    """tg_learn_compact_on with a general table (some values beyond a finite clip, a NaN observation in a valid row) against the
    restatement; with mean 0, rstd 1 and no clamp: the plain entry's rows, bit for bit."""
    K = tg.hip_ops
    x = R.case_inputs(c)
    d = _device_inputs(c, x, dev)
    ref = R.case_ref(c, x)
    assert x.nan_at is not None and ref.total > 100
    on = SimpleNamespace(table=_to(x.obs_tab.reshape(-1), dev), clip_value=float(c.on))
    _sweep(K, c, x, d, ref, dev, obs_norm=on)
    r = int(np.searchsorted(ref.idx, x.nan_at))
    mask0 = _mask_at(x.mask, 0, dev)
    got, _, _ = _compact(K, c, d, mask0, c.T * c.n, -1, on)
    v = got["xin"][r, c.S - 1]
    assert ((v & 0x7F80) == 0x7F80 and (v & 0x7F)) if c.bf16 else np.isnan(v.view(np.float32)), "the NaN observation must stay a NaN"
    ident = SimpleNamespace(table=_to(R.identity_table(c.S).reshape(-1), dev), clip_value=math.inf)
    got_id, _, _ = _compact(K, c, d, mask0, c.T * c.n, -1, ident)
    got_plain, _, _ = _compact(K, c, d, mask0, c.T * c.n, -1, None)
    assert set(got_id) == set(got_plain)
    for name in got_plain:
        assert R._same_bits(np.asarray(got_id[name]), np.asarray(got_plain[name])), (c.id, name)
    R.check_compact(got_plain, R.case_ref(c, x, obs_tab=None), c.T * c.n + GUARD, tag=c.id + " plain")


# --------------------------------------------------------------------------------------------------------------------------------
# 2. scatter, gather, bootstrap values
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("rows", R.ROW_COUNTS)
def test_scatter_and_gather_rows_match_the_restatement(tg, dev, rows, stride):
    K = tg.hip_ops
    src, idx, cells = R.row_inputs(rows, stride)
    src_d, idx_d, table = _to(src, dev), _to(idx, dev), _to(R.AFFINE_TABLE, dev)
    assert rows == 0 or src_d.stride(0) == stride               # (an empty tensor's strides are torch's business: 0 on the device)
    blank = R.sentinel(np.float32, (cells,))
    for tab_d, tab in ((None, None), (table, R.AFFINE_TABLE)):
        dst = _filled(cells, torch.float32, dev)
        K.scatter_rows(src_d, idx_d, dst, table=tab_d)
        torch.cuda.synchronize()
        want = R.scatter_ref(src, idx, blank, tab)                 # entries outside idx keep their 0xA5 bytes
        assert np.array_equal(_bits(dst), R.f32_bits(want)), (rows, stride, tab is not None)
    grid0, grid1 = _to(np.random.default_rng(rows).standard_normal(cells).astype(np.float32), dev), dst
    for second in (False, True):
        d0, d1 = _filled(rows + GUARD, torch.float32, dev), _filled(rows + GUARD, torch.float32, dev)
        K.gather_rows2(idx_d, grid0, d0, grid1 if second else None, d1 if second else None)
        torch.cuda.synchronize()
        w0, w1 = R.gather2_ref(idx, grid0.cpu().numpy(), R.sentinel(np.float32, (rows + GUARD,)), grid1.cpu().numpy() if second else None,
                               R.sentinel(np.float32, (rows + GUARD,)) if second else None)
        assert np.array_equal(_bits(d0), R.f32_bits(w0)) and (np.array_equal(_bits(d1), R.f32_bits(w1)) if second else _untouched(d1))
        if second and rows:
            assert np.array_equal(_bits(d1[:rows]), R.f32_bits(R.affine_ref(src[:, 0], R.AFFINE_TABLE)))      # scatter, then gather: the rows


@pytest.mark.parametrize("n", [1, 257, R.GRID_CAP_ROWS + 3])
def test_boot_values_affine_matches_the_restatement(tg, dev, n):
    K = tg.hip_ops
    src, _, _ = R.row_inputs(n, 4)
    v = _to(src, dev)[:, 0]
    assert v.stride(0) == 4
    timeout = (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)
    timeout[0], timeout[-1] = 1, n == 1
    buf = _filled(n + 2 * GUARD, torch.float32, dev)
    out = buf[GUARD:GUARD + n]
    K.boot_values_affine(v, _to(timeout, dev), _to(R.AFFINE_TABLE, dev), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), R.f32_bits(R.boot_affine_ref(src[:, 0], timeout, R.AFFINE_TABLE)))
    assert _untouched(buf[:GUARD]) and _untouched(buf[GUARD + n:])
    zeroed = out.cpu().numpy()[timeout == 0]                       # a slot without a timeout: +-0, the product with 0.0f
    assert n == 1 or (zeroed.size and not zeroed.any())


# --------------------------------------------------------------------------------------------------------------------------------
# 3. the launches around a rollout
# --------------------------------------------------------------------------------------------------------------------------------
def _traj(N, base, offs, T, n, f64):
    tr = N.Traj()
    tr.d_obs, tr.d_act, tr.d_rew, tr.d_mask, tr.d_len, tr.d_counters = [base + o for o in offs]
    tr.n, tr.horizon, tr.dtype = n, T, N.dtype_code(torch.float64 if f64 else torch.float32)
    return tr


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("T,n,S,A", R.BEGIN_SHAPES)
def test_rollout_begin_clears_the_six_buffers_and_nothing_else(tg, dev, T, n, S, A, f64):
    N = tg._native
    sizes = R.region_bytes(T, n, S, A, f64)
    offs, total = R.arena_layout(sizes)
    arena = _filled(total, torch.uint8, dev)
    assert arena.data_ptr() % 16 == 0 and offs[-1] + sizes[-1] + 32 <= total
    st = N.stream_ptr(dev)
    if T * n < 100:                                                # a buffer off the 16-byte grid is refused, nothing is written
        for k in range(6):
            bad = list(offs)
            bad[k] += 4
            tr = _traj(N, arena.data_ptr(), bad, T, n, f64)
            assert N.load().tg_rollout_begin(C.byref(tr), S, A, st) == N.TG_ERR_ARG and b"aligned" in N.load().tg_last_error()
        torch.cuda.synchronize()
        assert _untouched(arena)
    tr = _traj(N, arena.data_ptr(), offs, T, n, f64)
    N.check(N.load().tg_rollout_begin(C.byref(tr), S, A, st), "tg_rollout_begin")
    torch.cuda.synchronize()
    R.check_arena(arena.cpu().numpy(), offs, sizes, tag=f"rollout_begin {T}x{n} f64={f64}")


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("T,n", R.FINISH_SHAPES)
def test_rollout_finish_and_finish_stats_count_ended_slots_only(tg, dev, T, n, f64):
    """Lengths in [1, T], zeros and negatives (a running Pendulum slot): both entries count max(len, 0) and #(len > 0); the reward
    sum within the bound of a double sum in any order, and the same bits on a second call; the RNG stream advances by one."""
    N = tg._native
    lib, st = N.load(), N.stream_ptr(dev)
    ln, rew = R.finish_inputs(T, n, f64)
    ref = R.finish_ref(ln, rew, (13, 41))
    ln_d, rew_d = _to(ln, dev), _to(rew, dev)
    tr = N.Traj()
    tr.d_len, tr.d_rew, tr.n, tr.horizon, tr.dtype = ln_d.data_ptr(), rew_d.data_ptr(), n, T, N.dtype_code(rew_d.dtype)
    assert lib.tg_rollout_finish_stats_workspace() == 256 * 8
    sums = []
    rng = torch.tensor([13, 41], dtype=torch.int64, device=dev)
    for call, rng_arg in enumerate((rng, rng, None)):
        counters = _filled(4 + GUARD, torch.int64, dev)
        stats, work = _filled(3 + GUARD, torch.float64, dev), _filled(256 + GUARD, torch.float64, dev)
        tr.d_counters = counters.data_ptr()
        N.check(lib.tg_rollout_finish_stats(C.byref(tr), None if rng_arg is None else rng_arg.data_ptr(), stats.data_ptr(), work.data_ptr(), st),
                "tg_rollout_finish_stats")
        torch.cuda.synchronize()
        got = counters.cpu().numpy().view(np.uint64)
        R.check_finish(got[:2], ref, tag=f"finish_stats {T}x{n}")
        assert _untouched(counters[2:]) and _untouched(stats[3:]) and _untouched(work[256:])
        s = stats.cpu().numpy()
        assert s[1] == ref.stats1 == n and s[2] == ref.stats2 == float(got[0])
        assert abs(s[0] - ref.reward_sum) <= ref.reward_bound, (s[0], ref.reward_sum, ref.reward_bound)
        sums.append(s[:1].view(np.uint64)[0])
        assert rng.cpu().tolist() == [13, 41 + min(call + 1, 2)]    # NULL d_rng: the call succeeds, the stream stands
    assert sums[0] == sums[1] == sums[2]
    counters = _filled(4 + GUARD, torch.int64, dev)
    tr.d_counters = counters.data_ptr()
    N.check(lib.tg_rollout_finish(C.byref(tr), st), "tg_rollout_finish")
    torch.cuda.synchronize()
    R.check_finish(counters.cpu().numpy().view(np.uint64)[:2], ref, tag=f"finish {T}x{n}")
    assert _untouched(counters[2:])


@pytest.mark.parametrize("n_tensors", list(R.DIFFER_TABLES))
def test_params_differ_compares_bits_of_every_element(tg, dev, n_tensors):
    N = tg._native
    lib, st = N.load(), N.stream_ptr(dev)
    for name, (pairs, want) in R.differ_cases(n_tensors).items():
        keep = [(_to(a, dev), _to(b, dev)) for a, b in pairs]
        rows, first = [], 0
        for a, b in keep:
            rows.append([a.data_ptr(), b.data_ptr(), 0, 0, first])
            first += a.numel()
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        for preset in (0, 1):                                      # the kernel ORs: a flag that was 1 stays 1
            buf = _filled(3, torch.int32, dev)
            buf[1] = preset
            N.check(lib.tg_params_differ(table.data_ptr(), n_tensors, first, buf[1:].data_ptr(), st), "tg_params_differ")
            torch.cuda.synchronize()
            assert int(buf[1]) == (want | preset) == (R.differ_ref(pairs) | preset), (n_tensors, name, preset)
            assert _untouched(buf[:1]) and _untouched(buf[2:])
