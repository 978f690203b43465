"""DeviceActor.rsample / .q_evaluate without a GPU: the declarations, the args struct, and the workspace entry's sizes and refusals (it
reads widths alone)."""
import ctypes as C
import re

import policy_step_ref as R
import trajopt_grpo_amd as tg
from conftest import REPO
from trajopt_grpo_amd.policy_step import _widths

ENTRIES = ("tg_policy_sac_grad_workspace", "tg_policy_rsample_forward", "tg_policy_rsample_backward", "tg_policy_q_eval_forward",
           "tg_policy_q_eval_backward", "tg_policy_sac_weight_grad")


def workspace(actor, q1, q2, A, m):
    acts, grads, partial = (C.c_int64 * 3)(), (C.c_int64 * 3)(), (C.c_int64 * 2)()
    ref = lambda t: C.byref(t) if t is not None else None
    rc = tg._native.load().tg_policy_sac_grad_workspace(ref(actor), ref(q1), ref(q2), A, m, acts, grads, partial)
    return rc, list(acts), list(grads), list(partial)


def test_entries_are_declared_bound_and_exported_and_the_abi_is_still_13():
    N, lib = tg._native, tg._native.load()
    header = open(f"{REPO}/include/trajopt_grpo_hip.h").read()
    for name in ENTRIES:
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header).group(1).split(",")
        assert len(declared) == len(N.SIGNATURES[name][1]) and hasattr(lib, name), name
    body = re.search(r"typedef struct tg_policy_sac_grad_args \{(.*?)\} tg_policy_sac_grad_args;", header, re.S).group(1)
    assert re.findall(r"\s([a-z_0-9]+);", body) == [name for name, _ in N.PolicySacGradArgs._fields_]
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
    assert callable(tg.DeviceActor.rsample) and callable(tg.DeviceActor.q_evaluate)


def test_workspace_sizes_follow_the_nets_and_the_row_count():
    actor, q1, q2 = R.make_net(20, 256, 2, 8, "ReLU", 0), R.make_net(24, 256, 2, 1, "ReLU", 1), R.make_net(24, 256, 1, 1, "ReLU", 2)
    rc, acts, grads, partial = workspace(_widths(actor), _widths(q1), _widths(q2), 4, 130)
    assert rc == 0 and acts == [2 * 130 * 256, 2 * 130 * 256, 130 * 256]
    assert grads == [sum(p.numel() for p in net.parameters()) for net in (actor, q1, q2)]
    # 64 x 64 tiles (+ 64 bias sums), 130 rows are three 64-row slabs.  The actor's launch: first layer 4, 256 x 256 layer 16, head 4
    # (a head's tiles hold its float64 partials); the critics' launch: Q1's 4 + 16 + 4 and Q2's 4 + 4
    assert partial == [24 * 3 * (64 * 64 + 64), (24 + 8) * 3 * (64 * 64 + 64)]
    assert workspace(None, _widths(q1), None, 4, 130)[1:] == ([0, acts[1], 0], [0, grads[1], 0], [0, 24 * 3 * (64 * 64 + 64)])
    assert workspace(_widths(actor), None, None, 4, 64)[3] == [24 * (64 * 64 + 64), 0]


def test_workspace_refuses_what_the_kernels_do_not_take_with_a_message():
    err = lambda: tg._native.load().tg_last_error().decode()
    wide = _widths(R.make_net(20, 256, 2, 8, "ReLU", 0))
    wide.out_dim[0] = wide.in_dim[1] = wide.out_dim[1] = wide.in_dim[2] = 512
    assert workspace(wide, None, None, 4, 64)[0] != 0 and "hidden width 512" in err()
    assert workspace(None, wide, None, 4, 64)[0] != 0 and "hidden width 512" in err()
    gaussian = _widths(R.make_net(20, 64, 2, 4, "ReLU", 0))
    assert workspace(gaussian, None, None, 4, 64)[0] != 0 and "4 head outputs, 8 expected" in err()
    assert workspace(None, _widths(R.make_net(4, 64, 2, 1, "ReLU", 0)), None, 4, 64)[0] != 0 and "no observation beside 4 actions" in err()
    assert workspace(_widths(R.make_net(20, 64, 2, 8, "ReLU", 0)), None, None, 4, 0)[0] != 0 and "m=0" in err()
    # the LDS verdict cannot be reached from widths the kernels take: the largest net (32 inputs, five 256-wide hidden layers) needs
    # 48 KiB of ring + 32 KiB of first layer + 6 KiB of biases and head forward, and less backward -- it is accepted
    assert workspace(None, _widths(R.make_net(32, 256, 5, 1, "ReLU", 0)), None, 4, 64)[0] == 0
