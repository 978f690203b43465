"""DeviceActor.evaluate without a GPU: the declarations, the args struct, and the workspace entry's sizes and refusals (it reads widths alone)."""
import ctypes as C
import re

import policy_step_ref as R
import trajopt_grpo_amd as tg
from conftest import REPO
from trajopt_grpo_amd.policy_step import _widths

ENTRIES = ("tg_policy_eval_workspace", "tg_policy_eval_forward", "tg_policy_eval_backward", "tg_policy_eval_weight_grad")


def workspace(actor, critic, m):
    acts, grads, partial = (C.c_int64 * 2)(), (C.c_int64 * 2)(), C.c_int64()
    rc = tg._native.load().tg_policy_eval_workspace(C.byref(actor), C.byref(critic) if critic is not None else None, m, acts, grads,
                                                    C.byref(partial))
    return rc, list(acts), list(grads), partial.value


def test_entries_are_declared_bound_and_exported_and_the_abi_is_still_13():
    N, lib = tg._native, tg._native.load()
    header = open(f"{REPO}/include/trajopt_grpo_hip.h").read()
    for name in ENTRIES:
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header).group(1).split(",")
        assert len(declared) == len(N.SIGNATURES[name][1]) and hasattr(lib, name), name
    body = re.search(r"typedef struct tg_policy_eval_args \{(.*?)\} tg_policy_eval_args;", header, re.S).group(1)
    assert re.findall(r"\s([a-z_0-9]+);", body) == [name for name, _ in N.PolicyEvalArgs._fields_]
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
    assert callable(tg.DeviceActor.evaluate)


def test_workspace_sizes_follow_the_nets_and_the_row_count():
    actor, critic = R.make_net(20, 256, 2, 4, "ReLU", 0), R.make_net(20, 64, 1, 1, "Tanh", 1)
    rc, acts, grads, partial = workspace(_widths(actor), _widths(critic), 130)
    assert rc == 0 and acts == [2 * 130 * 256, 130 * 64]
    assert grads == [sum(p.numel() for p in actor.parameters()), sum(p.numel() for p in critic.parameters())]
    # 64 x 64 tiles (+ 64 bias sums): the actor's 4 + 16 + 4, the critic's 1 + 1; 130 rows are three 64-row slabs
    assert partial == (24 + 2) * 3 * (64 * 64 + 64)
    assert workspace(_widths(actor), None, 130)[1:3] == ([2 * 130 * 256, 0], [grads[0], 0])


def test_workspace_refuses_an_oversized_net_with_a_message():
    wide = _widths(R.make_net(20, 256, 2, 4, "ReLU", 0))
    wide.out_dim[0] = wide.in_dim[1] = wide.out_dim[1] = wide.in_dim[2] = 512
    assert workspace(wide, None, 64)[0] != 0 and "hidden width 512" in tg._native.load().tg_last_error().decode()
    five = _widths(R.make_net(20, 64, 2, 4, "ReLU", 0))
    five.out_dim[2] = 5
    assert workspace(five, None, 64)[0] != 0 and "5 head outputs" in tg._native.load().tg_last_error().decode()
    assert workspace(_widths(R.make_net(20, 64, 2, 4, "ReLU", 0)), None, 0)[0] != 0
