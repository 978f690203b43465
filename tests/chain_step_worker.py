"""The oracle's two-update learn() at the chain-kernel net shapes, for tests/test_oracle_golden.py::test_learn_at_chain_kernel_shapes.

Started as a fresh child process: `python chain_step_worker.py KIND TAG S A OUT.pt`, with PINNED_CPU_ENV in its environment.  The
fixtures it is compared with (oracle/tools/gen_goldens.py gen_chain_shape_steps) were written under the same CPU numerics: MKL's
reproducible AVX2 branch, ATen and oneDNN kernels capped at AVX2, one thread.  Without the pin the comparison depends on the host
CPU: any change of fp32 summation order (another thread count, another vendor's BLAS path) can flip the sign of a first-update
gradient entry that sits at rounding level, Adam's first step moves that weight by +-lr, and the second update's gradient lands
~1e-3 away (relative L2) from the fixture's."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# (read once, when MKL / ATen / oneDNN initialise: set in the environment of a fresh process, never in a running one)
PINNED_CPU_ENV = {"MKL_CBWR": "AVX2", "ATEN_CPU_CAPABILITY": "avx2", "ONEDNN_MAX_CPU_ISA": "AVX2"}


def run(kind, tag, S, A):
    """-> {"init", "first", "final", "last": {name: tensor}, "logs" (ppo) / "J" (grpo)}."""
    from conftest import keep_first_step_gradients, load_golden
    from oracle import learner as L

    g = load_golden(f"{kind}_step_{tag}.npz")
    hidden = tuple(int(h) for h in g["hidden"])
    torch.manual_seed(int(g["seed"]))
    pol = L.OraclePolicy(S, A, hidden, cov=float(g["cov"]), critic=kind == "ppo")
    nets = ("actor", "critic") if kind == "ppo" else ("actor",)
    named = lambda: [(f"{n}.{k}", p) for n in nets for k, p in getattr(pol, n).named_parameters()]
    out = {"init": {k: p.detach().clone() for k, p in named()}}
    opt = torch.optim.Adam(pol.parameters(), lr=float(g["lr"]))
    first = keep_first_step_gradients(opt, named)
    t = lambda k: torch.from_numpy(g[k])
    if kind == "ppo":
        logs = L.ppo_learn(pol, opt, t("obs"), t("act"), t("rew"), t("mask"), epsilon=0.2, gamma=float(g["gamma"]), c1=0.5, kl_coeff=0.5,
                           entropy_coeff=0.01, updates_per_iter=2)
        out["logs"] = [{"total": float(l["total"]), "critic": float(l["critic"])} for l in logs]
    else:
        old = L.OraclePolicy(S, A, hidden, cov=float(g["cov"]), critic=False)
        old.load_state_dict(pol.state_dict())
        gen = torch.Generator().manual_seed(int(g["seed"]))
        with torch.no_grad():
            for p_ in old.parameters():
                p_.add_(float(g["old_policy_perturbation"]) * torch.randn(p_.shape, generator=gen))
        out["J"] = [float(j) for j in L.grpo_learn(pol, old, opt, t("obs"), t("act"), t("rew"), t("mask"), epsilon=0.15,
                                                   gamma=float(g["gamma"]), updates_per_iter=2)]
    out["first"] = dict(first)
    out["final"] = {k: p.detach().clone() for k, p in named()}
    out["last"] = {k: p.grad.detach().clone() for k, p in named()}
    return out


if __name__ == "__main__":
    missing = {k: v for k, v in PINNED_CPU_ENV.items() if os.environ.get(k) != v}
    if missing:
        raise SystemExit(f"chain_step_worker.py needs {missing} in its environment (set before the process starts)")
    torch.set_num_threads(1)
    kind, tag, S, A, path = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    torch.save(run(kind, tag, S, A), path)
