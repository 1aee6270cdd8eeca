"""CPU checks of the device optimizers' yardstick and boundary (no GPU needed):

* tests/optim_ref.py against the installed torch's own CPU optimizers, one step at a time from torch's state, over
  optim_ref.CASES: the k torch shows in the bound of optim_ref's docstring is printed per case and must stay within the
  allowances written there (4 x the largest k recorded per kind);
* the argument validation of fdr_opt_step / fdr_fd_step_opt / fdr_fd_step_mix_opt, rejected before any device work;
* describe_optimizer: which optimizers the learner steps on the device, which go through the generic route.
"""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as oref

N = 4096
STEPS = 6


def _torch_optimizer(kind, h, p):
    if kind == "sgd":
        return torch.optim.SGD([p], lr=h["lr"], momentum=h["momentum"], dampening=h["dampening"],
                               weight_decay=h["weight_decay"], nesterov=h["nesterov"])
    cls = torch.optim.Adam if kind == "adam" else torch.optim.AdamW
    return cls([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"])


def _state_rows(kind, opt, p):
    st = opt.state[p] if p in opt.state else {}
    if kind == "sgd":
        b = st.get("momentum_buffer")
        return (None if b is None else b.detach().numpy().copy()), None
    if not st:
        return np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32)
    return st["exp_avg"].detach().numpy().copy(), st["exp_avg_sq"].detach().numpy().copy()


@pytest.mark.parametrize("case", sorted(oref.CASES))
def test_torch_cpu_optimizers_against_the_restatement(case):
    kind, kw = oref.CASES[case]
    h = oref.hyper(kind, **kw)
    rs = np.random.RandomState(len(case) + 17)
    p = torch.nn.Parameter(torch.from_numpy((rs.randn(N) * 0.1).astype(np.float32)))
    opt = _torch_optimizer(kind, h, p)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, STEPS + 1):
        g = rs.randn(N) * oref.GRAD_SCALES[t - 1]
        theta_old = p.detach().numpy().copy()
        s0, s1 = _state_rows(kind, opt, p)
        ref = oref.step(kind, h, t, theta_old, g, s0, s1)
        p.grad = torch.from_numpy(oref.grad32(g).copy())
        opt.step()
        n0, n1 = _state_rows(kind, opt, p)
        ks = oref.shown_k(ref, theta_old, p.detach().numpy(), n0, n1)
        worst = [max(a, b) for a, b in zip(worst, ks)]
    print("torch %s CPU %s: k theta %.2f, state0 %.2f, state1 %.2f (allowance %.1f)"
          % (torch.__version__, case, worst[0], worst[1], worst[2], oref.K[kind]))
    assert max(worst) <= oref.K[kind], worst


def test_allowances_are_four_times_the_recorded_k():
    for kind in ("adam", "adamw", "sgd"):
        assert oref.K[kind] == 4 * oref.K_MEASURED[kind]
    assert (oref.K_ADAM, oref.K_ADAMW, oref.K_SGD) == (oref.K["adam"], oref.K["adamw"], oref.K["sgd"])


def test_restatement_first_step_closed_forms():
    """Step 1 from a zero state has closed forms: Adam moves every element by lr sign(grad) / (1 + eps / |grad|)
    (bias corrections cancel); SGD's momentum buffer is the gradient itself."""
    g = np.array([0.5, -2.0, 1e-3])
    theta = np.array([0.1, -0.2, 0.3], np.float32)
    z = np.zeros(3, np.float32)
    r = oref.step("adam", oref.hyper("adam", lr=1e-2), 1, theta, g, z, z)
    gr = oref.grad32(g).astype(oref.LD)
    want = theta.astype(oref.LD) - oref.LD(1e-2) * np.sign(gr) / (1 + oref.LD(1e-8) / np.abs(gr))
    assert np.max(np.abs(r.theta - want)) < 1e-17
    r = oref.step("sgd", oref.hyper("sgd", lr=0.1, momentum=0.9), 1, theta, g, None)
    assert np.array_equal(r.state0, gr)
    assert np.max(np.abs(r.theta - (theta.astype(oref.LD) - oref.LD(0.1) * r.state0))) < 1e-18


# ---- the C boundary ----------------------------------------------------------------------------------------------
GOOD = dict(kind=1, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, momentum=0.0, dampening=0.0,
            nesterov=0, step=1, state0=8, state1=8)   # 8: a non-NULL pointer that is never dereferenced
BAD = [
    (dict(kind=0), b"kind"), (dict(kind=4), b"kind"),
    (dict(step=0), b"step"), (dict(step=-3), b"step"),
    (dict(lr=-1e-3), b"lr"), (dict(lr=float("nan")), b"lr"), (dict(lr=float("inf")), b"lr"),
    (dict(eps=-1e-8), b"eps"), (dict(eps=float("inf")), b"eps"),
    (dict(beta1=1.0), b"beta1"), (dict(beta1=-0.1), b"beta1"), (dict(beta2=1.5), b"beta2"),
    (dict(beta2=float("nan")), b"beta2"),
    (dict(state0=None), b"state0"), (dict(state1=None), b"state1"),
    (dict(kind=2, state1=None), b"state1"),
    (dict(kind=3, momentum=0.9, state0=None), b"state0"),
    (dict(kind=3, nesterov=1, momentum=0.0), b"nesterov"),
    (dict(kind=3, nesterov=1, momentum=0.9, dampening=0.1), b"nesterov"),
]


def _opt_block(a):
    vp = ctypes.c_void_p
    return (a["kind"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"], a["momentum"], a["dampening"],
            a["nesterov"], a["step"], vp(a["state0"]), vp(a["state1"]))


def _entries(lib, a):
    """The three entry points with every other argument NULL / 0: the optimizer block is checked first."""
    blk = _opt_block(a)
    return {
        "fdr_opt_step": lambda: lib.fdr_opt_step(None, blk[0], None, None, 0, 0, *blk[1:], None, None, None, None, 0,
                                                 None),
        "fdr_fd_step_opt": lambda: lib.fdr_fd_step_opt(None, None, 0, None, 0, 0, None, 0, 0.0, None, None, 1, 0.1, 0,
                                                       None, *blk, None, None, None, None, 0, None),
        "fdr_fd_step_mix_opt": lambda: lib.fdr_fd_step_mix_opt(None, None, 0, None, 0, 0, None, None, None, 0, 0.0, 0.0,
                                                               0.0, 1.0, 0.0, 0.0, None, None, 1, 0.1, None, *blk, None,
                                                               None, None, None, 0, None),
    }


@pytest.mark.parametrize("entry", ["fdr_opt_step", "fdr_fd_step_opt", "fdr_fd_step_mix_opt"])
def test_optimizer_arguments_are_validated_without_gpu(entry):
    from fdr import _lib
    lib = _lib.lib
    for change, field in BAD:
        a = dict(GOOD)
        a.update(change)
        rc = _entries(lib, a)[entry]()
        err = lib.fdr_last_error()
        assert rc == _lib.FDR_ERR_INVALID, (change, rc)
        assert err.startswith(field + b":"), (change, err)
    # a valid optimizer block gets past it: the next complaint is about the NULL pointers
    assert _entries(lib, dict(GOOD))[entry]() == _lib.FDR_ERR_INVALID
    assert b"NULL" in lib.fdr_last_error()
    # SGD without momentum needs no state row
    a = dict(GOOD, kind=3, state0=None, state1=None)
    assert _entries(lib, a)[entry]() == _lib.FDR_ERR_INVALID and b"NULL" in lib.fdr_last_error()


def test_optimizer_constants_and_exports():
    import os
    import re
    from conftest import REPO
    from fdr import _lib
    hdr = open(os.path.join(REPO, "include", "fdr.h")).read()
    for name, val in (("ADAM", 1), ("ADAMW", 2), ("SGD", 3)):
        assert int(re.search(r"#define FDR_OPT_%s (\d+)" % name, hdr).group(1)) == val == getattr(_lib, "FDR_OPT_" + name)
    for name in ("fdr_opt_workspace_bytes", "fdr_opt_step", "fdr_fd_step_opt", "fdr_fd_step_mix_opt"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.version().startswith("fdr 0.5")
    # [256 B counter][2 x column-block partials, 256 B padded][256 B statistics]
    assert _lib.lib.fdr_opt_workspace_bytes(6092) == 256 + 2 * 256 + 256
    assert _lib.lib.fdr_opt_workspace_bytes(131100) == 256 + 2 * 4352 + 256
    assert _lib.lib.fdr_opt_workspace_bytes(0) == -1


# ---- the learner's optimizer description ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    from policies import MujocoPolicy
    return MujocoPolicy(17, 6, device="cpu")


def test_optimizer_description(policy):
    from dsgd import DSGD
    from learner.finite_differences import describe_optimizer
    ps = list(policy.parameters())
    d = describe_optimizer(policy, torch.optim.Adam(policy.parameters(), lr=1e-2))
    assert (d.route, d.kind) == ("device", "adam")
    d = describe_optimizer(policy, torch.optim.AdamW(policy.parameters(), lr=1e-2))
    assert (d.route, d.kind) == ("device", "adamw")
    d = describe_optimizer(policy, torch.optim.SGD(policy.parameters(), lr=1e-2, momentum=0.9, nesterov=True))
    assert (d.route, d.kind) == ("device", "sgd")
    d = describe_optimizer(policy, torch.optim.Adam(policy.parameters(), lr=1e-2, amsgrad=True))
    assert (d.route, d.why) == ("generic", "amsgrad")
    d = describe_optimizer(policy, torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-2))
    assert (d.route, d.why) == ("generic", "2 param groups")
    d = describe_optimizer(policy, torch.optim.Adam(policy.parameters(), lr=1e-2, maximize=True))
    assert (d.route, d.why) == ("generic", "maximize")
    d = describe_optimizer(policy, torch.optim.Adam(policy.parameters(), lr=torch.tensor(1e-2)))
    assert (d.route, d.why) == ("generic", "tensor hyperparameter")
    d = describe_optimizer(policy, torch.optim.Adam(ps[:-1], lr=1e-2))                      # not all of the policy
    assert d.route == "generic"
    d = describe_optimizer(policy, torch.optim.Adam([torch.nn.Parameter(torch.zeros(policy.num_params))], lr=1e-2))
    assert (d.route, d.why) == ("generic", "parameters other than the policy's")
    assert describe_optimizer(policy, torch.optim.RMSprop(policy.parameters(), lr=1e-2)).route == "generic"
    assert describe_optimizer(policy, DSGD(policy.parameters(), lr=1e-2)).route == "dsgd"
