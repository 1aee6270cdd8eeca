"""The device optimizers (fdr_optim.hip: Adam, AdamW, SGD in the learner's apply launch) on the GPU:

* opt_apply_cb_kernel against tests/optim_ref.py, one step, at the column-block and ticket-tile seams, for every case
  of optim_ref.CASES at step 1 (first-step momentum buffer, bias corrections) and at step 7 from a non-zero state:
  theta and the state rows within the allowances of optim_ref (4 x what torch's own CPU optimizers show, measured by
  tests/test_optim_ref.py), out = [||d theta||, ||fl32(-g)||] to 1e-12 against the kernel's own theta, theta_hist
  bit-equal, the ticket counter left zero, a repeat on restored inputs bit-equal;
* the moments form (g to 1e-12 against learner_ref, theta within the allowances);
* fd_step_opt / fd_step_mix_opt bit-equal to fd_grad_fused* followed by opt_step;
* FiniteDifferences with torch.optim.Adam / SGD(momentum) / the mixed objective: three steps against the restatement
  driven by the learner's own gradient_memory, and optimizer.state_dict() carrying the state -- on a build where the
  learner ignores the optimizer (a DSGD step at Adam's lr) this test fails;
* the generic route (RMSprop, Adam(amsgrad=True)) against torch stepping a CPU copy; a DSGD learner bit-equal to
  engine.fd_step;
* SequentialRunner(opt_fn=torch.optim.Adam).
"""
import copy

import numpy as np
import pytest
import torch

import learner_cases as lc
import learner_ref as ref
import optim_ref as oref
from learner_cases import PR, SIGMA

pytestmark = pytest.mark.gpu

TOL = 1e-12
NAN = float("nan")
OPT_P = (1, 2, 255, 256, 257, 1023, 1025, 65536, 65537, 131100)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy()


def state_inputs(kind, h, P, t):
    """The f32 state rows a step number t starts from: zeros at t == 1 (SGD's buffer: NaN -- the first step must not
    read it), a non-zero state at t > 1.  None for rows the kind does not have."""
    rs = np.random.RandomState(P + 31 * t)
    if kind == "sgd":
        if h["momentum"] == 0:
            return None, None
        return (np.full(P, NAN, np.float32) if t == 1 else rs.randn(P).astype(np.float32)), None
    if t == 1:
        return np.zeros(P, np.float32), np.zeros(P, np.float32)
    return (rs.randn(P) * 0.3).astype(np.float32), ((rs.randn(P) * 0.5) ** 2).astype(np.float32)


def spec(eng, kind, h, t, s0, s1):
    kw = {k: v for k, v in h.items() if k != "lr"}
    return eng.OptSpec(kind, h["lr"], t, s0, s1, **kw)


def opt_counter(eng):
    """The standalone step's workspace: its ticket counter is the first 256 bytes."""
    ws = [buf for (key, _dev), buf in eng._WS.items() if key == "opt"]
    assert len(ws) == 1
    return ws[0][:256]


def check_step(kind, h, t, theta0, g_used, s0_in, s1_in, theta_d, s0_d, s1_d, out, what):
    """theta / state within the allowance of optim_ref; out against the norms of the kernel's own theta."""
    r = oref.step(kind, h, t, theta0, g_used, s0_in, s1_in)
    got = host(theta_d)
    ks = oref.shown_k(r, theta0, got, host(s0_d), host(s1_d))
    assert max(ks) <= oref.K[kind], "%s: k (theta, state0, state1) = %r, allowance %.1f" % (what, ks, oref.K[kind])
    upd, gn = oref.norms(theta0, got, r.grad)
    for a, b in ((out[0], upd), (out[1], gn)):
        assert abs(a - b) <= TOL * b or (a == 0 and b == 0), (what, a, b)
    return ks


@pytest.mark.parametrize("case", sorted(oref.CASES))
@pytest.mark.parametrize("P", OPT_P)
def test_kernel_single_step_against_the_restatement(eng, P, case):
    kind, kw = oref.CASES[case]
    h = oref.hyper(kind, **kw)
    theta0, g = lc.dsgd_inputs(P)
    gd = dev(g)
    worst = 0.0
    for t in (1, 7):
        s0_in, s1_in = state_inputs(kind, h, P, t)
        runs = []
        for _ in range(2):   # the second on restored inputs: bit-equal
            th, s0, s1 = dev(theta0), dev(s0_in), dev(s1_in)
            hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
            out = eng.opt_step(th, gd, False, spec(eng, kind, h, t, s0, s1), theta_hist=hist)
            assert not opt_counter(eng).any().item(), "ticket counter left non-zero"
            assert host(hist).tobytes() == host(th).tobytes()
            runs.append((host(th), host(s0), host(s1), host(out)))
        a, b = runs
        for x, y in zip(a, b):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), "a repeat on restored inputs differs"
        ks = check_step(kind, h, t, theta0, g, s0_in, s1_in, dev(a[0]), dev(a[1]), dev(a[2]), a[3],
                        "%s P %d step %d" % (case, P, t))
        worst = max(worst, max(ks))
    print("opt_step %s P %d: worst k %.2f (allowance %.1f)" % (case, P, worst, oref.K[kind]))


def test_sgd_without_momentum_touches_no_state(eng):
    """momentum == 0 with a state row given: the row is neither read (NaN) nor written."""
    P = 1025
    theta0, g = lc.dsgd_inputs(P)
    h = oref.hyper("sgd", lr=1e-2)
    s0 = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
    th = dev(theta0)
    out = host(eng.opt_step(th, dev(g), False, spec(eng, "sgd", h, 3, s0, None)))
    assert torch.isnan(s0).all().item()
    check_step("sgd", h, 3, theta0, g, None, None, th, None, None, out, "sgd, stray state row")


@pytest.mark.parametrize("case,t", [("adam_b_eps_wd", 1), ("sgd_momentum", 7)])
@pytest.mark.parametrize("P", [257, 70001])
def test_moments_form(eng, P, case, t):
    kind, kw = oref.CASES[case]
    h = oref.hyper(kind, **kw)
    theta0, mom = lc.dsgd_moments_inputs(P)
    s0_in, s1_in = state_inputs(kind, h, P, t)
    th, s0, s1 = dev(theta0), dev(s0_in), dev(s1_in)
    g_out = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
    out = host(eng.opt_step(th, dev(mom), True, spec(eng, kind, h, t, s0, s1), g_out=g_out))
    gd = host(g_out)
    e = ref.rel_l2(gd, ref.grad_from_moments(mom, P))
    assert e <= TOL, e
    check_step(kind, h, t, theta0, gd, s0_in, s1_in, th, s0, s1, out, "%s moments P %d" % (case, P))
    assert not opt_counter(eng).any().item()


# ---- fused routes ------------------------------------------------------------------------------------------------
class DevCase(object):
    def __init__(self, c):
        self.table = dev(c.table)
        self.idx = dev(np.repeat(c.idx_dirs, c.lpd))
        self.sign, self.n2, self.r_all = dev(c.sign), dev(c.n2), dev(c.r_all)


def fused_counter(eng, mode):
    ws = [buf for (key, _dev), buf in eng._WS.items() if key == "fused_%d" % mode]
    assert len(ws) == 1
    return ws[0]


@pytest.mark.parametrize("case,t", [("adam", 1), ("adamw", 7), ("sgd_nesterov_wd", 7)])
@pytest.mark.parametrize("n_dirs,P", [(65, 1000), (130, 257), (2304, 1500)])
@pytest.mark.parametrize("mixed", [False, True])
def test_fused_step_equals_gradient_then_opt_step(eng, n_dirs, P, case, t, mixed):
    from fdr import _lib
    assert (n_dirs, P) in lc.PLAN_TABLE
    kind, kw = oref.CASES[case]
    h = oref.hyper(kind, **kw)
    c = lc.make_case(n_dirs, P, 2)
    d = DevCase(c)
    theta0 = lc.dsgd_inputs(P)[0]
    s0_in, s1_in = state_inputs(kind, h, P, t)
    rs = np.random.RandomState(n_dirs)
    ch = (d.r_all, dev(rs.randn(c.n_all)), dev(rs.rand(c.n_all)))
    pv, coefs = (PR, 0.1, 0.4), (0.6, 0.3, 0.1)
    res = []
    for fused in (True, False):
        th, s0, s1 = dev(theta0), dev(s0_in), dev(s1_in)
        g = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        sp = spec(eng, kind, h, t, s0, s1)
        if fused and mixed:
            out = eng.fd_step_mix_opt(d.table, d.idx, ch, pv, coefs, d.sign, d.n2, 2, SIGMA, th, sp, g=g, theta_hist=hist)
        elif fused:
            out = eng.fd_step_opt(d.table, d.idx, d.r_all, PR, d.sign, d.n2, 2, SIGMA, th, sp, g=g, theta_hist=hist)
        else:
            if mixed:
                eng.fd_grad_fused_mix(d.table, d.idx, ch, pv, coefs, 0, d.sign, d.n2, 2, SIGMA, P, out=g)
            else:
                eng.fd_grad_fused(d.table, d.idx, d.r_all, PR, 0, d.sign, d.n2, 2, SIGMA, P, out=g)
            out = eng.opt_step(th, g, False, sp, theta_hist=hist)
        mode = _lib.FDR_WEIGHT_ZSCORE_MIX if mixed else _lib.FDR_WEIGHT_ZSCORE
        cb = int(_lib.lib.fdr_fd_grad_fused_counter_bytes(n_dirs, P))
        assert not fused_counter(eng, mode)[:cb].any().item(), "fused counters left non-zero"
        res.append([host(x) for x in (g, th, s0, s1, hist, out)])
    for name, a, b in zip(("g", "theta", "state0", "state1", "theta_hist", "out"), *res):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), name
    assert np.isfinite(res[0][1]).all() and res[0][4].tobytes() == res[0][1].tobytes()
    check_step(kind, h, t, theta0, res[0][0], s0_in, s1_in, dev(res[0][1]), dev(res[0][2]), dev(res[0][3]), res[0][5],
               "fused %s" % case)


# ---- the learner -------------------------------------------------------------------------------------------------
N_DIRS = 64


def make_learner(opt_fn, objective="reward", seed=124, **opt_kw):
    from learner import FiniteDifferences
    from policies import MujocoPolicy
    from utils import AdaptiveOmega, SharedNoiseTable
    torch.manual_seed(seed)
    pol = MujocoPolicy(17, 6, seed=seed)
    table = SharedNoiseTable(200_000, pol.num_params, random_seed=seed)
    omega = AdaptiveOmega()
    omega.omega = 0.3
    opt = opt_fn(pol.parameters(), **opt_kw)
    return pol, table, opt, FiniteDifferences(pol, opt, omega, table, noise_std=SIGMA, ent_coef=0.1,
                                              objective=objective)


def make_batch(eng, learner, pol, table, rs):
    """An antithetic FDBatch of N_DIRS directions with synthetic returns (and novelty / entropy channels)."""
    from learner import FDBatch
    P = pol.num_params
    idx = np.repeat(table.sample_batch(N_DIRS), 2)
    sign = np.tile(np.array([1, -1], np.int8), N_DIRS)
    idx_d, sign_d = dev(idx), dev(sign)
    n2 = eng.fd_lambda_norms(table.device_table(), idx_d, sign_d, None, SIGMA, None, P)
    n = 2 * N_DIRS
    return FDBatch(dev(rs.randn(n) * 3 + 1), dev(rs.rand(n)), dev(np.full(n, 10, np.int64)), n2, idx_d, sign_d, idx,
                   sign, learner.epoch, lanes_per_dir=2, novelty=dev(rs.rand(n)))


def flat_state(opt, key):
    sd = opt.state_dict()["state"]
    return np.concatenate([host(sd[i][key]).reshape(-1) for i in sorted(sd)])


@pytest.mark.parametrize("name,objective", [("adam", "reward"), ("sgd_momentum", "reward"), ("adam", "mixed")])
def test_learner_steps_with_the_given_optimizer(eng, name, objective):
    """Three learner steps: theta and the optimizer state against the restatement fed the learner's own
    gradient_memory; state_dict() carries the moments and the step count.  Where the learner runs DSGD whatever the
    optimizer (the behaviour before the device optimizers), theta moves by lr sqrt(P) in norm and this fails."""
    kind, kw = oref.CASES[name]
    h = oref.hyper(kind, **kw)
    if kind == "sgd":
        pol, table, opt, L = make_learner(torch.optim.SGD, objective, lr=h["lr"], momentum=h["momentum"])
    else:
        pol, table, opt, L = make_learner(torch.optim.Adam, objective, lr=h["lr"])
    P = pol.num_params
    rs = np.random.RandomState(5)
    s0 = s1 = np.zeros(P, np.float32)
    for t in (1, 2, 3):
        theta0 = pol.get_trainable_flat().copy()
        upd = L.step(make_batch(eng, L, pol, table, rs), 0.75, 0.1, 0.4)
        g = host(L.gradient_memory)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        r = oref.step(kind, h, t, theta0, g, s0, s1)
        got = pol.get_trainable_flat()
        theta_only = oref.Step(theta=r.theta, s_theta=r.s_theta, state0=None, state1=None, s_state0=None,
                               s_state1=None)
        k_theta = oref.shown_k(theta_only, theta0, got)[0]     # first: is this the optimizer's step at all?
        assert k_theta <= oref.K[kind], "step %d: theta k %.3g, allowance %.1f" % (t, k_theta, oref.K[kind])
        n0 = flat_state(opt, "momentum_buffer" if kind == "sgd" else "exp_avg")
        n1 = None if kind == "sgd" else flat_state(opt, "exp_avg_sq")
        ks = oref.shown_k(r, theta0, got, n0, n1)
        assert max(ks) <= oref.K[kind], "step %d: k %r, allowance %.1f" % (t, ks, oref.K[kind])
        want_upd, want_gn = oref.norms(theta0, got, r.grad)
        assert abs(upd - want_upd) <= TOL * want_upd
        assert abs(L._out[1].item() - want_gn) <= TOL * want_gn
        assert host(L.policy_history[-1][0]).tobytes() == got.tobytes() and L.policy_history[-1][1] == t
        s0, s1 = n0, n1
    sd = opt.state_dict()["state"]
    assert len(sd) == len(list(pol.parameters()))
    if kind != "sgd":
        assert all(float(sd[i]["step"]) == 3 for i in sd)
    assert opt.steps == 3 and L.epoch == 3


def test_learner_adopts_a_loaded_state_dict(eng):
    """load_state_dict replaces the published views: the next step starts from the loaded values and step count."""
    h = oref.hyper("adam", lr=1e-2)
    pol, table, opt, L = make_learner(torch.optim.Adam, lr=1e-2)
    rs = np.random.RandomState(6)
    for _ in range(2):
        L.step(make_batch(eng, L, pol, table, rs), 0.75, 0, 0)
    saved = copy.deepcopy(opt.state_dict())   # state_dict() hands out the live tensors
    m2, v2 = flat_state(opt, "exp_avg").copy(), flat_state(opt, "exp_avg_sq").copy()
    L.step(make_batch(eng, L, pol, table, rs), 0.75, 0, 0)          # moves the state on
    opt.load_state_dict(saved)                                       # back to after step 2
    theta0 = pol.get_trainable_flat().copy()
    L.step(make_batch(eng, L, pol, table, rs), 0.75, 0, 0)
    r = oref.step("adam", h, 3, theta0, host(L.gradient_memory), m2, v2)
    ks = oref.shown_k(r, theta0, pol.get_trainable_flat(), flat_state(opt, "exp_avg"), flat_state(opt, "exp_avg_sq"))
    assert max(ks) <= oref.K_ADAM, ks
    assert all(float(s["step"]) == 3 for s in opt.state_dict()["state"].values())


def test_lr_scheduler_is_honoured(eng):
    """The hyperparameters are read from param_groups[0] at every step."""
    pol, table, opt, L = make_learner(torch.optim.SGD, lr=1e-2)
    rs = np.random.RandomState(7)
    for lr in (1e-2, 1e-3):
        opt.param_groups[0]["lr"] = lr
        theta0 = pol.get_trainable_flat().copy()
        L.step(make_batch(eng, L, pol, table, rs), 0.75, 0, 0)
        r = oref.step("sgd", oref.hyper("sgd", lr=lr), 1, theta0, host(L.gradient_memory))
        assert max(oref.shown_k(r, theta0, pol.get_trainable_flat())) <= oref.K_SGD


@pytest.mark.parametrize("which", ["rmsprop", "adam_amsgrad"])
def test_generic_route_equals_torch_on_a_cpu_copy(eng, which):
    """Optimizers the device path does not take run the reference's literal sequence: the same as torch stepping a CPU
    copy of theta with the same fl32(-g), within the Adam allowance (the magnitude handled: the step's own)."""
    make = {"rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=1e-2),
            "adam_amsgrad": lambda ps: torch.optim.Adam(ps, lr=1e-2, amsgrad=True)}[which]
    pol, table, opt, L = make_learner(lambda ps: make(ps))
    assert L.opt_route.route == "generic"
    cpu = torch.nn.Parameter(torch.from_numpy(pol.get_trainable_flat().copy()))
    copt = make([cpu])
    rs = np.random.RandomState(8)
    for t in (1, 2, 3):
        theta0 = pol.get_trainable_flat().copy()
        upd = L.step(make_batch(eng, L, pol, table, rs), 0.75, 0, 0)
        g32 = oref.grad32(host(L.gradient_memory))
        cpu.grad = torch.from_numpy(g32.copy())
        copt.step()
        got, want = pol.get_trainable_flat(), cpu.detach().numpy()
        step = np.abs(want.astype(np.float64) - theta0)
        err = np.abs(got.astype(np.float64) - want)
        bound = np.spacing(np.maximum(np.abs(theta0), np.abs(want))) + oref.K_ADAM * 2.0 ** -24 * step
        assert (err <= bound).all(), (t, float((err / np.maximum(bound, 1e-300)).max()))
        d = (theta0 - got).astype(np.float64)
        assert abs(upd - np.sqrt((d * d).sum())) <= 1e-6 * upd
        assert abs(L._out[1].item() - np.sqrt((g32.astype(np.float64) ** 2).sum())) <= 1e-6 * L._out[1].item()
        with torch.no_grad():
            cpu.copy_(torch.from_numpy(got))   # compare step by step: the next one starts from the device's theta


def test_dsgd_learner_is_still_fd_step(eng):
    """A DSGD learner stepped beside the others is bit for bit what engine.fd_step gives."""
    from dsgd import DSGD
    pol, table, opt, L = make_learner(DSGD, lr=1e-2)
    assert L.opt_route.route == "dsgd"
    rs = np.random.RandomState(9)
    for _ in range(2):
        b = make_batch(eng, L, pol, table, rs)
        th = pol.flat.detach().clone()
        opt.adjust_lr(L.omega)
        g = torch.empty(pol.num_params, dtype=torch.float64, device="cuda")
        out = eng.fd_step(table.device_table(), b.idx, b.reward, 0.75, b.sign, b.norm2, 2, SIGMA, th, opt.lr,
                          opt.lr_scale, g=g)
        upd = L.step(b, 0.75, 0, 0)
        assert host(pol.flat).tobytes() == host(th).tobytes()
        assert host(L.gradient_memory).tobytes() == host(g).tobytes()
        assert upd == out[0].item()


def test_sequential_runner_with_adam(eng):
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id="CartPole-v1", opt_fn=torch.optim.Adam, learning_rate=0.01, batch_size=16,
                         episode_len=20, noise_table_size=200_000, verbose=False)
    assert r.learner.opt_route.route == "device" and r.learner.opt_route.kind == "adam"
    r.train(2)
    assert len(r.history) == 2 and r.learner.epoch == 2
    (before, e1), (after, e2) = r.learner.policy_history[-2:]
    assert (e1, e2) == (1, 2) and host(after).tobytes() == r.policy.get_trainable_flat().tobytes()
    d = (host(before) - host(after)).astype(np.float64)
    want = float(np.sqrt((d * d).sum()))
    assert want > 0 and abs(r.history[-1]["Update Magnitude"] - want) <= TOL * want
    # Adam's first steps move every parameter by about lr: nothing like DSGD's lr sqrt(P) lr_scale
    assert np.abs(d).max() <= 0.011
    sd = r.learner.gradient_optimizer.state_dict()["state"]
    assert all(float(s["step"]) == 2 for s in sd.values())
