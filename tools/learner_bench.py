"""Learner-kernel timings (GPU box): staged (fd_weights + fd_grad + dsgd) vs fused (fd_grad_fused [+ dsgd]) vs
one-launch fdr_fd_step, and the mixed objective's three entry points (fd_grad_fused mix, fd_step mix, fd_weights_mix
only), and the optimizer apply launches (opt_apply_cb_kernel beside dsgd_apply_cb_kernel), at BASELINE config 3's shape
(2048 directions x +-, P = 6092), HIP events over 50 calls (1000 for the apply launches alone).
    python tools/learner_bench.py [n_dirs P]
    python tools/learner_bench.py n_dirs P top     only the top-b direction section: the two weight kernels alone
        (fdr_top_dir_weights, b = n_dirs / 4) and fd_step_top next to fd_step z-score, alternating, 5 rounds of 200 calls
        each on the same build in the same process (e.g. 2048 6092 top; 16384 6092 top: the 8-rank direction count)"""
import os
import sys

import numpy as np
import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dfd-starter_amd")]
from fdr import engine  # noqa: E402

n_dirs = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
P = int(sys.argv[2]) if len(sys.argv) > 2 else 6092
dev = "cuda"
rs = np.random.RandomState(0)
table = torch.randn(25_000_000, device=dev)
idx_dirs = torch.as_tensor(rs.randint(0, 25_000_000 - P, size=n_dirs), device=dev)
idx = idx_dirs.repeat_interleave(2)
sign = torch.as_tensor(np.tile(np.array([1, -1], np.int8), n_dirs), device=dev)
rew = torch.randn(2 * n_dirs, dtype=torch.float64, device=dev)
n2 = torch.rand(2 * n_dirs, dtype=torch.float64, device=dev) + 1.0
theta = torch.randn(P, device=dev)
g = torch.empty(P, dtype=torch.float64, device=dev)


def timeit(name, fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    print("%-40s %8.2f us / call" % (name, us), flush=True)
    return us


def top_section():
    b = max(1, n_dirs // 4)
    t_w = timeit("top_dir_weights (select + weights), b = D/4", lambda: engine.top_dir_weights(rew, 0.0, 2, b, 0, 2 * n_dirs),
                 n=200)
    t_wd = timeit("top_dir_weights, b = D", lambda: engine.top_dir_weights(rew, 0.0, 2, n_dirs, 0, 2 * n_dirs), n=200)
    t_rk = timeit("rank_weights (centred rank, for scale)", lambda: engine.rank_weights(rew, 0, 2 * n_dirs), n=200)
    t_g = timeit("fd_grad_fused zscore", lambda: engine.fd_grad_fused(table, idx, rew, 0.0, 0, sign, n2, 2, 0.02, P, out=g),
                 n=200)
    t_gt = timeit("fd_grad_fused_top", lambda: engine.fd_grad_fused_top(table, idx, rew, 0.0, 0, sign, n2, 2, 0.02, P, b,
                                                                        out=g), n=200)
    rounds = []
    if P <= 65536:
        for k in range(5):      # alternating: the shared box's drift lands on both
            z = timeit("round %d  fd_step zscore" % k, lambda: engine.fd_step(table, idx, rew, 0.0, sign, n2, 2, 0.02, theta,
                                                                             0.01, 0.5, g=g), n=200)
            t = timeit("round %d  fd_step_top" % k, lambda: engine.fd_step_top(table, idx, rew, 0.0, sign, n2, 2, 0.02, theta,
                                                                              0.01, 0.5, b, g=g), n=200)
            rounds.append((z, t))
        zs, ts = np.array(rounds).T
        print("D %d P %d: fd_step zscore median %.2f us (min %.2f, max %.2f); fd_step_top median %.2f us (min %.2f, max "
              "%.2f); difference of medians %.2f us" % (n_dirs, P, np.median(zs), zs.min(), zs.max(), np.median(ts),
                                                        ts.min(), ts.max(), np.median(ts) - np.median(zs)))
    print("D %d: the two top-b kernels %.2f us (b = D/4) / %.2f us (b = D), centred rank's %.2f us, next to the gradient "
          "launch they precede, %.2f us (fd_grad_fused_top in all: %.2f us)" % (n_dirs, t_w, t_wd, t_rk, t_g, t_gt))


if len(sys.argv) > 3 and sys.argv[3] == "top":
    top_section()
    sys.exit(0)


def staged():
    c = engine.fd_weights(rew, 0.0, 0, sign, n2, 2, 0.02)
    gg = engine.fd_grad(table, idx_dirs, c, P, g)
    engine.dsgd_step(theta, gg, 0.01, 0.5)


timeit("staged weights+grad+dsgd (7 launches)", staged)
timeit("fd_weights only", lambda: engine.fd_weights(rew, 0.0, 0, sign, n2, 2, 0.02))
timeit("fd_grad_fused zscore", lambda: engine.fd_grad_fused(table, idx, rew, 0.0, 0, sign, n2, 2, 0.02, P, out=g))
timeit("fd_grad_fused moments", lambda: engine.fd_grad_fused(table, idx, rew, 0.0, 0, sign, n2, 2, 0.02, P,
                                                             mode="moments"))
timeit("dsgd_step_ex (fused single WG)", lambda: engine.dsgd_step_ex(theta, g, False, 0.01, 0.5))
if P <= 65536:
    timeit("fd_step (one launch)", lambda: engine.fd_step(table, idx, rew, 0.0, sign, n2, 2, 0.02, theta, 0.01, 0.5,
                                                          g=g))
# the mixed objective: random novelty / entropy channels, coefficients (0.6, 0.4, 0.05)
chan = (rew, 0.3 * torch.randn(2 * n_dirs, dtype=torch.float64, device=dev).abs(),
        1.4 + 0.05 * torch.randn(2 * n_dirs, dtype=torch.float64, device=dev))
pol, mix = (0.0, 0.2, 1.3), (0.6, 0.4, 0.05)
timeit("fd_grad_fused mix", lambda: engine.fd_grad_fused_mix(table, idx, chan, pol, mix, 0, sign, n2, 2, 0.02, P, out=g))
if P <= 65536:
    timeit("fd_step mix", lambda: engine.fd_step_mix(table, idx, chan, pol, mix, sign, n2, 2, 0.02, theta, 0.01, 0.5, g=g))
timeit("fd_weights_mix only", lambda: engine.fd_weights_mix(chan, pol, mix, 0, sign, n2, 2, 0.02))

# the apply launch alone: the optimizers' opt_apply_cb_kernel directly (fdr_opt_step from g is that one launch);
# dsgd_apply_cb_kernel only runs behind the gradient launch, so it is fd_step minus fd_grad_fused on the same build
m_row, v_row = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
adam = engine.OptSpec("adam", 1e-2, 7, m_row, v_row)
sgdm = engine.OptSpec("sgd", 1e-2, 7, m_row, None, momentum=0.9)
t_adam = timeit("opt_step adam (opt_apply_cb_kernel)", lambda: engine.opt_step(theta, g, False, adam), n=1000)
timeit("opt_step sgd momentum", lambda: engine.opt_step(theta, g, False, sgdm), n=1000)
t_grad = timeit("fd_grad_fused zscore (again)", lambda: engine.fd_grad_fused(table, idx, rew, 0.0, 0, sign, n2, 2, 0.02, P,
                                                                             out=g), n=1000)
t_step = timeit("fd_step (any P)", lambda: engine.fd_step(table, idx, rew, 0.0, sign, n2, 2, 0.02, theta, 0.01, 0.5, g=g),
                n=1000)
t_opt = timeit("fd_step_opt adam", lambda: engine.fd_step_opt(table, idx, rew, 0.0, sign, n2, 2, 0.02, theta, adam, g=g),
               n=1000)
print("apply launch by difference: dsgd_apply_cb_kernel %.2f us, opt_apply_cb_kernel<ADAM> %.2f us (alone: %.2f us)"
      % (t_step - t_grad, t_opt - t_grad, t_adam))
