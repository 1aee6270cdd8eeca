"""numpy restatement, in extended precision, of one step of the optimizers the learner applies on the device (Adam,
AdamW, SGD): the yardstick of opt_apply_cb_kernel's f32 arithmetic.  TEST INFRASTRUCTURE ONLY, in the style of
tests/learner_ref.py.

The inputs are what the kernel reads -- f32 theta, f32 state rows, the f64 gradient g -- and the hyperparameters as
Python floats.  grad = fl32(-g) is the one rounding restated (policy.set_grad_from_flat's cast); everything after it
is torch's single-tensor formula (torch/optim/adam.py, adamw.py, sgd.py; non-capturable, maximize = False, no amsgrad)
evaluated in np.longdouble with the exact hyperparameters, and left unrounded.

How far may a correct f32 evaluation be from that?  Every f32 operation adds up to 2^-24 of its result, and the
hyperparameter scalars reach f32 with 2^-24 of their own, so a chain of operations lands within k 2^-24 s of the
exact value, s the magnitude the chain handles, plus the final rounding of theta to f32:

    |theta - theta_ref| <= 1/2 ulp(max(|theta_old|, |theta_new|)) + k 2^-24 s_theta
    |state - state_ref| <=                                          k 2^-24 s_state

s is the same formula evaluated on magnitudes, so that cancellation inside it (the L2 term wd theta against the
gradient, momentum against gradient) does not count as error of the implementation:

    grad_mag = |grad| + wd |theta|                         (wd |theta|: the L2 kinds only)
    Adam / AdamW
      s_m     = |m| + (1 - beta1) (grad_mag + |m|)         the terms of lerp: m + w (grad - m)
      s_v     = beta2 v + (1 - beta2) |grad'| grad_mag     grad' the L2-adjusted gradient; >= v_new
      s_theta = |theta| (1 - lr wd)  (AdamW's decay term)  +  step_size (s_m / denom) (s_v / v_new)
                (s_v / v_new >= 1 carries v's relative error into denom; 1 when v_new == 0.  AdamW's decay is the
                product theta * fl32(1 - lr wd), param.mul_(1 - lr * weight_decay): the scalar's own rounding and the
                product's are each 2^-24 of |theta|, not of lr wd |theta|, so the term's magnitude is the product's)
    SGD
      s_buf   = momentum |buf| + |1 - dampening| grad_mag  (grad_mag on the first step)
      s_theta = lr d_mag,  d_mag = grad_mag | s_buf | grad_mag + momentum s_buf  (plain | momentum | nesterov)

k is not chosen here: tests/test_optim_ref.py measures the k that the installed torch's own CPU optimizers show
against this restatement over CASES, and the kernel is allowed 4 x the largest k torch shows per kind -- a different
but equally valid f32 ordering of a chain of about six operations.  The constants below are those allowances; the CPU
test asserts that torch itself stays within them, and nothing here was tuned against the kernel.
"""
import numpy as np

LD = np.longdouble
F32 = np.float32
U = LD(2.0) ** -24

# case name -> (kind, hyperparameters); the list of the issue that introduced the device optimizers
CASES = {
    "adam": ("adam", dict(lr=1e-2)),
    "adam_b_eps_wd": ("adam", dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)),
    "adamw": ("adamw", dict(lr=1e-2)),                       # torch's default weight_decay = 1e-2
    "sgd": ("sgd", dict(lr=1e-2)),
    "sgd_momentum": ("sgd", dict(lr=1e-2, momentum=0.9)),
    "sgd_nesterov_wd": ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-3)),
    "sgd_dampening": ("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.1)),
}
DEFAULTS = {
    "adam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "adamw": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
    "sgd": dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
}
GRAD_SCALES = (1e-3, 1e-2, 1e-1, 1.0, 10.0, 1e-1)   # one per step of the 6-step CPU comparison

# Allowances k: 4 x the largest k the installed torch's CPU optimizers show against this file (measured by
# tests/test_optim_ref.py::test_torch_cpu_optimizers_against_the_restatement, which prints them; DESIGN.md section 4
# records the values): torch 2.10 -- Adam 4.28 (theta, default case), AdamW 2.66 (exp_avg_sq), SGD 2.96 (theta, nesterov +
# weight decay), rounded up to one decimal.
K_MEASURED = {"adam": 4.3, "adamw": 2.7, "sgd": 3.0}
K_ADAM = 4 * K_MEASURED["adam"]
K_ADAMW = 4 * K_MEASURED["adamw"]
K_SGD = 4 * K_MEASURED["sgd"]
K = {"adam": K_ADAM, "adamw": K_ADAMW, "sgd": K_SGD}


def hyper(kind, **kw):
    h = dict(DEFAULTS[kind])
    h.update(kw)
    return h


class Step(object):
    """One step's exact results (longdouble) and the magnitudes s of their bounds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def grad32(g):
    return (-np.asarray(g, np.float64)).astype(F32)


def step(kind, h, t, theta, g, state0=None, state1=None):
    """One step number t (1 on the first) of `kind` with hyperparameters h (hyper()) from f32 theta, f64 g and the
    f32 state rows (adam / adamw: exp_avg, exp_avg_sq; sgd with momentum: momentum_buffer, ignored at t == 1).
    -> Step(theta, state0, state1, grad, s_theta, s_state0, s_state1); absent state rows are None."""
    th = np.asarray(theta, F32).astype(LD)
    gr32 = grad32(g)
    gr = gr32.astype(LD)
    lr, wd = LD(h["lr"]), LD(h["weight_decay"])
    a_th, a_gr = np.abs(th), np.abs(gr)
    if kind in ("adam", "adamw"):
        b1, b2, eps = LD(h["betas"][0]), LD(h["betas"][1]), LD(h["eps"])
        m, v = np.asarray(state0, F32).astype(LD), np.asarray(state1, F32).astype(LD)
        decay = np.zeros_like(th)
        grad_mag = a_gr
        if kind == "adamw":
            th1 = th * (1 - lr * wd)
            decay = th1 if h["weight_decay"] != 0 else decay
        else:
            th1 = th
            gr = gr + wd * th
            grad_mag = a_gr + wd * a_th
        m_new = m + (gr - m) * (1 - b1)
        v_new = b2 * v + (1 - b2) * gr * gr
        step_size = lr / (1 - b1 ** t)
        denom = np.sqrt(v_new) / np.sqrt(1 - b2 ** t) + eps
        new = th1 - step_size * m_new / denom
        s_m = np.abs(m) + (1 - b1) * (grad_mag + np.abs(m))
        s_v = b2 * v + (1 - b2) * np.abs(gr) * grad_mag
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(v_new > 0, s_v / v_new, LD(1))
        s_theta = np.abs(decay) + step_size * (s_m / denom) * f
        return Step(theta=new, state0=m_new, state1=v_new, grad=gr32, s_theta=s_theta, s_state0=s_m, s_state1=s_v)
    assert kind == "sgd", kind
    mom, damp = LD(h["momentum"]), LD(h["dampening"])
    grad_mag = a_gr + wd * a_th
    gr = gr + wd * th
    buf_new = s_buf = None
    d, d_mag = gr, grad_mag
    if h["momentum"] != 0:
        if t == 1:
            buf_new, s_buf = gr, grad_mag
        else:
            buf = np.asarray(state0, F32).astype(LD)
            buf_new = mom * buf + (1 - damp) * gr
            s_buf = mom * np.abs(buf) + abs(1 - damp) * grad_mag
        if h["nesterov"]:
            d, d_mag = gr + mom * buf_new, grad_mag + mom * s_buf
        else:
            d, d_mag = buf_new, s_buf
    return Step(theta=th - lr * d, state0=buf_new, state1=None, grad=gr32, s_theta=lr * d_mag, s_state0=s_buf,
                s_state1=None)


def half_ulp(theta_old, theta_new):
    """1/2 ulp of the larger of |theta_old|, |theta_new| (f32), as longdouble."""
    big = np.maximum(np.abs(np.asarray(theta_old, F32)), np.abs(np.asarray(theta_new, F32)))
    return np.spacing(big).astype(LD) / 2


def _ratio(err, s):
    """max over the elements of err / (2^-24 s); an element with s == 0 must have err <= 0 (else inf)."""
    err, s = np.asarray(err, LD), np.asarray(s, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / (U * s), np.where(err <= 0, LD(0), LD(np.inf)))
    return float(max(r.max(), 0)) if r.size else 0.0


def shown_k(ref, theta_old, theta_new, state0_new=None, state1_new=None):
    """The k an implementation's results show against a Step: (theta's, state0's, state1's); 0.0 for absent rows."""
    th_new = np.asarray(theta_new, F32)
    k_t = _ratio(np.abs(th_new.astype(LD) - ref.theta) - half_ulp(theta_old, th_new), ref.s_theta)
    ks = []
    for got, want, s in ((state0_new, ref.state0, ref.s_state0), (state1_new, ref.state1, ref.s_state1)):
        ks.append(0.0 if want is None else _ratio(np.abs(np.asarray(got, F32).astype(LD) - want), s))
    return k_t, ks[0], ks[1]


def norms(theta_old, theta_new, grad):
    """out = [||fl32(theta_old - theta_new)||, ||grad||] of an implementation's own f32 theta, in longdouble."""
    d = (np.asarray(theta_old, F32) - np.asarray(theta_new, F32)).astype(LD)
    gq = np.asarray(grad, F32).astype(LD)
    return float(np.sqrt((d * d).sum())), float(np.sqrt((gq * gq).sum()))
