"""CPU: the branch table of the five physics systems (tests/branch_cases.py) -- which decision of cartpole_step,
pendulum_step, acrobot_step, mountaincar_step and wrap_pi each seeded case takes, on the f32 restatement.  Nothing
here runs on a GPU; tests/test_gpu_physics_branches.py runs the same cases and the same check() on the kernels and
counts again on their own trajectories.

1. The census of the EXISTING linear cases, pinned as it stands: the gaps the branch cases close.
2. Every branch case takes the rows it is aimed at at least 8 times in at least 4 lanes, and check() passes on the
   restatement: the condition under which a GPU run of the case counts.
3. Every row of the table has a case aimed at it, or its reason in UNREACHABLE / SPARSE; the figures quoted there are
   recomputed here.
4. Acrobot's one-step f32-versus-f64 error over the whole legal box (ACROBOT_ERR_WIDE, beside ACROBOT_ERR), measured
   2.0e-5, 2.8e-5, 1.3e-2, 1.7e-2 on 10^6 states and asserted at that rounded up to one digit.
5. The checker is checked: restatements with one constant of one branch changed (branch_cases.MUTATIONS) make check()
   raise on the case aimed at that branch.
"""
import numpy as np
import pytest

import branch_cases as bc
import linear_cases as lc
import physics_ref2 as ref2

# ---- 1. the existing cases ----------------------------------------------------------------------------------------
# row -> (times, lanes); rows not listed are never taken
EXISTING = {
    "cartpole": {"th_hi": (22, 22), "th_lo": (15, 15)},
    "pendulum": {"u_hi": (185, 20), "u_lo": (226, 32), "thd_hi": (28, 11), "wrap_down": (34, 34), "wrap_up": (20, 20)},
    "acrobot": {"th2_down": (1, 1), "th2_up": (1, 1)},
    "mountaincar": {"wall": (22, 22), "goal": (30, 30)},
    "mountaincar_cont": {"v_lo": (16, 3), "wall": (27, 27), "goal": (37, 37), "f_hi": (998, 50), "f_lo": (983, 36),
                         "bonus": (37, 37)},
    "cartpole_long": {"th_hi": (10, 10), "th_lo": (18, 18)},
    "acrobot_ctrl": {"th1_down": (4, 3), "th1_up": (2, 1), "th2_down": (15, 9), "th2_up": (47, 16), "goal": (15, 15)},
    "cartpole_norm": {"th_hi": (20, 20), "th_lo": (44, 44)},
    "acrobot_norm": {},
    "cartpole_stats": {"th_hi": (18, 18), "th_lo": (18, 18)},
    "acrobot_stats": {},
    "cartpole_k3": {"th_hi": (18, 18), "th_lo": (20, 20)},
}


@pytest.mark.parametrize("name", lc.GPU_CASES)
def test_census_of_the_existing_cases(name):
    """What tests/linear_cases.py reaches today: no x exit, no Pendulum clamp at -8, no Acrobot velocity clamp, the
    MountainCar speed limit in 3 lanes of one case.  simulate() with no knob turned is linear_ref.run bit for bit."""
    c = lc.case(name)
    o, r = bc.simulate(c), c.run()
    np.testing.assert_array_equal(o["steps"], r["steps"])
    np.testing.assert_array_equal(o["ret"], r["ret"])
    np.testing.assert_array_equal(np.isnan(o["states"]), np.isnan(r["states"]))
    np.testing.assert_array_equal(np.nan_to_num(o["states"]).view(np.uint32), np.nan_to_num(r["states"]).view(np.uint32))
    cen = bc.census(c, o["states"], o["steps"])
    assert set(cen) == set(bc.ROWS[c.env])
    assert {k: v for k, v in cen.items() if v[0] and k != "thd_any"} == EXISTING[name]
    S = o["states"]
    if c.env == "cartpole":
        assert np.nanmax(np.abs(S[:, :, 0])) < 1.05           # nowhere near the x bound
    if c.env == "acrobot":
        assert np.nanmax(np.abs(S[:, :, 4])) < 7.1 and np.nanmax(np.abs(S[:, :, 5])) < 16.1


def test_census_of_the_existing_mlp_cases():
    """The same for the MLP suite's long cases (cart_long of test_gpu_physics_envs.py, the three case_long of
    test_gpu_physics_envs2.py) through the oracle's episode loop: CartPole comes within 0.004 of the x bound and lanes
    do leave through it, but no test names the side; neither MountainCar ever reaches -0.07 (nor +0.07, nor 0.6);
    Acrobot stays far inside its velocity clamps.  The mlp_* controller lanes of branch_cases.py close the first two."""
    import test_gpu_physics_envs as m1
    import test_gpu_physics_envs2 as m2
    o = m1.cartpole_oracle(*m1.case_long(), m1.SEED_LONG)
    mx = max(np.abs(o["states"][l, :n, 0]).max() for l, n in enumerate(o["steps"]))
    assert 2.39 < mx < 2.4 and (np.abs(o["env"].s[:, 0]) > 2.4).sum() > 8
    for name in ("mountaincar", "mountaincar_cont"):
        o = m2.oracle_episodes(name, *m2.case_long(name), m2.SEED_LONG)
        rec = np.concatenate([o["states"][l, :n] for l, n in enumerate(o["steps"])])
        assert rec[:, 1].min() > -0.0601 and rec[:, 1].max() < 0.0682 and rec[:, 0].max() < 0.5
        assert 1 <= (rec[:, 0] == np.float32(-1.2)).sum() <= 4
    o = m2.oracle_episodes("acrobot", *m2.case_long("acrobot"), m2.SEED_LONG)
    rec = np.concatenate([o["states"][l, :n] for l, n in enumerate(o["steps"])])
    assert np.abs(rec[:, 4]).max() < 5.7 and np.abs(rec[:, 5]).max() < 10.5


# ---- 2. the branch cases ------------------------------------------------------------------------------------------
# the census of each case over its launches, on this restatement
CENSUS = {
    "cart_x_hi": {"x_hi": (104, 104)},
    "cart_x_lo": {"x_lo": (106, 106)},
    "cart_theta": {"th_hi": (43, 43), "th_lo": (33, 33)},
    "pend_speed": {"u_hi": (6076, 90), "u_lo": (6377, 96), "thd_hi": (1948, 63), "thd_lo": (2019, 65),
                   "wrap_down": (349, 82), "wrap_up": (368, 87)},
    "acro_whirl": {"th1_down": (29, 24), "th1_up": (31, 15), "th2_down": (4308, 153), "th2_up": (3597, 159),
                   "thd1_hi": (7, 5), "thd1_lo": (21, 5), "thd2_hi": (15, 2), "thd2_lo": (1, 1), "thd_any": (31, 12),
                   "goal": (235, 235)},
    "mc_wall": {"v_lo": (411, 109), "wall": (210, 128)},
    "mc_goal": {"wall": (48, 48), "goal": (62, 62)},
    "mcc_wall": {"v_lo": (1324, 119), "wall": (240, 126), "goal": (12, 12), "f_hi": (15837, 128), "f_lo": (19866, 128),
                 "bonus": (12, 12)},
    "mcc_goal": {"v_lo": (29, 7), "wall": (59, 59), "goal": (68, 68), "f_hi": (1936, 94), "f_lo": (1957, 70),
                 "bonus": (68, 68)},
    # the controller lanes of the MLP kernels (one launch each)
    "mlp_cart_x_hi": {"x_hi": (64, 64)},
    "mlp_cart_x_lo": {"x_lo": (64, 64)},
    "mlp_mc_wall": {"v_lo": (193, 52), "wall": (102, 64)},
}
_CHECKED = {}


def _checked(name):
    if name not in _CHECKED:
        _CHECKED[name] = bc.check_case(name, None)
    return _CHECKED[name]


@pytest.mark.parametrize("name", bc.NAMES + bc.MLP_NAMES)
def test_branch_case_takes_its_rows_and_passes_the_check(name):
    reports, cen = _checked(name)
    assert {k: v for k, v in cen.items() if v[0]} == CENSUS[name]
    for row in bc.AIMS[name]:
        assert bc.reached(cen, row)
    c = bc.case(name)
    assert c.T <= 500 and len(c.ids) == 64 and all(bc.case(name, off).lane_offset == off for off in bc.OFFSETS[name])
    assert name in bc.MLP_NAMES or bc.OFFSETS[name][:2] == (0, 64)
    if name.startswith("cart_x"):       # the pole is upright where the cart leaves
        assert max(r["exit_theta"] for r in reports.values()) < 0.035
    if name == "acro_whirl":            # far outside the old box, and the clamps are checked where they act
        assert sum(r["outside_box"] for r in reports.values()) > 10000
        assert sum(sum(r["pinned"].values()) for r in reports.values()) >= 30
    if name in ("mc_wall", "mcc_wall", "mlp_mc_wall"):
        assert all(r["pinned"]["v_lo"] >= 100 and r["pinned"]["wall"] >= 64 for r in reports.values())
    if name == "pend_speed":
        assert all(r["pinned"]["thd_hi"] >= 500 and r["pinned"]["thd_lo"] >= 500 for r in reports.values())
    if c.env in bc.FORCE_CLAMP:         # steps beyond the force clamp are present and checked
        assert all(r["checked"][0] > 0.99 * r["checked"][1] for r in reports.values())


def test_mlp_controllers_follow_their_rule():
    """The hand-built DiscretePolicy vectors of the MLP cases take the last action where gain (w . x) + bias >= 0 and
    action 0 elsewhere (the oracle's forward, on visited observations away from the switching surface)."""
    from oracle import policies as opol
    for name in bc.MLP_NAMES:
        c = bc.case(name)
        theta = c.theta()
        assert theta.dtype == np.float32 and theta.size == opol.num_params("discrete", c.n_in, c.n_act)
        S = bc.simulate(c)["states"]
        obs = S[:, ::7][np.isfinite(S[:, ::7, 0])]
        x = np.clip((obs - c.obs_mean) / c.obs_std, -10, 10).astype(np.float32)
        s = x.astype(np.float64) @ c.w
        clear = np.abs(s) > 10 * c.AMBIGUOUS
        assert clear.mean() > 0.9 and len(obs) > 1000
        p = opol.lanes_forward("discrete", c.n_in, c.n_act, np.broadcast_to(theta, (len(obs), theta.size)), x)
        np.testing.assert_array_equal(np.argmax(p, -1)[clear], c.actions(obs)[clear])
        assert set(np.unique(c.actions(obs))) == {0, c.n_act - 1}
        assert np.all(p.max(-1)[clear] > 0.99)


def test_x_exit_episodes_have_no_whole_episode_reference():
    """Why everything is checked along the launch's own trajectory: the f32 restatement and its f64 twin disagree on the
    step count of most lanes of the x-exit cases (closed-loop bang-bang control is chaotic)."""
    c = bc.case("cart_x_hi")
    a, b = c.run(np.float32), c.run(np.float64)
    assert (a["steps"] != b["steps"]).sum() >= 16


# ---- 3. every row is accounted for --------------------------------------------------------------------------------
def test_every_row_has_a_case_or_a_reason():
    aimed = {(bc.case(n).env, row) for n in bc.NAMES for row in bc.AIMS[n]}
    for env, rows in bc.ROWS.items():
        for row in rows:
            key = (env, row)
            assert (key in aimed) + (key in bc.UNREACHABLE) + (key in bc.SPARSE) == 1, key
    for (env, row), why in list(bc.UNREACHABLE.items()) + list(bc.SPARSE.items()):
        assert len(why) > 40
        if row != "cost_wrap":          # (not a row a recorded transition can show)
            assert row in bc.ROWS[env]
            assert all(cen.get(row, (0, 0)) == (0, 0) or (env, row) in bc.SPARSE
                       for n, (_, cen) in ((n, _checked(n)) for n in bc.NAMES) if bc.case(n).env == env)


@pytest.mark.parametrize("cont", [False, True])
def test_mountaincar_right_speed_limit_is_out_of_reach(cont):
    """The evidence of UNREACHABLE: the fastest rightward run (from rest at any turning point on the left slope, the
    wall included, full push to the right) stays below 0.07, and the branch cases' own maxima lie below that."""
    p0 = np.linspace(-1.2, -0.53, 400)
    for dt, step in ((np.float64, ref2.mountaincar_step_f64), (np.float32, ref2.mountaincar_step_f32)):
        p, v = p0.astype(dt), np.zeros(len(p0), dt)
        vmax = np.zeros(len(p0))
        live = np.ones(len(p0), bool)
        for _ in range(200):
            p, v, done, _ = step(p, v, np.full(len(p0), 5.0, dt) if cont else np.full(len(p0), 2), cont)
            vmax = np.where(live, np.maximum(vmax, v), vmax)
            live &= ~done
        assert p0[np.argmax(vmax)] < -1.19                   # the wall is the best start (up to the phase of the steps)
        name = "mountaincar_cont" if cont else "mountaincar"
        assert 0.06 < vmax.max() < bc.MAX_V_RIGHT[name] < 0.07
    for n in ("mcc_wall", "mcc_goal") if cont else ("mc_wall", "mc_goal"):
        for off in bc.OFFSETS[n]:
            S = bc.simulate(bc.case(n, off))["states"]
            assert np.nanmax(S[:, :, 1]) < bc.MAX_V_RIGHT[name] and np.nanmax(S[:, :, 0]) < (0.45 if cont else 0.5)


# ---- 4. Acrobot's f32 step error on the whole legal box -----------------------------------------------------------
def test_acrobot_f32_step_error_vs_f64_on_the_whole_box():
    """As test_physics_ref2.py::test_acrobot_f32_step_error_vs_f64 on |thd1| <= 6, |thd2| <= 10, here up to the clamps.
    The GPU tolerance outside the old box is ten times these, the project's ratio."""
    assert ref2.ACROBOT_ERR_WIDE == (2e-5, 3e-5, 2e-2, 2e-2)
    N = 1000000
    rs = np.random.RandomState(0)
    s = np.stack([rs.uniform(-np.pi, np.pi, N), rs.uniform(-np.pi, np.pi, N), rs.uniform(-4 * np.pi, 4 * np.pi, N),
                  rs.uniform(-9 * np.pi, 9 * np.pi, N)], axis=-1).astype(np.float32)
    a = rs.randint(0, 3, N)
    d = ref2.acrobot_step_f32(s, a).astype(np.float64) - ref2.acrobot_step_f64(s.astype(np.float64), a)
    d[:, :2] = (d[:, :2] + np.pi) % (2 * np.pi) - np.pi      # the angles live on the circle
    err = np.abs(d).max(axis=0)
    print("acrobot f32 vs f64 one-step max error per component, whole box:", err)
    for e, bound in zip(err, ref2.ACROBOT_ERR_WIDE):
        assert bound / 10 < e <= bound
    np.testing.assert_allclose(bc.ACRO_STEP_TOL_WIDE, [2e-4, 2e-4, 3e-4, 3e-4, 2e-1, 2e-1], rtol=1e-12)


# ---- 5. the checker notices a wrong kernel ------------------------------------------------------------------------
def test_mutations_cover_the_list():
    knobs = set()
    for turned, name in bc.MUTATIONS.values():
        assert name in bc.NAMES and set(turned) <= set(bc.KNOBS)
        knobs |= set(turned)
    # every constant of a reachable branch is turned by some mutation (mc_hi: the +0.07 side is out of reach)
    assert knobs == set(bc.KNOBS) - {"mc_hi"}


@pytest.mark.filterwarnings("ignore::RuntimeWarning")           # an Acrobot without clamps overflows
@pytest.mark.parametrize("mutation", sorted(bc.MUTATIONS))
def test_check_raises_on_a_mutated_restatement(mutation):
    """The restatement with one constant changed stands in for a subtly wrong kernel: check() must raise on the case
    aimed at that branch (and passes on the unmutated restatement: test_branch_case_takes_its_rows_...)."""
    turned, name = bc.MUTATIONS[mutation]
    with pytest.raises(AssertionError) as ei:
        bc.check_case(name, None, mutation=turned)
    print("%s on %s: %s" % (mutation, name, str(ei.value).splitlines()[0][:200]))
