"""CPU checks of what tests/test_robust_classes_gpu.py rests on, from the references alone: the
recorded REF_DEV against a recomputation, the slab and width class every shape stands for, the start
value of the 1 x 1 problem on its floor, the floored sweep, the pick margins of every forced-path
case, the poison conditions of the stopped-chain cases and the accept / reject margins of the
device-RNG seeds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rng_reference as R
import robust_cases as RC
import robust_class_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble


@pytest.mark.parametrize("name", CC.ref_dev_names())
def test_recorded_deviations_match_a_recomputation(name):
    """Within a factor 4 (BLAS summation order differs between machines), both sides taken no smaller
    than 2^-52 as the bar takes them.  The recorded table stays the authority for the bar."""
    got = CC.recompute_ref_dev(name)
    assert len(got) == len(CC.REF_DEV[name])
    for rec, new in zip(CC.REF_DEV[name], got):
        rec, new = max(rec, CC.DEV_FLOOR), max(new, CC.DEV_FLOOR)
        print(f"{name}: recorded {rec:.3e}, recomputed {new:.3e}")
        assert rec / 4 <= new <= 4 * rec
    assert set(CC.REF_DEV) == set(CC.ref_dev_names())


def test_shapes_stand_for_their_slab_and_width_classes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler is required"
    exe = str(tmp_path / "robust_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(HERE, "robust_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (rows_per_wave, kernel width, rows of each wave's slab)
    want = {(1, 1): (4, 4, (1, 0, 0, 0)), (2, 1): (4, 4, (2, 0, 0, 0)), (4, 2): (4, 4, (4, 0, 0, 0)),
            (5, 4): (4, 4, (4, 1, 0, 0)), (16, 8): (4, 8, (4, 4, 4, 4)), (17, 9): (8, 16, (8, 8, 1, 0)),
            (40, 31): (12, 32, (12, 12, 12, 4)), (256, 3): (64, 4, (64, 64, 64, 64))}
    assert set(want) == set(CC.SHAPES)
    for (n, k), (rpw, kc, rows) in want.items():
        head, slabs = subprocess.run([exe, "slabs", str(n), str(k)], capture_output=True, text=True,
                                     check=True).stdout.split("|")
        head = [int(v) for v in head.split()]
        got = tuple(int(b) - int(a) for a, b in (s.split("-") for s in slabs.split()))
        assert (head[0], head[4], got) == (rpw, kc, rows), (n, k)
        assert n >= k
    assert set(CC.COL_MAJOR) <= set(CC.SHAPES) and set(CC.NU_SHAPES) <= set(CC.SHAPES)


def test_dense_prior_feeds_the_off_diagonals_and_pb0():
    for n, k in CC.SHAPES:
        b0, C0 = CC.problem(n, k)[2][:2]
        P = np.linalg.inv(C0)
        assert np.all(np.linalg.eigvalsh(C0) >= 1.0 - 1e-12) and np.all(np.abs(P @ b0) > 0)
        if k > 1:
            assert np.abs(P[np.tril_indices(k, -1)]).min() > 0


def test_start_value_of_1x1_is_on_the_floor():
    """One row, one column: the OLS residual is zero up to rounding, so both sides start at 1e-6;
    every other shape starts above it."""
    assert CC.start_sigma2(1, 1) < 1e-20
    assert CC.start_sigma2(1, 1, np.float64) < 1e-20
    for n, k in CC.SHAPES[1:]:
        assert CC.start_sigma2(n, k) > 1e-3
    s, w = CC.fixed_reference(1, 1)
    assert np.isfinite(s.astype(np.float64)).all() and np.isfinite(w.astype(np.float64)).all()


@pytest.mark.parametrize("n,k", CC.SHAPES)
def test_fixed_nu_references_are_finite_and_burnt_in(n, k):
    s, w = CC.fixed_reference(n, k)
    assert s.shape == (CC.CHAINS, CC.ITERS, k + 1) and w.shape == (CC.CHAINS, n)
    assert np.isfinite(s.astype(np.float64)).all() and (w > 0).all()
    # the burn-in matters: the weights of the same variates without it differ
    xi, g, gl = CC.fixed_inputs(n, k)
    _, w0 = CC.run_fixed(n, k, xi[:1], g[:1], gl[:1], 0, CC.BURN + CC.ITERS)
    assert RC.weight_deviation(w0[0], w[0]) > 1e-3
    assert not np.array_equal(xi[0], xi[1]) and not np.array_equal(gl[1], gl[2])


def test_floored_sweep_of_the_reference():
    """G_t = 1e300 puts sigma2 on its floor: the recorded sigma is exactly 1e-3 in both references
    (sqrt(1e-6) rounds to it) and every later row is finite."""
    assert np.sqrt(np.float64(1e-6)) == 1e-3 and np.float64(np.sqrt(LD(1e-6))) == 1e-3
    n, k = CC.FLOOR_SHAPE
    clean = CC.fixed_reference(n, k)[0]
    for dtype in (LD, np.float64):
        s, w = CC.floor_reference(dtype)
        assert np.isfinite(s.astype(np.float64)).all() and np.isfinite(w.astype(np.float64)).all()
        for c, t0 in enumerate(CC.FLOOR_SWEEPS):
            assert CC.BURN <= t0 < CC.BURN + CC.ITERS - 1
            assert np.float64(s[c, t0 - CC.BURN, k]) == 1e-3
            assert (s[c, :, k] > 1e-3).sum() == CC.ITERS - 1          # no other sweep reaches the floor
            if dtype is LD:                                           # the rows before it are the clean chain's
                assert np.array_equal(s[c, :t0 - CC.BURN], clean[c, :t0 - CC.BURN])


@pytest.mark.parametrize("name", CC.NU_CASES + ("D",))
def test_pick_margins_of_the_forced_path_cases(name):
    """No pick of the long-double reference lies within MARGIN_FLOOR of a boundary and float64 picks
    the same: the GPU's picks can be compared exactly.  The forced paths stay on values of positive
    weight and move."""
    case, ref, f64 = CC.nu_case(name), CC.nu_reference(name), CC.nu_reference(name, np.float64)
    G = len(case["grid"])
    assert case["weight"][case["init"]] > 0 and (case["weight"][case["paths"]] > 0).all()
    for c in range(CC.CHAINS):
        assert ref[c]["margin"].min() >= R.MARGIN_FLOOR
        assert np.array_equal(ref[c]["idx"], f64[c]["idx"])
        assert np.count_nonzero(np.diff(case["paths"][c])) >= (case["burn"] + case["iters"]) // 4 - 1
        assert (case["weight"][ref[c]["idx"]] > 0).all()              # never a value of weight zero
    picks = np.concatenate([r["idx"] for r in ref])
    if G <= 9 and name != "E-zero":
        assert {0, G - 1} <= set(picks.tolist())
    if G == 64:
        assert {0, 63} <= set(case["paths"].ravel().tolist()) and len(np.unique(picks)) > 32


def test_zero_weight_edge_and_non_finite_cases_are_what_they_claim():
    zero = CC.nu_case("E-zero")
    assert np.array_equal(np.flatnonzero(zero["weight"] == 0), CC.ZERO_WEIGHT) and len(zero["grid"]) == 9
    picks = np.concatenate([r["idx"] for r in CC.nu_reference("E-zero")])
    assert set(picks.tolist()) == set(range(9)) - set(CC.ZERO_WEIGHT)      # 1 and 7 are the ends in reach
    # the edges of u: the first and the last grid value, each with a margin
    edges, ref = CC.nu_case("E-edges"), CC.nu_reference("E-edges")[0]
    lo, hi = (t - CC.GRID_BURN for t in CC.EDGE_SWEEPS)
    assert edges["u"][0, CC.EDGE_SWEEPS[0]] == 2.0 ** -53 and edges["u"][0, CC.EDGE_SWEEPS[1]] == 1 - 2.0 ** -53
    assert ref["idx"][lo] == 0 and ref["idx"][hi] == 8
    assert min(ref["margin"][lo], ref["margin"][hi]) >= R.MARGIN_FLOOR
    # lambda = 0: T_t = -inf, the pick is the index in force, the chain goes on
    c, t1 = CC.NONFINITE_CHAIN, CC.NONFINITE_SWEEP
    case = CC.nu_case("E-nonfinite")
    for dtype in (LD, np.float64):
        r = CC.nu_reference("E-nonfinite", dtype)[c]
        assert r["tstat"][t1 - CC.GRID_BURN] == -np.inf and np.isfinite(np.delete(r["tstat"], t1 - CC.GRID_BURN)).all()
        assert r["idx"][t1 - CC.GRID_BURN] == case["paths"][c, t1 - 1]
        assert np.isfinite(r["samples"].astype(np.float64)).all() and (r["weights"] > 0).all()


@pytest.mark.parametrize("kind", CC.POISONS)
def test_poisons_stop_the_reference_where_the_gpu_test_expects(kind):
    n, k = CC.STOP_SHAPE
    t0, burn, iters = CC.STOP_T0, CC.STOP_BURN, CC.STOP_ITERS
    clean, wclean = CC.run_fixed(n, k, *CC.fixed_inputs(n, k, burn, iters), burn, iters)
    assert np.isfinite(clean.astype(np.float64)).all()
    xi, g, gl = CC.poisoned(kind)
    s, w = CC.run_fixed(n, k, xi, g, gl, burn, iters)
    for c in (0, 2):                                            # the other chains' variates are untouched
        assert np.array_equal(s[c], clean[c]) and np.array_equal(w[c], wclean[c])
    bad = ~np.isfinite(s[1].astype(np.float64)).all(axis=1)
    first = t0 - burn if kind == "nan" else t0 + 1 - burn
    assert int(np.argmax(bad)) == first and bad[first:].all() and not bad[:first].any()
    assert np.array_equal(s[1, :first], clean[1, :first])
    assert np.isnan(s[1, t0 + 1 - burn:].astype(np.float64)).all() and np.isnan(w[1].astype(np.float64)).all()
    piv = CC.pivots_after(n, k, xi[1], g[1], gl[1], t0)
    if kind == "inf":
        assert piv[0] == np.inf
    elif kind == "negative":
        assert all(p > 0 for p in piv[:-1]) and piv[-1] < -1.0   # a clear margin, not a rounding accident
    else:
        assert np.isnan(np.float64(piv[0]))
        assert bad[first] and np.isnan(np.float64(s[1, first, k])) and np.isfinite(np.float64(s[1, first, 3]))
    # an early poison leaves no kept row; the same on the grid form's case
    xi, g, gl = CC.poisoned(kind, t0=CC.STOP_EARLY_T0)
    s, _ = CC.run_fixed(n, k, xi, g, gl, burn, iters)
    assert CC.STOP_EARLY_T0 + 1 < burn and np.isnan(s[1].astype(np.float64)).all()
    case = CC.nu_case("D")
    xi, g, gl = CC.nu_poisoned(kind)
    r = CC.run_nu(case, xi, g, gl, case["u"])[1]
    ref = CC.nu_reference("D")[1]
    assert not np.isfinite(np.float64(r["tstat"][t0 - burn])) and r["idx"][t0 - burn] == case["paths"][1, t0 - 1]
    assert np.array_equal(r["idx"][:t0 - burn], ref["idx"][:t0 - burn])
    assert np.isnan(r["samples"][t0 + 1 - burn:].astype(np.float64)).all()


def test_margins_of_the_device_seeds():
    """No Marsaglia-Tsang attempt of the device-RNG cases (the chain-level gamma stream and
    STREAM_ROBUST, at shape 2.5 over 87 sweeps and at the boosted shape 0.75) and no pick of the grid
    case lies within MARGIN_FLOOR of a boundary; float64 takes the long-double path."""
    for s, w, margin in CC.burn_device_reference() + CC.low_reference():
        assert margin >= R.MARGIN_FLOOR
        assert np.isfinite(s.astype(np.float64)).all() and (w > 0).all()
    assert (CC.LOW_NU + 1) / 2 < 1 and (CC.LOW_GRID[0] + 1) / 2 < 1 and CC.LOW_INIT == 0
    for (r, mt), (f, _) in zip(CC.low_nu_reference(), CC.low_nu_reference(np.float64)):
        assert r["margin"].min() >= R.MARGIN_FLOOR and mt >= R.MARGIN_FLOOR
        assert np.array_equal(r["path"], f["path"]) and len(np.unique(r["path"])) > 1
        assert np.count_nonzero(r["path"] == 0) > 0                 # sweeps drawn at the boosted shape
