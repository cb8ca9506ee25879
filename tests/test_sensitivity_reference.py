"""The numpy reference of the power-scaling sensitivity (tests/sens_reference.py) against what its
definition implies, on the CPU; and the two problems of the end-to-end diagnosis tests
(tests/test_sensitivity_gpu.py) are chosen here, where the long-double reference can say how far
from the 0.05 threshold they lie."""
import os

import numpy as np
import pytest

import sens_reference as SR

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))


def _golden(name):
    with np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_cjs_is_zero_for_uniform_weights(dtype):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(501)
    cjs, mean, sd = SR.cjs_distance(x, np.full(501, 1.0 / 501), dtype)
    assert cjs <= 1e-7      # sqrt of a sum of roundings: exact 0 in exact arithmetic
    assert abs(mean - x.mean()) < 1e-13 and abs(sd - x.std()) < 1e-13
    # a power of two draws: every P_j and Q_j is exact and so is the zero
    x = rng.standard_normal(512)
    assert SR.cjs_distance(x, np.full(512, 1.0 / 512), dtype)[0] == 0


def test_cjs_is_zero_for_a_constant_column():
    w = np.random.default_rng(2).random(100)
    assert SR.cjs_distance(np.full(100, 3.25), w / w.sum(), LD)[0] == 0


def test_cjs_is_invariant_under_positive_affine_maps():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(400)
    w = np.exp(0.3 * rng.standard_normal(400))
    w /= w.sum()
    base = SR.cjs_distance(x, w, LD)[0]
    assert base > 1e-3
    for a, b in ((2.0, 0.0), (0.125, -7.0), (1e6, 3.0), (3.7, 1e3)):
        assert abs(SR.cjs_distance(a * x + b, w, LD)[0] - base) < 1e-12 * base * max(1.0, abs(b))


def test_elementwise_form_is_the_definition():
    """The per-element form float64 needs is the definition as written, to long-double rounding."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal(300)
    x[10:40] = x[10]                  # a run of ties
    w = np.exp(0.2 * rng.standard_normal(300))
    w[5] = 0.0
    w /= w.sum()
    a = SR.cjs_distance(x, w, LD, elementwise=True)[0]
    b = SR.cjs_distance(x, w, LD, elementwise=False)[0]
    assert a > 1e-3 and abs(a - b) < 1e-12 * a
    # in float64 the written form loses digits to the cancellation, the element-wise one does not
    assert abs(SR.cjs_distance(x, w, np.float64, elementwise=True)[0] - a) < 1e-12 * a


def test_cjs_is_symmetric_in_the_two_distributions_of_a_two_point_sample():
    # two draws 0 and 1 with weights (q, 1 - q) against (1/2, 1/2): only j = 1 has a gap
    q = LD(0.3)
    cjs = SR.cjs_distance([0.0, 1.0], [q, 1 - q], LD)[0]
    P, m = LD(0.5), (LD(0.5) + q) / 2
    want = np.sqrt((P * np.log2(P / m) + q * np.log2(q / m)) / (P + q))
    assert abs(cjs - want) < 1e-17


def test_weights_follow_psis_row_and_sum_to_one():
    rng = np.random.default_rng(5)
    lp = -0.5 * rng.standard_normal(400) ** 2 * 30
    for alpha in (0.5, 0.99, 1.01, 2.0):
        w, k = SR.psis_weights(lp, alpha, LD)
        assert abs(w.sum() - 1) < 1e-17 and (w >= 0).all() and np.isfinite(k)
        # monotone in lp, in the direction of alpha - 1
        o = np.argsort(lp)
        dw = np.diff(w[o])
        assert (dw >= -1e-20).all() if alpha > 1 else (dw <= 1e-20).all()
    w, k = SR.psis_weights(lp[:24], 1.01, LD)                       # M = 4: raw weights
    raw = np.exp((LD(1.01) - 1) * lp[:24].astype(LD))
    assert k == np.inf and np.abs(w - raw / raw.sum()).max() < 1e-18
    w, k = SR.psis_weights(np.zeros(100), 1.01, LD)                 # one repeated value
    assert k == np.inf and np.all(w == LD(1) / 100)


def test_likelihood_sensitivity_vanishes_without_a_design():
    """A = 0: the likelihood does not depend on beta; beta and sigma independent draws.  Its
    power-scaling reweights by sigma alone and leaves the coefficients where they are."""
    A, y, theta, prior, _ = SR.random_case(40, 2, 4000, 11)
    A = np.zeros_like(A)
    theta[:, 2] = 0.9            # a fixed sigma: the likelihood is constant over the draws
    out = SR.sensitivity(A, y, theta, prior, dtype=LD)
    p_lik = SR.psens(out["cjs"][1, 0], out["cjs"][1, 1])
    assert np.all(p_lik[:2] < 1e-12)     # uniform weights: the roundings of j / S and of the sums
    assert np.all(out["pareto_k"][1] == np.inf)      # a tail of one repeated value
    p_prior = SR.psens(out["cjs"][0, 0], out["cjs"][0, 1])
    assert np.all(p_prior[:2] > 1e-3)


def test_conjugate_toy_has_a_large_prior_sensitivity():
    A, y, prior = SR.conflict_problem()
    theta = SR.conjugate_draws(A, y, prior, 2000, 5, 0.5)
    out = SR.sensitivity(A, y, theta, prior, dtype=LD)
    p_prior = SR.psens(out["cjs"][0, 0, 0], out["cjs"][0, 1, 0])
    p_lik = SR.psens(out["cjs"][1, 0, 0], out["cjs"][1, 1, 0])
    # the diagnosis test's first problem: both a factor 2 above the threshold
    assert p_prior >= 2 * SR.THRESHOLD and p_lik >= 2 * SR.THRESHOLD
    assert SR.diagnose(p_prior, p_lik) == "prior-data conflict"
    # the analytic shift: scaling the prior by alpha moves the posterior mean by about
    # (alpha - 1) (b0 - mean) / (C0 prec); the weighted mean follows it
    b0, C0 = 0.0, 0.05
    prec = 1 / C0 + float(A[:, 0] @ A[:, 0]) / 0.25
    mean = (float(A[:, 0] @ y) / 0.25) / prec
    shift = 0.01 * (b0 - mean) / (C0 * prec)
    got = out["mean"][0, 1, 0] - theta[:, 0].mean()
    assert abs(got - shift) < 0.25 * abs(shift)


def test_reference_defaults_on_the_golden_problem_show_no_prior_sensitivity():
    """The diagnosis test's second problem: the reference's own priors on its 629 x 3 problem
    (the golden chain stands in for the GPU's chains: the same posterior)."""
    g = _golden("gibbs_ortho629x3")
    prior = [g["b0"], g["C0"], float(g["nu0"]), float(g["s20"])]
    out = SR.sensitivity(g["X"], g["y"], g["samples"][200:], prior, g["Vt"], dtype=LD)
    p_prior = SR.psens(out["cjs"][0, 0], out["cjs"][0, 1])
    p_lik = SR.psens(out["cjs"][1, 0], out["cjs"][1, 1])
    assert p_prior.max() <= SR.THRESHOLD / 2
    assert all(SR.diagnose(p, l) == "-" for p, l in zip(p_prior, p_lik))


def test_float64_reference_is_close_to_long_double():
    A, y, theta, prior, Vt = SR.random_case(29, 3, 700, 21, n_models=2)
    a = SR.sensitivity(A, y, theta, prior, Vt, dtype=np.float64)
    b = SR.sensitivity(A, y, theta, prior, Vt, dtype=LD)
    assert np.abs(a["cjs"] - b["cjs"]).max() < 1e-10
    assert np.abs(a["weights"] - b["weights"]).max() < 1e-12
    assert np.abs(a["pareto_k"] - b["pareto_k"]).max() < 1e-8


def test_non_finite_input_is_nan_where_defined():
    A, y, theta, prior, Vt = SR.random_case(20, 2, 100, 31, n_models=2)
    bad = theta.copy()
    bad[7, 1] = np.nan
    out = SR.sensitivity(A, y, bad, prior, Vt, dtype=np.float64)
    assert out["component_flags"].all() and np.isnan(out["cjs"]).all()
    bad = theta.copy()
    bad[3, 2] = -0.5
    out = SR.sensitivity(A, y, bad, prior, Vt, components=SR.COMPONENTS, dtype=np.float64)
    assert out["component_flags"].all()
    Vb = Vt.copy()
    Vb[0, 1] = np.nan
    out = SR.sensitivity(A, y, theta, prior, Vb, dtype=np.float64)
    assert list(out["column_flags"]) == [False, False, False, False, True]
    assert np.isnan(out["cjs"][:, :, 4]).all() and np.isfinite(out["cjs"][:, :, :4]).all()
