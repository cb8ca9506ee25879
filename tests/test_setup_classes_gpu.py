"""The set-up kernels of kernels_setup.hip, one shape per launch class, against exact references
(-m gpu): residual_rss_kernel<T, VEC, NB> at every (storage type, rows per lane) pair and batch
width, flat and two-level tickets and a second trip of the panel loop; panelize_kernel<T> with
padded leading dimensions in both layouts at 1, 2 and 4 rows per lane; centre_kernel<VEC> ->
rotate_kernel<double, VEC, 8> -> unpanelize_kernel at rotate's column-group and panel-count edges.

The class each shape reaches is pinned on the CPU (tests/test_setup_plan.py); the references are
numpy longdouble with a running error bound (tests/setup_reference.py, checked alone by
tests/test_setup_reference_host.py), so every comparison here is |device - exact| <= bound with no
tolerance chosen by hand.  Each test prints its worst deviation / bound ("ratio ...", pytest -s).

Not covered: residual_rss's non-temporal branch (panels past keep_panels, matrices above 190 MB).
It needs a 200 MB problem and differs from the branch tested here only in the loads' cache policy."""
import ctypes as C

import numpy as np
import pytest

import setup_cases as sc
import setup_reference as R
from gpu_common import gpu_ctx
from oracle import bmc_oracle as O

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-12


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def within(label, got, ref, bound):
    ratio = R.worst_ratio(got, ref, bound)
    print(f"ratio {label}: {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)
    return ratio


# --------------------------------------------------------------------------- residual_rss
@pytest.mark.parametrize("key", list(sc.RSS_CASES), ids=sc.case_id)
def test_rss_class(key):
    dt, n, k = key
    cls = sc.RSS_CASES[key]
    label = f"rss {dt} vec={cls['vec']} G={cls['G']} {cls['ticket']} trips={cls['trips']}"
    y, X, B = sc.rss_inputs(*key)
    val, bound = sc.rss_reference(*key)
    ctx = gpu_ctx()
    ctx.set_problem(y, X, dtype=sc.np_dtype(dt))
    alone = np.array([ctx.residual_rss(b)[0] for b in B])          # NB = 1, one vector per launch
    within(label + " each alone", alone, val[:8], bound[:8])
    for nb in sc.RSS_BATCHES:
        got = ctx.residual_rss(B[:nb])
        within(f"{label} nb={nb}", got, val[:nb], bound[:nb])
        # the accumulators of a batch are independent per vector
        assert np.array_equal(bits(got), bits(alone[:nb])), nb
        # and the launch left its ticket words zero: the same call again, the same bits
        assert np.array_equal(bits(ctx.residual_rss(B[:nb])), bits(got)), nb
    within(label + " b=0 (y'y)", ctx.residual_rss(np.zeros(k)), val[8:], bound[8:])
    if dt == "f64":
        # sigma2_init = rss(b_ols) / n, as replay_against_oracle asserts it
        prior = sc.diagonal_prior(k)
        ctx.set_prior(*prior)
        want = O.chain_setup(y, X, prior)["sigma2_init"]
        s2i = ctx.basis()[2]
        print(f"sigma2_init {label}: rel {abs(s2i - want) / want:.3e}")
        assert abs(s2i - want) <= STEP_TOL * want


def test_rss_flat_ticket_after_two_level_on_one_context():
    """A two-level launch leaves all 17 ticket words zero: the flat-ticket shape that follows it on
    the same context (and a two-level one after that) still meets its reference."""
    ctx = gpu_ctx()
    for key in (("f64", 70001, 3), ("f64", 1237, 5), ("f64", 131073, 2), ("f64", 63, 2)):
        y, X, B = sc.rss_inputs(*key)
        val, bound = sc.rss_reference(*key)
        ctx.set_problem(y, X)
        for nb in (8, 1):
            within(f"rss sequence {sc.case_id(key)} nb={nb}", ctx.residual_rss(B[:nb]), val[:nb], bound[:nb])


# --------------------------------------------------------------------------- panelize
@pytest.mark.parametrize("key", list(sc.PANELIZE_CASES), ids=sc.case_id)
def test_panelize_padded_leading_dimension(key):
    """Row-major with ldx = k + 3 and col-major with ldx = n + 5, the padding NaN: the same Gram,
    bit for bit, as the contiguous matrix, both within 1e-12 of numpy on the storage-rounded data,
    and residual_rss of the padded problem within its bound."""
    from pybmc_amd import _lib
    dt, n, k = key
    t = sc.np_dtype(dt)
    y, X, B = sc.rss_inputs(*key)
    val, bound = sc.rss_reference(*key)
    ctx = gpu_ctx()
    lib = _lib.load_library()
    ctx.set_problem(y, X, dtype=t)
    want = ctx.gram()
    Xa = np.column_stack([X.astype(np.float64), y.astype(np.float64)])
    exact = Xa.T @ Xa
    assert rel(want, exact) < STEP_TOL
    Xr = np.full((n, k + 3), np.nan, dtype=t)
    Xr[:, :k] = X
    Xc = np.full((k, n + 5), np.nan, dtype=t)
    Xc[:, :n] = X.T
    for name, buf, ldx, layout in (("row-major", Xr, k + 3, _lib.BMC_ROW_MAJOR),
                                   ("col-major", Xc, n + 5, _lib.BMC_COL_MAJOR)):
        ctx.problem_generation += 1
        rc = lib.bmc_set_problem(ctx._h, buf.ctypes.data_as(C.c_void_p), n, k, ldx, layout,
                                 y.ctypes.data_as(C.c_void_p), _lib.BMC_F32 if dt == "f32" else _lib.BMC_F64)
        assert rc == 0, name
        ctx.n, ctx.k = n, k
        got = ctx.gram()
        assert np.array_equal(bits(got), bits(want)), name
        assert rel(got, exact) < STEP_TOL, name
        within(f"panelize {dt} vec={sc.PANELIZE_CASES[key]['vec']} {name} rss", ctx.residual_rss(B), val[:8],
               bound[:8])


# --------------------------------------------------------------------------- orthogonalize
def run_orthogonalize(ctx, F, truth, k, pad):
    """ctx.orthogonalize, or with pad > 0 straight through bmc_orthogonalize with ldf = km + pad and
    NaN in the padding."""
    if pad == 0:
        return ctx.orthogonalize(F, truth, k)
    from pybmc_amd import _lib
    n, km = F.shape
    Fp = np.full((n, km + pad), np.nan)
    Fp[:, :km] = F
    mu, yc, U, S, Vt = np.empty(n), np.empty(n), np.empty((k, n)), np.empty(k), np.empty((k, km))
    ctx.problem_generation += 1
    rc = ctx._lib.bmc_orthogonalize(ctx._h, _lib._dptr(Fp), n, km, km + pad, _lib._dptr(truth), k,
                                    _lib._dptr(mu), _lib._dptr(yc), _lib._dptr(U), _lib._dptr(S), _lib._dptr(Vt))
    assert rc == 0
    ctx.n, ctx.k = n, k
    return mu, yc, U.T, S, Vt


@pytest.mark.parametrize("key", list(sc.ORTHO_CASES), ids=sc.case_id)
def test_orthogonalize_class(key):
    """mu, yc and U_hat against centre -> rotate -> unpanelize in longdouble, with W built from the
    Vt and S the call itself returned."""
    n, km, k, pad = key
    cls = sc.ORTHO_CASES[key]
    label = f"ortho vec={cls['vec']} np={cls['np']} KO={k} ncg={cls['ncg']} ldf=km+{pad}"
    F, truth = sc.ortho_inputs(n, km)
    ctx = gpu_ctx()
    mu, yc, U, S, Vt = run_orthogonalize(ctx, F, truth, k, pad)
    assert U.shape == (n, k) and np.isfinite(U).all()
    assert np.isfinite(S).all() and np.isfinite(Vt).all() and np.all(S > 0)
    ref = R.ortho_ref(F, truth, Vt, S)
    within(label + " mu", mu, ref["mu"], ref["dmu"])
    within(label + " yc", yc, ref["yc"], ref["dyc"])
    within(label + " U", U, ref["U"], ref["dU"])
    # what W stands for: U_hat has orthonormal columns (the eigen-solver's part, loosely)
    assert np.abs(U.T @ U - np.eye(k)).max() < 1e-9
    if pad:
        # the padded matrix is the same problem: the same bits as the contiguous call
        mu0, yc0, U0, S0, Vt0 = ctx.orthogonalize(F, truth, k)
        for a, b in ((mu, mu0), (yc, yc0), (U, U0), (S, S0), (Vt, Vt0)):
            assert np.array_equal(bits(a), bits(b))
