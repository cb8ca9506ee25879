"""Every route of the predictive leg's order statistics and every tile edge of its GEMM (-m gpu).

(a), (b): the shared cases of tests/predict_cases.py write each point's draws exactly (preds = 0,
Vt_hat = 0, sigma = 1, replayed noise), so the returned draws are the noise bit for bit and the
percentiles and coverage counts are numpy's on them, exactly -- for every instantiation of
predict_select_kernel and predict_orderstat_kernel the plan can choose (tests/test_predict_plan.py
proves on the CPU that the case list reaches them all, with rows of every branch of the selection
in one call).  (c): random operands at the edges of the weight and GEMM tiles against an
extended-precision reference, with a derived bar.  (d): the argument checks of the C ABI.
"""
import ctypes as C

import numpy as np
import pytest

import predict_cases as PC
import predict_reference as PR
from gpu_common import gpu_ctx
from pybmc_amd import coverage
from pybmc_amd import _lib as L

pytestmark = pytest.mark.gpu


def run_case(ctx, case, inp, **kw):
    return ctx.predict(inp["preds"], inp["theta"], inp["Vt"], noise=inp["noise"], q=case.q,
                       truth=inp["truth"], cov_percentiles=case.cov, **kw)


@pytest.fixture(scope="module")
def forward():
    """All cases on one context, in list order: name -> (draws, bands, coverage)."""
    ctx = gpu_ctx()
    return {case.name: run_case(ctx, case, PC.case_inputs(case)) for case in PC.CASES}


# ---- (a) order statistics -----------------------------------------------------------------------

@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_order_statistics_are_exact(forward, case):
    ctx = gpu_ctx()
    inp = PC.case_inputs(case)
    draws, bands, cov = forward[case.name]
    assert np.array_equal(draws, inp["noise"])
    assert bands.shape == (len(case.q), case.M)
    assert np.array_equal(bands, np.percentile(draws, case.q, axis=0))
    if case.cov is None:
        assert cov is None
    else:
        assert cov == coverage(case.cov, draws, {"truth": inp["truth"]}, "truth")
    none, bands2, cov2 = run_case(ctx, case, inp, want_draws=False)
    assert none is None and np.array_equal(bands2, bands) and cov2 == cov
    draws_f, bands3, cov3 = run_case(ctx, case, inp, draws_order="F")
    assert draws_f.flags.f_contiguous and np.array_equal(draws_f, draws)
    assert np.array_equal(bands3, bands) and cov3 == cov


# ---- (b) state ----------------------------------------------------------------------------------

def test_results_do_not_depend_on_the_calls_before(forward):
    """The same cases in reverse order on the same context (small calls after big ones, calls
    that hand no point back after calls that did): every result bit for bit the forward pass's.
    A stale fail_count or hit counter, or stale slack behind the padded operands, would show."""
    ctx = gpu_ctx()
    for case in reversed(PC.CASES):
        draws, bands, cov = run_case(ctx, case, PC.case_inputs(case))
        want = forward[case.name]
        assert np.array_equal(draws, want[0]), case.name
        assert np.array_equal(bands, want[1]), case.name
        assert cov == want[2], case.name


# ---- (c) GEMM and weights edges -----------------------------------------------------------------
# A thin covering set: every Km in {1, 4, 9, 12, 13, 16, 17, 24, 28, 32, 48, 257} (Km_pad mod 16 =
# 4, 8, 12 and 0 with one slab and with several), k in {1, 4, 5, 7, 256} (the weights' chains of four
# and their tail), M in {1, 63, 64, 65} and S in {1, 15, 16, 17, 64, 65} (tile and draw-group edges),
# and two shapes with more than 16 tiles along an axis for the super-tile map.
GEMM_SHAPES = [  # (M, Km, k, S)
    (1, 1, 1, 1), (63, 4, 4, 15), (64, 9, 5, 16), (65, 12, 7, 17), (1, 13, 256, 64), (63, 16, 1, 65),
    (64, 17, 4, 1), (65, 24, 5, 15), (1, 28, 7, 16), (63, 32, 256, 17), (64, 48, 1, 64),
    (65, 257, 4, 65), (65, 16, 5, 65), (64, 12, 256, 64), (1100, 2, 3, 1100), (1025, 2, 2, 64)]
Q5 = (2.5, 50, 97.5, 0, 100)


@pytest.mark.parametrize("M,Km,k,S", GEMM_SHAPES)
def test_draws_meet_the_derived_bar(M, Km, k, S):
    """|got - ref| <= (Km + k + 4) 2^-53 (sum_m |p_m| (sum_i |theta_i V_im| + 1/Km) + |z| sigma):
    the bound of a sum of that many fused terms in any order, against an extended-precision
    reference.  Percentiles and coverage are numpy's on the returned draws."""
    assert PR.longdouble_is_extended()
    ctx = gpu_ctx()
    rng = np.random.default_rng(100000 * M + 1000 * Km + 10 * k + S)
    preds = rng.standard_normal((M, Km)) + 3
    theta = np.column_stack([rng.standard_normal((S, k)), rng.uniform(0.5, 1.5, S)])
    Vt = rng.standard_normal((k, Km))
    noise = rng.standard_normal((S, M))
    truth = preds.mean(1) + rng.standard_normal(M)
    ref, bar = PR.predictive_reference(preds, theta, Vt, noise)
    draws, bands, cov = ctx.predict(preds, theta, Vt, noise=noise, q=Q5, truth=truth,
                                    cov_percentiles=PC.COV21)
    assert draws.shape == (S, M)
    ratio = float((np.abs(draws.astype(np.longdouble) - ref) / bar).max())
    print(f"M={M} Km={Km} k={k} S={S}: worst |got - ref| / bar = {ratio:.4f}")
    assert ratio <= 1.0
    assert np.array_equal(bands, np.percentile(draws, Q5, axis=0))
    assert cov == coverage(PC.COV21, draws, {"truth": truth}, "truth")


# ---- (d) refusals -------------------------------------------------------------------------------

def test_requests_outside_the_limits_are_refused():
    ctx = gpu_ctx()
    M, Km, k = 3, 2, 1

    def call(S, q=(50,), cov=None):
        theta = np.column_stack([np.zeros((S, k)), np.ones(S)])
        return ctx.predict(np.zeros((M, Km)), theta, np.zeros((k, Km)), noise=np.ones((S, M)), q=q,
                           truth=None if cov is None else np.zeros(M), cov_percentiles=cov)

    with pytest.raises(ValueError, match="16384"):
        call(16385)
    with pytest.raises(ValueError, match="n_q and n_cov"):
        call(100, q=tuple(np.linspace(0, 100, 65)))
    with pytest.raises(ValueError, match="n_q and n_cov"):
        call(100, cov=list(np.linspace(0, 100, 65)))
    # a rank index >= S, through the C ABI itself
    S = 100
    theta = np.column_stack([np.zeros((S, k)), np.ones(S)])
    preds, Vt, noise = np.zeros((M, Km)), np.zeros((k, Km)), np.ones((S, M))
    bands, hits, truth = np.empty((1, M)), np.zeros(1, dtype=np.int64), np.zeros(M)
    i32p, dp = C.POINTER(C.c_int32), L._dptr

    def raw(qi, lo, hi):
        qi, lo, hi = (np.array([v], dtype=np.int32) for v in (qi, lo, hi))
        return ctx._lib.bmc_predict(
            ctx._h, dp(preds), M, Km, dp(theta), S, k, dp(Vt), L.BMC_RNG_REPLAY, 0, dp(noise),
            qi.ctypes.data_as(i32p), dp(np.zeros(1)), 1, dp(truth), lo.ctypes.data_as(i32p),
            hi.ctypes.data_as(i32p), 1, None, dp(bands), hits.ctypes.data_as(C.POINTER(C.c_int64)))

    assert raw(S, 0, S - 1) == L.BMC_EINVAL
    assert raw(0, S, S - 1) == L.BMC_EINVAL
    assert raw(0, 0, S) == L.BMC_EINVAL
    assert raw(-1, 0, S - 1) == L.BMC_EINVAL
    assert raw(S - 1, 0, S - 1) == L.BMC_OK
    assert np.array_equal(bands, np.ones((1, M))) and hits[0] == 0    # truth 0 is outside [1, 1]
    # and the context serves the next call as if nothing had happened
    draws, b, _ = call(S)
    assert np.array_equal(draws, np.ones((S, M))) and np.array_equal(b, np.ones((1, M)))
