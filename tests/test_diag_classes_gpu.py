"""Every launch class of the chain-diagnostics kernels (kernels_diag.hip) on the GPU (-m gpu), through
the raw entry bmc_chain_autocov / pybmc_amd.chain_autocovariance: each autocovariance of each lag
lane, each per-sequence mean and M2 of the shapes of tests/diag_cases.py against the exact longdouble
sums of tests/diag_exact_reference.py, within the error bound computed beside each value (worst
ratio <= 1, no point left out); lags >= n exactly 0; the middle draws exact; and the pairs of calls
that must agree bit for bit.  test_diag_plan.py pins, on the CPU, the class every shape reaches."""
import functools

import numpy as np
import pytest

import diag_cases as dc
import diag_exact_reference as X
from pybmc_amd import chain_autocovariance

pytestmark = pytest.mark.gpu

KEYS = ("seq_mean", "seq_m2", "shift", "acov")


def call(x, burn, cols, t0, nl):
    return chain_autocovariance(x, burn=burn, cols=cols, first_lag=t0, n_lags=nl)


@functools.lru_cache(maxsize=None)
def acov_result(tag):
    return call(*dc.acov_call(tag))


def assert_same_bits(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def check_against_exact(name, got, ref, x, burn, t0):
    """Worst |got - exact| / bound of the three outputs, printed, then asserted; the zero lags and
    the middle draws exactly."""
    x = x if x.ndim == 3 else x[None]
    C, T, P = x.shape
    n, M = ref["n"], 2 * C
    odd = (T - burn) % 2
    assert got["seq_mean"].shape == got["seq_m2"].shape == ((3 if odd else 2) * C, P)
    assert got["acov"].shape == ref["acov"].shape
    assert np.array_equal(got["shift"], x[0, burn])
    ratios = {"acov": X.worst_ratio(got["acov"], ref["acov"], ref["dacov"]),
              "seq_mean": X.worst_ratio(got["seq_mean"][:M], ref["seq_mean"], ref["dmean"]),
              "seq_m2": X.worst_ratio(got["seq_m2"][:M], ref["seq_m2"], ref["dm2"])}
    print("%s: n = %d, worst |got - exact| / bound: acov %.4f, seq_mean %.4f, seq_m2 %.4f"
          % (name, n, ratios["acov"], ratios["seq_mean"], ratios["seq_m2"]))
    assert np.isfinite(got["acov"]).all() and max(ratios.values()) <= 1.0, ratios
    dead = t0 + np.arange(got["acov"].shape[1]) >= n
    assert np.all(got["acov"][:, dead] == 0.0)
    if odd:
        assert np.array_equal(got["seq_mean"][M:], x[:, burn + n] - got["shift"])
        assert np.all(got["seq_m2"][M:] == 0.0)


@pytest.mark.parametrize("tag", list(dc.ACOV_CASES))
def test_acov_class(tag):
    x, burn, cols, t0, nl = dc.acov_call(tag)
    got = acov_result(tag)
    check_against_exact(tag, got, dc.acov_reference(tag), x, burn, t0)
    n = (x.shape[1] - burn) // 2
    if tag in ("A1", "C", "G"):
        assert t0 + nl > n              # these rows carry lags past the end


@pytest.mark.parametrize("key", list(dc.MOMENT_CASES), ids=dc.moment_id)
def test_moment_class(key):
    C, T, burn, P = key
    x = dc.samples(C, T, P)
    got = call(x, burn, None, 0, 1)
    check_against_exact(dc.moment_id(key), got, dc.moment_reference(key), x, burn, 0)


@pytest.mark.parametrize("tag", list(dc.ACOV_CASES))
def test_repeated_call_and_device_entry_same_bits(tag):
    import torch
    x, burn, cols, t0, nl = dc.acov_call(tag)
    first = acov_result(tag)
    assert_same_bits(first, call(x, burn, cols, t0, nl), "repeat")
    t = torch.as_tensor(np.array(x), device="cuda:0")
    assert_same_bits(first, call(t, burn, cols, t0, nl), "device")


@pytest.mark.parametrize("tag", list(dc.ACOV_CASES))
def test_padded_rows_same_bits(tag):
    """ld = P + 3 with NaN in the padding: read in place, and no padding is ever read."""
    x, burn, cols, t0, nl = dc.acov_call(tag)
    C, T, P = x.shape
    wide = np.full((C, T, P + 3), np.nan)
    wide[:, :, :P] = x
    view = wide[:, :, :P]
    assert view.strides == (T * (P + 3) * 8, (P + 3) * 8, 8)
    assert_same_bits(acov_result(tag), call(view, burn, cols, t0, nl), "padded")


def test_column_order_does_not_move_a_columns_bits():
    """The plan depends on n_active alone: shape H's columns in another order, and with the
    columns it left out swapped in, give each column the same bits."""
    x, burn, cols, t0, nl = dc.acov_call("H")
    first = acov_result("H")
    order = np.random.Generator(np.random.PCG64(8)).permutation(len(cols))
    assert np.any(order != np.arange(len(cols)))
    again = call(x, burn, cols[order], t0, nl)
    assert again["acov"].tobytes() == first["acov"][order].tobytes()
    for k in ("seq_mean", "seq_m2", "shift"):
        assert again[k].tobytes() == first[k].tobytes(), k
    # the other 19 columns and two of the first call's: still 21 active
    rest = np.setdiff1d(np.arange(x.shape[2]), cols)
    mixed = np.concatenate([rest[:10], cols[:2], rest[10:]]).astype(np.int32)
    assert len(mixed) == len(cols)
    other = call(x, burn, mixed, t0, nl)
    assert other["acov"][10:12].tobytes() == first["acov"][:2].tobytes()
    full = call(x, burn, None, t0, nl)          # 40 active: another plan, the same sums in another order
    ref = dc.acov_reference("H")
    assert X.worst_ratio(full["acov"][cols], ref["acov"], ref["dacov"]) <= 1.0
    assert full["seq_m2"].tobytes() == first["seq_m2"].tobytes()


def test_nan_stays_in_its_column():
    x, burn, cols, t0, nl = dc.acov_call("B")
    clean = acov_result("B")
    bad = np.array(x)
    bad[1, 37, 1] = np.nan                      # half 0 of chain 1: sequence 2
    got = call(bad, burn, cols, t0, nl)
    for j in (0, 2):
        assert got["acov"][j].tobytes() == clean["acov"][j].tobytes()
        for k in ("seq_mean", "seq_m2"):
            assert got[k][:, j].tobytes() == clean[k][:, j].tobytes(), (k, j)
    assert np.isnan(got["acov"][1]).all()
    assert np.isnan(got["seq_mean"][2, 1]) and np.isnan(got["seq_m2"][2, 1])
    keep = [0, 1, 3]
    assert got["seq_mean"][keep, 1].tobytes() == clean["seq_mean"][keep, 1].tobytes()
    assert got["seq_m2"][keep, 1].tobytes() == clean["seq_m2"][keep, 1].tobytes()
    assert got["shift"].tobytes() == clean["shift"].tobytes()
    # the column's first kept draw is its shift: then every output of the column is NaN
    bad = np.array(x)
    bad[0, 0, 1] = np.nan
    got = call(bad, burn, cols, t0, nl)
    assert np.isnan(got["acov"][1]).all() and np.isnan(got["seq_mean"][:, 1]).all()
    assert np.isnan(got["seq_m2"][:, 1]).all() and np.isnan(got["shift"][1])
    assert got["acov"][[0, 2]].tobytes() == clean["acov"][[0, 2]].tobytes()


def test_bad_arguments_raise():
    from pybmc_amd import _lib
    x = np.array(dc.samples(2, 260, 3))
    with pytest.raises(ValueError, match="cols"):
        chain_autocovariance(x, cols=[0, 3])
    with pytest.raises(ValueError, match="cols"):
        chain_autocovariance(x, cols=[-1])
    with pytest.raises(ValueError, match="n_active"):
        chain_autocovariance(x, cols=[])
    with pytest.raises(ValueError, match="first_lag"):
        chain_autocovariance(x, first_lag=-1)
    with pytest.raises(ValueError, match="n_lags"):
        chain_autocovariance(x, n_lags=0)
    with pytest.raises(ValueError, match="n = "):
        chain_autocovariance(x, burn=253)
    # and the C ABI's own checks, past the Python wrapper
    ctx = _lib.default_context(0)
    with ctx.lock:
        with pytest.raises(ValueError, match=r"cols\[1\] = 3"):
            ctx.chain_autocov(x, 2, 260, 3, 3, cols=[0, 3])
        with pytest.raises(ValueError, match=r"cols\[0\] = -1"):
            ctx.chain_autocov(x, 2, 260, 3, 3, cols=[-1])
        with pytest.raises(ValueError, match="n_active"):
            ctx.chain_autocov(x, 2, 260, 3, 3, cols=[])
        with pytest.raises(ValueError, match="first_lag"):
            ctx.chain_autocov(x, 2, 260, 3, 3, first_lag=-1)
        with pytest.raises(ValueError, match="n_lags"):
            ctx.chain_autocov(x, 2, 260, 3, 3, n_lags=0)
        with pytest.raises(ValueError, match="ld must be >= n_cols"):
            ctx.chain_autocov(x, 2, 260, 3, 2)
        ok = ctx.chain_autocov(x, 2, 260, 3, 3, first_lag=120, n_lags=64)     # t0 + n_lags > n
    assert np.all(ok["acov"][:, 10:] == 0.0) and np.all(ok["acov"][:, :10] != 0.0)
