"""The host side of the rank-normalised diagnostics on the CPU: g++ builds tests/rank_math_check.cpp
and tests/rank_plan_check.cpp from the headers the library is built from (bmc_math.h: ndtri and the
sort key; bmc_rank_plan.h: limits, sort geometry, batches, scratch sizes), once more with
-fsanitize=address,undefined as stand-alone programs; and the numpy reference is checked against
the definitions it restates."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import ndtri

import diag_reference as D
import rank_reference as RR

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
P_MIN = 6e-8      # (1 - 3/8) / (S + 1/4) at S = 7.4 M and beyond: the smallest argument in use


def _build(tmp, src, name, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp / name
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(HERE, src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exes(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rank_" + request.param)
    extra = SAN if request.param == "sanitized" else ()
    return {"math": _build(tmp, "rank_math_check.cpp", "rank_math_check", extra),
            "plan": _build(tmp, "rank_plan_check.cpp", "rank_plan_check", extra)}


def _run(exe, args, text=""):
    r = subprocess.run([exe, *map(str, args)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _ndtri(exe, p):
    out = _run(exe, ["ndtri"], "\n".join(float(v).hex() for v in p))
    return np.array([float.fromhex(s) for s in out.split()])


def _grid():
    tail = np.logspace(np.log10(P_MIN), np.log10(0.5), 20001)
    r = np.linspace(4.9, 5.1, 4001)                       # the split of the two tail approximations
    edge = np.concatenate([0.5 - np.linspace(0.42, 0.43, 2001), 0.5 + np.linspace(0.42, 0.43, 2001),
                           np.exp(-r * r), 1.0 - np.exp(-r * r)])
    p = np.concatenate([tail, 1.0 - tail, np.linspace(0.01, 0.99, 20001), edge,
                        [P_MIN, 1.0 - P_MIN, 0.5, 0.075, 0.925, np.exp(-25.0), 1.0 - np.exp(-25.0)]])
    return p[(p >= P_MIN) & (p <= 1.0 - P_MIN)]


def test_ndtri_against_scipy(exes):
    p = _grid()
    z = _ndtri(exes["math"], p)
    err = np.abs(z - ndtri(p))
    print("ndtri: max |err| = %.3e at p = %r, max |z| = %.3f" % (err.max(), p[err.argmax()], np.abs(z).max()))
    assert np.abs(z).max() <= 5.4
    assert err.max() <= 1e-14
    assert _ndtri(exes["math"], [0.5])[0] == 0.0


def test_ndtri_is_exactly_odd_where_one_minus_p_is_exact(exes):
    rng = np.random.default_rng(0)
    # multiples of 2^-40 in (0, 1): p and 1 - p are both exact
    k = rng.integers(1, 2 ** 40, size=20000)
    k = np.concatenate([k, rng.integers(1, 2 ** 17, size=5000)])      # and small p (the tails)
    p = k / 2.0 ** 40
    p = p[p >= P_MIN]
    assert np.all(1.0 - (1.0 - p) == p)
    a, b = _ndtri(exes["math"], p), _ndtri(exes["math"], 1.0 - p)
    assert np.array_equal(a, -b)


def test_key_transform_preserves_order_and_ties_the_zeros(exes):
    tiny = np.nextafter(0.0, 1.0)
    vals = [-np.inf, -1e308, -3.5, -1.0, -2.2250738585072014e-308, -1e-310, -tiny, -0.0, 0.0, tiny, 1e-310,
            2.2250738585072014e-308, 1.0, 1.0000000000000002, 3.5, 1e308, np.inf]
    out = _run(exes["math"], ["keys"], "\n".join(float(v).hex() for v in vals)).split()
    keys = [int(s, 16) for s in out[0::2]]
    back = [float.fromhex(s) for s in out[1::2]]
    for (a, ka), (b, kb) in zip(zip(vals, keys), zip(vals[1:], keys[1:])):
        if a == b:
            assert ka == kb, (a, b)             # -0.0 and +0.0
        else:
            assert ka < kb, (a, b)
    assert np.signbit(vals[7]) and not np.signbit(vals[8])
    assert keys[7] == keys[8] == 1 << 63
    assert back == [v + 0.0 for v in vals]      # the key inverts to the value (-0.0 to +0.0)
    assert not np.signbit(back[7])
    # NaNs land outside the infinities: a total order for the sort
    nan_key = int(_run(exes["math"], ["keys"], float("nan").hex()).split()[0], 16)
    assert nan_key > keys[-1] or nan_key < keys[0]


def plan(exe, C, iters, P, ld, burn, n_probs=3, cpb=0, budget=1 << 40):
    out = _run(exe, ["plan", C, iters, P, ld, burn, n_probs, cpb, budget])
    first = out.splitlines()[0]
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in first.split())


def test_readme_shape(exes):
    p = plan(exes["plan"], 64, 50000, 33, 33, 0)
    assert p["ok"] == 1 and p["n"] == 25000 and p["S"] == 3200000
    assert p["tile"] == 4096 and p["tiles"] == 782 and p["passes"] == 8
    assert p["cols_per_batch"] == 33 and p["n_batches"] == 1
    assert p["bytes_keys"] == 33 * 3200000 * 8 and p["bytes_derived"] == 4 * p["bytes_keys"]
    # a 2 GiB budget: 56 bytes a draw and the histograms -> 11 columns at a time
    q = plan(exes["plan"], 64, 50000, 33, 33, 0, budget=2 << 30)
    assert q["ok"] == 1 and q["cols_per_batch"] == 11 and q["n_batches"] == 3 and q["bytes_total"] <= 2 << 30


@pytest.mark.parametrize("S,tiles", [(4095 * 2, 2), (4096, 1), (4094, 1), (4098, 2), (8192, 2), (10000, 3), (8, 1)])
def test_tiles_cover_the_split_draws(exes, S, tiles):
    assert S % 2 == 0
    p = plan(exes["plan"], 1, S, 1, 1, 0)          # one chain: S = 2 (iters // 2)
    assert p["ok"] == 1 and p["S"] == S and p["tiles"] == tiles
    assert (p["tiles"] - 1) * p["tile"] < S <= p["tiles"] * p["tile"]


def test_cols_per_batch_is_honoured(exes):
    for cpb, want, nb in ((1, 1, 5), (2, 2, 3), (5, 5, 1), (9, 5, 1)):
        p = plan(exes["plan"], 4, 2000, 5, 7, 0, cpb=cpb, budget=1)      # (a request ignores the budget)
        assert (p["ok"], p["cols_per_batch"], p["n_batches"]) == (1, want, nb)
    assert plan(exes["plan"], 4, 2000, 5, 7, 0, cpb=0, budget=1)["ok"] == 0     # auto: nothing fits in 1 byte


@pytest.mark.parametrize("args", [
    dict(C=1, iters=7, P=1, ld=1, burn=0),             # n = 3
    dict(C=1, iters=20, P=1, ld=1, burn=13),           # n = 3 after the burn
    dict(C=0, iters=100, P=1, ld=1, burn=0),
    dict(C=65537, iters=100, P=1, ld=1, burn=0),
    dict(C=1, iters=100, P=0, ld=1, burn=0),
    dict(C=1, iters=100, P=65537, ld=65537, burn=0),
    dict(C=1, iters=100, P=3, ld=2, burn=0),
    dict(C=1, iters=100, P=1, ld=1, burn=-1),
    dict(C=1, iters=100, P=1, ld=1, burn=0, n_probs=17),
    dict(C=1, iters=100, P=1, ld=1, burn=0, n_probs=-1),        # a probability of 1.5
    dict(C=1, iters=2 ** 31, P=1, ld=1, burn=0),                # S = 2^31
    dict(C=65536, iters=32768, P=1, ld=1, burn=0),              # S = 2^31
])
def test_limits_are_rejected(exes, args):
    assert plan(exes["plan"], **args)["ok"] == 0


def test_limits_are_accepted(exes):
    assert plan(exes["plan"], 1, 8, 1, 1, 0)["ok"] == 1
    assert plan(exes["plan"], 1, 9, 1, 1, 0, n_probs=16)["n"] == 4
    p = plan(exes["plan"], 1, 2 ** 31 - 1, 1, 1, 0)
    assert p["ok"] == 1 and p["S"] == 2 ** 31 - 2
    assert plan(exes["plan"], 65536, 32767, 65536, 65536, 0)["ok"] == 1


def test_sweep(exes):
    out = _run(exes["plan"], ["sweep"])
    plans, fails = out.split()[-2:]
    assert int(plans) == 6 * 10 * 6 * 4 * 5 * 5 * 3 and int(fails) == 0


def test_live_passes(exes):
    run = lambda *m: int(_run(exes["plan"], ["passes", *m]))
    assert run("ff", "ff") == 0                                   # one key: nothing to sort
    assert run("8000000000000003", "8000000000000000") == 1      # only the lowest digit differs
    assert run("c000000000000000", "8000000000000000") == 128
    assert run("ff", "ff", "ff00", "0100") == 2                   # any segment keeps a pass alive
    assert run("ffffffffffffffff", "0") == 255


def test_order_statistic_plan_is_numpys(exes):
    from pybmc_amd._lib import order_stat_plan
    for S in (8, 9, 4096, 16000, 3200000):
        for p in (0.0, 0.05, 0.5, 0.95, 1.0, 0.3333, 0.975):
            i, g = _run(exes["plan"], ["orderstat", S, float(p).hex()]).split()
            qi, qg = order_stat_plan(S, [np.float64(p) * 100])
            vi = (S - 1) * np.float64(p)
            assert int(i) == min(int(np.floor(vi)), S - 1)
            if p in (0.0, 0.5, 1.0):        # (percent / 100 is then exactly p)
                assert (int(i), float.fromhex(g)) == (int(qi[0]), float(qg[0]))
            if int(i) < S - 1:
                assert float.fromhex(g) == vi - np.floor(vi)


def test_reference_restates_the_definitions():
    rng = np.random.default_rng(5)
    x = D.ar1(rng, 2, 41, 2, 0.5)
    x[0, 3, 1] = -0.0
    x[1, 7, 1] = 0.0
    z = RR.rank_normalize(x, burn=0)
    assert z.shape == (4, 20, 2)
    assert z[0, 3, 1] == z[2, 7, 1]                  # the zeros tie (chain 1's first half is sequence 2)
    # ranks by counting: r = #(v < x) + (#(v == x) + 1) / 2
    s = RR.split(x)
    col = s[:, :, 0].reshape(-1)
    r = np.array([(col < v).sum() + ((col == v).sum() + 1) / 2 for v in col])
    np.testing.assert_array_equal(z[:, :, 0].reshape(-1), ndtri((r - 0.375) / (80 + 0.25)))
    # the middle draw of an odd T' is in no sequence
    assert not np.isin(x[:, 20, 0], s[:, :, 0]).any()
    d = RR.diagnostics(x)
    assert d["stop"].shape == (4, 2) and d["counts"].shape == (2, 2)
    np.testing.assert_array_equal(d["counts"][0], (s <= np.quantile(s.reshape(80, 2), 0.05, axis=0)).sum((0, 1)))
    c = D.diagnostics(RR.derived(x)[0]["z"].reshape(2, 40, 2))
    np.testing.assert_allclose(d["ess_bulk"], c["ess"], rtol=1e-12)    # (that one shifts by the first draw)
