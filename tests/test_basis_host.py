"""CPU checks of the prior-basis algebra (bmc_basis.h over host_linalg.hpp; g++ builds
tests/basis_check.cpp): the K x K host computation that turns X'X, X'y and a prior into a chain's
set-up arrays for bmc_set_prior and for every fold of bmc_kfold_cv / bmc_cv_path.

Cases: k = 1, 3, 17 (the tight_scaled problem of cv_reference.py: 90 x 17, snr 1e5, scale 1e3), 64
and 65 (the branch without G, u0, g0), each with a non-diagonal SPD C0 and a non-zero b0.

Exact (no tolerance): the leading block of a wider C0 against the contiguous copy, a second call,
the FoldArrays packing against the single-problem output (W transposed, the least-squares point,
W u0 as one in-order extended-precision sum per entry), the statuses, numerically_regular.

Identities, numpy as the reference: P C0 = I; W'(sym(P) + 1e-6 I)W = I; W'AW = diag(lam); G = W'AW;
c1 = W'P b0; c2 = W'xty; g0 = c2 - G u0; u0_j = c2_j / G_jj.  A residual is the largest absolute
difference, evaluated in extended precision, over the largest term of the sum it rounds (the
largest entry of the product of the absolute factors).  The bar of an identity and case is 10 x the
residual the identity leaves when numpy builds the basis in float64 from the same inputs (inv,
cholesky, eigh) -- the factor allows for another eigen-solver and summation order -- and at least
k x 2.2e-16.

Measured (g++, x86-64), residual of the header / of numpy, every identity and case (the test prints
them with the bar); the last column is the floor k x 2.2e-16 of the bars:
  k     P C0 = I           W'BW = I           W'AW = diag(lam)   G = W'AW           floor
  1     6.7e-17 / 6.7e-17  2.5e-16 / 2.5e-16  3.6e-17 / 3.6e-17  3.6e-17 / 3.6e-17  2.2e-16
  3     6.0e-17 / 2.1e-16  3.7e-16 / 1.5e-16  1.3e-16 / 3.1e-16  3.5e-17 / 1.2e-16  6.6e-16
  17    4.3e-16 / 4.7e-16  1.0e-15 / 1.2e-15  4.4e-16 / 8.0e-16  5.3e-17 / 1.9e-16  3.7e-15
  64    1.3e-15 / 5.3e-16  2.3e-15 / 1.2e-15  1.7e-15 / 8.4e-16  5.0e-17 / 2.2e-16  1.4e-14
  65    7.5e-16 / 4.7e-16  1.8e-15 / 1.3e-15  1.6e-15 / 1.0e-15  (not computed)     1.4e-14
  k     c1 = W'P b0        c2 = W'xty         g0 = c2 - G u0     u0 = c2 / diag G
  1     7.9e-17 / 7.9e-17  1.5e-17 / 1.5e-17  0       / 2.7e-17  2.7e-17 / 2.7e-17
  3     6.0e-17 / 4.6e-17  3.8e-17 / 5.8e-17  2.2e-20 / 6.6e-17  2.9e-17 / 3.7e-17
  17    2.6e-17 / 9.6e-17  2.7e-17 / 9.5e-17  5.8e-20 / 7.6e-17  9.3e-17 / 3.4e-17
  64    1.5e-17 / 7.5e-17  4.2e-17 / 1.1e-16  2.7e-19 / 8.9e-17  6.8e-17 / 4.1e-17
  65    1.8e-17 / 7.6e-17  3.7e-17 / 8.1e-17  (not computed)     (not computed)
(g0 is one extended-precision sum.)  The largest share of a bar used is W'BW = I at k = 3:
3.7e-16 of 1.5e-15.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cv_reference as CV

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.2e-16
LD = np.longdouble

# k: (n, snr, scale) of CV.problem
CASES = {1: (50, 10.0, 1.0), 3: (150, 10.0, 1.0), 17: (90, 1e5, 1e3), 64: (300, 10.0, 1.0), 65: (200, 10.0, 1.0)}
OUTPUTS = ("P", "Li", "Pb0", "lam", "W", "c1", "c2", "bols")
GRAM = ("G", "u0", "g0", "Wu0")


def build(tmp, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp / name
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                        os.path.join(HERE, "basis_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("basis"), "basis_check")


_inputs = {}


def inputs(k):
    """(C0, b0, A, xty, dtot) of a case, computed once and left unchanged"""
    if k not in _inputs:
        n, snr, scale = CASES[k]
        X, y, prior, _ = CV.problem(n, k, snr, scale=scale)
        rng = np.random.default_rng(1000 + k)
        R = rng.standard_normal((k, k))
        C0 = scale ** 2 * (10.0 * np.eye(k) + R @ R.T / k)        # SPD, not diagonal
        C0 = 0.5 * (C0 + C0.T)
        b0 = scale * rng.standard_normal(k)
        A = X.T @ X
        _inputs[k] = (C0, b0, 0.5 * (A + A.T), X.T @ y, np.diag(A).copy())
    return _inputs[k]


def put(d, **arrays):
    for name, a in arrays.items():
        np.ascontiguousarray(a, dtype=np.float64).tofile(os.path.join(str(d), name + ".f64"))


def get(d, name, shape):
    return np.fromfile(os.path.join(str(d), name + ".f64"), dtype=np.float64).reshape(shape)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def shape_of(name, k):
    return (k, k) if name in ("P", "Li", "W", "G") else (k,)


def run_basis(exe, d, k, C0, b0, A, xty, ldc=None):
    """the outputs of one `basis` call as {name: array}, after asserting its status is ok"""
    ldc = k if ldc is None else ldc
    Cw, bw = np.full((k, ldc), 7.5), np.full(ldc, -3.25)       # what lies outside the block is not read
    Cw[:, :k], bw[:k] = C0, b0
    os.makedirs(str(d), exist_ok=True)
    put(d, C0=Cw, b0=bw, A=A, xty=xty)
    assert run(exe, "basis", d, k, ldc, int(k <= 64)) == "ok"
    names = OUTPUTS + (GRAM if k <= 64 else ())
    assert not (k > 64 and os.path.exists(os.path.join(str(d), "G.f64")))
    return {name: get(d, name, shape_of(name, k)) for name in names}


_ours = {}


def ours(exe, tmp, k):
    if k not in _ours:
        _ours[k] = run_basis(exe, tmp / f"k{k}", k, *inputs(k)[:4])
    return _ours[k]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("basis_runs")


@pytest.mark.parametrize("k", list(CASES))
def test_leading_block_and_second_call_give_the_same_bytes(exe, tmp, k):
    first = ours(exe, tmp, k)
    wide = run_basis(exe, tmp / f"wide{k}", k, *inputs(k)[:4], ldc=k + 3)
    again = run_basis(exe, tmp / f"again{k}", k, *inputs(k)[:4])
    for name, v in first.items():
        assert v.tobytes() == wide[name].tobytes(), name
        assert v.tobytes() == again[name].tobytes(), name
        assert np.isfinite(v).all(), name


@pytest.mark.parametrize("k", [k for k in CASES if k <= 64])
@pytest.mark.parametrize("f", (0, 1, 2))
def test_fold_packing_holds_the_single_problem_output(exe, tmp, k, f):
    F = 3
    C0, b0, A, xty, dtot = inputs(k)
    one = ours(exe, tmp, k)
    d = tmp / f"fold{k}_{f}"
    os.makedirs(str(d))
    put(d, C0=C0, b0=b0, A=A, xty=xty, dtot=dtot)
    assert run(exe, "fold", d, k, F, f) == "ok"
    for name, src in (("G", one["G"]), ("WT", one["W"].T), ("lam", one["lam"]), ("c1", one["c1"]),
                      ("c2", one["c2"]), ("u0", one["u0"]), ("g0", one["g0"])):
        got = get(d, "fa_" + name, (F,) + src.shape)
        assert got[f].tobytes() == np.ascontiguousarray(src).tobytes(), name
        assert not got[[g for g in range(F) if g != f]].any(), name      # the other folds: untouched
    beta = get(d, "fa_beta", (2 * F, k))
    assert beta[f].tobytes() == one["bols"].tobytes()
    # row F + f is W u0 of the single problem: every entry one in-order extended-precision sum,
    # rounded once -- as the driver forms it from the ChainBasis, and as an explicit loop forms it here
    assert beta[F + f].tobytes() == one["Wu0"].tobytes()
    if np.finfo(LD).nmant >= 63:
        W, u0 = one["W"].astype(LD), one["u0"].astype(LD)
        loop = np.empty(k)
        for i in range(k):
            s = LD(0)
            for j in range(k):
                s += W[i, j] * u0[j]
            loop[i] = np.float64(s)
        assert beta[F + f].tobytes() == loop.tobytes()
    assert not beta[[g for g in range(2 * F) if g not in (f, F + f)]].any()
    assert not get(d, "fa_scal", (F, 4)).any()               # filled by the rss stage, not here


def test_every_failure_has_its_own_status(exe, tmp):
    for k in (1, 3, 17):
        C0, b0, A, xty, dtot = inputs(k)
        d = tmp / f"status{k}"
        os.makedirs(str(d))
        put(d, C0=np.ones((k, k)) if k > 1 else np.zeros((1, 1)), b0=b0, A=A, xty=xty, dtot=dtot)
        assert run(exe, "basis", d, k, k, 1) == "c0_singular"
        assert run(exe, "fold", d, k, 3, 1) == "c0_singular"
        put(d, C0=-np.eye(k))                                # the inverse exists, no Cholesky factor
        assert run(exe, "basis", d, k, k, 1) == "not_pd"
        assert run(exe, "fold", d, k, 3, 1) == "not_pd"
        if k > 1:
            n, snr, scale = CASES[k]
            X, y, _, _ = CV.problem(n, k, snr, scale=scale)
            X[:, k - 1] = X[:, 0]                             # rank deficient
            put(d, C0=C0, A=X.T @ X, xty=X.T @ y, dtot=np.diag(X.T @ X))
            assert run(exe, "fold", d, k, 3, 1) == "a_singular"


def test_numerically_regular(exe, tmp):
    for k in CASES:
        C0, b0, A, xty, dtot = inputs(k)
        d = tmp / f"regular{k}"
        os.makedirs(str(d))
        put(d, A=A, dtot=dtot)
        assert run(exe, "regular", d, k) == "regular"
        if k > 1:
            n, snr, scale = CASES[k]
            X = CV.problem(n, k, snr, scale=scale)[0]
            X[:, k - 1] = X[:, 0]
            put(d, A=X.T @ X, dtot=np.diag(X.T @ X))
            assert run(exe, "regular", d, k) == "deficient"


def numpy_basis(k, C0, b0, A, xty):
    """The same quantities built by numpy in float64 (inv, cholesky, eigh): the yardstick of the bars"""
    P = np.linalg.inv(C0)
    B = 0.5 * (P + P.T) + 1e-6 * np.eye(k)
    Li = np.linalg.inv(np.linalg.cholesky(B))
    M = Li @ A @ Li.T
    lam, Q = np.linalg.eigh(0.5 * (M + M.T))
    W = Li.T @ Q
    out = {"P": P, "W": W, "lam": lam, "c1": W.T @ (P @ b0), "c2": W.T @ xty}
    G = W.T @ A @ W
    out["G"] = 0.5 * (G + G.T)
    out["u0"] = out["c2"] / np.diag(out["G"])
    out["g0"] = out["c2"] - out["G"] @ out["u0"]
    return out


def residuals(b, k, C0, b0, A, xty):
    """{identity: residual relative to its largest term}; sums in extended precision"""
    x = {name: np.asarray(v).astype(LD) for name, v in b.items()}
    C0, b0, A, xty = (np.asarray(v).astype(LD) for v in (C0, b0, A, xty))
    eye = np.eye(k, dtype=LD)
    P, W, lam = x["P"], x["W"], x["lam"]
    B = 0.5 * (P + P.T) + LD(1e-6) * eye
    aW = np.abs(W)

    def rel(diff, term):
        return float(np.abs(diff).max() / np.abs(term).max())

    WAW = W.T @ A @ W
    r = {"P C0 = I": rel(P @ C0 - eye, np.abs(P) @ np.abs(C0)),
         "W'BW = I": rel(W.T @ B @ W - eye, aW.T @ np.abs(B) @ aW),
         "W'AW = diag(lam)": rel(WAW - np.diag(lam), aW.T @ np.abs(A) @ aW),
         "c1 = W'P b0": rel(x["c1"] - W.T @ (P @ b0), aW.T @ (np.abs(P) @ np.abs(b0))),
         "c2 = W'xty": rel(x["c2"] - W.T @ xty, aW.T @ np.abs(xty))}
    if "G" in x:
        G, u0 = x["G"], x["u0"]
        r["G = W'AW"] = rel(G - WAW, aW.T @ np.abs(A) @ aW)
        r["g0 = c2 - G u0"] = rel(x["g0"] - (x["c2"] - G @ u0), np.maximum(np.abs(x["c2"]), np.abs(G) @ np.abs(u0)))
        r["u0 = c2 / diag G"] = rel(u0 - x["c2"] / np.diag(G), u0)
    return r


@pytest.mark.parametrize("k", list(CASES))
def test_identities_hold_as_well_as_numpys_basis(exe, tmp, k):
    C0, b0, A, xty, _ = inputs(k)
    got = residuals(ours(exe, tmp, k), k, C0, b0, A, xty)
    ref = residuals(numpy_basis(k, C0, b0, A, xty), k, C0, b0, A, xty)
    assert k > 64 or len(got) == 8
    failed = []
    for name, r in got.items():
        bar = max(10.0 * ref[name], k * EPS)
        print(f"k={k} {name}: header {r:.2e}, numpy {ref[name]:.2e}, bar {bar:.2e}")
        if not r <= bar:
            failed.append(name)
    assert not failed


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    san = build(tmp_path, "basis_check_san", "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=undefined")
    for k in CASES:
        C0, b0, A, xty, dtot = inputs(k)
        run_basis(san, tmp_path / f"k{k}", k, C0, b0, A, xty)
        run_basis(san, tmp_path / f"wide{k}", k, C0, b0, A, xty, ldc=k + 3)
        put(tmp_path / f"k{k}", dtot=dtot)
        assert run(san, "regular", tmp_path / f"k{k}", k) == "regular"
        if k <= 64:
            assert run(san, "fold", tmp_path / f"k{k}", k, 3, 2) == "ok"
    d = tmp_path / "k3"
    put(d, C0=np.ones((3, 3)))
    assert run(san, "basis", d, 3, 3, 1) == "c0_singular"
    put(d, C0=-np.eye(3))
    assert run(san, "fold", d, 3, 3, 0) == "not_pd"
