"""Every launch class of the Student-t sampler on the MI355X (-m gpu): robust_chain_kernel<KC, NU_FREE>
through bmc_robust_run* at one shape per slab edge and kernel width, under a dense prior and with
burn-in, against the long-double numpy references of tests/robust_reference.py and
tests/robust_nu_reference.py; the burn-only call, the sigma2 floor inside a sweep, the stopped-chain
contract of include/pybmc_amd.h, grids of 2 .. 64 values with zero weights, edge uniforms and a T_t that
is not finite, and the device generator below shape 1.

Bars, the rule of test_robust_gpu.py: BAR_FACTOR = 1000 x the deviation of the FLOAT64 numpy
reference from the long-double one on the same case (robust_class_cases.REF_DEV, taken no smaller than
2^-52), samples relative to each column's scale, weights to the largest, T_t to n.  Picks are compared
exactly; test_robust_classes_host.py proves their margins, and every other condition assumed here, from
the references alone.

Measured on one MI355X, the GPU chains deviate from the long-double reference by (smallest .. largest
over the chains of a section):
  A  fixed nu, the eight shapes   samples 1.2e-16 .. 1.1e-14   weights 1.1e-16 .. 8.5e-16
  A  forced paths, four shapes    samples 3.7e-16 .. 7.3e-15   weights 2.2e-16 .. 8.6e-16   T_t 2.6e-16 .. 1.9e-15
  B  device RNG, burn 37          samples 7.8e-16 .. 8.0e-16   weights 3.6e-16 .. 4.3e-16
  C  floored sweep                samples 1.1e-14 .. 1.4e-12   weights 1.5e-15 .. 3.7e-14
  E  the seven grid cases         samples 3.0e-16 .. 2.1e-15   weights 1.2e-16 .. 5.0e-16   T_t 1.7e-16 .. 1.9e-15
  F  device RNG, nu = 0.5         samples 1.3e-15 .. 5.8e-15   weights 1.3e-15 .. 3.7e-15
  F  device RNG, grid from 0.5    samples 9.7e-16 .. 1.0e-15   weights 4.6e-16 .. 5.5e-16   T_t 1.9e-15 .. 3.5e-15
Every pick agrees with the reference's.  Section C is the largest because the sweeps after sigma2 = 1e-6
factor a Q of order 1e7; its float64 reference deviates by 7.4e-13 / 6.5e-14 on the same variates.
"""
import ctypes

import numpy as np
import pytest

from pybmc_amd import _lib

import robust_cases as RC
import robust_class_cases as CC
from test_robust_gpu import BAR_FACTOR, DEVICE_DEV

pytestmark = pytest.mark.gpu

I32P = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_case(ctx, n, k):
    y, X, prior = CC.problem(n, k)
    ctx.set_problem(y, CC.as_passed(n, k, X))
    ctx.set_prior(*prior)


def assert_pair(label, name, out, w, ref, wref):
    """samples and weights of one chain against the reference, to the bars of REF_DEV[name]"""
    bar = CC.bars(name)
    ds, dw = RC.scaled_deviation(out, ref), RC.weight_deviation(w, wref)
    print(f"{label}: samples {ds:.3e} (bar {bar[0]:.3e}), weights {dw:.3e} (bar {bar[1]:.3e})")
    assert ds <= bar[0]
    assert dw <= bar[1]


def assert_nu(label, name, n, out, w, ts, idx, ref):
    bar = CC.bars(name)
    assert_pair(label, name, out, w, ref["samples"], ref["weights"])
    dt = CC.tstat_deviation(ts, ref["tstat"], n)
    print(f"{label}: T {dt:.3e} (bar {bar[2]:.3e})")
    assert dt <= bar[2]
    assert np.array_equal(idx, ref["idx"])


def run_nu_case(ctx, name):
    c = CC.nu_case(name)
    set_case(ctx, c["n"], c["k"])
    return ctx.robust_run(None, CC.CHAINS, c["iters"], burn=c["burn"], xi=c["xi"], g=c["g"], gl=c["gl"],
                          u_nu=c["u"], nu_path=c["paths"], nu_grid=c["grid"], nu_weight=c["weight"],
                          nu_init=c["init"], want_tstat=True)


# ---- A: replay parity per slab and width class, with burn-in ----------------------------------------
@pytest.mark.parametrize("n,k", CC.SHAPES)
def test_fixed_nu_replay_parity_with_burn_in(ctx, n, k):
    xi, g, gl = CC.fixed_inputs(n, k)
    ref, wref = CC.fixed_reference(n, k)
    set_case(ctx, n, k)
    out, w, stats = ctx.robust_run(CC.NU, CC.CHAINS, CC.ITERS, burn=CC.BURN, xi=xi, g=g, gl=gl)
    assert stats["iterations"] == CC.BURN + CC.ITERS and stats["launches"] == 1
    for c in range(CC.CHAINS):
        assert_pair(f"N={n} k={k} chain {c}", f"{n}x{k}", out[c], w[c], ref[c], wref[c])


@pytest.mark.parametrize("name", [f"A-{n}x{k}" for n, k in CC.NU_SHAPES])
def test_forced_path_replay_parity_with_burn_in(ctx, name):
    ref = CC.nu_reference(name)
    out, w, idx, ts, _ = run_nu_case(ctx, name)
    for c in range(CC.CHAINS):
        assert_nu(f"{name} chain {c}", name, CC.nu_case(name)["n"], out[c], w[c], ts[c], idx[c], ref[c])


# ---- B: no kept sweep; device mode with burn-in -----------------------------------------------------
@pytest.mark.parametrize("burn", (0, 10))
def test_no_kept_sweep_gives_zero_weights(ctx, burn):
    n, k = 5, 4
    xi, g, gl = (a[:, :burn] for a in CC.fixed_inputs(n, k))
    set_case(ctx, n, k)
    out, w, stats = ctx.robust_run(CC.NU, CC.CHAINS, 0, burn=burn, xi=xi, g=g, gl=gl)   # BMC_OK: no raise
    assert out.shape == (CC.CHAINS, 0, k + 1) and stats["iterations"] == burn
    assert w.shape == (CC.CHAINS, n) and np.array_equal(w, np.zeros((CC.CHAINS, n)))
    assert not np.signbit(w).any()


def test_device_mode_weights_with_burn_in(ctx):
    y, X, prior = RC.device_problem()
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    out, w, st = ctx.robust_run(RC.DEVICE_NU, len(CC.BURN_DEVICE_SEEDS), CC.BURN_DEVICE_ITERS,
                                burn=CC.BURN_DEVICE_BURN, seeds=list(CC.BURN_DEVICE_SEEDS))
    assert st["iterations"] == CC.BURN_DEVICE_BURN + CC.BURN_DEVICE_ITERS
    for c, (ref, wref, _) in enumerate(CC.burn_device_reference()):
        ds, dw = RC.scaled_deviation(out[c], ref), RC.weight_deviation(w[c], wref)
        print(f"device RNG, burn 37, chain {c}: samples {ds:.3e}, weights {dw:.3e}")
        assert ds <= BAR_FACTOR * DEVICE_DEV[0]
        assert dw <= BAR_FACTOR * DEVICE_DEV[1]


# ---- C: the sigma2 floor in a sweep -----------------------------------------------------------------
def test_sigma2_floor_inside_a_sweep(ctx):
    n, k = CC.FLOOR_SHAPE
    xi, g, gl = CC.floor_inputs()
    ref, wref = CC.floor_reference()
    set_case(ctx, n, k)
    out, w, _ = ctx.robust_run(CC.NU, CC.CHAINS, CC.ITERS, burn=CC.BURN, xi=xi, g=g, gl=gl)
    assert np.isfinite(out).all() and np.isfinite(w).all()
    for c, t0 in enumerate(CC.FLOOR_SWEEPS):
        assert out[c, t0 - CC.BURN, k] == 1e-3                  # sqrt(1e-6), exactly
        assert_pair(f"floor at sweep {t0}, chain {c}", "C", out[c], w[c], ref[c], wref[c])


# ---- D: stopped chains ------------------------------------------------------------------------------
SENTINEL = 12345.0


def raw_fixed(ctx, xi, g, gl, burn=CC.STOP_BURN, iters=CC.STOP_ITERS):
    """bmc_robust_run on the test's own buffers (Context.robust_run raises before returning them):
    (return code, message, samples, weights)."""
    C = len(xi)
    xi, g, gl = (np.ascontiguousarray(a, dtype=np.float64) for a in (xi, g, gl))
    out, w = np.full((C, iters, ctx.k + 1), SENTINEL), np.full((C, ctx.n), SENTINEL)
    st = _lib.Stats()
    rc = ctx._lib.bmc_robust_run(ctx._h, CC.NU, C, iters, burn, _lib.BMC_RNG_REPLAY, None, _lib._dptr(xi),
                                 _lib._dptr(g), _lib._dptr(gl), _lib._dptr(out), _lib._dptr(w), ctypes.byref(st))
    return rc, (ctx._lib.bmc_last_error(ctx._h) or b"").decode(), out, w


def raw_nu(ctx, case, xi, g, gl):
    """bmc_robust_run_nu likewise: (return code, message, samples, weights, picks, T_t)."""
    C, iters, burn = len(xi), case["iters"], case["burn"]
    xi, g, gl, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (xi, g, gl, case["u"]))
    grid, wt = (np.ascontiguousarray(a, dtype=np.float64) for a in (case["grid"], case["weight"]))
    path = np.ascontiguousarray(case["paths"], dtype=np.int32)
    out, w = np.full((C, iters, ctx.k + 1), SENTINEL), np.full((C, ctx.n), SENTINEL)
    idx, ts = np.full((C, iters), 77, dtype=np.int32), np.full((C, iters), SENTINEL)
    st = _lib.Stats()
    rc = ctx._lib.bmc_robust_run_nu(ctx._h, _lib._dptr(grid), _lib._dptr(wt), len(grid), int(case["init"]), C, iters,
                                    burn, _lib.BMC_RNG_REPLAY, None, _lib._dptr(xi), _lib._dptr(g), _lib._dptr(gl),
                                    _lib._dptr(u), path.ctypes.data_as(I32P), _lib._dptr(out), _lib._dptr(w),
                                    idx.ctypes.data_as(I32P), _lib._dptr(ts), ctypes.byref(st))
    return rc, (ctx._lib.bmc_last_error(ctx._h) or b"").decode(), out, w, idx, ts


def assert_stopped(kind, t0, out, w, clean, wclean, stopped=(1,)):
    """The header's contract on samples and weights; returns the first NaN row of a stopped chain."""
    first = max(t0 + 1 - CC.STOP_BURN, 0)
    for c in range(CC.CHAINS):
        if c not in stopped:
            assert np.array_equal(out[c], clean[c]) and np.array_equal(w[c], wclean[c])
            continue
        assert np.isnan(out[c, first:]).all() and np.isnan(w[c]).all()
        same = first - 1 if kind == "nan" and first > 0 else first    # the NaN variate's own row
        assert np.array_equal(out[c, :same], clean[c, :same])
    return first


@pytest.mark.parametrize("kind", CC.POISONS)
def test_stopped_chain_contract(ctx, kind):
    n, k = CC.STOP_SHAPE
    t0, burn, iters = CC.STOP_T0, CC.STOP_BURN, CC.STOP_ITERS
    set_case(ctx, n, k)
    rc, _, clean, wclean = raw_fixed(ctx, *CC.fixed_inputs(n, k, burn, iters))
    assert rc == _lib.BMC_OK and np.isfinite(clean).all() and np.isfinite(wclean).all()
    # chain 1 alone
    xi, g, gl = CC.poisoned(kind)
    rc, msg, out, w = raw_fixed(ctx, xi, g, gl)
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg
    first = assert_stopped(kind, t0, out, w, clean, wclean)
    assert first == t0 + 1 - burn
    if kind == "nan":       # the row of the NaN variate itself: NaN where the reference's arithmetic puts it
        ref, _ = CC.run_fixed(n, k, xi[1:2], g[1:2], gl[1:2], burn, iters)
        assert np.array_equal(np.isnan(out[1, first - 1]), np.isnan(ref[0, first - 1].astype(np.float64)))
        assert np.isnan(out[1, first - 1, k])
    # chains 1 and 2: the message names the first
    rc, msg, out, w = raw_fixed(ctx, *CC.poisoned(kind, chains=(1, 2)))
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg and "(chain 2)" not in msg
    assert_stopped(kind, t0, out, w, clean, wclean, stopped=(1, 2))
    # a poison inside the burn-in: no kept row survives
    rc, msg, out, w = raw_fixed(ctx, *CC.poisoned(kind, t0=CC.STOP_EARLY_T0))
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg
    assert assert_stopped(kind, CC.STOP_EARLY_T0, out, w, clean, wclean) == 0 and np.isnan(out[1]).all()
    # the Python surface raises, and the context then gives the clean result bit for bit
    with pytest.raises(np.linalg.LinAlgError, match=r"\(chain 1\)"):
        ctx.robust_run(CC.NU, CC.CHAINS, iters, burn=burn, xi=xi, g=g, gl=gl)
    xi, g, gl = CC.fixed_inputs(n, k, burn, iters)
    again, wagain, _ = ctx.robust_run(CC.NU, CC.CHAINS, iters, burn=burn, xi=xi, g=g, gl=gl)
    assert np.array_equal(again, clean) and np.array_equal(wagain, wclean)


@pytest.mark.parametrize("kind", CC.POISONS)
def test_stopped_chain_contract_on_the_grid(ctx, kind):
    case = CC.nu_case("D")
    n, t0, burn, iters = case["n"], CC.STOP_T0, case["burn"], case["iters"]
    ref = CC.nu_reference("D")
    set_case(ctx, n, case["k"])
    rc, _, clean, wclean, iclean, tclean = raw_nu(ctx, case, case["xi"], case["g"], case["gl"])
    assert rc == _lib.BMC_OK
    for c in range(CC.CHAINS):
        assert np.array_equal(iclean[c], ref[c]["idx"]) and np.isfinite(tclean[c]).all()
    xi, g, gl = CC.nu_poisoned(kind)
    rc, msg, out, w, idx, ts = raw_nu(ctx, case, xi, g, gl)
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg
    first = assert_stopped(kind, t0, out, w, clean, wclean)
    for c in (0, 2):
        assert np.array_equal(idx[c], iclean[c]) and np.array_equal(ts[c], tclean[c])
    assert np.array_equal(idx[1, first:], np.full(iters - first, -1))       # rows never reached
    assert np.isnan(ts[1, first:]).all()
    # before the stop: the reference's picks (a T_t that is not finite keeps the index in force)
    pois = CC.run_nu(case, xi, g, gl, case["u"])[1]
    assert np.array_equal(idx[1, :first], pois["idx"][:first])
    assert idx[1, first - 1] == case["paths"][1, t0 - 1] and not np.isfinite(ts[1, first - 1])
    assert np.array_equal(ts[1, :first - 1], tclean[1, :first - 1])
    # both later chains stopped: still chain 1; inside the burn-in: nothing of chain 1 was reached
    rc, msg, out, w, idx, ts = raw_nu(ctx, case, *CC.nu_poisoned(kind, chains=(1, 2)))
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg and "(chain 2)" not in msg
    assert_stopped(kind, t0, out, w, clean, wclean, stopped=(1, 2))
    assert (idx[1:, first:] == -1).all() and np.isnan(ts[1:, first:]).all()
    rc, msg, out, w, idx, ts = raw_nu(ctx, case, *CC.nu_poisoned(kind, t0=CC.STOP_EARLY_T0))
    assert rc == _lib.BMC_ESINGULAR and "(chain 1)" in msg
    assert assert_stopped(kind, CC.STOP_EARLY_T0, out, w, clean, wclean) == 0
    assert (idx[1] == -1).all() and np.isnan(ts[1]).all() and np.array_equal(idx[2], iclean[2])
    # the Python surface raises, and the context then gives the clean result bit for bit
    kw = dict(burn=burn, u_nu=case["u"], nu_path=case["paths"], nu_grid=case["grid"], nu_weight=case["weight"],
              nu_init=case["init"], want_tstat=True)
    with pytest.raises(np.linalg.LinAlgError, match=r"\(chain 1\)"):
        ctx.robust_run(None, CC.CHAINS, iters, xi=xi, g=g, gl=gl, **kw)
    again = ctx.robust_run(None, CC.CHAINS, iters, xi=case["xi"], g=case["g"], gl=case["gl"], **kw)
    for a, b in zip(again[:4], (clean, wclean, iclean, tclean)):
        assert np.array_equal(a, b)


# ---- E: grid sizes and degenerate weights -----------------------------------------------------------
@pytest.mark.parametrize("name", [f"E-G{G}" for G in CC.GRID_SIZES] + ["E-zero", "E-edges", "E-nonfinite"])
def test_grid_sizes_and_degenerate_weights(ctx, name):
    case, ref = CC.nu_case(name), CC.nu_reference(name)
    out, w, idx, ts, _ = run_nu_case(ctx, name)
    for c in range(CC.CHAINS):
        assert_nu(f"{name} chain {c}", name, case["n"], out[c], w[c], ts[c], idx[c], ref[c])
    assert idx.min() >= 0 and (case["weight"][idx] > 0).all()          # never a value of weight zero
    if name == "E-edges":
        lo, hi = (t - case["burn"] for t in CC.EDGE_SWEEPS)
        assert idx[0, lo] == 0 and idx[0, hi] == len(case["grid"]) - 1
    if name == "E-nonfinite":
        c, row = CC.NONFINITE_CHAIN, CC.NONFINITE_SWEEP - case["burn"]
        assert ts[c, row] == -np.inf and idx[c, row] == case["paths"][c, CC.NONFINITE_SWEEP - 1]
        assert np.isfinite(np.delete(ts[c], row)).all() and np.isfinite(out).all() and np.isfinite(w).all()


# ---- F: device RNG below shape 1 --------------------------------------------------------------------
def test_device_rng_below_shape_one(ctx):
    y, X, prior = CC.low_problem()
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    out, w, _ = ctx.robust_run(CC.LOW_NU, len(CC.LOW_SEEDS), CC.LOW_T, seeds=list(CC.LOW_SEEDS))
    for c, (ref, wref, _) in enumerate(CC.low_reference()):
        assert_pair(f"device RNG nu = 0.5 chain {c}", "F-fixed", out[c], w[c], ref, wref)


def test_device_rng_on_a_grid_that_starts_below_shape_one(ctx):
    y, X, prior = CC.low_problem()
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    out, w, idx, ts, _ = ctx.robust_run(None, len(CC.LOW_NU_SEEDS), CC.LOW_T, seeds=list(CC.LOW_NU_SEEDS),
                                        nu_grid=CC.LOW_GRID, nu_weight=CC.LOW_WEIGHT, nu_init=CC.LOW_INIT,
                                        want_tstat=True)
    for c, (ref, _) in enumerate(CC.low_nu_reference()):
        assert np.array_equal(idx[c], ref["idx"]), f"chain {c}: the index path left the reference's"
        assert_nu(f"device RNG grid chain {c}", "F-nu", CC.LOW_N, out[c], w[c], ts[c], idx[c], ref)
