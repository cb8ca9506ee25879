"""Every reachable loop-kernel instantiation against the oracle (-m gpu).

tests/kernel_census.txt gives, per compiled loop kernel, the cheapest recipe (shape, chain count,
tuning) whose plan launches it on a 256-CU MI355X in SPX mode.  Each recipe is run in replay mode
and compared with the CPU oracle; Context.last_kernels() must name the recipe's kernel and equal
the CPU planner's prediction launch by launch.  Data: columns of unequal scale, X far from
orthonormal, an outlier in the last row (census_common.py).  Every chain slot that is first, last
or in the middle of a launch or a bundle replays a different stream and is compared with its OWN
oracle chain.

Bars.  f64 storage: |out - ref|.max() < 1e-9 max(1, |ref|.max()) (the project's replay bar).  f32
storage: 1e-5 relative on posterior_summary (test_t2_float32_storage's bar) and, on the chain
itself, ten times the largest move of the oracle chain over the f32 problems when its residual is
computed from X W rounded to f32 (capped at 1e-5): derived on the CPU from the oracle alone.
Simplex: chain within 1e-9 max(1, |ref|.max()), acceptance count and uniforms consumed equal
(test_replay_matches_the_reference); stream seeds are searched on the CPU for a smallest
accept/reject margin >= 1e-6 (f32 storage rounds X and y only, so the same margin holds).
Sensitivity, per problem, on the CPU: the oracle with the last row dropped from the residual, with
the last column zero in it, or with another chain's gamma stream moves by >= 100 bars."""
import numpy as np
import pytest

import census_common as cc
from gpu_common import gpu_ctx
from oracle import bmc_oracle as O
from pybmc_amd.chains import posterior_summary

pytestmark = pytest.mark.gpu

TABLE = cc.read_table()
RECIPES = sorted(((name, r) for name, r in TABLE if r is not None), key=lambda nr: (cc.problem_key(nr[1]), nr[0]))
REACHABLE = {name for name, _ in RECIPES}
FAMILY_FIRST = {}           # the first recipe of every kernel family also runs T = 1 and T = 64
for _name, _r in RECIPES:
    FAMILY_FIRST.setdefault(_name.split("<")[0], _name)
SEEN = set()                # union of last_kernels() over the recipes that ran
WORST = {}                  # (family, storage) -> (error relative to max(1, |ref|.max()), kernel)
_problem = {}               # the current problem's data and oracle chains (one at a time)


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return cc.replan(cc.build_planner(tmp_path_factory.mktemp("planner")))


@pytest.fixture(scope="module")
def f32_chain_bar():
    """Ten times the largest oracle-chain move over the f32 Gibbs problems (see the docstring)."""
    worst = 0.0
    for key in sorted({cc.problem_key(r) for _, r in RECIPES if r["sampler"] == "gibbs" and r["f32"]}):
        y, X, prior = cc.gibbs_problem(key[1], key[2], 1)
        worst = max(worst, cc.f32_rotation_error(y, X, prior, *cc.gibbs_streams(y, X, prior, 1)[0]))
    bar = min(10.0 * worst, cc.F32_CHAIN_CAP)
    print(f"f32 chain bar {bar:.3e} (largest oracle move {worst:.3e})")
    return bar


def gibbs_case(r, bar):
    """Data, oracle chains (made once per problem) and the sensitivity check of a Gibbs problem."""
    key = cc.problem_key(r)
    if _problem.get("key") != key:
        _problem.clear()
        y, X, prior = cc.gibbs_problem(r["n"], r["k"], r["f32"])
        most = max(q["chains"] for _, q in RECIPES if cc.problem_key(q) == key)
        streams = cc.gibbs_streams(y, X, prior, cc.N_STREAMS if most > 2 else most)
        chains = [cc.gibbs_chain(y, X, prior, Z, G) for Z, G in streams]
        for what, d in cc.gibbs_sensitivity(y, X, prior, streams, chains[0][0]).items():
            assert d >= 100 * bar, (key, what, d, bar)
        _problem.update(key=key, y=y, X=X, prior=prior, streams=streams, chains=chains, xi=None)
    return _problem


def record(name, f32, err):
    k = (name.split("<")[0], "f32" if f32 else "f64")
    if err > WORST.get(k, (-1.0, ""))[0]:
        WORST[k] = (err, name)


def check_kernels(ctx, name, plan):
    """last_kernels() names the recipe's kernel and is the CPU plan (with the recipe's pack answer,
    or the other one where the device decides), launch by launch.  Returns the launches."""
    got = ctx.last_kernels()
    assert name in got, (name, got)
    for launches in plan:
        if got == [l[0] for l in launches]:
            return launches
    raise AssertionError((name, got, plan))


@pytest.mark.parametrize("name,r", [nr for nr in RECIPES if nr[1]["sampler"] == "gibbs"],
                         ids=[n for n, r in RECIPES if r["sampler"] == "gibbs"])
def test_gibbs_recipe(name, r, plans, f32_chain_bar):
    bar = f32_chain_bar if r["f32"] else cc.F64_BAR
    p = gibbs_case(r, bar)
    y, X, prior, k = p["y"], p["X"], p["prior"], r["k"]
    ctx = gpu_ctx()
    ctx.set_tuning(r["G"], r["W"], r["res"], r["ppw"], 0, r["cpp"], 0, r["cu"])
    try:
        ctx.set_problem(y, X, dtype=np.float32 if r["f32"] else np.float64)
        ctx.set_prior(*prior)
        if p["xi"] is None:   # (the basis belongs to the problem and the prior, not to the tuning)
            W, lam, _ = ctx.basis()
            st = O.chain_setup(y, X, prior)
            p["xi"] = [O.innovations_in_basis(st, y, X, ref, W, lam, trace) for ref, trace in p["chains"]]
        nc = r["chains"]
        # the slot colouring needs the launches: those of the plan the device is expected to take
        colour = cc.colour_slots(plans[name][0], len(p["chains"]), plans[name][1])
        for T in ((1, 64, cc.T_GIBBS) if FAMILY_FIRST[name.split("<")[0]] == name else (cc.T_GIBBS,)):
            xi = np.stack([p["xi"][colour[c]][:T] for c in range(nc)])
            g = np.stack([p["streams"][colour[c]][1][:T] for c in range(nc)])
            out, stats = ctx.gibbs_run(nc, T, xi=xi, g=g)
            launches = check_kernels(ctx, name, plans[name])
            cc.assert_separated(colour, launches)   # (launches and bundles of the plan the device took)
            SEEN.update(ctx.last_kernels())
            worst = 0.0
            for c in range(nc):
                ref = p["chains"][colour[c]][0][:T]
                err = np.abs(out[c] - ref).max() / max(1.0, np.abs(ref).max())
                worst = max(worst, err)
                assert err < bar, (name, T, "chain", c, "first bad row", int(np.argmax(np.abs(out[c] - ref).max(1) >= bar * max(1.0, np.abs(ref).max()))),
                                   "column", int(np.abs(out[c] - ref).max(0).argmax()), err, bar)
                if r["f32"] and T == cc.T_GIBBS:
                    a, b = posterior_summary(out[c]), posterior_summary(ref)
                    for key in b:
                        assert rel(a[key], b[key]) < cc.F32_SUMMARY_BAR, (name, c, key)
            record(name, r["f32"], worst)
            print(f"{name} T={T} chains={nc} max rel err {worst:.3e} (bar {bar:.1e})")
    finally:
        ctx.set_tuning()


@pytest.mark.parametrize("name,r", [nr for nr in RECIPES if nr[1]["sampler"] == "simplex"],
                         ids=[n for n, r in RECIPES if r["sampler"] == "simplex"])
def test_simplex_recipe(name, r, plans):
    key = cc.problem_key(r)
    if _problem.get("key") != key:
        _problem.clear()
        c = cc.simplex_case(r["n"], r["k"], r["f32"], r["ow"])
        tt = cc.BURN_SIMPLEX + cc.T_SIMPLEX
        assert 0 < c["acc_all"] < tt and c["margin"] >= cc.MARGIN
        assert c["seed"] == cc.SIMPLEX_SEED, (key, c["seed"], c["margin"])   # the recorded seed
        for what, d in cc.simplex_sensitivity(c).items():
            assert d >= 100 * cc.F64_BAR, (key, what, d)
        _problem.update(key=key, case=c)
    c = _problem["case"]
    ctx = gpu_ctx()
    ctx.set_tuning(r["G"], r["W"], r["res"], r["ppw"], 0, 0, 0, r["cu"])
    try:
        ctx.set_problem(c["y"], c["X"], dtype=np.float32 if r["f32"] else np.float64)
        out, accepted, used, _ = ctx.simplex_run(c["Vt_hat"], c["S_hat"], cc.T_SIMPLEX, 1.0, 0.02, cc.BURN_SIMPLEX,
                                                 c["stepsize"], xi=c["Z"], unif=c["U"], g=c["G"], return_stats=True)
        check_kernels(ctx, name, plans[name])
        SEEN.update(ctx.last_kernels())
        ref = c["chain"]
        err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
        record(name, r["f32"], err)
        print(f"{name} seed={c['seed']} stepsize={c['stepsize']} accepted {c['acc_all']} margin {c['margin']:.2e} "
              f"max rel err {err:.3e}")
        assert accepted == c["acc"] and used == c["used"], (name, accepted, c["acc"], used, c["used"])
        assert err < cc.F64_BAR, (name, "first bad row", int(np.argmax(np.abs(out - ref).max(1) >= cc.F64_BAR)), err)
    finally:
        ctx.set_tuning()


def test_every_reachable_kernel_ran():
    """No kernel of the table is left out: executed and compared, or unreached."""
    for k, (err, name) in sorted(WORST.items()):
        print(f"worst {k[0]} {k[1]}: {err:.3e} ({name})")
    print(f"executed {len(SEEN & REACHABLE)} of {len(REACHABLE)} reachable loop kernels")
    assert SEEN == REACHABLE, ("run the whole module: with -k or a subset of the recipes this check fails by design",
                               sorted(REACHABLE - SEEN), sorted(SEEN - REACHABLE))
