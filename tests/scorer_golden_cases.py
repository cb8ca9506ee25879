"""The calls whose bits tests/test_scorer_golden_gpu.py holds and scripts/record_scorer_golden.py
records: everything that runs the Pareto tail fit (bmc_psis.h), the staging kernels (pad_points,
pad_rows) or the key gather, through the C ABI of a context.  The inputs are the seeded cases of the
reference modules and of the GPU tests of each family; nothing here computes a reference.

FAMILIES   name -> function(ctx) -> {case: {key: array}}
A family's arrays go to tests/golden/scorers/<family>.<i>.npz, as many files as keep each below
64 KB (split_files); an array is stored as its uint64 bit pattern, so that a NaN is held too."""
import glob
import os

import numpy as np

import ppc_reference as PP
import psis_reference as P
import score_reference as R
import tscore_reference as TR

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scorers")
FILE_BYTES = 64 * 1024
ROW, COL = 0, 1     # BMC_ROW_MAJOR, BMC_COL_MAJOR


def strided(A, th, col_major, pad_a, pad_t):
    """A in the layout asked for with lda wider than its rows by pad_a, theta with ldt wider by
    pad_t, the slack NaN: (A buffer, lda, layout, theta buffer, ldt)"""
    n, k = A.shape
    if col_major:
        buf = np.full((k, n + pad_a), np.nan)
        buf[:, :n] = A.T
    else:
        buf = np.full((n, k + pad_a), np.nan)
        buf[:, :k] = A
    tb = np.full((th.shape[0], k + 1 + pad_t), np.nan)
    tb[:, :k + 1] = th
    return buf, buf.shape[1], COL if col_major else ROW, tb, tb.shape[1]


def call(fn, A, y, th, col_major=False, pad_a=0, pad_t=0, extra=()):
    """One scoring entry point of a context on (A, y, theta)"""
    buf, lda, layout, tb, ldt = strided(A, th, col_major, pad_a, pad_t)
    return fn(buf, A.shape[0], A.shape[1], lda, layout, np.ascontiguousarray(y), tb, th.shape[0], ldt, *extra)


# n on both sides of the 64-point tile; S below and at the M >= 5 rule, and the one size at which
# the radix select runs
SHAPE_N = (63, 64, 65)
SHAPE_S = (24, 25, 4097)


def shape_runs(fn, k):
    """The cases of P.shape_cases(k) at SHAPE_N x SHAPE_S, laid out as
    test_shapes_on_both_sides_of_every_rule lays them out (layout and slack by the case number)"""
    out = {}
    for case, n, S, (A, y, th) in P.shape_cases(k):
        if n in SHAPE_N and S in SHAPE_S:
            out[f"k{k}_n{n}_S{S}"] = call(fn, A, y, th, case % 2 == 1, (case % 3) * 2, (case % 2) * 3)
    return out


def ties_case():
    """test_a_run_of_ties_across_the_cutoff of test_psis_gpu.py and test_loo_predict_gpu.py"""
    A, y, th = R.random_case(200, 5, 9000, 77)
    rep = th[0].copy()
    rep[:5] += 0.5
    t2 = th.copy()
    t2[np.random.default_rng(3).permutation(9000)[:4500]] = rep
    return A, y, t2


def psis_loo(ctx):
    out = {}
    for k in (4, 16, 17):
        out.update(shape_runs(ctx.psis_loo, k))
    A, y, th = R.random_case(300, 7, 2, 5)
    out["identical_draws"] = call(ctx.psis_loo, A, y, np.repeat(th[:1], 6001, axis=0))
    out["ties"] = call(ctx.psis_loo, *ties_case())
    A, y, th = R.random_case(200, 5, 7000, 9)
    A = A.copy()
    A[17, 2] = np.nan
    out["nan_point"] = call(ctx.psis_loo, A, y, th)
    return out


def psis_loo_student(ctx):
    A, y, th = TR.shape_case(5, 65, 513)
    index = (np.arange(513) % len(TR.NUS)).astype(np.int32)
    return {"t": call(ctx.psis_loo_t, A, y, th, extra=(TR.NUS[1],)),
            "tv": call(ctx.psis_loo_tv, A, y, th, extra=(TR.NUS, index))}


def psis_loo_predict(ctx):
    import loo_predict_reference as L
    out = {}
    for k in (3, 33):
        out.update(shape_runs(ctx.psis_loo_predict, k))
    out["mirror"] = call(ctx.psis_loo_predict, *L.mirror_case())
    out["ties"] = call(ctx.psis_loo_predict, *ties_case())
    return out


def pointwise_loglik(ctx):
    out = {}
    for n in (63, 65):
        for k in (1, 17):
            A, y, th = R.random_case(n, k, 65, 900 + 10 * k + n)
            out[f"n{n}_k{k}"] = call(ctx.pointwise_loglik, A, y, th, True, 5, 2)
    return out


def ppc(ctx):
    """Points across the 64-point tile, k at and past the 16-column slab (PP.grid_shapes), with and
    without an offset, both layouts, lda and ldt wider than the rows"""
    out = {}
    for k in (16, 17):
        for _, n, S, data_seed in PP.grid_shapes(k):
            if n not in (63, 64, 65) or S != 65:
                continue
            A, y, th = PP.make_case(n, k, S, data_seed)
            off = 1.0 + 0.5 * np.random.default_rng(data_seed + 7).standard_normal(n)
            for given in (False, True):
                for col_major in (False, True):
                    buf, lda, layout, tb, ldt = strided(A, th, col_major, 2 if col_major else 4, 3)
                    out[f"k{k}_n{n}_off{int(given)}_col{int(col_major)}"] = ctx.ppc(
                        buf, n, k, lda, layout, np.ascontiguousarray(y), tb, S, ldt,
                        off if given else None, PP.grid_noise_seed(data_seed), 0.0)
    return out


def _sens(ctx, A, y, theta, prior, Vt, alphas, mask, cols_per_batch=0):
    r = ctx.power_sensitivity(np.ascontiguousarray(A), A.shape[0], A.shape[1], A.shape[1], ROW,
                              np.ascontiguousarray(y), np.ascontiguousarray(theta), theta.shape[0],
                              theta.shape[1], prior, Vt, alphas, mask, cols_per_batch, True)
    out = {key: r[key] for key in ("pareto_k", "mean", "sd", "cjs")}
    out["flags"] = np.concatenate([r["component_flags"], r["column_flags"]]).astype(np.float64)
    for j, row in enumerate(r["logdens"]):
        out[f"logdens{j}"] = row
    for w in range(r["weights"].shape[1]):
        out[f"weights{w}"] = np.ascontiguousarray(r["weights"][:, w])
    return out


def sensitivity(ctx):
    """S = 24 and 25 (either side of the M >= 5 rule; even and odd: the pad key), alpha below and
    above 1, every component; the tied chain with its constant column (S = 3001) at two batch sizes"""
    import test_sensitivity_gpu as TS
    out = {}
    for name in ("S24_no_fit", "S25_first_fit", "all_components"):
        A, y, _, pooled, prior, Vt, _, _, _ = TS._make(name)
        out[name] = _sens(ctx, A, y, pooled, prior, Vt, (0.99, 1.01, 0.8, 1.25), 15)
    A, y, theta, prior, Vt = TS._tied_case()
    for cpb in (0, 1):
        out[f"tied_batch{cpb}"] = _sens(ctx, A, y, theta, prior, Vt, (0.5, 2.0), 3, cpb)
    assert all(np.array_equal(v, out["tied_batch1"][key], equal_nan=True) for key, v in out["tied_batch0"].items())
    del out["tied_batch1"]     # the same bits (asserted here, in every run): held once
    out["tied"] = out.pop("tied_batch0")
    return out


def rank(ctx):
    """S = 2 * 2 * 350 = 1400 split draws, no multiple of the 1024-key gather tile: z raw and folded,
    the diagnostics; and the same chains with an infinity in one column"""
    import diag_reference as D
    x = np.ascontiguousarray(D.ar1(np.random.default_rng(3), 2, 701, 3, 0.5))
    bad = x.copy()
    bad[1, 400, 1] = np.inf
    out = {}
    for tag, v in (("ar1", x), ("inf_column", bad)):
        out[tag] = {"z": ctx.rank_normalize(v, 2, 701, 3, 3, 0, False),
                    "z_folded": ctx.rank_normalize(v, 2, 701, 3, 3, 0, True)}
        out[tag].update(ctx.rank_diagnostics(v, 2, 701, 3, 3))
    return out


FAMILIES = {"psis_loo": psis_loo, "psis_loo_student": psis_loo_student, "psis_loo_predict": psis_loo_predict,
            "pointwise_loglik": pointwise_loglik, "ppc": ppc, "sensitivity": sensitivity, "rank": rank}


def flatten(cases):
    """{case: {key: array}} -> {"case/key": uint64 bit pattern, shape kept}"""
    return {f"{case}/{key}": np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
            for case, arrays in cases.items() for key, v in arrays.items()}


def split_files(flat):
    """The arrays in order, a new file whenever the next one would take it past FILE_BYTES
    (2 KB kept for the archive's own records, 512 bytes per array for its header)"""
    files, size = [{}], 0
    for name, v in flat.items():
        need = v.nbytes + 512
        assert need <= FILE_BYTES - 2048, name
        if size + need > FILE_BYTES - 2048:
            files.append({})
            size = 0
        files[-1][name] = v
        size += need
    return files


def golden_files(family):
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, family + ".*.npz")))
