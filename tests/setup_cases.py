"""Shapes and inputs of the set-up kernel class tests (kernels_setup.hip: residual_rss, panelize,
centre -> rotate -> unpanelize), shared by the CPU tests that pin each shape's launch class and
check the references (test_setup_plan.py, test_setup_reference_host.py) and by the GPU tests that
run them (test_setup_classes_gpu.py).

Every shape is the smallest that reaches its class: the classes are decided by the panel count
(choose_vec, rss_groups_of in bmc_plan.h), not by the column count, so the problems are narrow and
the largest input is about 8 MB."""
import functools

import numpy as np

# residual_rss_kernel<T, VEC, NB>: (storage type, n, k) -> the class the shape must reach:
# rows per lane, panels, rows of the last panel, workgroups, ticket form, panels per wave slot
RSS_CASES = {
    # one row per lane, f64: one panel; 20 panels with a ragged last one; both flat tickets
    ("f64", 63, 2): dict(vec=1, np=1, last_rows=63, G=1, ticket="flat", trips=1),
    ("f64", 1237, 5): dict(vec=1, np=20, last_rows=21, G=5, ticket="flat", trips=1),
    # two-level ticket, sub-words of 18 and 17 arrivals
    ("f64", 70001, 3): dict(vec=1, np=1094, last_rows=49, G=274, ticket="two-level", trips=1),
    # the panel loop goes round twice: slots 0 and 1 of 4096 walk two panels
    ("f64", 262209, 2): dict(vec=1, np=4098, last_rows=1, G=1024, ticket="two-level", trips=2),
    # two rows per lane; G = 257 is the smallest two-level grid (17 arrivals at sub-word 0, 16 elsewhere)
    ("f64", 131073, 2): dict(vec=2, np=1025, last_rows=1, G=257, ticket="two-level", trips=1),
    # second trip at two rows per lane (slot 0 alone)
    ("f64", 524289, 2): dict(vec=2, np=4097, last_rows=1, G=1024, ticket="two-level", trips=2),
    ("f32", 1237, 5): dict(vec=1, np=20, last_rows=21, G=5, ticket="flat", trips=1),
    ("f32", 131073, 2): dict(vec=2, np=1025, last_rows=1, G=257, ticket="two-level", trips=1),
    # four rows per lane exists for f32 only
    ("f32", 524289, 3): dict(vec=4, np=2049, last_rows=1, G=513, ticket="two-level", trips=1),
}
RSS_BATCHES = (1, 2, 3, 4, 5, 8)     # vectors per call: NB = 1, 2, 4, 4, 8, 8 (b >= nb zero-padded)

# panelize_kernel<T> with a padded leading dimension: (storage type, n, k) -> rows per lane, panels
PANELIZE_CASES = {
    ("f32", 777, 6): dict(vec=1, np=13),
    ("f64", 131073, 2): dict(vec=2, np=1025),
    ("f32", 524289, 3): dict(vec=4, np=2049),
}

# bmc_orthogonalize: (n, n_models, components kept, ldf - n_models) -> rows per lane and panels of
# the (n x kept) problem, rotate's column groups per panel and the columns of its last wave
ORTHO_CASES = {
    (63, 3, 1, 0): dict(vec=1, np=1, ncg=1, last_wave_cols=1),
    (577, 10, 7, 0): dict(vec=1, np=10, ncg=1, last_wave_cols=7),
    (577, 10, 8, 0): dict(vec=1, np=10, ncg=1, last_wave_cols=8),
    (577, 10, 9, 0): dict(vec=1, np=10, ncg=1, last_wave_cols=1),
    (1000, 41, 31, 0): dict(vec=1, np=16, ncg=1, last_wave_cols=7),
    (1000, 41, 32, 0): dict(vec=1, np=16, ncg=1, last_wave_cols=8),
    (1000, 41, 33, 0): dict(vec=1, np=16, ncg=2, last_wave_cols=1),
    (1000, 41, 40, 0): dict(vec=1, np=16, ncg=2, last_wave_cols=8),
    (131073, 5, 3, 0): dict(vec=2, np=1025, ncg=1, last_wave_cols=3),
    (577, 10, 7, 3): dict(vec=1, np=10, ncg=1, last_wave_cols=7),
}


def np_dtype(name):
    return {"f64": np.float64, "f32": np.float32}[name]


def case_id(key):
    return "-".join(str(v) for v in key)


@functools.lru_cache(maxsize=None)
def rss_inputs(dt, n, k):
    """(y, X, B) in the storage type (B float64, 8 x k): entries O(1), B = 0.1 x standard normals.
    The arrays are shared between tests: read-only."""
    rng = np.random.Generator(np.random.PCG64([n, k, dt == "f32"]))
    X = rng.standard_normal((n, k)).astype(np_dtype(dt))
    y = (X.astype(np.float64) @ (0.3 * rng.standard_normal(k)) + rng.standard_normal(n)).astype(np_dtype(dt))
    B = 0.1 * rng.standard_normal((8, k))
    for a in (y, X, B):
        a.setflags(write=False)
    return y, X, B


@functools.lru_cache(maxsize=None)
def ortho_inputs(n, km):
    """(F, truth): standard normals plus a per-row common shift, as test_orthogonalize_gpu.py's
    test_large_sizes.  Read-only."""
    rng = np.random.Generator(np.random.PCG64([n, km]))
    F = rng.standard_normal((n, km)) + rng.standard_normal(n)[:, None] * 3
    truth = F.mean(1) + rng.standard_normal(n)
    F.setflags(write=False)
    truth.setflags(write=False)
    return F, truth


@functools.lru_cache(maxsize=None)
def rss_reference(dt, n, k):
    """rss_ref of the case's 8 vectors and of b = 0 (index 8): (values (9,), bounds (9,)), computed
    once; the chain length comes from the case's pinned class."""
    import setup_reference as R
    y, X, B = rss_inputs(dt, n, k)
    c = (RSS_CASES.get((dt, n, k)) or PANELIZE_CASES[(dt, n, k)])
    m = R.rss_chain_length(c["vec"], c.get("trips", 1))
    return R.rss_ref(y, X, np.vstack([B, np.zeros((1, k))]), m)


def diagonal_prior(k):
    """A simple diagonal prior (b0, C0, nu0, sigma20)."""
    return np.zeros(k), np.diag(10.0 + np.arange(k)), 1.0, 0.5
