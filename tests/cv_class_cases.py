"""The case table of the cross-validation class tests (no GPU): one case per instantiation, tile
edge, chunk edge, staging flush and grid-stride trip of kernels_cv.hip that the shape of a public
call can select.  test_cv_classes_gpu.py runs every row on the device; test_cv_classes_host.py
holds the table against the host plan (bmc_cv_plan.h, bmc_cvpath_plan.h), so that a row cannot
leave, or a constant move, without the census noticing.  TEST INFRASTRUCTURE ONLY.

Data come from the generators the CV tests share (cv_reference.problem, cv_reference.unequal_folds).
Balanced labels are default_rng(n).permutation(arange(n) % F); labels of given fold sizes are
default_rng(n).permutation(repeat(arange(F), sizes)).

what a row reaches (DESIGN.md 4.8 carries the same table):
  width_15 .. width_63  every (tiles, KMAX) pair of cv_tiles / cv_kmax on both sides of its edge:
                 (1, 16) at 15, (2, 16) at 16, (2, 32) at 31, (3, 32) at 32, (3, 64) at 47, (4, 64)
                 at 48 and 63; cv_fold_gram_kernel<4> at 48 and 63; at 15, 31, 47 and 63 y is
                 column 15 of the last tile and no column of [A | y] is padding
  nt4_tight      the near-cancelling fit (rss 1e-10 of |y|^2) at 4 tiles / KMAX 64
  chunk_edges    folds of 1, 2, 3, 63, 64, 65, 511, 512, 513 rows: the Gram chunk (512) full, and
                 followed by one real and three zero rows; the rss chunk (64) likewise; row padding
                 of 3, 2, 1 and 0 rows
  loo            leave-one-out as exact CV: every fold one real row and three zero rows; T = 64
  max_folds      F = 1024: 2048 coefficient vectors in cv_block_rss_kernel (gridDim.y = 32), one
                 chain launch of exactly CV_MAX_CHAINS_PER_LAUNCH blocks, 1024 host-pool problems
  gather_wrap    n_pad * ldz = 2 160 000 elements: the second trip of cv_gather_kernel's loop
  unrotate_wrap  128 chains x 300 draws x 65 = 2 496 000 elements: the second trip of
                 cv_unrotate_kernel's loop; chains 108 .. 127 lie (partly) behind the wrap
  t_edges        the 64-row output staging of cv_chain: T = 63, 64, 65, 128, and T = 1 (with two
                 chains the two pooled draws bmc_kfold_cv asks for)
  path tile_fill      the path's own gather and Gram at 4 tiles; the exact-fill widths as leading
                 blocks of a wider Gram
  path split_classes  a launch boundary and a width-class boundary in one batch: 2100 chains per
                 class, launches 2048 + 52 in class 16, then 2048 + 52 in class 8
"""
import functools

import numpy as np

import cv_reference as CV

WIDTHS = (15, 16, 31, 32, 47, 48, 63)
EXACT_FILL = (15, 31, 47, 63)              # k + 1 is a whole number of 16-column tiles
CHUNK_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513)
T_EDGES = (1, 63, 64, 65, 128)
T_EDGE_CASE, T_EDGE_CHAINS = "unequal", 2  # cv_reference.CASES["unequal"]: 150 x 3, F = 5

# name: (n, k, folds: F (balanced) or the fold sizes, chains, T, snr, scale)
CASES = {f"width_{k}": (6 * k + 1, k, 3, 1, 65, 10.0, 1.0) for k in WIDTHS}
CASES.update({
    "nt4_tight": (180, 50, 3, 1, 300, 1e5, 1e3),
    "chunk_edges": (sum(CHUNK_SIZES), 5, CHUNK_SIZES, 1, 65, 10.0, 1.0),
    "loo": (130, 3, 130, 2, 64, 10.0, 1.0),
    "max_folds": (1024, 2, 1024, 2, 20, 10.0, 1.0),
    "gather_wrap": (27000, 64, 2, 1, 65, 10.0, 1.0),
    "unrotate_wrap": (400, 64, 2, 64, 300, 10.0, 1.0),
})

# global chains f * C + c held against gibbs_sampler where a case has more than 16
PICKS = {
    "loo": (0, 1, 128, 129, 258, 259),            # folds 0, 64, 129, both chains
    "max_folds": (0, 1023, 1024, 2047),
    "unrotate_wrap": (0, 107, 108, 127),          # 127: every draw behind the wrap
}

# name: (n, k, F (balanced) or "fold_labels", chains, T, components, global chains or None)
PATH_CASES = {
    "tile_fill": (380, 63, 2, 1, 65, WIDTHS, None),
    "split_classes": (200, 9, "fold_labels", 70, 20, (8, 9), (0, 2047, 2048, 2099, 2100, 4147, 4148, 4199)),
}
SPLIT_FOLDS = 30                                   # cv.fold_labels(200, 30, seed=1)


def balanced(n, F):
    return np.random.default_rng(n).permutation(np.arange(n) % F).astype(np.int64)


def sized(n, sizes):
    lab = np.repeat(np.arange(len(sizes)), sizes)
    assert len(lab) == n
    return np.random.default_rng(n).permutation(lab).astype(np.int64)


@functools.lru_cache(maxsize=None)
def labels(name):
    """The fold labels of a row of CASES (read-only)."""
    n, k, spec = CASES[name][:3]
    lab = balanced(n, spec) if isinstance(spec, int) else sized(n, spec)
    lab.setflags(write=False)
    return lab


def n_folds(name):
    spec = CASES[name][2]
    return spec if isinstance(spec, int) else len(spec)


def case(name):
    """(A, y, prior, folds, F, C, T) of a row of CASES."""
    n, k, spec, C, T, snr, scale = CASES[name]
    A, y, prior, _ = CV.problem(n, k, snr, scale)
    return A, y, prior, labels(name), n_folds(name), C, T


def t_edge_case():
    """(A, y, prior, folds, F, C) of the t_edges runs; T takes the values of T_EDGES."""
    A, y, prior, folds, F, _ = CV.case(T_EDGE_CASE)
    return A, y, prior, folds, F, T_EDGE_CHAINS


def path_labels(name):
    n, k, spec = PATH_CASES[name][:3]
    if spec == "fold_labels":
        from pybmc_amd import cv
        return cv.fold_labels(n, SPLIT_FOLDS, seed=1)
    return balanced(n, spec)


def path_case(name):
    """(A, y, prior, folds, C, T, components, picks) of a row of PATH_CASES."""
    n, k, spec, C, T, comps, picks = PATH_CASES[name]
    A, y, prior, _ = CV.problem(n, k, 10.0)
    return A, y, prior, path_labels(name), C, T, comps, picks


def rows_behind(folds, F, k, element):
    """The source rows whose gathered row [A | y | 0-pad] has an element at or behind ``element`` of
    the gathered matrix: the layout of cv_segments restated (folds in order, each padded to a
    multiple of 4 rows, ldz = k + 1 rounded up to 16)."""
    ldz = (k + 1 + 15) // 16 * 16
    out, at = [], 0
    for f in range(F):
        src = np.flatnonzero(folds == f)
        pos = at + np.arange(len(src))
        out.append(src[(pos + 1) * ldz > element])
        at += (len(src) + 3) // 4 * 4
    return np.concatenate(out)
