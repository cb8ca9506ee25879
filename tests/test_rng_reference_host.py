"""tests/rng_reference.py checked on the CPU, so that the GPU tests (tests/test_rng_streams_gpu.py)
never compare a kernel with a wrong oracle: Philox known answers through the vectorised function,
the long-double normals against the CPU build of pybmc_amd/csrc/bmc_math.h (g++, the way
tests/test_host_math.py builds), the reference's own distributions, and the two conditions the GPU
comparison of the gamma stream rests on -- the rejection path is exercised, and no element of the
chosen cases sits within 1e-9 of an accept / reject boundary (so none may be left out there)."""
import functools

import numpy as np
from scipy import stats

import rng_host_build as H
import rng_reference as R

U52 = 2.0 ** -52


def test_philox_known_answers_vectorised():
    # Random123 kat_vectors, philox4x32-10 -- all three in one call, and one at a time
    F = 0xFFFFFFFF
    ctr = [[0, 0, 0, 0], [F, F, F, F], [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]]
    key = [[0, 0], [F, F], [0xa4093822, 0x299f31d0]]
    want = np.array([[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8],
                     [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd],
                     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]], dtype=np.uint32)
    assert np.array_equal(R.philox4x32_10(ctr, key), want)
    for c, k, w in zip(ctr, key, want):
        assert np.array_equal(R.philox4x32_10(c, k), w)
    # a key shared by many counters, counters of another shape
    many = R.philox4x32_10(np.tile(np.array(ctr[2]), (5, 3, 1)), key[2])
    assert many.shape == (5, 3, 4) and (many == want[2]).all()
    # stream_words: the counter is (index lo, index hi, stream, sub), the key (seed lo, seed hi)
    got = R.stream_words(0x299f31d0a4093822, np.array([0x85a308d3243f6a88], dtype=np.uint64),
                         0x13198a2e, 0x03707344)
    assert np.array_equal(got[0], want[2])


def test_u53_keeps_53_bits_and_excludes_zero():
    F = 0xFFFFFFFF
    assert R.u53_open0(0, 0) == 2.0 ** -53 and R.u53_open0(F, F) == 1.0
    assert R.u53_open0(0, 1 << 11) == 2 * 2.0 ** -53        # the lowest bit that is kept
    assert R.u53_open0(0, (1 << 11) - 1) == 2.0 ** -53      # the 11 bits that are dropped
    assert R.u53_open0(1, 0) == (2 ** 21 + 1) * 2.0 ** -53
    u = R.uniforms(3, 100_001)
    assert u.shape == (100_001,) and u.min() > 0 and u.max() <= 1
    assert np.any((u * 2.0 ** 53) % 2 ** 21 != 0)            # bits below the high word are alive
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * len(u))
    assert stats.kstest(u, "uniform").pvalue > 1e-4


def test_stream_constants_are_distinct():
    ids = {R.STREAM_NORMAL, R.STREAM_GAMMA, R.STREAM_PRED_NORMAL, R.STREAM_UNIFORM}
    assert len(ids) == 4 and all(0 < s < 2 ** 32 for s in ids)
    # and so are the streams: same seed, same index, four different outputs
    w = [R.stream_words(9, np.arange(4, dtype=np.uint64), s) for s in sorted(ids)]
    for i in range(4):
        for j in range(i):
            assert not np.any(w[i] == w[j])


def test_normals_against_the_cpu_build():
    """2 10^6 elements: the long-double reference and bmc::box_muller_pair compiled by g++ differ
    by at most 2.5 units of 2^-52 |z| (0.5 log (1.01 ulp) + sqrt 0.5 + sincos 2.01 + product 0.5,
    rounded; observed 1.98, and 1.37 in units of 2^-52 rad)."""
    n = 2_000_000
    z, rad = R.normals(12345, n, return_rad=True)
    zc = H.normals(12345, n)
    assert z.dtype == R.LD and zc.dtype == np.float64 and zc.shape == (n,)
    d = np.abs(zc.astype(R.LD) - z)
    worst_z = float((d / np.abs(z)).max()) / U52
    worst_rad = float((d / rad).max()) / U52
    print(f"CPU build vs long double: {worst_z:.3f} units of 2^-52 |z|, {worst_rad:.3f} of 2^-52 rad")
    assert worst_z <= 2.5
    # prefix-stable, odd tail, and a function of the seed
    assert np.array_equal(R.normals(12345, 1001), z[:1001])
    assert np.array_equal(H.normals(12345, 1001), zc[:1001])
    assert not np.any(R.normals(12346, 1000) == z[:1000])


def test_reference_normals_are_standard_normal():
    z = R.normals(12345, 2_000_001).astype(np.float64)
    assert abs(z.mean()) < 5 / np.sqrt(len(z))
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / len(z))
    assert abs(stats.skew(z)) < 0.01 and abs(stats.kurtosis(z)) < 0.02
    assert stats.kstest(z[:200000], "norm").pvalue > 1e-4
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5 / np.sqrt(len(z))


@functools.lru_cache(maxsize=None)
def gamma_case(shape):
    return R.gammas(R.GAMMA_SEED, shape, R.GAMMA_N)


def test_reference_gammas_are_gamma():
    for shape in R.GAMMA_SHAPES:
        g, attempts, _ = gamma_case(shape)
        n = len(g)
        assert g.shape == (R.GAMMA_N,) and np.all(g > 0) and np.isfinite(g).all()
        assert abs(g.mean() - shape) < 5 * np.sqrt(shape / n), shape
        assert abs(g.var() / shape - 1) < 0.02, shape
        assert stats.kstest(g[:100000], "gamma", args=(shape,)).pvalue > 1e-4, shape
        assert attempts.max() < 64
    # prefix-stable
    g, a, m = gamma_case(2.5)
    g2, a2, m2 = R.gammas(R.GAMMA_SEED, 2.5, 5000)
    assert np.array_equal(g2, g[:5000]) and np.array_equal(a2, a[:5000]) and np.array_equal(m2, m[:5000])


def test_gamma_cases_exercise_the_rejection_path():
    """First-attempt reject share at seed 12345: 2.7 % at shape 0.5, 1.4 % at 2.5, 0.03 % at 75.5,
    0 at 100000.5 -- the small shapes carry the retry path, the large ones the no-reject path."""
    two = three = 0
    for shape in R.GAMMA_SHAPES:
        attempts = gamma_case(shape)[1]
        two += int((attempts >= 2).sum())
        three += int((attempts >= 3).sum())
        print(f"shape {shape}: reject share {(attempts >= 2).mean():.5f}, max attempts {attempts.max()}")
    assert two >= 1000 and three >= 10, (two, three)
    assert (gamma_case(100000.5)[1] == 1).all()
    share = (gamma_case(0.5)[1] >= 2).mean()
    assert 0.02 < share < 0.035


def test_gamma_cases_have_no_element_near_a_decision_boundary():
    """An element whose decision margin is below 1e-9 could take the other branch on the device
    (its x differs by a couple of ulp) and would have to be left out of the GPU comparison.  The
    cap on such elements is zero: the chosen seed and shapes have none (smallest margin 2e-7)."""
    for shape in R.GAMMA_SHAPES:
        margin = gamma_case(shape)[2]
        assert np.isfinite(margin).all()
        print(f"shape {shape}: smallest decision margin {margin.min():.3e}")
        assert int((margin < R.MARGIN_FLOOR).sum()) == 0, shape


def test_predict_noise_formula_uses_every_counter_half_once():
    for S, M in [(64, 1), (1000, 65), (37, 13), (10, 8)]:
        e, half = R.predict_noise_index(S, M)
        assert e.shape == (S, M) and half.shape == (M,)
        slot = 2 * e.astype(np.int64) + half[None, :]
        assert len(np.unique(slot)) == S * M                      # no two entries share a variate
        p = np.arange(M)
        assert np.array_equal(half, (p // 4) % 2)
        assert np.array_equal(e[0].astype(np.int64), (p - 4 * half) * S)
        assert np.array_equal((e - e[0]).astype(np.int64), np.tile(np.arange(S)[:, None], (1, M)))
    z = R.predict_noise(5, 300, 13)
    zc = H.predict_noise(5, 300, 13)
    assert z.shape == zc.shape == (300, 13)
    assert float((np.abs(zc - z) / np.abs(z)).max()) <= 2.5 * U52
    assert len(np.unique(zc)) == zc.size
    # point p + 4 holds the sine half of point p's pairs: z_p^2 + z_{p+4}^2 = -2 log u1
    u1, _, _ = R.predict_noise_uniforms(5, 300, 13)
    assert np.allclose((z[:, 0] ** 2 + z[:, 4] ** 2).astype(float), -2 * np.log(u1[:, 0]), rtol=1e-14)
    zf = z.astype(np.float64)
    assert stats.kstest(zf.ravel(), "norm").pvalue > 1e-4
