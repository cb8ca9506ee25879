"""The library's four variate streams restated on the host.  TEST INFRASTRUCTURE ONLY.

numpy (vectorised uint64), numpy.longdouble (64-bit mantissa on x86-64) and nothing of the
kernels' text: Philox4x32-10 from the paper (Salmon, Moraes, Dror, Shaw, SC'11), Box-Muller and
Marsaglia & Tsang (2000) from their definitions, the counter layouts from DESIGN.md "Variate
streams".  Every stream is keyed by the 64-bit seed (key = (seed lo, seed hi)) and counter word 2
names the stream:

  normals(seed, n)[e]       half e & 1 of the Box-Muller pair of counter (e/2 lo, e/2 hi, NORMAL, 0)
  gammas(seed, a, n)[t]     attempt m of element t: counters (t lo, t hi, GAMMA, 2m) and (.., 2m+1)
  uniforms(seed, n)[i]      word pair i & 1 of counter (i/2 lo, i/2 hi, UNIFORM, 0)
  predict_noise(seed, S, M)[s, p]   half (p >> 2) & 1 of counter (e lo, e hi, PRED_NORMAL, 0),
                                    e = (p - 4 ((p >> 2) & 1)) S + s

The normal transforms are evaluated in long double and returned in long double, so that a
float64 implementation can be measured against them in units of 2^-52 |z|; callers round with
``.astype(np.float64)`` when they need variates to feed a replay run.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy.longdouble must carry a 64-bit mantissa"

STREAM_NORMAL = 0x4E4F524D        # "NORM"
STREAM_GAMMA = 0x47414D4D         # "GAMM"
STREAM_PRED_NORMAL = 0x50524544   # "PRED"
STREAM_UNIFORM = 0x554E4946       # "UNIF"

# The fill-kernel cases of tests/test_rng_streams_gpu.py.  tests/test_rng_reference_host.py proves on
# the CPU that none of their elements sits within 1e-9 of an accept / reject boundary, which is
# what lets the GPU test compare every element.
GAMMA_SEED = 12345
GAMMA_SHAPES = (0.5, 0.9, 1.0, 2.5, 315.0, 5000.5, 100000.5)
GAMMA_N = 600_001
MARGIN_FLOOR = 1e-9

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PI_2 = LD("1.5707963267948966192313216916397514421")


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) or (2,): unsigned 32-bit words.  Returns (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        kr0 = (k0 + np.uint64((r * _W0) & 0xFFFFFFFF)) & _LO
        kr1 = (k1 + np.uint64((r * _W1) & 0xFFFFFFFF)) & _LO
        p0, p1 = _M0 * c0, _M1 * c2                  # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ kr0, p1 & _LO, (p0 >> _S32) ^ c3 ^ kr1, p0 & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u53_open0(hi, lo):
    """The top 53 bits of (hi : lo) -> (0, 1]: (m + 1) 2^-53, exact in float64."""
    m = ((np.asarray(hi, dtype=np.uint64) << _S32) | np.asarray(lo, dtype=np.uint64)) >> np.uint64(11)
    return (m + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)


def stream_words(seed, index, stream, sub=0):
    """Philox output of counters (index lo, index hi, stream, sub) under key = seed."""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.empty(index.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = index & _LO
    ctr[..., 1] = index >> _S32
    ctr[..., 2] = stream
    ctr[..., 3] = sub
    return philox4x32_10(ctr, _key(seed))


def pair_uniforms(words):
    """(u1, u2) of a Box-Muller pair: u1 from words (x, y), u2 from (z, w)."""
    return u53_open0(words[..., 0], words[..., 1]), u53_open0(words[..., 2], words[..., 3])


def box_muller(u1, u2):
    """z0 = rad cos(2 pi u2), z1 = rad sin(2 pi u2), rad = sqrt(-2 log u1), in long double.
    4 u2 = q + r with q the nearest integer is exact in float64; sin / cos are taken of (pi/2) r,
    |r| <= 1/2, and moved to the quadrant q, so the result is accurate relative to z itself next
    to the zeros of sin and cos.  Also returns rad."""
    rad = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    t = 4.0 * u2
    q = np.rint(t)
    x = (t - q).astype(LD) * _PI_2
    s, c = np.sin(x), np.cos(x)
    iq = q.astype(np.int64) & 3
    odd = (iq & 1) == 1
    a, b = np.where(odd, c, s), np.where(odd, s, c)
    sn = np.where((iq & 2) != 0, -a, a)
    cs = np.where(((iq + 1) & 2) != 0, -b, b)
    return rad * cs, rad * sn, rad


def normal_pair_uniforms(seed, n, stream=STREAM_NORMAL):
    return pair_uniforms(stream_words(seed, np.arange((n + 1) // 2, dtype=np.uint64), stream))


def interleave(z0, z1, n):
    out = np.empty(2 * len(z0), dtype=z0.dtype)
    out[0::2], out[1::2] = z0, z1
    return out[:n]


def normals(seed, n, return_rad=False):
    """(n,) long double.  With return_rad also sqrt(-2 log u1) of each element's pair."""
    z0, z1, rad = box_muller(*normal_pair_uniforms(seed, n))
    z = interleave(z0, z1, n)
    return (z, interleave(rad, rad, n)) if return_rad else z


def uniforms(seed, n):
    w = stream_words(seed, np.arange((n + 1) // 2, dtype=np.uint64), STREAM_UNIFORM)
    return interleave(*pair_uniforms(w), n)


def gammas(seed, shape, n, max_attempts=64, detail=False):
    """Gamma(shape, 1) by Marsaglia & Tsang: d = a - 1/3, c = 1/sqrt(9 d) (float64, as a float64
    implementation computes them), x the first normal of the attempt's first counter, u the first
    uniform of its second; v = (1 + c x)^3 is rejected when 1 + c x <= 0, accepted when
    u < 1 - 0.0331 x^4 or log u < x^2/2 + d (1 - v + log v); the value is d v.  For shape < 1 the
    sampler runs at shape + 1 and the value is multiplied by U^(1/shape), U the SECOND uniform of
    the accepting attempt's second counter.

    Returns (values float64, attempts int64, margin float64): margin is, per element, the
    smallest distance of any test it went through from flipping -- |1 + c x|, |u - (1 - 0.0331 x^4)|
    and |log u - (x^2/2 + d (1 - v + log v))| over its attempts.  With detail also
    |c x / (1 + c x)| of the accepting attempt, a third of the factor by which a relative error
    of x enters v."""
    a = float(shape)
    boost = a < 1.0
    aa = a + 1.0 if boost else a
    d = np.float64(aa) - np.float64(1.0) / np.float64(3.0)
    c = np.float64(1.0) / np.sqrt(np.float64(9.0) * d)
    dl, cl = LD(d), LD(c)
    val = np.full(n, dl, dtype=LD)          # what 64 rejections in a row would leave
    attempts = np.full(n, max_attempts, dtype=np.int64)
    margin = np.full(n, np.inf)
    amplification = np.zeros(n)
    inv_a = LD(np.float64(1.0) / np.float64(a))      # the exponent as float64 arithmetic gives it
    todo = np.arange(n, dtype=np.uint64)
    for m in range(max_attempts):
        if len(todo) == 0:
            break
        x, _, _ = box_muller(*pair_uniforms(stream_words(seed, todo, STREAM_GAMMA, 2 * m)))
        w1 = stream_words(seed, todo, STREAM_GAMMA, 2 * m + 1)
        u, ub = pair_uniforms(w1)
        lin = LD(1) + cl * x
        mg = np.abs(lin)
        pos = lin > 0
        v = np.where(pos, lin, LD(1)) ** 3
        x2 = x * x
        squeeze = LD(1) - LD(0.0331) * x2 * x2
        rhs = LD(0.5) * x2 + dl * (LD(1) - v + np.log(v))
        ul = u.astype(LD)
        lu = np.log(ul)
        tests = np.minimum(np.abs(ul - squeeze), np.abs(lu - rhs))
        mg = np.where(pos, np.minimum(mg, tests), mg)
        idx = todo.astype(np.int64)
        margin[idx] = np.minimum(margin[idx], mg.astype(np.float64))
        ok = pos & ((ul < squeeze) | (lu < rhs))
        res = dl * v
        if boost:
            res = res * ub.astype(LD) ** inv_a
        val[idx[ok]] = res[ok]
        attempts[idx[ok]] = m + 1
        amplification[idx[ok]] = np.abs(cl * x / lin)[ok].astype(np.float64)
        todo = todo[~ok]
    out = (val.astype(np.float64), attempts, margin)
    return out + (amplification,) if detail else out


def predict_noise_index(n_draws, n_points):
    """(counter (S, M), half (M,)) of the standard normal added to draw s of point p: points come
    in groups of eight, p and p + 4 (p mod 8 < 4) share the pair of counter p S + s -- the cosine
    half goes to p, the sine half to p + 4."""
    p = np.arange(n_points, dtype=np.uint64)
    half = (p >> np.uint64(2)) & np.uint64(1)
    base = p - np.uint64(4) * half
    e = base[None, :] * np.uint64(n_draws) + np.arange(n_draws, dtype=np.uint64)[:, None]
    return e, half.astype(np.int64)


def predict_noise_uniforms(seed, n_draws, n_points):
    e, half = predict_noise_index(n_draws, n_points)
    u1, u2 = pair_uniforms(stream_words(seed, e, STREAM_PRED_NORMAL))
    return u1, u2, half


def predict_noise(seed, n_draws, n_points):
    """(n_draws, n_points) long double: the noise of a device-mode predictive run."""
    u1, u2, half = predict_noise_uniforms(seed, n_draws, n_points)
    z0, z1, _ = box_muller(u1, u2)
    return np.where(half[None, :] == 1, z1, z0)
