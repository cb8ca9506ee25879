"""Plain numpy longdouble references of the set-up kernels (kernels_setup.hip), each with a running
error bound computed beside the value: a bound on |kernel - exact| for ANY correct float64
evaluation in the kernel's order, from the standard model fl(a op b) = (a op b)(1 + d), |d| <= u
(fma: one rounding), gamma_q = q u / (1 - q u), u = 2^-53.  (numpy adds longdouble arrays pairwise,
so the references' own error is a few 2^-64 relative: three orders below the bounds.)

rss_ref    residual_rss_kernel: rss_b = sum_i (y_i - x_i . b)^2
ortho_ref  centre_kernel -> rotate_kernel -> unpanelize_kernel of bmc_orthogonalize, from the
           device's returned Vt and S, so that the eigen-solver's freedom drops out"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53


def gamma(q):
    q = LD(q)
    return q * U / (1 - q * U)


def rss_chain_length(vec, trips):
    """Length of residual_rss_kernel's longest addition chain behind one output: a lane's fma chain
    over its vec rows of each of the trips panels its wave slot walks, the wave sum (6 levels), the
    workgroup's 4 waves (3), the last workgroup's lane sum over up to 16 partials, its wave sum (6)."""
    return vec * trips + 6 + 3 + 16 + 6


def rss_ref(y, X, B, m):
    """y (n,), X (n, k): values of the storage type (any float dtype, widened here); B (nb, k)
    float64; m = rss_chain_length of the shape.  Returns (rss (nb,), bound (nb,)) as longdouble:
    r_i is k fmas from y_i, so |r_i computed - r_i| <= e_i = gamma_k (|y_i| + sum_j |x_ij b_j|);
    then sum_i (2 |r_i| e_i + e_i^2) for the squares of perturbed residuals and gamma_m sum_i r_i^2
    for the summation."""
    yl, Xl = np.asarray(y).astype(LD), np.asarray(X).astype(LD)
    Bl = np.atleast_2d(np.asarray(B, dtype=np.float64)).astype(LD)
    k = Xl.shape[1]
    Xa = np.abs(Xl)
    val, bound = np.empty(len(Bl), LD), np.empty(len(Bl), LD)
    for i, b in enumerate(Bl):
        r = yl - Xl @ b
        e = gamma(k) * (np.abs(yl) + Xa @ np.abs(b))
        rr = np.sum(r * r)
        val[i] = rr
        bound[i] = np.sum(2 * np.abs(r) * e + e * e) + gamma(m) * rr
    return val, bound


def ortho_ref(F, truth, Vt, S):
    """F (n, km), truth (n,) float64; Vt (k, km), S (k,) as bmc_orthogonalize returned them.
    Returns a dict of longdouble arrays: mu, yc, Fc, U = Fc W with W[i, q] = fl64(Vt[q, i] / S[q])
    (the host's own division), and the bounds dmu, dyc, dU:
      mu  km - 1 additions and a division:                  gamma_{km+1} mean_j |F_ij|
      yc  fl(truth - mu computed):                          u |yc_i| + dmu_i
      U   km fmas over Fc computed = fl(F - mu computed):   gamma_km sum_j |Fc_ij W_jq|
                                                            + sum_j dFc_ij |W_jq|, dFc = u |Fc| + dmu"""
    Fl, tl = np.asarray(F, np.float64).astype(LD), np.asarray(truth, np.float64).astype(LD)
    km = Fl.shape[1]
    mu = np.sum(Fl, axis=1) / km
    dmu = gamma(km + 1) * (np.sum(np.abs(Fl), axis=1) / km)
    yc = tl - mu
    dyc = U * np.abs(yc) + dmu
    Fc = Fl - mu[:, None]
    W = (np.asarray(Vt, np.float64).T / np.asarray(S, np.float64)[None, :])      # float64 division
    Wl = np.abs(W.astype(LD))
    Uh = Fc @ W.astype(LD)
    dFc = U * np.abs(Fc) + dmu[:, None]
    dU = gamma(km) * (np.abs(Fc) @ Wl) + dFc @ Wl
    return dict(mu=mu, dmu=dmu, yc=yc, dyc=dyc, Fc=Fc, W=W, U=Uh, dU=dU)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0): at most 1 for a correct kernel."""
    dev = np.abs(np.asarray(got).astype(LD) - ref)
    bound = np.broadcast_to(bound, dev.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0, LD(0), dev / bound)
    return float(np.max(ratio))
