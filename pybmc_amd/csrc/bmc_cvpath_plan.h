// Host-only plan of the component path (bmc_cv_path): cross-validation of every
// candidate component count in one call.  A PROBLEM is a (candidate, fold) pair, numbered
// p = candidate * F + fold; its C chains are chains p * C .. p * C + C - 1.  Here: the check of the
// candidate list, the split of the problems into batches that fit the device memory, the launches
// of a batch (one width class of cv_kmax each, widest first, at most 2048 one-wave chains), the
// per-problem descriptors the chain kernel reads, and the memory estimate.  No HIP types:
// tests/cvpath_plan_check.cpp compiles it with g++.
#pragma once
#include "bmc_cv_plan.h"

namespace bmc {

// "" when comps[0 .. m) is a strictly increasing list of component counts in 1 .. k_max
inline std::string cvpath_check(int32_t k_max, const int32_t* comps, int32_t m) {
    if (k_max < 1 || k_max > CV_MAX_K)
        return "k must be between 1 and " + std::to_string(CV_MAX_K) + "; got " + std::to_string(k_max);
    if (!comps || m < 1) return "need at least one candidate component count";
    if (m > k_max) return "more candidates than columns";
    for (int32_t j = 0; j < m; ++j) {
        if (comps[j] < 1 || comps[j] > k_max)
            return "candidate " + std::to_string(comps[j]) + " is outside 1 .. " + std::to_string(k_max);
        if (j && comps[j] <= comps[j - 1])
            return "candidates must be strictly increasing; got " + std::to_string(comps[j]) +
                   " after " + std::to_string(comps[j - 1]);
    }
    return "";
}

// What chain kernel block b of a launch needs of its problem: the local chain l = chain0 + b
// belongs to problem l / C of the batch, chain l % C of it.  Offsets are in doubles: g_off into G,
// v_off into lam, c1, c2, u0 and g0, s_off into scal (set-up arrays of ALL problems, candidate
// after candidate, each [F][k][k] or [F][k]); xi_off, gam_off, u_off and d_off the problem's first
// chain in the batch's variates, rotated draws and kept draws (chain c of it follows at c * T * k,
// c * T, c * T * (k + 1) and c * kept * (k + 1)).
struct CvPathDesc {
    int32_t k, cand, fold, pad;
    int64_t g_off, v_off, s_off, xi_off, gam_off, u_off, d_off;
};

struct CvPathLaunch {
    int32_t kmax;       // the width class: cv_kmax of every chain in the launch
    int64_t chain0;     // first local chain of the batch
    int32_t n_chains;
};

struct CvPathBatch {
    int32_t p0, p1;                       // problems [p0, p1)
    size_t bytes;                         // device bytes of the batch's chains
    int64_t xi_len, gam_len, u_len, d_len;   // doubles of the four chain buffers
    std::vector<CvPathDesc> desc;         // [p1 - p0]
    std::vector<CvPathLaunch> launches;
};

// device bytes of problem (candidate k, any fold): its C chains
inline size_t cvpath_problem_bytes(int32_t k, int32_t C, int64_t T, int64_t kept) {
    return cv_chain_bytes(k, T, kept) * (size_t)C;
}

// first element of candidate j's block in the set-up arrays: [F][k][k] (matrix) or [F][k] (vector)
inline void cvpath_setup_offsets(int32_t F, const int32_t* comps, int32_t m, std::vector<int64_t>& mat,
                                 std::vector<int64_t>& vec) {
    mat.assign(m + 1, 0);
    vec.assign(m + 1, 0);
    for (int32_t j = 0; j < m; ++j) {
        mat[j + 1] = mat[j] + (int64_t)F * comps[j] * comps[j];
        vec[j + 1] = vec[j] + (int64_t)F * comps[j];
    }
}

// Batches are runs of whole problems in order, filled greedily up to `budget` bytes.  false: the
// problem *too_big (its bytes in *need) does not fit on its own; nothing is planned.
inline bool plan_cvpath(int32_t F, int32_t C, const int32_t* comps, int32_t m, int64_t T, int64_t kept,
                        size_t budget, std::vector<CvPathBatch>& out, int32_t* too_big = nullptr,
                        size_t* need = nullptr) {
    out.clear();
    const int32_t P = m * F;
    for (int32_t j = 0; j < m; ++j) {
        const size_t b = cvpath_problem_bytes(comps[j], C, T, kept);
        if (b == 0 || b > budget) {
            if (too_big) *too_big = j * F;
            if (need) *need = b;
            return false;
        }
    }
    std::vector<int64_t> mat, vec;
    cvpath_setup_offsets(F, comps, m, mat, vec);
    for (int32_t p0 = 0; p0 < P;) {
        CvPathBatch b;
        b.p0 = p0;
        b.bytes = 0;
        b.xi_len = b.gam_len = b.u_len = b.d_len = 0;
        int32_t p = p0;
        for (; p < P; ++p) {
            const int32_t j = p / F, f = p - j * F, k = comps[j];
            const size_t pb = cvpath_problem_bytes(k, C, T, kept);
            if (p > p0 && b.bytes + pb > budget) break;
            CvPathDesc d;
            d.k = k; d.cand = j; d.fold = f; d.pad = 0;
            d.g_off = mat[j] + (int64_t)f * k * k;
            d.v_off = vec[j] + (int64_t)f * k;
            d.s_off = (int64_t)p * 4;
            d.xi_off = b.xi_len; d.gam_off = b.gam_len; d.u_off = b.u_len; d.d_off = b.d_len;
            b.xi_len += (int64_t)C * T * k;
            b.gam_len += (int64_t)C * T;
            b.u_len += (int64_t)C * T * (k + 1);
            b.d_len += (int64_t)C * kept * (k + 1);
            b.bytes += pb;
            b.desc.push_back(d);
        }
        b.p1 = p;
        // candidates ascend, so a width class is one run of the batch's problems
        for (int kmax = 64; kmax >= 8; kmax >>= 1) {
            int32_t a = -1, e = -1;
            for (int32_t q = 0; q < b.p1 - b.p0; ++q)
                if (cv_kmax(b.desc[q].k) == kmax) {
                    if (a < 0) a = q;
                    e = q + 1;
                }
            if (a < 0) continue;
            const int64_t c0 = (int64_t)a * C, c1 = (int64_t)e * C;
            for (int64_t c = c0; c < c1; c += CV_MAX_CHAINS_PER_LAUNCH)
                b.launches.push_back(CvPathLaunch{kmax, c, (int32_t)(c1 - c < CV_MAX_CHAINS_PER_LAUNCH
                                                                         ? c1 - c : CV_MAX_CHAINS_PER_LAUNCH)});
        }
        out.push_back(b);
        p0 = p;
    }
    return true;
}

}  // namespace bmc
