// spd_device.hpp -- the small symmetric positive-definite algebra of the least-squares solvers, in fp64 and templated on the
// number of unknowns N: the normal equations of k_fix, k_fix_atm, k_raim_*, k_vel and k_doppler_fix (N = 4, through nav_device.hpp)
// and of k_coarse_fix (N = 5).  Sym<N>, the packed lower triangle; add_row, the rank-1 update n += w h h^T, g += w h res;
// factor, Cholesky with the ONE pivot rule of the tree; solve; inverse_lower, M = L^-1; inverse_diagonal and inverse_along, the
// dilution figures read from M.  Nothing else, and nothing of GPS.
// Every index is a compile-time constant and every loop is fully unrolled, so a Sym<N> lives in registers.  The order of the
// operations is part of the contract: the loops run k upwards, a sum starts with its first term and not with 0, and M is formed
// with reciprocals, so that N = 4 gives the bits of the ten-term formulas it replaced (tests/test_spd.py holds their transcript).
// The functions also compile for the host (SPD_HD, as ACQ_HD of acq_math.hpp): tests/emul/emul_spd.cpp calls them from the CPU suite.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SPD_HD __host__ __device__ __forceinline__
#else
#define SPD_HD inline
#endif

namespace acq {

constexpr double TINY = 1e-13;  // a Cholesky pivot below TINY times its diagonal entry: singular

// the lower triangle of a symmetric N x N, row by row: a normal matrix, its Cholesky factor L, or M = L^-1
template <int N>
struct Sym {
    double v[N * (N + 1) / 2];
    static constexpr int at(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i
    SPD_HD double& operator()(int i, int j) { return v[at(i, j)]; }
    SPD_HD const double& operator()(int i, int j) const { return v[at(i, j)]; }
};

// n += (w h) h^T: one row h of weight w into the normal matrix
template <int N>
SPD_HD void add_row(Sym<N>& n, const double (&h)[N], double w) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double wh = w * h[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) n(i, j) += wh * h[j];
    }
}

// and g += (w h) res, its residual into the right-hand side
template <int N>
SPD_HD void add_row(Sym<N>& n, double (&g)[N], const double (&h)[N], double w, double res) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double wh = w * h[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) n(i, j) += wh * h[j];
        g[i] += wh * res;
    }
}

// Cholesky A = L L^T.  false: singular -- the first pivot is not above 0, or a later one not above TINY times its diagonal
// entry (a NaN fails either test)
template <int N>
SPD_HD bool factor(const Sym<N>& a, Sym<N>& l) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double p = a(j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) p -= l(j, k) * l(j, k);
        if (!(p > (j == 0 ? 0.0 : TINY * a(j, j)))) return false;
        l(j, j) = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = a(i, j);
#pragma unroll
            for (int k = 0; k < j; ++k) v -= l(i, k) * l(j, k);
            l(i, j) = v / l(j, j);
        }
    }
    return true;
}

// L L^T d = g
template <int N>
SPD_HD void solve(const Sym<N>& l, const double (&g)[N], double (&d)[N]) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= l(i, k) * y[k];
        y[i] = v / l(i, i);
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= l(k, i) * d[k];
        d[i] = v / l(i, i);
    }
}

// M = L^-1 (lower): m_ii = 1 / l_ii, m_ij = -(sum over k = j .. i-1 of l_ik m_kj) m_ii.  N divides, the rest multiplies
template <int N>
SPD_HD void inverse_lower(const Sym<N>& l, Sym<N>& m) {
#pragma unroll
    for (int i = 0; i < N; ++i) m(i, i) = 1.0 / l(i, i);
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = l(i, j) * m(j, j);
#pragma unroll
            for (int k = j + 1; k < i; ++k) v += l(i, k) * m(k, j);
            m(i, j) = -v * m(i, i);
        }
    }
}

// the diagonal of (L L^T)^-1 = M^T M: q_j = the sum over i >= j of m_ij^2
template <int N>
SPD_HD void inverse_diagonal(const Sym<N>& m, double (&q)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        q[j] = m(j, j) * m(j, j);
#pragma unroll
        for (int i = j + 1; i < N; ++i) q[j] += m(i, j) * m(i, j);
    }
}

// v^T (L L^T)^-1 v = |M v|^2 for a direction v in the first K unknowns (its other entries are zero and are not multiplied)
template <int N, int K>
SPD_HD double inverse_along(const Sym<N>& m, const double (&v)[K]) {
    static_assert(K <= N, "a direction has at most N entries");
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double c = m(i, 0) * v[0];
#pragma unroll
        for (int j = 1; j <= i && j < K; ++j) c += m(i, j) * v[j];
        q = i == 0 ? c * c : q + c * c;
    }
    return q;
}

}  // namespace acq
