// Host build of gnss-gps-sdr_amd/csrc/spd_device.hpp, the solvers' Cholesky piece, for tests/test_spd.py: the same templates the
// kernels instantiate, N = 4 and N = 5, behind a C interface over packed lower triangles.  Test infrastructure, part of
// libemul_acq.so (-ffp-contract=off, as the host flags are: what the test compares is the order of the operations).
#include "../../gnss-gps-sdr_amd/csrc/spd_device.hpp"

using namespace acq;

namespace {
template <int N>
void rows_of(int rows, const double* h, const double* w, const double* res, double* n_out, double* g_out, double* m_out) {
    Sym<N> n = {}, m = {};
    double g[N] = {};
    for (int r = 0; r < rows; ++r) {
        double row[N];
        for (int i = 0; i < N; ++i) row[i] = h[r * N + i];
        add_row(n, g, row, w[r], res[r]);
        add_row(m, row, w[r]);
    }
    for (int k = 0; k < N * (N + 1) / 2; ++k) n_out[k] = n.v[k], m_out[k] = m.v[k];
    for (int i = 0; i < N; ++i) g_out[i] = g[i];
}

// everything read from one matrix: L, d with L L^T d = g, M = L^-1, the diagonal q of (L L^T)^-1 and |M v|^2 for a direction v
// in the first three unknowns.  Returns factor()'s verdict; at 0 nothing else is written
template <int N>
int chain_of(const double* a_in, const double* g_in, const double* v_in, double* l_out, double* d_out, double* m_out, double* q_out, double* along) {
    Sym<N> a, l, m;
    for (int k = 0; k < N * (N + 1) / 2; ++k) a.v[k] = a_in[k];
    if (!factor(a, l)) return 0;
    double g[N], d[N], q[N];
    for (int i = 0; i < N; ++i) g[i] = g_in[i];
    solve(l, g, d);
    inverse_lower(l, m);
    inverse_diagonal(m, q);
    const double v[3] = {v_in[0], v_in[1], v_in[2]};
    *along = inverse_along(m, v);
    for (int k = 0; k < N * (N + 1) / 2; ++k) l_out[k] = l.v[k], m_out[k] = m.v[k];
    for (int i = 0; i < N; ++i) d_out[i] = d[i], q_out[i] = q[i];
    return 1;
}
}  // namespace

extern "C" {
double emul_spd_tiny(void) { return TINY; }
int emul_spd_rows(int N, int rows, const double* h, const double* w, const double* res, double* n_out, double* g_out, double* m_out) {
    if (N == 4) rows_of<4>(rows, h, w, res, n_out, g_out, m_out);
    else if (N == 5) rows_of<5>(rows, h, w, res, n_out, g_out, m_out);
    else return -1;
    return 0;
}
int emul_spd_chain(int N, const double* a, const double* g, const double* v, double* l, double* d, double* m, double* q, double* along) {
    if (N == 4) return chain_of<4>(a, g, v, l, d, m, q, along);
    if (N == 5) return chain_of<5>(a, g, v, l, d, m, q, along);
    return -1;
}
}
