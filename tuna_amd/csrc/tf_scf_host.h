// tf_scf_host.h -- the host arithmetic of one SCF iteration, shared by the restricted and the unrestricted cycle (tf_scf.hip.h): the
// DIIS history with its Pulay equations (apply_DIIS scf:991-1059), the tail of the dynamic damping factor
// (calculate_damping_factor scf:763-868) and the convergence test (scf:261-333).  No HIP in here: tests/scf_host_model compiles it
// for the CPU.  The device side -- history matrices, scalar products, extrapolation -- stays in tf_scf.hip.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/tunafock.h"

namespace tfscf {

inline bool small_solve(int m, std::vector<double> A, std::vector<double> b, std::vector<double> &x)
{
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r)
            if (std::fabs(A[r * m + c]) > std::fabs(A[piv * m + c])) piv = r;
        if (A[piv * m + c] == 0.0 || !std::isfinite(A[piv * m + c])) return false;
        if (piv != c) {
            for (int k = 0; k < m; ++k) std::swap(A[c * m + k], A[piv * m + k]);
            std::swap(b[c], b[piv]);
        }
        for (int r = c + 1; r < m; ++r) {
            const double f = A[r * m + c] / A[c * m + c];
            if (f == 0.0) continue;
            for (int k = c; k < m; ++k) A[r * m + k] -= f * A[c * m + k];
            b[r] -= f * b[c];
        }
    }
    x.assign(m, 0.0);
    for (int r = m - 1; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < m; ++k) s -= A[r * m + k] * x[k];
        x[r] = s / A[r * m + r];
    }
    return true;
}

// The DIIS history of a cycle.  Logical entry k (0 = oldest) lives in physical slot slot[k] of the device history: trimming the
// oldest entry renumbers, nothing is copied.  An iteration calls make_room(), writes its entry into slot_of(n_hist), counts it
// (++n_hist), enters its row of scalar products, and -- when it extrapolates -- solve().
struct DiisHistory {
    int max_diis, n_hist = 0;
    std::vector<int> slot;
    std::vector<double> B;       // [max_diis][max_diis] scalar products of the error vectors, logical order
    explicit DiisHistory(int depth) : max_diis(depth), slot((size_t)depth), B((size_t)depth * depth, 0.0) { std::iota(slot.begin(), slot.end(), 0); }
    int slot_of(int k) const { return slot[k]; }
    void make_room()             // trim to max_diis - 1 entries (scf:943-946), so that the slot of the new entry is known
    {
        if (n_hist != max_diis) return;
        std::rotate(slot.begin(), slot.begin() + 1, slot.end());     // the oldest entry's slot becomes the newest
        for (int r = 0; r + 1 < n_hist; ++r)
            for (int c = 0; c + 1 < n_hist; ++c) B[r * max_diis + c] = B[(r + 1) * max_diis + c + 1];
        --n_hist;
    }
    void enter_dots(const double *row)   // row[k] = <e_k, e_newest>, k < n_hist (the newest entry counted)
    {
        for (int k = 0; k < n_hist; ++k) B[(n_hist - 1) * max_diis + k] = B[k * max_diis + (n_hist - 1)] = row[k];
    }
    // x[n_hist] in logical order, or false with the history emptied ("Resetting DIIS", scf:1042-1048; the slots stay as they stand)
    bool solve(std::vector<double> &x)
    {
        const int m = n_hist + 1;
        std::vector<double> A((size_t)m * m, 0.0), rhs(m, 0.0);
        for (int r = 0; r < n_hist; ++r) {
            for (int c = 0; c < n_hist; ++c) A[r * m + c] = B[r * max_diis + c];
            A[r * m + n_hist] = -1.0; A[n_hist * m + r] = -1.0;
        }
        rhs[n_hist] = -1.0;
        if (small_solve(m, A, rhs, x)) return true;
        n_hist = 0;
        return false;
    }
};

// Dynamic damping factor from the Mulliken populations of the two partitions: alpha = num / den per partition (the caller forms
// both from its own densities), weighted by the partitions' basis functions, not below zero, MAXDAMP where it reaches min(MAXDAMP, 1).
inline double damping_factor_tail(const tf_scf_opts &o, const double num[2], const double den[2])
{
    double alpha[2] = {0.0, 0.0};
    if (den[0] != 0.0 && den[1] != 0.0)
        for (int a = 0; a < 2; ++a) alpha[a] = num[a] / den[a];
    double f;
    if (o.n_atoms >= 2) {
        const double r0 = o.n_atom_ao[0], r1 = o.n_atom_ao[1];
        f = (alpha[0] * r0 + alpha[1] * r1) / (r0 + r1);
    } else f = alpha[0] * o.n_atom_ao[0];
    f = std::max(f, 0.0);
    return (f < std::min(o.max_damping, 1.0)) ? f : o.max_damping;
}

inline bool scf_converged(const tf_scf_opts &o, double dE, double maxDP, double rmsDP, double commutator)
{
    return std::fabs(dE) < o.conv_delta_E && std::fabs(maxDP) < o.conv_max_DP && std::fabs(rmsDP) < o.conv_rms_DP &&
           std::fabs(commutator) < o.conv_commutator;
}

}  // namespace tfscf
