// tf_cc_diis.h -- the host side of the coupled-cluster DIIS (update_DIIS, tuna_cc.py:363-408 and :482): which slot of the device history
// holds which vector, the error dots by slot, and the Pulay equations.  No HIP in here: tests/cc_diis_model compiles it for the CPU.
// The device side -- the history copies, cc_diis_dots_kernel, cc_mix_kernel -- stays with the drivers (tf_corr_host.hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace tfccd {

// The Pulay equations of update_DIIS (tuna_cc.py:363-381): B c = rhs with -1 borders, solved by elimination with partial pivoting.
// false: an exactly singular (or non-finite) matrix -- numpy.linalg.solve's LinAlgError, where the reference clears its history.
inline bool diis_solve(int n, const double *Bee /* [n][n] error dots */, double *coef /* [n] */)
{
    const int m = n + 1;
    double A[33 * 34];
    if (m > 33) return false;
    for (int r = 0; r < m; ++r) {
        for (int c = 0; c < m; ++c) A[r * (m + 1) + c] = (r < n && c < n) ? Bee[r * n + c] : ((r == n && c == n) ? 0.0 : -1.0);
        A[r * (m + 1) + m] = r == n ? -1.0 : 0.0;
    }
    for (int c = 0; c < m; ++c) {
        int p = c;
        for (int r = c + 1; r < m; ++r) if (fabs(A[r * (m + 1) + c]) > fabs(A[p * (m + 1) + c])) p = r;
        const double piv = A[p * (m + 1) + c];
        if (!(fabs(piv) > 0.0) || !std::isfinite(piv)) return false;
        if (p != c) for (int q = 0; q <= m; ++q) std::swap(A[p * (m + 1) + q], A[c * (m + 1) + q]);
        for (int r = c + 1; r < m; ++r) {
            const double f = A[r * (m + 1) + c] / piv;
            if (f != 0.0) for (int q = c; q <= m; ++q) A[r * (m + 1) + q] -= f * A[c * (m + 1) + q];
        }
    }
    double x[33];
    for (int r = m - 1; r >= 0; --r) {
        double s = A[r * (m + 1) + m];
        for (int q = r + 1; q < m; ++q) s -= A[r * (m + 1) + q] * x[q];
        x[r] = s / A[r * (m + 1) + r];
    }
    for (int r = 0; r < n; ++r) { if (!std::isfinite(x[r])) return false; coef[r] = x[r]; }
    return true;
}

// The history of one iteration loop.  A step that stores calls, in this order: store() -> the slot s the caller copies (t_new, dt)
// into; drop_oldest(step); enter_dots(s, row) with row[m] = <e_order[m], e_s> over the order as it then stands (s is its last entry);
// and, from step 3 on, solve(coef).
struct __attribute__((visibility("hidden"))) DiisHistory {
    int keep = 1;                // vectors of the history after the oldest has left (at most 32 here)
    int nslot = 0;               // slots of the device history: steps 1 and 2 store without dropping (tuna_cc.py:482); 0 without DIIS
    std::vector<int> order;      // slots in use, oldest first
    std::vector<double> Bee;     // error dots by slot, [nslot][nslot]

    void init(bool use_diis, int max_diis)
    {
        keep = std::max(1, std::min(max_diis, 32));
        nslot = use_diis ? std::max(keep, 2) + 1 : 0;
        order.clear();
        Bee.assign((size_t)std::max(1, nslot) * std::max(1, nslot), 0.0);
    }
    int store()                  // the next free slot, now the newest of the history
    {
        int s = 0;
        while (std::find(order.begin(), order.end(), s) != order.end()) ++s;
        order.push_back(s);
        return s;
    }
    void drop_oldest(int step) { if (step > 2 && (int)order.size() > keep) order.erase(order.begin()); }
    void enter_dots(int s, const double *row)
    {
        for (size_t m = 0; m < order.size(); ++m) Bee[(size_t)order[m] * nslot + s] = Bee[(size_t)s * nslot + order[m]] = row[m];
    }
    // coef [order.size()] in the order of the history, or false with the history cleared ("(Resetting DIIS)", tuna_cc.py:398-408)
    bool solve(double *coef)
    {
        const int n = (int)order.size();
        std::vector<double> B((size_t)n * n);
        for (int p = 0; p < n; ++p)
            for (int q = 0; q < n; ++q) B[(size_t)p * n + q] = Bee[(size_t)order[p] * nslot + order[q]];
        if (diis_solve(n, B.data(), coef)) return true;
        order.clear();
        return false;
    }
};

}  // namespace tfccd
