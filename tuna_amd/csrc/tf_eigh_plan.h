// tf_eigh_plan.h -- the plan of the symmetric eigensolver (tf_eigh.hip.h): where every part of its buffers lies, which words of the
// small scalar and status arrays are whose, the owner of its grow-only blocks and the state it keeps between solves.  Plain C++17, no
// HIP: tests/eigh_plan_model compiles it with g++ (tests/test_eigh_plan.py).  DESIGN.md 4.4b.
#pragma once
#include <cstddef>
#include <vector>

namespace tfscf {

// ---- the refinement block of one spin (doubles): X | Xn | G | Y | S | E | lam | wocc | bmax[2g] | homo, lumo | pad[6] | vcls ----
// X: the current vectors (rows); Xn, G, Y, S, E: the work matrices of a step (G's slot hands back the occupied rows); bmax: the
// per-workgroup maxima of k_ref_E (g = workgroups of 256 over nn); vcls: n ints, the block label of every vector.  bmax and the
// homo/lumo pair are read back together: npin doubles of pinned memory.
struct RefLayout {
    size_t n, nn, g;
    explicit RefLayout(int n_) : n((size_t)n_), nn((size_t)n_ * (size_t)n_), g(((size_t)n_ * (size_t)n_ + 255) / 256) {}
    size_t X() const { return 0; }
    size_t Xn() const { return nn; }
    size_t G() const { return 2 * nn; }
    size_t Y() const { return 3 * nn; }
    size_t S() const { return 4 * nn; }
    size_t E() const { return 5 * nn; }
    size_t lam() const { return 6 * nn; }
    size_t wocc() const { return lam() + n; }
    size_t bmax() const { return wocc() + n; }
    size_t homo_lumo() const { return bmax() + 2 * g; }
    size_t vcls() const { return homo_lumo() + 8; }
    size_t total() const { return vcls() + n; }
    size_t npin() const { return 2 * g + 2; }
};

// ---- the symmetry blocks of a class vector (eigh_blocked, ref_refine_blocks) -----------------------------------------------------
// Block b is the b-th class that has members, in class order.  Host index table: [4][mmax] original index of member t of block b
// (-1: padding) | cls[n] | sizes[4].  Device work buffer (doubles): B [nb][mmax][mmax] | D [nb][mmax] | E [nb][mmax] | flag (4).
const int SYM_LDS_BLOCK = 64;                 // the largest block the in-LDS Jacobi kernel takes
struct SymPlan {
    int n = 0, nb = 0, mmax = 0;
    int m[4] = {0, 0, 0, 0}, blk_of[4] = {-1, -1, -1, -1};
    std::vector<int> idx;
    bool build(const std::vector<int> &cls)   // false: a class outside 0 ... 3 (nothing is changed)
    {
        int cnt[4] = {0, 0, 0, 0};
        for (int c : cls) { if (c < 0 || c > 3) return false; ++cnt[c]; }
        *this = SymPlan();
        n = (int)cls.size();
        for (int c = 0; c < 4; ++c) if (cnt[c] > 0) { blk_of[c] = nb; m[nb] = cnt[c]; ++nb; mmax = mmax > cnt[c] ? mmax : cnt[c]; }
        idx.assign(idx_len(), -1);
        int fill[4] = {0, 0, 0, 0};
        for (int i = 0; i < n; ++i) { const int b = blk_of[cls[i]]; idx[(size_t)b * mmax + fill[b]++] = i; idx[idx_cls() + i] = cls[i]; }
        for (int b = 0; b < 4; ++b) idx[idx_sizes() + b] = b < nb ? m[b] : 0;
        return true;
    }
    bool worth_blocking() const { return nb >= 2 && 4 * mmax <= 3 * n; }   // else one class holds (nearly) everything
    bool lds_blocks() const { return mmax <= SYM_LDS_BLOCK; }              // batched Jacobi kernel; else dsyevd_strided_batched
    size_t idx_cls() const { return (size_t)4 * mmax; }
    size_t idx_sizes() const { return idx_cls() + (size_t)n; }
    size_t idx_len() const { return idx_sizes() + 4; }
    size_t blocks_len() const { return (size_t)nb * mmax * mmax; }         // B; also the block vectors of a spin and of the last solve
    size_t B() const { return 0; }
    size_t D() const { return blocks_len(); }
    size_t E() const { return D() + (size_t)nb * mmax; }
    size_t flag() const { return E() + (size_t)nb * mmax; }
    size_t buf_len() const { return flag() + 4; }
};

// ---- the words of blk_ints (ints): occupied vectors per block of spin 0 | status[4][2] | combined[2] | .. | the same of spin 1 ----
enum BlkInts : int { BI_NOCC0 = 0, BI_STATUS = 4, BI_COMBINED = 12, BI_NOCC1 = 16, BI_LEN = 32 };

// ---- the words of Workspace::d_scal (doubles) ----------------------------------------------------------------------------------
// The cycles' own (invariant 3) and the eigensolver's; each range [first, first + length).
enum ScalWord : int {
    SC_POP = 0, SC_POP_LEN = 8,               // Mulliken populations of four densities
    SC_DELTA = 16, SC_DELTA_LEN = 2,          // density changes; the read-back at the end of an iteration starts here
    SC_ENERGY = 18, SC_ENERGY_LEN = 5,        // energy terms of spin 0; spin 1 SC_ENERGY_SPIN further on
    SC_ENERGY_SPIN = 6,
    SC_FAIL_RHF = 23,                         // solver status of an iteration, restricted cycle
    SC_FAIL_UHF = 30,                         // the same, unrestricted cycle
    SC_PROBE_RESID = 32,                      // eigh_probe: residual of dsyevj
    SC_PROBE_INFO = 40,                       // eigh_probe: status word of dsyevdx / dsyevx
    SC_AMAX = 48,                             // eigh: bits of max |a_ij|
    SC_REF_STATUS = 62,                       // in-LDS refinement: two ints (converged, steps)
    SC_HIST = 128, SC_HIST_SPIN = 64,         // scalar products of the DIIS history, SC_HIST_SPIN per spin
    SC_LEN = 256
};
static_assert(SC_POP + SC_POP_LEN <= SC_DELTA && SC_DELTA + SC_DELTA_LEN == SC_ENERGY && SC_ENERGY + SC_ENERGY_LEN == SC_FAIL_RHF &&
              SC_FAIL_RHF + 1 == SC_ENERGY + SC_ENERGY_SPIN && SC_ENERGY + SC_ENERGY_SPIN + SC_ENERGY_LEN <= SC_FAIL_UHF &&
              SC_FAIL_UHF < SC_PROBE_RESID && SC_PROBE_RESID < SC_PROBE_INFO && SC_PROBE_INFO < SC_AMAX && SC_AMAX < SC_REF_STATUS &&
              SC_REF_STATUS < SC_HIST && SC_HIST + 2 * SC_HIST_SPIN == SC_LEN,
              "the words of d_scal do not overlap and end with the array");

// ---- owner of N named, grow-only blocks ------------------------------------------------------------------------------------------
// `alloc` returns 0 on success (else its code is handed on); a slot is either null with capacity 0 or a block of `cap` bytes.
typedef int (*BlockAllocFn)(void **p, size_t bytes);
typedef void (*BlockFreeFn)(void *p);
template <int N> struct Blocks {
    void *p[N] = {};
    size_t cap[N] = {};                       // bytes
    BlockAllocFn alloc_fn = nullptr;
    BlockFreeFn free_fn = nullptr;
    Blocks() {}
    Blocks(BlockAllocFn a, BlockFreeFn f) : alloc_fn(a), free_fn(f) {}
    int ensure(int slot, size_t bytes)        // keeps a block that is large enough, else frees it and asks for one of `bytes`
    {
        if (p[slot] && cap[slot] >= bytes) return 0;
        drop(slot);
        void *q = nullptr;
        const int rc = alloc_fn(&q, bytes);
        if (rc != 0) return rc;
        p[slot] = q; cap[slot] = bytes;
        return 0;
    }
    void drop(int slot)
    {
        if (p[slot]) free_fn(p[slot]);
        p[slot] = nullptr; cap[slot] = 0;
    }
    void release() { for (int k = 0; k < N; ++k) drop(k); }
    template <class T> T *at(int slot) const { return static_cast<T *>(p[slot]); }
};

// the device blocks of the eigensolver
enum EigBlock : int {
    EB_JAC_SCRATCH,                           // [n][n] eigenvector scratch of the Jacobi kernel when it does not fit LDS
    EB_JAC_PREV,                              // [n][n] eigenvectors of the previous solve (warm start inside one cycle)
    EB_JAC_IN,                                // [n][n] the matrix handed to the Jacobi kernel (to solve it again with dsyevd)
    EB_REF0, EB_REF1,                         // RefLayout: the refinement block of each spin
    EB_BLK_X0, EB_BLK_X1,                     // [nb][mmax][mmax] compact: the blocks' current vectors of each spin (blocked refinement)
    EB_BLK_INTS,                              // BlkInts
    EB_SYM_IDX,                               // ints: SymPlan::idx
    EB_SYM_BUF,                               // SymPlan: B | D | E | flag
    EB_SYM_SRC,                               // ints [n]: block * mmax + member of the eigenvalue of global rank r
    EB_SYM_PREV,                              // [nb][mmax][mmax]: block eigenvectors of the previous solve (warm start, batched Jacobi)
    EB_COUNT
};

// What the warm start of one spin consists of: its two blocks, for which n each part is valid (0: not), where its noccs[4] live
struct SpinVectors {
    int ref_slot, blk_slot, nocc_off;
    int ref_n = 0;                            // n when rows of X are a valid start
    int vcls_n = 0;                           // n when the vectors carry block labels (vcls)
    int blk_n = 0;                            // n when the block vectors and noccs are valid
};

// Everything the eigensolver keeps between calls.  The second spin of an unrestricted cycle is cur = 1 around its solves.
struct EigState {
    Blocks<EB_COUNT> dev;
    Blocks<1> pin;                            // pinned host memory: the per-step read-back of the refinement overlaps the next GEMMs
    SpinVectors spin[2] = {{EB_REF0, EB_BLK_X0, BI_NOCC0}, {EB_REF1, EB_BLK_X1, BI_NOCC1}};
    int cur = 0;
    int jac_prev_n = 0;                       // 0 = no valid warm start of the full-matrix Jacobi kernel
    bool warm_ok = false;                     // set by run_rhf for the duration of one SCF cycle
    // symmetry blocks: class of every basis function (set_symmetry; empty = none known) and the tables built from it
    std::vector<int> sym_cls;
    SymPlan sym;
    int sym_n = 0;                            // n > 0: `sym` and the device tables (EB_SYM_IDX, _BUF, _SRC; _PREV if lds_blocks()) are whole for it
    int sym_prev_n = 0;                       // 0 = no valid warm start of the batched Jacobi kernel
    bool sym_last_blocked = false;            // the last eigh() went block by block: EB_SYM_SRC names the block of every eigenvector it returned
    // solver status words (`info` of the Jacobi kernels and of rocSOLVER): checked at once (one read-back per solve), or -- inside the
    // iterations of a native cycle, which must not wait on the device per solve -- counted on the device into *eig_fail, which the cycle
    // reads back with the density changes of the iteration
    double *eig_fail = nullptr;
    long long ref_solves = 0, ref_steps = 0, ref_fallbacks = 0;
    long long blk_solves = 0, blk_fallbacks = 0;
    long long sym_solves = 0, sym_declined = 0;
    long long jac_fallbacks = 0;              // full-matrix Jacobi solves that did not converge and went to dsyevd
    EigState() {}
    EigState(BlockAllocFn da, BlockFreeFn df, BlockAllocFn pa, BlockFreeFn pf) : dev(da, df), pin(pa, pf) {}
    SpinVectors &sv() { return spin[cur]; }
    void forget_vectors() { for (SpinVectors &s : spin) { s.ref_n = 0; s.vcls_n = 0; s.blk_n = 0; } }   // no refinement start, either spin
    void forget_tables()                      // no tables, and nothing that was built on them
    {
        sym_n = 0; sym_prev_n = 0;
        for (SpinVectors &s : spin) s.blk_n = 0;
    }
    void release() { dev.release(); pin.release(); }
};

}  // namespace tfscf
