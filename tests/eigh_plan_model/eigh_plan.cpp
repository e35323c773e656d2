// TEST INFRASTRUCTURE: the HIP-free plan of the symmetric eigensolver (tuna_amd/csrc/tf_eigh_plan.h) behind a C interface for
// tests/test_eigh_plan.py.  No GPU code.
#include "owner_checks.h"

extern "C" {

// out = {X, Xn, G, Y, S, E, lam, wocc, bmax, homo_lumo, vcls, total, npin} of the refinement block for n (doubles)
void eighm_ref_layout(int n, long long out[13])
{
    const tfscf::RefLayout L(n);
    const size_t v[13] = {L.X(), L.Xn(), L.G(), L.Y(), L.S(), L.E(), L.lam(), L.wocc(), L.bmax(), L.homo_lumo(), L.vcls(), L.total(), L.npin()};
    for (int k = 0; k < 13; ++k) out[k] = (long long)v[k];
}

// The plan of a class vector.  hdr = {n, nb, mmax, m[4], blk_of[4], worth blocking, LDS blocks, idx_cls, idx_sizes, idx_len, blocks_len, B, D,
// E, flag, buf_len}; idx: the host index table (at most idx_cap words are written).  Returns 1, or 0 if the vector was refused (then hdr is
// that of the plan before: an empty one)
int eighm_sym_plan(const int *cls, int n, long long hdr[22], int *idx, long long idx_cap)
{
    tfscf::SymPlan P;
    const int ok = P.build(std::vector<int>(cls, cls + n)) ? 1 : 0;
    hdr[0] = P.n; hdr[1] = P.nb; hdr[2] = P.mmax;
    for (int k = 0; k < 4; ++k) { hdr[3 + k] = P.m[k]; hdr[7 + k] = P.blk_of[k]; }
    hdr[11] = P.worth_blocking() ? 1 : 0; hdr[12] = P.lds_blocks() ? 1 : 0;
    const size_t v[9] = {P.idx_cls(), P.idx_sizes(), P.idx_len(), P.blocks_len(), P.B(), P.D(), P.E(), P.flag(), P.buf_len()};
    for (int k = 0; k < 9; ++k) hdr[13 + k] = (long long)v[k];
    for (size_t k = 0; k < P.idx.size() && (long long)k < idx_cap; ++k) idx[k] = P.idx[k];
    return ok;
}

// out = {BI_NOCC0, BI_NOCC1, BI_STATUS, BI_COMBINED, BI_LEN, SYM_LDS_BLOCK, EB_COUNT}
void eighm_ints(long long out[7])
{
    using namespace tfscf;
    const long long v[7] = {BI_NOCC0, BI_NOCC1, BI_STATUS, BI_COMBINED, BI_LEN, SYM_LDS_BLOCK, EB_COUNT};
    for (int k = 0; k < 7; ++k) out[k] = v[k];
}

// the ranges of d_scal as (first, length) pairs: populations, density changes, energy terms of spin 0 and 1, the two solver status words,
// the eigensolver's four (the refinement status: two ints in one double), the history's scalar products of spin 0 and 1; then SC_LEN
int eighm_scal_words(long long out[25])
{
    using namespace tfscf;
    const long long v[25] = {SC_POP, SC_POP_LEN, SC_DELTA, SC_DELTA_LEN, SC_ENERGY, SC_ENERGY_LEN, SC_ENERGY + SC_ENERGY_SPIN, SC_ENERGY_LEN,
                             SC_FAIL_RHF, 1, SC_FAIL_UHF, 1, SC_PROBE_RESID, 1, SC_PROBE_INFO, 1, SC_AMAX, 1, SC_REF_STATUS, 1,
                             SC_HIST, SC_HIST_SPIN, SC_HIST + SC_HIST_SPIN, SC_HIST_SPIN, SC_LEN};
    for (int k = 0; k < 25; ++k) out[k] = v[k];
    return 12;
}

// the owner sequence: ops = {kind, slot, bytes} each; returns their number
int eighm_owner_ops(long long *ops)
{
    for (int i = 0; i < eighm::NOPS; ++i) { ops[3 * i] = eighm::SEQ[i].kind; ops[3 * i + 1] = eighm::SEQ[i].slot; ops[3 * i + 2] = (long long)eighm::SEQ[i].bytes; }
    return eighm::NOPS;
}
// owner_run's figures and the verdict of the C++ model on them (0: all hold)
int eighm_owner(int k, long long *per_op, long long *totals)
{
    eighm::owner_run(k, per_op, totals);
    return eighm::owner_verdict(k, per_op, totals);
}
int eighm_refused(void) { return eighm::REFUSED; }
int eighm_state(long long *out)
{
    eighm::state_run(out);
    return eighm::state_verdict(out);
}

}
