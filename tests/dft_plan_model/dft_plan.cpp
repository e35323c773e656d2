// TEST INFRASTRUCTURE: the HIP-free plan of the Kohn-Sham grid (tuna_amd/csrc/tf_dft_plan.h) behind a C interface for
// tests/test_dft_plan.py.  No GPU code.
#include "owner_checks.h"

extern "C" {

// out = {buffers of the base set, of the spin set, VSPLIT, NPART, SPT}
void dftm_info(long long out[5])
{
    out[0] = tfdft::GB_COUNT; out[1] = tfdft::GS_COUNT; out[2] = tfdft::VSPLIT; out[3] = tfdft::NPART; out[4] = tfdft::SPT;
}

// the lengths (doubles) of set 0 (base) or 1 (spin) in their listed order; returns their number
int dftm_lengths(int set, long long G, int N, int gga, long long *out)
{
    size_t len[tfdft::GridBlocks::MAX];
    const int n = dftm::set_lengths(set, G, N, gga, len);
    for (int k = 0; k < n; ++k) out[k] = (long long)len[k];
    return n;
}

// out = {Kc, rem, first_rem, nparts, rem_slot, sum_off, doubles of the buffer, part_off[0 .. nparts)}
void dftm_split(long long G, long long width, long long *out)
{
    const tfdft::SplitPlan S = tfdft::split_plan(G, width);
    out[0] = S.Kc; out[1] = S.rem; out[2] = S.first_rem; out[3] = S.nparts; out[4] = S.rem_slot; out[5] = S.sum_off();
    out[6] = (long long)tfdft::split_doubles((size_t)width);
    for (int s = 0; s < S.nparts; ++s) out[7 + s] = S.part_off(s);
}

// owner_run's figures, then the bytes of every request in the order they were made; returns the number of requests
int dftm_owner(int set, long long G, int N, int gga, int k, long long *out11, long long *bytes)
{
    dftm::owner_run(set, G, N, gga, k, out11);
    for (int r = 0; r < dftm::book.requests && r < dftm::MAXB; ++r) bytes[r] = (long long)dftm::book.bytes[r];
    return dftm::book.requests;
}

int dftm_refused(void) { return dftm::REFUSED; }
int dftm_grid_release(long long G, int N, int gga) { return dftm::grid_release_check(G, N, gga); }

}
