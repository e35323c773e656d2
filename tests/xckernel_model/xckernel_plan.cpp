// TEST INFRASTRUCTURE: the HIP-free launch plan of the exchange-correlation kernel build (tuna_amd/csrc/tf_xckernel_plan.h) behind a C
// interface for tests/test_xckernel_plan.py.  No GPU code.
#include "../../tuna_amd/csrc/tf_xckernel_plan.h"

extern "C" {

// out = {n_b, n_tiles, n_slabs, slab_len, lds_bytes, partial_doubles, XCK_CHUNK, XCK_SLAB_MIN, XCK_TILE, XCK_ROW, XCK_THREADS, XCK_LDS_LIMIT}
void xckm_plan(long long dim, long long G, long long *out)
{
    const XckPlan P = xck_plan(dim, G);
    out[0] = P.n_b; out[1] = P.n_tiles; out[2] = P.n_slabs; out[3] = P.slab_len; out[4] = (long long)P.lds_bytes;
    out[5] = (long long)P.partial_doubles; out[6] = XCK_CHUNK; out[7] = XCK_SLAB_MIN; out[8] = XCK_TILE; out[9] = XCK_ROW;
    out[10] = XCK_THREADS; out[11] = XCK_LDS_LIMIT;
}

// bounds[2 s], bounds[2 s + 1] = [first, last) of slab s, for s < n_slabs
void xckm_slabs(long long dim, long long G, long long *bounds)
{
    const XckPlan P = xck_plan(dim, G);
    for (int s = 0; s < P.n_slabs; ++s) xck_slab_bounds(P, s, bounds + 2 * s, bounds + 2 * s + 1);
}

}
