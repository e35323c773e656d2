// TEST INFRASTRUCTURE: the HIP-free launch plan of the spin-blocked exchange-correlation kernel build (tuna_amd/csrc/tf_xckernel_plan.h)
// behind a C interface for tests/test_xckernel_spin_plan.py.  No GPU code.
#include <vector>

#include "../../tuna_amd/csrc/tf_xckernel_plan.h"

extern "C" {

// out = {n_b alpha, n_b beta, n_tiles, n_slabs, slab_len, lds_bytes, partial_doubles, dim, XCK_CHUNK, XCK_SLAB_MIN, XCK_TILE, XCK_ROW,
//        XCK_LDS_LIMIT, cols}; cols = 0 asks for the library's default shape
void xcksm_plan(long long d_alpha, long long d_beta, long long G, int cols, long long *out)
{
    const XckSpinPlan P = cols ? xck_spin_plan(d_alpha, d_beta, G, cols) : xck_spin_plan(d_alpha, d_beta, G);
    out[0] = P.n_b[0]; out[1] = P.n_b[1]; out[2] = P.n_tiles; out[3] = P.n_slabs; out[4] = P.slab_len; out[5] = (long long)P.lds_bytes;
    out[6] = (long long)P.partial_doubles; out[7] = P.dim; out[8] = XCK_CHUNK; out[9] = XCK_SLAB_MIN; out[10] = XCK_TILE; out[11] = XCK_ROW;
    out[12] = XCK_LDS_LIMIT; out[13] = P.cols;
}

// per block b < n_b alpha + n_b beta: blocks[3 b ..] = {spin, first element within the spin's part, the part's offset in the compound index}
void xcksm_blocks(long long d_alpha, long long d_beta, long long G, long long *blocks)
{
    const XckSpinPlan P = xck_spin_plan(d_alpha, d_beta, G, 1);
    for (int b = 0; b < P.n_b[0] + P.n_b[1]; ++b) {
        int spin;
        xck_spin_block(P, b, &spin, blocks + 3 * b + 1, blocks + 3 * b + 2);
        blocks[3 * b] = spin;
    }
}

// tiles[3 t ..] = (row block, first column block, column blocks) of tile t < n_tiles: the list the host uploads for the kernel
void xcksm_tiles(long long d_alpha, long long d_beta, long long G, int cols, long long *tiles)
{
    const XckSpinPlan P = xck_spin_plan(d_alpha, d_beta, G, cols);
    std::vector<XckSpinTile> t((size_t)P.n_tiles);
    xck_spin_tiles(P, t.data());
    for (long long k = 0; k < P.n_tiles; ++k) { tiles[3 * k] = t[k].bi; tiles[3 * k + 1] = t[k].bj; tiles[3 * k + 2] = t[k].nc; }
}

}
