// tf_xckernel_plan.h -- the launch plan of the exchange-correlation kernel build (tf_xckernel.hip.h), stated ONCE: tile and chunk
// shape, the LDS carve-out, the cut of the grid into slabs and the size of the slab partials.  A pure function of (dim, G): nothing
// of the device (CU count, free memory) enters, so two calls -- and two machines -- sum the same slabs in the same order and give
// the same bits.  No HIP: tests/xckernel_model compiles it for the CPU, tests/test_xckernel_plan.py checks it.  DESIGN.md section 4.5d.
#pragma once
#include <algorithm>
#include <cstddef>

enum {
    XCK_TILE = 64,                // rows and columns of the output tile of one workgroup: four waves, a 16 x 64 strip each
    XCK_CHUNK = 32,               // grid points staged in LDS per step: eight 16x16x4 contractions
    XCK_ROW = XCK_TILE + 16,      // doubles between the grid points of a staged operand: 80 = 16 (mod 32), so that the four k-rows
                                  // of a matrix-core operand read land in different halves of the 64 LDS banks
    XCK_THREADS = 256,
    XCK_SLAB_MIN = 8 * XCK_CHUNK, // no slab is planned shorter than this (the staging prologue would dominate)
    XCK_WG_TARGET = 1024,         // workgroups wanted in flight: four per CU of the largest part this runs on, a constant here
    XCK_LDS_LIMIT = 160 * 1024    // LDS of a gfx950 workgroup
};

struct XckPlan {
    long long dim = 0, G = 0;
    int n_b = 0;                  // 64-wide blocks of the compound index
    long long n_tiles = 0;        // tiles with row block <= column block: n_b (n_b + 1) / 2
    int n_slabs = 1;              // cuts of the grid; slab s covers [s slab_len, min(G, (s + 1) slab_len))
    long long slab_len = 0;       // a multiple of XCK_CHUNK
    size_t lds_bytes = 0;         // left operand | right operand | u_S | u_T of one chunk
    size_t partial_doubles = 0;   // [n_slabs][2][dim][dim]
};

// The cut of the grid into slabs for n_tiles tiles, stated once for both plans: as many slabs as bring tiles x slabs to XCK_WG_TARGET
// workgroups, none shorter than XCK_SLAB_MIN points, each a whole number of chunks
static inline void xck_slab_cut(long long n_tiles, long long G, long long *slab_len, int *n_slabs)
{
    const long long want = std::max<long long>(1, (XCK_WG_TARGET + n_tiles - 1) / std::max<long long>(1, n_tiles));
    const long long most = std::max<long long>(1, G / XCK_SLAB_MIN);              // slabs of at least XCK_SLAB_MIN points
    const long long n = std::min(want, most);
    const long long per = (G + n - 1) / n;
    *slab_len = std::max<long long>(XCK_CHUNK, (per + XCK_CHUNK - 1) / XCK_CHUNK * XCK_CHUNK);
    *n_slabs = (int)std::max<long long>(1, (G + *slab_len - 1) / *slab_len);
}

static inline XckPlan xck_plan(long long dim, long long G)
{
    XckPlan P;
    P.dim = dim; P.G = G;
    P.n_b = (int)((dim + XCK_TILE - 1) / XCK_TILE);
    P.n_tiles = (long long)P.n_b * (P.n_b + 1) / 2;
    xck_slab_cut(P.n_tiles, G, &P.slab_len, &P.n_slabs);
    P.lds_bytes = (size_t)(2 * XCK_CHUNK * XCK_ROW + 2 * XCK_CHUNK) * sizeof(double);
    P.partial_doubles = (size_t)P.n_slabs * 2 * (size_t)dim * (size_t)dim;
    return P;
}

// [first, last) of slab s
static inline void xck_slab_bounds(const XckPlan &P, int s, long long *first, long long *last)
{
    *first = std::min(P.G, (long long)s * P.slab_len);
    *last = std::min(P.G, (long long)(s + 1) * P.slab_len);
}

// ---- the spin-blocked build (tfxck::xck_spin_kernel): K of an unrestricted reference, compound index = the alpha block (d_alpha = o_a v_a
// elements) then the beta block (d_beta), as tf_ucis.hip.h.  Blocks of XCK_TILE are cut PER SPIN -- the last alpha block is padded with
// zeros, not continued into beta.  A tile is one row block times `cols` adjacent column blocks OF ONE SPIN (cols = 1: 64 x 64; cols = 2:
// 64 x 128, the last group of a spin with an odd number of blocks is one block wide), so every tile is spin-pure and has one weight vector
// (u_aa, u_ab or u_bb).  Listed row block by row block are the tiles that hold an element with row <= column: the beta-alpha rectangle is
// the transpose of alpha-beta and is never computed.  An empty spin block has no block and no tile.  The slab cut is xck_slab_cut on this
// tile count; a pure function of (d_alpha, d_beta, G, cols).
enum { XCK_SPIN_COLS = 1 };       // the tile shape the library runs unless told otherwise (tf_xc_kernel_spin_cols): 64 x 64, which measured
                                  // 0.203 s against 0.213 s for 64 x 128 at N = 400

struct XckSpinPlan {
    long long d[2] = {0, 0}, dim = 0, G = 0;
    int n_b[2] = {0, 0};          // 64-wide blocks of each spin's part of the compound index
    int cols = 1;                 // column blocks per tile: 1 or 2
    long long n_tiles = 0;        // cols = 1: n (n + 1) / 2 with n = n_b[0] + n_b[1]
    int n_slabs = 1;
    long long slab_len = 0;       // a multiple of XCK_CHUNK
    size_t lds_bytes = 0;         // left operand | right operand | u of one chunk
    size_t partial_doubles = 0;   // [n_slabs][dim][dim]
};

struct XckSpinTile { int bi, bj, nc; };   // row block, first column block, column blocks (1 .. cols; all of one spin)

// The tiles of the plan in launch order into out (may be null); returns their number
static inline long long xck_spin_tiles(const XckSpinPlan &P, XckSpinTile *out)
{
    const int nb = P.n_b[0] + P.n_b[1];
    long long n = 0;
    for (int bi = 0; bi < nb; ++bi)
        for (int t = 0; t < 2; ++t) {
            const int first = t ? P.n_b[0] : 0, last = first + P.n_b[t];          // the column blocks of spin t
            for (int c0 = first; c0 < last; c0 += P.cols) {
                const int nc = std::min(P.cols, last - c0);
                if (c0 + nc - 1 < bi) continue;                                   // wholly left of the row block: no element with row <= column
                if (out) out[n] = XckSpinTile{bi, c0, nc};
                ++n;
            }
        }
    return n;
}

static inline XckSpinPlan xck_spin_plan(long long d_alpha, long long d_beta, long long G, int cols = XCK_SPIN_COLS)
{
    XckSpinPlan P;
    P.d[0] = d_alpha; P.d[1] = d_beta; P.dim = d_alpha + d_beta; P.G = G;
    P.cols = cols == 1 ? 1 : 2;
    for (int s = 0; s < 2; ++s) P.n_b[s] = (int)((P.d[s] + XCK_TILE - 1) / XCK_TILE);
    P.n_tiles = xck_spin_tiles(P, nullptr);
    xck_slab_cut(P.n_tiles, G, &P.slab_len, &P.n_slabs);
    P.lds_bytes = (size_t)(XCK_CHUNK * XCK_ROW + XCK_CHUNK * (P.cols * XCK_TILE + 16) + XCK_CHUNK) * sizeof(double);
    P.partial_doubles = (size_t)P.n_slabs * (size_t)P.dim * (size_t)P.dim;
    return P;
}

// Block b of the spin-blocked grid: its spin, its first element within that spin's part, and that part's offset in the compound index
static inline void xck_spin_block(const XckSpinPlan &P, int b, int *spin, long long *first_local, long long *offset)
{
    *spin = b >= P.n_b[0] ? 1 : 0;
    *first_local = (long long)(b - (*spin ? P.n_b[0] : 0)) * XCK_TILE;
    *offset = *spin ? P.d[0] : 0;
}

static_assert((XCK_CHUNK * XCK_ROW + XCK_CHUNK * (2 * XCK_TILE + 16) + 2 * XCK_CHUNK) * sizeof(double) <= 64 * 1024, "the static LDS of the kernel build exceeds 64 KB");
