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

static inline XckPlan xck_plan(long long dim, long long G)
{
    XckPlan P;
    P.dim = dim; P.G = G;
    P.n_b = (int)((dim + XCK_TILE - 1) / XCK_TILE);
    P.n_tiles = (long long)P.n_b * (P.n_b + 1) / 2;
    const long long want = std::max<long long>(1, (XCK_WG_TARGET + P.n_tiles - 1) / std::max<long long>(1, P.n_tiles));
    const long long most = std::max<long long>(1, G / XCK_SLAB_MIN);              // slabs of at least XCK_SLAB_MIN points
    const long long n = std::min(want, most);
    const long long per = (G + n - 1) / n;
    P.slab_len = std::max<long long>(XCK_CHUNK, (per + XCK_CHUNK - 1) / XCK_CHUNK * XCK_CHUNK);
    P.n_slabs = (int)std::max<long long>(1, (G + P.slab_len - 1) / P.slab_len);
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
