// TEST INFRASTRUCTURE: the owner of the Kohn-Sham grid's buffer sets (tfdft::GridBlocks, tuna_amd/csrc/tf_dft_plan.h) against a
// malloc-backed allocator that keeps books and can refuse its k-th request.  Shared by the library behind tests/test_dft_plan.py
// (dft_plan.cpp) and by the stand-alone program that the test also builds with the sanitizers (owner_main.cpp).  No GPU code.
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../tuna_amd/csrc/tf_dft_plan.h"

namespace dftm {

const int REFUSED = 77;                       // what the allocator returns for the request it refuses
const int MAXB = 64;

struct Book {
    int fail_at = -1, requests = 0, handed = 0, good_frees = 0, bad_frees = 0;   // bad: a block freed twice, or one never handed out
    size_t bytes[MAXB] = {};
    void *block[MAXB] = {};
    bool live[MAXB] = {};
    int leaked() const { int n = 0; for (int k = 0; k < handed; ++k) n += live[k] ? 1 : 0; return n; }
};
static Book book;

static int book_alloc(void **p, size_t bytes)
{
    if (book.requests < MAXB) book.bytes[book.requests] = bytes;
    if (book.requests++ == book.fail_at || book.handed >= MAXB) return REFUSED;
    char *q = (char *)malloc(bytes ? bytes : 1);
    if (!q) return REFUSED;
    q[0] = 1; q[bytes ? bytes - 1 : 0] = 1;    // (both ends are the block's own)
    book.block[book.handed] = q; book.live[book.handed++] = true;
    *p = q;
    return 0;
}
static void book_free(void *p)
{
    for (int k = 0; k < book.handed; ++k)
        if (book.block[k] == p && p) {
            if (!book.live[k]) { ++book.bad_frees; return; }
            book.live[k] = false; ++book.good_frees;
            free(p);
            return;
        }
    ++book.bad_frees;
}

static int set_lengths(int set, long long G, int N, int gga, size_t *len)
{
    if (set == 0) { tfdft::grid_base_lengths(G, N, gga != 0, len); return tfdft::GB_COUNT; }
    tfdft::grid_spin_lengths(G, N, len);
    return tfdft::GS_COUNT;
}
static int non_null(const tfdft::GridBlocks &b) { int n = 0; for (int k = 0; k < tfdft::GridBlocks::MAX; ++k) n += b.p[k] ? 1 : 0; return n; }

// The allocator refuses request k (k < 0: none).  out = {acquire's code, requests, blocks handed out, leaked after acquire, non-null table
// entries after acquire, held(), good frees after release, bad frees, leaked, non-null entries, good frees after a second release}
static void owner_run(int set, long long G, int N, int gga, int k, long long out[11])
{
    book = Book();
    book.fail_at = k;
    size_t len[tfdft::GridBlocks::MAX];
    const int n = set_lengths(set, G, N, gga, len);
    tfdft::GridBlocks own;
    out[0] = own.acquire(len, n, book_alloc, book_free);
    out[1] = book.requests; out[2] = book.handed; out[3] = book.leaked(); out[4] = non_null(own); out[5] = own.held() ? 1 : 0;
    own.release();
    out[6] = book.good_frees; out[7] = book.bad_frees; out[8] = book.leaked(); out[9] = non_null(own);
    own.release();
    out[10] = book.good_frees;
}

// What must hold of owner_run's figures; 0: all of it
static inline int owner_verdict(int n, int k, const long long o[11])
{
    if (k >= 0 && k < n)                      // refused at k: the code is the allocator's, the k blocks are freed once each, the table is null
        return (o[0] == REFUSED && o[1] == k + 1 && o[2] == k && o[3] == 0 && o[4] == 0 && o[5] == 0 && o[6] == k && o[7] == 0 && o[8] == 0 &&
                o[9] == 0 && o[10] == k) ? 0 : 1;
    return (o[0] == 0 && o[1] == n && o[2] == n && o[3] == n && o[4] == n && o[5] == 1 && o[6] == n && o[7] == 0 && o[8] == 0 && o[9] == 0 &&
            o[10] == n) ? 0 : 1;
}

// A whole grid: both sets held, then tfdft::release: G back to 0, every block freed once, a second release frees nothing.  0: all of it
static int grid_release_check(long long G, int N, int gga)
{
    book = Book();
    tfdft::Grid g;
    size_t len[tfdft::GridBlocks::MAX];
    g.G = G; g.N = N; g.gga = gga != 0;
    int n = set_lengths(0, G, N, gga, len);
    if (g.base.acquire(len, n, book_alloc, book_free) != 0) return 1;
    n += set_lengths(1, G, N, gga, len);
    if (g.spin.acquire(len, tfdft::GS_COUNT, book_alloc, book_free) != 0) return 2;
    if (g.spin.acquire(len, tfdft::GS_COUNT, book_alloc, book_free) == 0) return 3;      // (a held set is not acquired again)
    if (g.b(tfdft::GB_PART) != book.block[tfdft::GB_PART] || g.s(tfdft::GS_IO) != book.block[tfdft::GB_COUNT + tfdft::GS_IO]) return 4;
    tfdft::release(g);
    if (g.G != 0 || g.N != 0 || g.base.held() || g.spin.held() || non_null(g.base) || non_null(g.spin)) return 5;
    if (book.good_frees != n || book.bad_frees != 0 || book.leaked() != 0) return 6;
    tfdft::release(g);
    return (book.good_frees == n && book.bad_frees == 0) ? 0 : 7;
}

}  // namespace dftm
