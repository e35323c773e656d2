// TEST INFRASTRUCTURE: the owners of a context's lifetimes (tuna_amd/csrc/tf_ctx_plan.h: the named grow-only blocks, the stream / event
// set of the tensor build, the event pairs of the J/K profile) against a runtime that keeps books and can refuse its k-th request.
// Shared by the library behind tests/test_ctx_plan.py (ctx_model.cpp) and by the stand-alone program that the test also builds with the
// sanitizers (owner_main.cpp).  No GPU code.
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../tuna_amd/csrc/tf_ctx_plan.h"

namespace ctxm {

const int REFUSED = 77;                       // what the runtime returns for the request it refuses
const int MAXB = 256;

// Every block, stream and event is a malloc'ed byte, so that the sanitizers see a leak, a double free and a use after free as well.
struct Book {
    int fail_at = -1, requests = 0, handed = 0, good_frees = 0, bad_frees = 0;   // bad: freed twice, or never handed out
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
    for (int k = book.handed - 1; k >= 0; --k)            // (the newest first: malloc may hand an address out again)
        if (book.block[k] == p && p) {
            if (!book.live[k]) { ++book.bad_frees; return; }
            book.live[k] = false; ++book.good_frees;
            free(p);
            return;
        }
    ++book.bad_frees;
}
struct FakeHandles {
    typedef void *Stream;
    typedef void *Event;
    static int stream_create(Stream *s) { return book_alloc(s, 1); }
    static int event_create(Event *e) { return book_alloc(e, 2); }
    static int timing_event_create(Event *e) { return book_alloc(e, 3); }
    static void stream_destroy(Stream s) { book_free(s); }
    static void event_destroy(Event e) { book_free(e); }
};
typedef tfctx::BuildStreams<FakeHandles> Streams;
typedef tfscf::Blocks<tfctx::CB_COUNT> CtxBlocks;

static int null_slots(const CtxBlocks &b) { int n = 0; for (int k = 0; k < tfctx::CB_COUNT; ++k) n += (!b.p[k] && b.cap[k] == 0) ? 1 : 0; return n; }

// One slot through ensure below / at / above the held size, replace twice, release twice.  0: everything held; else the failing step
static int block_growth_check(int slot)
{
    book = Book();
    CtxBlocks b(book_alloc, book_free);
    if (b.ensure(slot, 100) != 0 || !b.p[slot] || b.cap[slot] != 100 || book.requests != 1) return 1;
    void *first = b.p[slot];
    if (b.ensure(slot, 40) != 0 || b.p[slot] != first || b.cap[slot] != 100 || book.requests != 1) return 2;     // below: kept
    if (b.ensure(slot, 100) != 0 || b.p[slot] != first || book.requests != 1) return 3;                            // at: kept
    if (b.ensure(slot, 101) != 0 || b.cap[slot] != 101 || book.requests != 2 || book.good_frees != 1 || book.leaked() != 1) return 4;   // above: free, then allocate
    if (tfctx::replace(b, slot, 8) != 0 || b.cap[slot] != 8 || book.requests != 3 || book.good_frees != 2) return 5;   // smaller, and still a fresh block
    if (tfctx::replace(b, slot, 8) != 0 || b.cap[slot] != 8 || book.requests != 4 || book.good_frees != 3 || book.leaked() != 1) return 6;
    if (null_slots(b) != tfctx::CB_COUNT - 1) return 7;
    b.release();
    if (null_slots(b) != tfctx::CB_COUNT || book.good_frees != 4 || book.leaked() != 0) return 8;
    b.release();
    return (book.good_frees == 4 && book.bad_frees == 0) ? 0 : 9;
}

// Every slot is filled in turn and the runtime refuses request k (k < 0: none), once through ensure over held blocks (grow = 1: every
// slot holds a smaller block first) and once through replace.  0: the refused slot is {nullptr, 0}, the code is the runtime's, every
// other slot is untouched, and after release nothing is leaked and nothing was freed twice
static int block_refusal_check(int k, int grow, int use_replace)
{
    book = Book();
    CtxBlocks b(book_alloc, book_free);
    const int n = tfctx::CB_COUNT;
    if (grow)
        for (int s = 0; s < n; ++s) if (b.ensure(s, 16) != 0) return 1;
    book.fail_at = k < 0 ? -1 : book.requests + k;
    for (int s = 0; s < n; ++s) {
        const int rc = use_replace ? tfctx::replace(b, s, 64 + s) : b.ensure(s, 64 + s);
        if (s == k) {
            if (rc != REFUSED || b.p[s] || b.cap[s] != 0) return 2;
        } else if (rc != 0 || !b.p[s] || b.cap[s] != (size_t)(64 + s)) return 3;
    }
    if (book.leaked() != (k < 0 || k >= n ? n : n - 1)) return 4;
    b.release();
    if (null_slots(b) != n || book.leaked() != 0 || book.bad_frees != 0) return 5;
    return 0;
}

// create() with the runtime refusing request k (k < 0: none), then destroy() twice.  out = {create's code, requests, handles handed out,
// live after create, leaked after create, non-null handles after create, good frees after destroy, bad frees, leaked, live, non-null
// handles, good frees after a second destroy, requests after a second create on a live set}
static void streams_run(int k, long long out[13])
{
    book = Book();
    book.fail_at = k;
    Streams s;
    auto non_null = [&] { int n = 0; for (void *h : s.streams) n += h ? 1 : 0; for (void *h : s.sev) n += h ? 1 : 0; return n; };
    out[0] = s.create();
    out[1] = book.requests; out[2] = book.handed; out[3] = s.live ? 1 : 0; out[4] = book.leaked(); out[5] = non_null();
    book.fail_at = -1;
    const int before = book.requests;
    if (s.live) (void)s.create();             // a live set is not made again
    out[12] = book.requests - before;
    s.destroy();
    out[6] = book.good_frees; out[7] = book.bad_frees; out[8] = book.leaked(); out[9] = s.live ? 1 : 0; out[10] = non_null();
    s.destroy();
    out[11] = book.good_frees;
}
static inline int streams_verdict(int k, const long long o[13])
{
    const int n = Streams::N_STREAMS + Streams::N_EVENTS;
    if (k >= 0 && k < n)                      // refused at k: the k handles made are destroyed once each inside create(), the set is not live
        return (o[0] == REFUSED && o[1] == k + 1 && o[2] == k && o[3] == 0 && o[4] == 0 && o[5] == 0 && o[6] == k && o[7] == 0 && o[8] == 0 &&
                o[9] == 0 && o[10] == 0 && o[11] == k && o[12] == 0) ? 0 : 1;
    return (o[0] == 0 && o[1] == n && o[2] == n && o[3] == 1 && o[4] == n && o[5] == n && o[6] == n && o[7] == 0 && o[8] == 0 && o[9] == 0 &&
            o[10] == 0 && o[11] == n && o[12] == 0) ? 0 : 1;
}

// the named handles are the handles of the arrays, each a different one
static int streams_names_check()
{
    book = Book();
    Streams s;
    if (s.create() != 0) return 1;
    if (s.cstream() != s.streams[Streams::NSTREAM_MAX]) return 2;
    for (int set = 0; set < 2; ++set)
        if (s.slab_done(set) != s.sev[Streams::NSTREAM_MAX + set] || s.slab_lists(set) != s.sev[Streams::NSTREAM_MAX + 2 + set]) return 3;
    for (int a = 0; a < book.handed; ++a)
        for (int b = 0; b < a; ++b) if (book.block[a] == book.block[b]) return 4;
    s.destroy();
    return book.leaked() == 0 ? 0 : 5;
}

// `pairs` spans with the runtime refusing request k: a pair is made whole or not at all, used events are handed out again after
// `used = 0`, destroy() frees every event once.  0: all of it
static int event_pairs_check(int pairs, int k)
{
    book = Book();
    book.fail_at = k;
    tfctx::EventPairs<FakeHandles> p;
    int made = 0;
    for (int q = 0; q < pairs; ++q) {
        void *a = nullptr, *b = nullptr;
        const bool ok = p.next(a, b);
        if (ok) { ++made; if (!a || !b || a == b) return 1; }
        if (p.ev.size() != (size_t)2 * made || p.used != (size_t)2 * made || book.leaked() != 2 * made) return 2;
    }
    if (k >= 0 && k < 2 * pairs && made == pairs) return 3;
    const int requests = book.requests;
    p.used = 0;
    for (int q = 0; q < made; ++q) { void *a, *b; if (!p.next(a, b) || a != p.ev[2 * q]) return 4; }
    if (book.requests != requests) return 5;
    p.destroy();
    if (book.leaked() != 0 || book.bad_frees != 0 || !p.ev.empty() || p.used != 0) return 6;
    p.destroy();
    return book.bad_frees == 0 ? 0 : 7;
}

}  // namespace ctxm
