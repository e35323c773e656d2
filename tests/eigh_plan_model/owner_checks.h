// TEST INFRASTRUCTURE: the owner of the eigensolver's grow-only blocks (tfscf::Blocks<N>, tuna_amd/csrc/tf_eigh_plan.h) and the
// eigensolver's state (tfscf::EigState) against a malloc-backed allocator that keeps books and can refuse its k-th request.  Shared by the
// library behind tests/test_eigh_plan.py (eigh_plan.cpp) and by the stand-alone program that the test also builds with the sanitizers
// (owner_main.cpp).  No GPU code.
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../tuna_amd/csrc/tf_eigh_plan.h"

namespace eighm {

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
    for (int k = book.handed - 1; k >= 0; --k)  // (malloc may hand an address out again: the latest block at it is the one meant)
        if (book.block[k] == p && p) {
            if (!book.live[k]) { ++book.bad_frees; return; }
            book.live[k] = false; ++book.good_frees;
            free(p);
            return;
        }
    ++book.bad_frees;
}

// The sequence: grow, keep, shrink (kept) and grow again on slot 0; every slot touched; a drop and a fresh block behind it; a dropped
// empty slot.  kind 0: ensure(slot, bytes), 1: drop(slot)
struct Op { int kind, slot; size_t bytes; };
const int NSLOT = 4;
static const Op SEQ[] = {{0, 0, 100}, {0, 1, 50}, {0, 0, 100}, {0, 0, 40}, {0, 0, 200}, {0, 2, 8}, {0, 3, 16}, {0, 1, 60}, {1, 2, 0}, {0, 2, 32},
                         {1, 2, 0}, {1, 2, 0}, {0, 3, 16}, {0, 3, 17}};
const int NOPS = (int)(sizeof(SEQ) / sizeof(SEQ[0]));
const int PER_OP = 6, TOTALS = 8;

// The allocator refuses request k (k < 0: none) and the sequence goes on.  per_op[i] = {code, requests made so far, slot non-null, its
// capacity, its pointer is the one before the operation, good frees so far}; out = {requests, blocks handed out, live before release,
// good frees after release, bad frees, leaked, non-null or non-zero slots after release, good frees after a second release}
static void owner_run(int k, long long *per_op, long long out[TOTALS])
{
    book = Book();
    book.fail_at = k;
    tfscf::Blocks<NSLOT> own(book_alloc, book_free);
    for (int i = 0; i < NOPS; ++i) {
        const Op &o = SEQ[i];
        void *before = own.p[o.slot];
        int rc = 0;
        if (o.kind == 0) rc = own.ensure(o.slot, o.bytes); else own.drop(o.slot);
        if (own.p[o.slot]) { char *q = (char *)own.p[o.slot]; q[0] = 2; q[own.cap[o.slot] - 1] = 2; }    // the capacity is the block's own
        long long *r = per_op + (size_t)i * PER_OP;
        r[0] = rc; r[1] = book.requests; r[2] = own.p[o.slot] ? 1 : 0; r[3] = (long long)own.cap[o.slot]; r[4] = own.p[o.slot] == before ? 1 : 0;
        r[5] = book.good_frees;
    }
    out[0] = book.requests; out[1] = book.handed; out[2] = book.leaked();
    own.release();
    out[3] = book.good_frees; out[4] = book.bad_frees; out[5] = book.leaked();
    out[6] = 0;
    for (int s = 0; s < NSLOT; ++s) out[6] += (own.p[s] ? 1 : 0) + (own.cap[s] ? 1 : 0);
    own.release();
    out[7] = book.good_frees;
}

// What must hold of owner_run's figures, from a model of the slots' capacities; 0: all of it
static inline int owner_verdict(int k, const long long *per_op, const long long out[TOTALS])
{
    size_t cap[NSLOT] = {};
    int requests = 0, handed = 0, frees = 0;
    for (int i = 0; i < NOPS; ++i) {
        const Op &o = SEQ[i];
        const long long *r = per_op + (size_t)i * PER_OP;
        const bool had = cap[o.slot] > 0;
        int rc = 0;
        bool same = true;
        if (o.kind == 1) { if (had) { ++frees; same = false; } cap[o.slot] = 0; }
        else if (!(had && cap[o.slot] >= o.bytes)) {
            if (had) ++frees;                                     // the old block goes before the request is made
            cap[o.slot] = 0;
            if (requests++ == k) { rc = REFUSED; same = !had; }   // refused: null with capacity 0
            else { cap[o.slot] = o.bytes; ++handed; same = false; }
        }
        if (r[0] != rc || r[1] != requests || r[2] != (cap[o.slot] ? 1 : 0) || r[3] != (long long)cap[o.slot] || (same && r[4] != 1) || r[5] != frees)     // (a new block may lie where the old one lay)
            return 1 + i;
    }
    int live = 0;
    for (int s = 0; s < NSLOT; ++s) live += cap[s] ? 1 : 0;
    if (out[0] != requests || out[1] != handed || out[2] != live) return 100;
    if (out[3] != handed || out[4] != 0 || out[5] != 0 || out[6] != 0 || out[7] != handed) return 101;
    return 0;
}
static int requests_without_refusal()
{
    long long per_op[NOPS * PER_OP], out[TOTALS];
    owner_run(-1, per_op, out);
    return (int)out[0];
}

// EigState: forget_tables() leaves no spin with a valid block start (and no tables), forget_vectors() no start of any kind but the tables
// alone; its two owners free every block once.  out = {after forget_tables: sym_n, sym_prev_n, blk_n[0], blk_n[1], ref_n[0], ref_n[1],
// vcls_n[0], vcls_n[1], jac_prev_n; the same nine after forget_vectors (on a fresh state); cur after both; slots of spin 0 and 1 (ref,
// blk, noccs); blocks handed out, good frees, bad frees, leaked after release(), good frees after a second release()}
const int STATE_OUT = 30;
static void state_run(long long out[STATE_OUT])
{
    book = Book();
    for (int pass = 0; pass < 2; ++pass) {
        tfscf::EigState e(book_alloc, book_free, book_alloc, book_free);
        e.sym_n = 7; e.sym_prev_n = 7; e.jac_prev_n = 7; e.cur = 1;
        for (tfscf::SpinVectors &s : e.spin) { s.ref_n = 7; s.vcls_n = 7; s.blk_n = 7; }
        if (pass == 0) e.forget_tables(); else e.forget_vectors();
        long long *o = out + 9 * pass;
        o[0] = e.sym_n; o[1] = e.sym_prev_n; o[2] = e.spin[0].blk_n; o[3] = e.spin[1].blk_n; o[4] = e.spin[0].ref_n; o[5] = e.spin[1].ref_n;
        o[6] = e.spin[0].vcls_n; o[7] = e.spin[1].vcls_n; o[8] = e.jac_prev_n;
        out[18] = e.cur;
        if (pass == 1) {
            for (int sp = 0; sp < 2; ++sp) { out[19 + 3 * sp] = e.spin[sp].ref_slot; out[20 + 3 * sp] = e.spin[sp].blk_slot; out[21 + 3 * sp] = e.spin[sp].nocc_off; }
            for (int s = 0; s < tfscf::EB_COUNT; ++s) (void)e.dev.ensure(s, 8 + (size_t)s);
            (void)e.pin.ensure(0, 24);
            e.release();
            out[25] = book.handed; out[26] = book.good_frees; out[27] = book.bad_frees; out[28] = book.leaked();
            e.release();
            out[29] = book.good_frees;
        }
    }
}
static inline int state_verdict(const long long o[STATE_OUT])
{
    const long long want[STATE_OUT] = {0, 0, 0, 0, 7, 7, 7, 7, 7,   7, 7, 0, 0, 0, 0, 0, 0, 7,   1,
                                       tfscf::EB_REF0, tfscf::EB_BLK_X0, tfscf::BI_NOCC0, tfscf::EB_REF1, tfscf::EB_BLK_X1, tfscf::BI_NOCC1,
                                       tfscf::EB_COUNT + 1, tfscf::EB_COUNT + 1, 0, 0, tfscf::EB_COUNT + 1};
    for (int k = 0; k < STATE_OUT; ++k) if (o[k] != want[k]) return 1 + k;
    return 0;
}

}  // namespace eighm
