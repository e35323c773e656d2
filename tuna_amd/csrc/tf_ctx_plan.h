// tf_ctx_plan.h -- the owners of what a context (tf_ctx, tf_ctx.hip.h) keeps for its whole life: the names of its grow-only device blocks
// and the stream / event sets of the tensor build and of the J/K profile.  Plain C++17, no HIP: the runtime is reached through an `Api`
// type, so tests/ctx_model drives the owners with a counting fake (tests/test_ctx_plan.py).  DESIGN.md section 3.2.
#pragma once
#include <cstddef>
#include <vector>

#include "tf_eigh_plan.h"          // tfscf::Blocks<N>: the owner of N named, grow-only blocks

namespace tfctx {

// ---- the device blocks of context lifetime: slots of tf_ctx::blk.  ensure() grows by free-then-allocate (contents are not kept);
// tf_destroy releases all of them in one call.
enum CtxBlock : int {
    CB_ERI,                                   // the stored tensor: kept across builds (tf_build_eri decides when it is replaced)
    CB_SCR0, CB_SCR1, CB_SCR2,                // scratch of the tensor build's slabs
    CB_MO_POOL,                               // work space of the short-index-first AO->MO transformation (tfmp2::transform_q1)
    CB_JKSTAGE,                               // [2][nd][N][N] + status word: staging buffer of the [J;K] exchange over the ranks
    CB_AGREE,                                 // 16 doubles: decision values summed over the ranks (agree_over_ranks)
    CB_LREC, CB_TUP,                          // per-(La,Lb|Lc,Ld) records and index words of eri_cfact_kernel: fresh for every build
    CB_GTAB,                                  // global-memory tables of the top angular momenta (eri_cfact_kernel<true, true>)
    CB_CSR_PTR, CB_CSR_IDX, CB_CSR_VAL,       // AO-level CSR of the Cartesian -> output map: fresh for every build
    CB_COUNT
};

// a fresh block of `bytes` in `slot`, whatever it held (tables that change with every build)
template <int N> inline int replace(tfscf::Blocks<N> &b, int slot, size_t bytes)
{
    b.drop(slot);
    return b.ensure(slot, bytes);
}

// ---- streams and events of the tensor build (the J/K passes fork onto the same streams): all of them or none.
// Api: types Stream, Event; int stream_create(Stream *), int event_create(Event *) (0: made), void stream_destroy(Stream),
// void event_destroy(Event).
template <class Api> struct BuildStreams {
    static const int NSTREAM_MAX = 8;
    static const int N_STREAMS = NSTREAM_MAX + 1, N_EVENTS = NSTREAM_MAX + 4;
    typename Api::Stream streams[N_STREAMS] = {};   // [0, NSTREAM_MAX): the class launches of a slab, side by side; then cstream
    typename Api::Event sev[N_EVENTS] = {};         // [0, NSTREAM_MAX): one per stream; then slab_done[2], slab_lists[2]
    bool live = false;
    typename Api::Stream cstream() const { return streams[NSTREAM_MAX]; }   // uploads of a slab's index lists (beside the kernels of the previous slab)
    typename Api::Event slab_done(int set) const { return sev[NSTREAM_MAX + set]; }
    typename Api::Event slab_lists(int set) const { return sev[NSTREAM_MAX + 2 + set]; }
    int create()                              // 0: live (made now or earlier); else the code of the create that failed, and nothing is held
    {
        if (live) return 0;
        int rc = 0, ns = 0, ne = 0;
        while (ns < N_STREAMS && (rc = Api::stream_create(&streams[ns])) == 0) ++ns;
        while (rc == 0 && ne < N_EVENTS && (rc = Api::event_create(&sev[ne])) == 0) ++ne;
        if (rc != 0) { undo(ns, ne); return rc; }
        live = true;
        return 0;
    }
    void destroy()
    {
        if (live) undo(N_STREAMS, N_EVENTS);
        live = false;
    }
    void undo(int ns, int ne)
    {
        for (int k = 0; k < ns; ++k) { Api::stream_destroy(streams[k]); streams[k] = typename Api::Stream(); }
        for (int k = 0; k < ne; ++k) { Api::event_destroy(sev[k]); sev[k] = typename Api::Event(); }
    }
};

// ---- (before, after) event pairs of the J/K profile, made on demand.  Api as above, plus int timing_event_create(Event *).
template <class Api> struct EventPairs {
    std::vector<typename Api::Event> ev;
    size_t used = 0;
    bool next(typename Api::Event &before, typename Api::Event &after)   // false: no further pair could be made
    {
        if (used + 2 > ev.size()) {
            typename Api::Event a, b;
            if (Api::timing_event_create(&a) != 0) return false;
            if (Api::timing_event_create(&b) != 0) { Api::event_destroy(a); return false; }
            ev.push_back(a); ev.push_back(b);
        }
        before = ev[used]; after = ev[used + 1];
        used += 2;
        return true;
    }
    void destroy()
    {
        for (typename Api::Event e : ev) Api::event_destroy(e);
        ev.clear(); used = 0;
    }
};

}  // namespace tfctx
