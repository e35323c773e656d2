// TEST INFRASTRUCTURE: the owner checks of owner_checks.h as a program of its own, so that they can run under AddressSanitizer and
// UndefinedBehaviorSanitizer (build.sh builds it with -fsanitize=address,undefined where the runtime is installed).  Every slot's growth,
// every refusal position of the blocks, of the stream / event set and of the event pairs, and the runs without a refusal; exit code 0:
// all hold.  No GPU code.
#include <cstdio>

#include "owner_checks.h"

int main()
{
    int cases = 0, bad = 0;
    auto note = [&](int rc, const char *what, int a, int b) { ++cases; if (rc) { ++bad; printf("FAILED: %s (%d, %d): step %d\n", what, a, b, rc); } };
    for (int slot = 0; slot < tfctx::CB_COUNT; ++slot) note(ctxm::block_growth_check(slot), "block growth, slot", slot, 0);
    for (int k = -1; k < tfctx::CB_COUNT; ++k)
        for (int mode = 0; mode < 4; ++mode) note(ctxm::block_refusal_check(k, mode & 1, mode >> 1), "block refusal at, mode", k, mode);
    const int n = ctxm::Streams::N_STREAMS + ctxm::Streams::N_EVENTS;
    for (int k = -1; k < n; ++k) {
        long long o[13];
        ctxm::streams_run(k, o);
        note(ctxm::streams_verdict(k, o), "stream / event set refused at", k, 0);
    }
    note(ctxm::streams_names_check(), "names of the set", 0, 0);
    for (int k = -1; k < 8; ++k) note(ctxm::event_pairs_check(4, k), "event pairs refused at", k, 0);
    printf("owner checks: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
