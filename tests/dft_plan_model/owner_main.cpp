// TEST INFRASTRUCTURE: the owner checks of owner_checks.h as a program of its own, so that they can run under AddressSanitizer and
// UndefinedBehaviorSanitizer (build.sh builds it with -fsanitize=address,undefined where the runtime is installed).  Every failure
// position of both buffer sets and the run without a failure, at two shapes and both gga values; exit code 0: all hold.  No GPU code.
#include <cstdio>

#include "owner_checks.h"

int main()
{
    int cases = 0, bad = 0;
    const long long Gs[2] = {1, 129};
    const int Ns[2] = {1, 17};
    for (int shape = 0; shape < 2; ++shape)
        for (int gga = 0; gga < 2; ++gga) {
            for (int set = 0; set < 2; ++set) {
                const int n = set == 0 ? (int)tfdft::GB_COUNT : (int)tfdft::GS_COUNT;
                for (int k = -1; k < n; ++k) {
                    long long o[11];
                    dftm::owner_run(set, Gs[shape], Ns[shape], gga, k, o);
                    ++cases;
                    if (dftm::owner_verdict(n, k, o)) { ++bad; printf("FAILED: set %d G %lld N %d gga %d refused at %d\n", set, Gs[shape], Ns[shape], gga, k); }
                }
            }
            const int rc = dftm::grid_release_check(Gs[shape], Ns[shape], gga);
            ++cases;
            if (rc) { ++bad; printf("FAILED: grid release, G %lld N %d gga %d: step %d\n", Gs[shape], Ns[shape], gga, rc); }
        }
    printf("owner checks: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
