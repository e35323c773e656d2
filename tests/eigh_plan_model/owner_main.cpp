// TEST INFRASTRUCTURE: the owner checks of owner_checks.h as a program of its own, so that they can run under AddressSanitizer and
// UndefinedBehaviorSanitizer (build.sh builds it with -fsanitize=address,undefined where the runtime is installed).  The block sequence
// with every request refused in turn and with none refused, then the state's two forget functions and its release; exit code 0: all
// hold.  No GPU code.
#include <cstdio>

#include "owner_checks.h"

int main()
{
    int cases = 0, bad = 0;
    const int n = eighm::requests_without_refusal();
    for (int k = -1; k < n; ++k) {
        long long per_op[eighm::NOPS * eighm::PER_OP], out[eighm::TOTALS];
        eighm::owner_run(k, per_op, out);
        const int rc = eighm::owner_verdict(k, per_op, out);
        ++cases;
        if (rc) { ++bad; printf("FAILED: request %d refused: check %d\n", k, rc); }
    }
    long long st[eighm::STATE_OUT];
    eighm::state_run(st);
    const int rc = eighm::state_verdict(st);
    ++cases;
    if (rc) { ++bad; printf("FAILED: state: figure %d\n", rc - 1); }
    printf("owner checks: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
