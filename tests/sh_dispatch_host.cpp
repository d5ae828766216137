// What gs_sh_dispatch (csrc/gs_sh.h) answers over a grid of (active degree, row stride), one line each:
// "degree stride verdict D S" -- verdict: invalid (hipErrorInvalidValue), called (f's own return value came back), other; D = S = -1: f did not run.
// Host code only: built and run by tests/test_sh_dispatch_host.py, no device.
#include "gs_sh.h"
#include <cstdio>

int main() {
    for (int deg = -2; deg <= 5; ++deg)
        for (int stride = -1; stride <= 80; ++stride) {
            int d = -1, s = -1;
            const hipError_t e = gs_sh_dispatch(deg, stride, [&](auto D, auto S) {
                d = decltype(D)::value; s = decltype(S)::value ? 1 : 0;
                return hipErrorNotReady;
            });
            printf("%d %d %s %d %d\n", deg, stride, e == hipErrorInvalidValue ? "invalid" : e == hipErrorNotReady ? "called" : "other", d, s);
        }
    return 0;
}
