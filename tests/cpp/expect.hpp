// expect.hpp -- the failure counter, EXPECT and the closing line of the stand-alone host programs of this directory.
// tests/host_support.py accepts a run by its exit status and the line "OK: 0 failure(s)", which finish() prints only when
// nothing failed.
#pragma once
#include <cstdio>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// the last statement of main(): `return finish();`
static inline int finish() {
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
