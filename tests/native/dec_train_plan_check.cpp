// Stand-alone host check of csrc/dec_train_plan.h, built with -fsanitize=address,undefined and run on the CPU
// (tests/test_decoder_train_host.py): for row counts around every edge of the plan, the slabs cover the rows exactly once, stay within
// the limit, and every (slab, value, channel) index the kernels form lies inside the workspace -- written here into a real buffer of
// the size the library reports, so that a wrong size is a sanitizer error and not only a failed comparison.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dec_train_plan.h"

using namespace ptx;

static int check(long n, int C, int nv)
{
    const TrPlan p = tr_plan(n);
    if (p.S < 1 || p.S > kTrMaxSlabs || p.per < 1) return 1;
    const long slab_rows = (long)p.per * kTrChunk;
    long covered = 0;
    for (int s = 0; s < p.S; ++s) {
        const long left = n - (long)s * slab_rows;
        if (left <= 0) return 2;                            // an empty slab: the merge would divide by zero
        covered += left < slab_rows ? left : slab_rows;
    }
    if (covered != n) return 3;
    const size_t bytes = tr_workspace_bytes(n, C, nv);
    if (bytes != (size_t)p.S * nv * C * sizeof(double)) return 4;
    std::vector<double> ws(bytes / sizeof(double), 0.0);
    for (int s = 0; s < p.S; ++s)
        for (int v = 0; v < nv; ++v)
            for (int c = 0; c < C; c += 63) ws[((size_t)s * nv + v) * C + c] += 1.0;      // the kernels' index formula
    ws[((size_t)(p.S - 1) * nv + (nv - 1)) * C + (C - 1)] += 1.0;
    return 0;
}

int main()
{
    const long edges[] = {1, 2, 255, 256, 257, 511, 512, 513, 20820, 1024l * 256 - 1, 1024l * 256, 1024l * 256 + 1, 1024l * 256 + 257, 2048l * 256, 2048l * 256 + 1,
                          (1l << 24) - 1, 1l << 24};
    for (long n : edges)
        for (int C : {64, 256, 512})
            for (int nv : {1, 2, 9, 10}) {
                const int rc = check(n, C, nv);
                if (rc) { std::printf("n=%ld C=%d nv=%d: check %d failed\n", n, C, nv, rc); return 1; }
            }
    if (tr_workspace_bytes(0, 64, 2) || tr_workspace_bytes((1l << 24) + 1, 64, 2) || tr_workspace_bytes(5, 96, 2) || tr_workspace_bytes(5, 64, 11) ||
        tr_workspace_bytes(5, 64, 0) || tr_workspace_bytes(-1, 64, 2) || tr_workspace_bytes(5, 576, 2)) {
        std::printf("an out-of-range request got a size\n");
        return 1;
    }
    std::printf("dec_train_plan OK\n");
    return 0;
}
