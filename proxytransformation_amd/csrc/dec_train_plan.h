// The row-slab plan of decoder_train.hip's reductions and the size of their workspace: plain C++ (no device code), so that a stand-alone
// host program can walk it under a sanitizer (tests/native/dec_train_plan_check.cpp).
#pragma once
#include <cstddef>

namespace ptx {

constexpr int kTrChunk = 256, kTrMaxSlabs = 1024, kTrMaxVals = 10;
constexpr long kTrMaxRows = 1l << 24;

// rows -> 256-row chunks -> at most 1024 slabs of `per` consecutive chunks each; slab s holds the rows from s * per * 256 on
struct TrPlan { long chunks; int per, S; };

inline TrPlan tr_plan(long n)
{
    TrPlan p;
    p.chunks = (n + kTrChunk - 1) / kTrChunk;
    p.per = (int)((p.chunks + kTrMaxSlabs - 1) / kTrMaxSlabs);
    if (p.per < 1) p.per = 1;
    p.S = (int)((p.chunks + p.per - 1) / p.per);
    return p;
}

// (S, nv, C) doubles; 0 where n, C (a multiple of 64 from 64 to 512) or nv (1 to 10) is out of range
inline size_t tr_workspace_bytes(long n, int C, int nv)
{
    if (n < 1 || n > kTrMaxRows || C < 64 || C > 512 || C % 64 != 0 || nv < 1 || nv > kTrMaxVals) return 0;
    return (size_t)tr_plan(n).S * (size_t)nv * (size_t)C * sizeof(double);
}

}  // namespace ptx
