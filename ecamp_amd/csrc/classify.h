// What the classification kernels of classify.hip (the probe: forward, head, loss) and finetune.hip (their backwards) share on the host:
// the limits of the head kernels and the split of a sample's rows over workgroups.
#pragma once
#include "common.h"

constexpr int CLS_MAX_CLASSES = 64;
constexpr int CLS_MAX_GRID = 2048;      // workgroups per launch: beyond it a workgroup takes several items in turn
constexpr int POOL_THREADS = 256;
constexpr int POOL_TARGET_WG = 1024;    // four workgroups per CU (4 x 16-byte accesses per thread in flight) before the row range stops being split further
constexpr int POOL_MAX_CHUNKS = 64;

struct PoolPlan {
    int vec, nv, cw, rows_par, nslab, nchunk, chunk_len;
};

// How `nrow` rows of every sample of x [B, T, D] are spread over workgroups: a 256-thread workgroup covers `cw` 16-byte column vectors x
// `rows_par` row lanes, `nslab` of them cover D, and the rows are cut into `nchunk` chunks of `chunk_len`.  ecamp_pool_norm splits the
// tokens it reads (nrow = t1 - t0), ecamp_pool_norm_bwd the rows it writes (nrow = T).  A function of (B, nrow, D, dtype) alone, so that the
// *_workspace_bytes entries and the launches agree.
static PoolPlan pool_plan(int64_t B, int nrow, int D, int dtype) {
    PoolPlan p;
    p.vec = (dtype == ECAMP_F32) ? 4 : (D % 8 == 0 ? 8 : 4);
    p.nv = D / p.vec;
    p.cw = p.nv < POOL_THREADS ? p.nv : POOL_THREADS;
    p.rows_par = POOL_THREADS / p.cw;
    p.nslab = ceil_div(p.nv, p.cw);
    int64_t want = (POOL_TARGET_WG + B * p.nslab - 1) / (B * p.nslab);
    const int most = ceil_div(nrow, (int64_t)p.rows_par * 4);   // a thread keeps at least four rows of its lane
    if (want > most) want = most;
    if (want > POOL_MAX_CHUNKS) want = POOL_MAX_CHUNKS;
    if (want < 1) want = 1;
    p.chunk_len = ceil_div(nrow, want);
    p.nchunk = ceil_div(nrow, p.chunk_len);
    return p;
}

static bool pool_shape_ok(int64_t B, int32_t T, int32_t D, int32_t t0, int32_t t1, int32_t dtype) {
    return B >= 1 && T >= 1 && D >= 4 && D % 4 == 0 && t0 >= 0 && t0 < t1 && t1 <= T && (dtype == ECAMP_F32 || dtype == ECAMP_BF16);
}
