// isv_pgo_types.h -- the two records the pose-graph host code (isv_pgo_host.h) fills and k_pgo (isv_posegraph.hip) reads.
// Both are memset to zero before their members are set, so that the padding bytes that travel to the device are defined.
#pragma once
#include <cstdint>

struct PgEdge {                  // one residual block
    int32_t kind;                // 0 roll/pitch (a), 1 relative pose (a -> b), 2 loop closure (a = matched keyframe, b = the one that closed)
    int32_t a, b;                // local pose indices
    int32_t fa, fb;              // their free (non-constant) indices, -1 if constant
    int32_t dim, robust, _pad;
    double meas_t[3], meas_R[9], sqrt_info[36];
};

struct PgGraph {                 // offsets of one pose graph into the handle's pools
    int32_t P1, nf, ne, nblk;    // poses, free poses, residual blocks, skyline blocks
    int32_t pose0, free0, edge0, blk0, adj0, col0, vec0, _pad;
    int32_t max_iter, _pad2;
    double huber;
};
