// isv_chain.h -- block layout of the speed/bias chain elimination of k_build_solve_sb and k_build_solve_st.
// The speed/bias blocks are eliminated from both ends of the window towards the middle frame M = N / 2 (two chains); node i's
// fill couples it to the poses nlo(i, M)..nhi(i, M, N): 0..i+1 for i < M, i-1..N-1 for i > M, every pose for node M.
#pragma once
#include "isv_device_math.h"

DEV int sblk(int I, int J, int N) { return (J * N - J * (J - 1) / 2 + (I - J)) * 36; }   // pose block (I, J), I >= J, of the packed lower block triangle
DEV int pairidx(int a, int b) { return a * (a + 1) / 2 + b; }      // entry (a, b), a >= b, of a packed lower triangle
__host__ __device__ __forceinline__ int nlo(int i, int M) { return i > M ? i - 1 : 0; }
__host__ __device__ __forceinline__ int nhi(int i, int M, int N) { return i < M ? i + 1 : N - 1; }
DEV int npar(int i, int M) { return i < M ? i + 1 : (i > M ? i - 1 : -1); }   // parent of node i in its chain (-1: node M)
// doubles of the fill blocks Y_i of all nodes: [6][9] per pose nlo..nhi of each node, summed in T (k_build_solve_sb's hand-over
// area sums in size_t, k_build_solve_st's scratch in int)
template <class T = int>
__host__ __device__ inline T chain_fill_doubles(int N) {
    const int M = N / 2;
    T o = 0;
    for (int i = 0; i < N; i++) o += (T)(nhi(i, M, N) - nlo(i, M) + 1) * 54;
    return o;
}
