// One LDS stage of a 64 x 64 tile product, shared by sparse.hip (FITC accumulators) and particles.hip (k_*^T Kinv k_* at many points).
// A 256-thread workgroup, 16 results per thread; operands are [SP_KB][SP_T + 1] LDS arrays (k-major, one padding column).
#pragma once
#include <hip/hip_runtime.h>

#define SP_T   64      // tile edge of every matrix product here (a 256-thread workgroup, 16 results per thread)
#define SP_KB  16       // depth of one LDS stage

// One stage of a 64 x 64 tile product, out[row][col] += sum_k A[k][row] * B[k][col], in two forms (MF = false | true):
//   FMA:  a thread owns rows ty + 16 a and columns tx + 16 b, acc[a][b]; k ascending.
//   MFMA: v_mfma_f64_16x16x4_f64.  Wave w = ty >> 2 owns rows 16 w ... 16 w + 15 as four 16 x 16 blocks b; operands are one double per lane,
//         A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15]; a lane holds column tx = lane & 15 of block b in rows
//         (lane >> 4) + 4 a: acc[b][a].  Four k per instruction, instructions in ascending k.
// sp_row / sp_acc say where result (a, b) of a thread sits; its column is tx + 16 b in both forms.
typedef double sp_d4 __attribute__((ext_vector_type(4)));
template <bool MF> static __device__ __forceinline__ int sp_row(int ty, int a) { return MF ? 16 * (ty >> 2) + (ty & 3) + 4 * a : ty + 16 * a; }
template <bool MF> static __device__ __forceinline__ double& sp_acc(double (&acc)[4][4], int a, int b) { return MF ? acc[b][a] : acc[a][b]; }

template <bool MF>
static __device__ __forceinline__ void sp_stage(const double (*A)[SP_T + 1], const double (*B)[SP_T + 1], int tx, int ty, double (&acc)[4][4]) {
    if (MF) {
        const int kq = ty & 3, r = 16 * (ty >> 2) + tx;
#pragma unroll
        for (int kk = 0; kk < SP_KB / 4; ++kk) {
            const double a = A[4 * kk + kq][r];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sp_d4 c = {acc[b][0], acc[b][1], acc[b][2], acc[b][3]};
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, B[4 * kk + kq][16 * b + tx], c, 0, 0, 0);
                acc[b][0] = c.x; acc[b][1] = c.y; acc[b][2] = c.z; acc[b][3] = c.w;
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < SP_KB; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = A[k][ty + 16 * q]; b[q] = B[k][tx + 16 * q]; }
#pragma unroll
        for (int qa = 0; qa < 4; ++qa)
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) acc[qa][qb] = fma(a[qa], b[qb], acc[qa][qb]);
    }
}
