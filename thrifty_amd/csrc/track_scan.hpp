// A segmented scan for an associative operator that is NOT commutative and whose combination needs every slot of
// both partners at once -- what seg_scan (seg_reduce.hpp) cannot carry: it moves eight independent slots at a time.
// The tiles, fragments and slabs are seg_reduce.hpp's: a workgroup scans a tile of kTile positions, one per thread,
// by Hillis-Steele steps through two alternating LDS buffers of N * kTile doubles.
//
// Two operators are stated here, both on 2 x 2 blocks in closed form (Sarkka & Garcia-Fernandez, "Temporal
// parallelization of Bayesian smoothers", 2021):
//   FilterOp  14 doubles (A, b, C sym, eta, J sym), forwards: the Kalman filter of one axis;
//   SmoothOp   9 doubles (E, g, L sym), backwards: the Rauch-Tung-Striebel smoother.
// The tree a position is combined in depends on where it lies in its tile and on nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "seg_reduce.hpp"

// a shuffled input must give the same bytes: no a * b + c may become an fma wherever this is inlined
#pragma clang fp contract(off)

namespace thr {
namespace trk {

using seg::kTile;

// ---------------------------------------------------------------- the filter's element
// e = A00 A01 A10 A11 | b0 b1 | C00 C01 C11 | eta0 eta1 | J00 J01 J11
struct FilterOp {
    static constexpr int N = 14;
    // out = i (x) j, i the earlier rows, j the later ones.  With T = I + C_i J_j and M = inv(T):
    //   A = A_j M A_i,  b = A_j M (b_i + C_i eta_j) + b_j,  C = A_j M C_i A_j' + C_j,
    //   eta = A_i' N (eta_j - J_j b_i) + eta_i,  J = A_i' N J_j A_i + J_i,  N = inv(I + J_j C_i) = M' (C, J symmetric)
    // b is computed as A_j (b_i + M C_i (eta_j - J_j b_i)) + b_j, which is the same number (M (I + C_i J_j) = I): when
    // a state with a large covariance meets a block that holds fresh measurements, T is badly conditioned, and this
    // form lets its error act on the innovation instead of on the whole position
    static __device__ __forceinline__ void combine(const double (&i)[N], const double (&j)[N], double (&o)[N]) {
        const double t00 = 1.0 + (i[6] * j[11] + i[7] * j[12]), t01 = i[6] * j[12] + i[7] * j[13];
        const double t10 = i[7] * j[11] + i[8] * j[12], t11 = 1.0 + (i[7] * j[12] + i[8] * j[13]);
        const double det = t00 * t11 - t01 * t10;
        const double m00 = t11 / det, m01 = -t01 / det, m10 = -t10 / det, m11 = t00 / det;
        // c = M C_i
        const double c00 = m00 * i[6] + m01 * i[7], c01 = m00 * i[7] + m01 * i[8];
        const double c10 = m10 * i[6] + m11 * i[7], c11 = m10 * i[7] + m11 * i[8];
        // d = eta_j - J_j b_i,  u = b_i + c d
        const double d0 = j[9] - (j[11] * i[4] + j[12] * i[5]), d1 = j[10] - (j[12] * i[4] + j[13] * i[5]);
        const double u0 = i[4] + (c00 * d0 + c01 * d1), u1 = i[5] + (c10 * d0 + c11 * d1);
        // X = A_j M,  Y = A_j c
        const double x00 = j[0] * m00 + j[1] * m10, x01 = j[0] * m01 + j[1] * m11;
        const double x10 = j[2] * m00 + j[3] * m10, x11 = j[2] * m01 + j[3] * m11;
        const double y00 = j[0] * c00 + j[1] * c10, y01 = j[0] * c01 + j[1] * c11;
        const double y10 = j[2] * c00 + j[3] * c10, y11 = j[2] * c01 + j[3] * c11;
        // W = A_i' M' = (M A_i)'
        const double w00 = m00 * i[0] + m01 * i[2], w10 = m00 * i[1] + m01 * i[3];
        const double w01 = m10 * i[0] + m11 * i[2], w11 = m10 * i[1] + m11 * i[3];
        // Z = W J_j
        const double z00 = w00 * j[11] + w01 * j[12], z01 = w00 * j[12] + w01 * j[13];
        const double z10 = w10 * j[11] + w11 * j[12], z11 = w10 * j[12] + w11 * j[13];
        o[0] = x00 * i[0] + x01 * i[2];
        o[1] = x00 * i[1] + x01 * i[3];
        o[2] = x10 * i[0] + x11 * i[2];
        o[3] = x10 * i[1] + x11 * i[3];
        o[4] = (j[0] * u0 + j[1] * u1) + j[4];
        o[5] = (j[2] * u0 + j[3] * u1) + j[5];
        o[6] = (y00 * j[0] + y01 * j[1]) + j[6];
        o[7] = (y00 * j[2] + y01 * j[3]) + j[7];
        o[8] = (y10 * j[2] + y11 * j[3]) + j[8];
        o[9] = (w00 * d0 + w01 * d1) + i[9];
        o[10] = (w10 * d0 + w11 * d1) + i[10];
        o[11] = (z00 * i[0] + z01 * i[2]) + i[11];
        o[12] = (z00 * i[1] + z01 * i[3]) + i[12];
        o[13] = (z10 * i[1] + z11 * i[3]) + i[13];
    }
};

// ---------------------------------------------------------------- the smoother's element
// e = E00 E01 E10 E11 | g0 g1 | L00 L01 L11
struct SmoothOp {
    static constexpr int N = 9;
    // out = i (x) j, i the rows nearer the track's start, j the ones after them:
    //   E = E_i E_j,  g = E_i g_j + g_i,  L = E_i L_j E_i' + L_i
    static __device__ __forceinline__ void combine(const double (&i)[N], const double (&j)[N], double (&o)[N]) {
        const double y00 = i[0] * j[6] + i[1] * j[7], y01 = i[0] * j[7] + i[1] * j[8];
        const double y10 = i[2] * j[6] + i[3] * j[7], y11 = i[2] * j[7] + i[3] * j[8];
        o[0] = i[0] * j[0] + i[1] * j[2];
        o[1] = i[0] * j[1] + i[1] * j[3];
        o[2] = i[2] * j[0] + i[3] * j[2];
        o[3] = i[2] * j[1] + i[3] * j[3];
        o[4] = (i[0] * j[4] + i[1] * j[5]) + i[4];
        o[5] = (i[2] * j[4] + i[3] * j[5]) + i[5];
        o[6] = (y00 * i[0] + y01 * i[1]) + i[6];
        o[7] = (y00 * i[2] + y01 * i[3]) + i[7];
        o[8] = (y10 * i[2] + y11 * i[3]) + i[8];
    }
};

template <class Op>
constexpr int scan_lds() { return 2 * Op::N * kTile; }  // doubles of LDS that nc_scan alternates between

// Segmented inclusive scan of the workgroup's kTile positions.  Forwards (BACKWARD = false): v of thread t becomes
// e[lo] (x) ... (x) e[t], lo = the fragment's first position in the tile; `bound` = lo.  Backwards: v becomes
// e[t] (x) ... (x) e[hi - 1], `bound` = hi, one past the fragment's last position in the tile.  One barrier per
// step: the buffer written in step i + 2 was last read in step i, before the barrier of step i + 1.
template <class Op, bool BACKWARD>
__device__ __forceinline__ void nc_scan(double (&v)[Op::N], int t, int bound, double* lds) {
    constexpr int N = Op::N;
    int buf = 0;
    for (int d = 1; d < kTile; d <<= 1) {
        double* b = lds + buf * (N * kTile);
#pragma unroll
        for (int k = 0; k < N; ++k) b[k * kTile + t] = v[k];
        __syncthreads();
        const int u = BACKWARD ? t + d : t - d;
        if (BACKWARD ? u < bound : u >= bound) {  // u stays inside the tile: 0 <= bound <= kTile
            double o[N], r[N];
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = b[k * kTile + u];
            if (BACKWARD) Op::combine(v, o, r); else Op::combine(o, v, r);
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = r[k];
        }
        buf ^= 1;
    }
    __syncthreads();  // the next trip starts writing buffer 0 again
}

}  // namespace trk
}  // namespace thr
