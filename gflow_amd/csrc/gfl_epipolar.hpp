// The epipolar core that the move masks (gfl_epi.hip) and depth and camera (gfl_sfm.hip) share: the cyclic Jacobi, the tail of
// the normalised 8-point fit, the Sampson error, and the exact lower median by radix selection.  Everything is float64; the
// only atomics are integer ones, whose sums do not depend on their order.
#pragma once
#include <cmath>

#include "gfl_common.hpp"

namespace gfl {

// ---------------------------------------------------------------------------------------------------- small dense algebra
// Cyclic Jacobi on a symmetric N x N matrix (upper triangle of M is used and ends as the eigenvalues on the diagonal), V
// ends as the eigenvectors in its columns.  Every index is a compile-time constant after unrolling: inlined into a kernel,
// the matrices live in registers.
template <int N>
__host__ __device__ inline void jacobi_sym(double (&M)[N * N], double (&V)[N * N]) {
#pragma unroll
    for (int i = 0; i < N * N; ++i) V[i] = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) V[i * N + i] = 1.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            diag += fabs(M[p * N + p]);
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += fabs(M[p * N + q]);
        }
        if (!(off > 1e-36 * diag)) break;                        // (also leaves on a NaN)
#pragma unroll
        for (int p = 0; p < N - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = M[p * N + q];
                if (apq != 0.0) {
                    const double theta = (M[q * N + q] - M[p * N + p]) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    M[p * N + p] -= t * apq;
                    M[q * N + q] += t * apq;
                    M[p * N + q] = 0.0;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if (k != p && k != q) {
                            const int kp = k < p ? k * N + p : p * N + k, kq = k < q ? k * N + q : q * N + k;
                            const double akp = M[kp], akq = M[kq];
                            M[kp] = c * akp - s * akq;
                            M[kq] = s * akp + c * akq;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        const double vkp = V[k * N + p], vkq = V[k * N + q];
                        V[k * N + p] = c * vkp - s * vkq;
                        V[k * N + q] = s * vkp + c * vkq;
                    }
                }
            }
        }
    }
}

// the column of V that belongs to the smallest diagonal entry of M (first among equals), without a run-time index
template <int N>
__host__ __device__ inline void smallest_column(const double (&M)[N * N], const double (&V)[N * N], double (&v)[N]) {
    double best = M[0];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = V[i * N];
#pragma unroll
    for (int j = 1; j < N; ++j) {
        const bool less = M[j * N + j] < best;
        best = less ? M[j * N + j] : best;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = less ? V[i * N + j] : v[i];
    }
}

__host__ __device__ inline bool finite9(const double* F) {
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && std::isfinite(F[i]);
    return ok;
}

// The tail of the normalised 8-point fit.  M: the upper triangle of A^T A of the rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1,
// y1, 1] of Hartley-normalised points (x2^T F x1 = 0 with F row-major); (s, cx, cy): the two normalisations,
// T = [s 0 -s cx; 0 s -s cy; 0 0 1].  F = T2^T Fn T1 with Fn the null vector forced to rank 2, ||F||_F = 1, its entry of
// largest magnitude positive.  Returns whether F is finite.
// (The Jacobi runs on a copy declared ahead of V -- free once the arrays are registers: which product of a sum the compiler
// fuses has been seen to follow the order of these declarations, and with this order gfl_epi_fundamental keeps its bits.)
__host__ __device__ __forceinline__ bool fundamental_from_normal(const double (&M)[81], double s1, double c1x, double c1y, double s2,
                                                                 double c2x, double c2y, double (&F)[9]) {
    double A[81], V[81], f[9];
#pragma unroll
    for (int i = 0; i < 81; ++i) A[i] = M[i];
    jacobi_sym<9>(A, V);
    smallest_column<9>(A, V, f);
    // rank 2: drop the smallest singular value, F - (F v) v^T with v the eigenvector of F^T F's smallest eigenvalue
    double G[9], W3[9], v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[i * 3 + j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
    jacobi_sym<3>(G, W3);
    smallest_column<3>(G, W3, v);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fv = f[r * 3] * v[0] + f[r * 3 + 1] * v[1] + f[r * 3 + 2] * v[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) f[r * 3 + j] -= fv * v[j];
    }
    const double t1[9] = {s1, 0.0, -s1 * c1x, 0.0, s1, -s1 * c1y, 0.0, 0.0, 1.0};
    const double t2[9] = {s2, 0.0, -s2 * c2x, 0.0, s2, -s2 * c2y, 0.0, 0.0, 1.0};
    double ft[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) ft[i * 3 + j] = f[i * 3] * t1[j] + f[i * 3 + 1] * t1[3 + j] + f[i * 3 + 2] * t1[6 + j];
    double norm2 = 0.0, big = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double g = t2[i] * ft[j] + t2[3 + i] * ft[3 + j] + t2[6 + i] * ft[6 + j];
            F[i * 3 + j] = g;
            norm2 += g * g;
            big = fabs(g) > fabs(big) ? g : big;                 // (first among equal magnitudes)
        }
    const double scale = (big < 0.0 ? -1.0 : 1.0) / sqrt(norm2);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        F[i] *= scale;
        ok = ok && std::isfinite(F[i]);
    }
    return ok;
}

// The Sampson error as include/gflow_hip.h writes it down: d1 = F h1, d2 = F^T h2, z = h2 . d1, z^2 / (d1x^2 + d1y^2 + d2x^2 +
// d2y^2); sums from the left, every product and sum rounded on its own (no contraction), so that a float64 restatement
// evaluates the same expression.  A zero denominator (the pixel is the epipole on both sides, or F is zero) gives 0.
__host__ __device__ inline double sampson_error(const double* F, double x1, double y1, double x2, double y2) {
#pragma clang fp contract(off)
    const double d1x = (F[0] * x1 + F[1] * y1) + F[2];
    const double d1y = (F[3] * x1 + F[4] * y1) + F[5];
    const double d1z = (F[6] * x1 + F[7] * y1) + F[8];
    const double d2x = (F[0] * x2 + F[3] * y2) + F[6];
    const double d2y = (F[1] * x2 + F[4] * y2) + F[7];
    const double z = (x2 * d1x + y2 * d1y) + d1z;
    const double den = ((d1x * d1x + d1y * d1y) + d2x * d2x) + d2y * d2y;
    return den == 0.0 ? 0.0 : (z * z) / den;
}

// ------------------------------------------------------------------------------------------ exact lower median, M rows
// Radix selection on an order-preserving 64-bit key, 11 bits a pass and 9 in the last.  A pass is the caller's histogram
// kernel (grid (chunks, M): every value of row m whose key agrees with prefix[m] above this pass's digit is counted by digit,
// in LDS bins, and the bins are flushed to the row of `hist`) and then select_kernel.  `hist` is zero before pass 0.
constexpr int SELECT_BLOCK = 256;
constexpr int SELECT_BINS = 2048;                               // 11 bits
constexpr int SELECT_PASSES = 6;
static_assert(SELECT_BINS * sizeof(uint32_t) <= 64 * 1024, "LDS budget");

__host__ __device__ inline int select_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
__host__ __device__ inline int select_width(int pass) { return pass < 5 ? 11 : 9; }

// a double that is not a NaN as an unsigned key that orders like the value
__host__ __device__ inline unsigned long long order_key(double v) {
    const long long b = __builtin_bit_cast(long long, v);       // negative: every bit flipped; else the sign bit set
    return (unsigned long long)b ^ ((unsigned long long)(b >> 63) | (1ull << 63));
}
__host__ __device__ inline double order_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    return __builtin_bit_cast(double, (long long)b);
}

struct Select { uint32_t* hist; unsigned long long* prefix; uint32_t* rank; uint32_t* count; };

inline Select select_carve(Arena& a, int M) {
    Select s;
    s.hist = a.take<uint32_t>("select hist", (size_t)M * SELECT_BINS);
    s.prefix = a.take<unsigned long long>("select prefix", M);
    s.rank = a.take<uint32_t>("select rank", M);
    s.count = a.take<uint32_t>("select count", M);
    return s;
}

// whether `key` is still a candidate in this pass (it agrees with the prefix found so far), and its digit
__device__ __forceinline__ bool select_digit(unsigned long long key, unsigned long long want, int pass, uint32_t& digit) {
    const int shift = select_shift(pass), width = select_width(pass);
    digit = (uint32_t)(key >> shift) & (uint32_t)((1 << width) - 1);
    return (pass == 0 ? 0ull : key >> (shift + width)) == want;
}

// One lane's contribution to the LDS bins.  Neighbours share their leading bits: the lanes that agree with the first active
// lane add once.  Every lane of the wave calls this, in uniform control flow (ballots inside).
__device__ __forceinline__ void select_lane_add(uint32_t* bins, bool active, uint32_t digit, int lane) {
    const unsigned long long any = __ballot(active);
    if (any) {
        const int leader = __ffsll((long long)any) - 1;
        const uint32_t ld = (uint32_t)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(active && digit == ld);
        if (lane == leader) atomicAdd(&bins[ld], (uint32_t)__popcll(same));
        else if (active && digit != ld) atomicAdd(&bins[digit], 1u);
    }
}

// the workgroup's non-empty bins to the row, once every lane has added (the whole workgroup calls this)
__device__ __forceinline__ void select_flush(const uint32_t* bins, uint32_t* __restrict__ row, int pass) {
    __syncthreads();
    const int nbins = 1 << select_width(pass);
    for (int b = threadIdx.x; b < nbins; b += SELECT_BLOCK)
        if (bins[b]) atomicAdd(&row[b], bins[b]);
}

// one workgroup per row: pass 0 learns the number of values (the rank is (count - 1) / 2); the bin that holds the wanted rank
// becomes the next digit of the prefix; the row of counts is zeroed for the next pass.  A row without values is skipped
// after pass 0.  Nothing of prefix, rank or count is read before pass 0 has written it.
static __global__ void __launch_bounds__(SELECT_BLOCK) select_kernel(uint32_t* __restrict__ hist, unsigned long long* __restrict__ prefix,
                                                                     uint32_t* __restrict__ rank, uint32_t* __restrict__ count, int pass) {
    __shared__ uint32_t scan[SELECT_BLOCK];
    const int m = blockIdx.x, tid = threadIdx.x;
    if (pass > 0 && count[m] == 0) return;
    const int width = select_width(pass), nbins = 1 << width, per = nbins / SELECT_BLOCK;   // 8 or 2
    uint32_t* row = hist + (size_t)m * SELECT_BINS;
    // read before the scan's barriers: the one thread that finds the bin stores both after them
    const uint32_t r_in = pass == 0 ? 0u : rank[m];
    const unsigned long long pref = pass == 0 ? 0ull : prefix[m];
    uint32_t c[8], total = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        c[j] = j < per ? row[tid * per + j] : 0u;
        total += c[j];
    }
    scan[tid] = total;
    __syncthreads();
    for (int s = 1; s < SELECT_BLOCK; s <<= 1) {                // inclusive scan
        const uint32_t add = tid >= s ? scan[tid - s] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const uint32_t all = scan[SELECT_BLOCK - 1];
    const uint32_t r = pass == 0 ? (all > 0 ? (all - 1u) / 2u : 0u) : r_in;
    const uint32_t before = scan[tid] - total;
    if (all > 0 && r >= before && r < before + total) {         // exactly one thread
        uint32_t cum = before;
        int bin = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!found && j < per) {
                if (r < cum + c[j]) { bin = j; found = true; }
                else cum += c[j];
            }
        }
        prefix[m] = (pref << width) | (unsigned long long)(tid * per + bin);
        rank[m] = r - cum;
    }
    if (pass == 0 && tid == 0) count[m] = all;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < per) row[tid * per + j] = 0u;
}

inline void select_launch(const Select& s, int M, int pass, hipStream_t st) {
    select_kernel<<<M, SELECT_BLOCK, 0, st>>>(s.hist, s.prefix, s.rank, s.count, pass);
}

// the median of row m after the six passes (NaN for a row without values)
__device__ inline double median_of(const unsigned long long* prefix, const uint32_t* count, int m) {
    return count[m] ? order_unkey(prefix[m]) : (double)NAN;
}

}  // namespace gfl
