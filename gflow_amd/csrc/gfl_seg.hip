// DAVIS J & F counts of a clip's masks in one launch (gfl_seg_score; include/gflow_hip.h, gflow_amd/segmentation.py).
//
// Per frame six integer counts: |pred & gt|, |pred | gt|, the boundary pixels of pred and of gt, and the boundary pixels of
// either that have a boundary pixel of the other inside the disc dx^2 + dy^2 <= radius^2 -- what the reference's
// db_eval_iou and db_eval_boundary sum (gflow/utils/measures/jaccard.py:14-34, f_boundary.py:15-132: seg2bmap at equal
// size, binary_dilation with disk(bound_pix) and a zero border, boundary * dilated_other).
//
// Grid (64-pixel column tiles, SEG_TH-row tiles, frames).  A workgroup works on bit rows, one 64-bit word per 64 pixels:
//   1. every wave turns 64-pixel row segments of both masks into __ballot words: the tile's rows plus `radius` rows above and
//      radius + 1 below, three words per row (the tile's own columns in the middle one; only the radius + 1 columns beside
//      it are loaded) and the one pixel right of them;
//   2. the boundary words follow from the mask words by shifts and XORs, with the image's last row / column rules;
//   3. a lane whose pixel is a boundary pixel tests, for every dy, the bit range of half-width floor(sqrt(r^2 - dy^2)) of
//      the other mask's boundary row; the counts are popcounts of wave-uniform words and of the ballot of the hits.
// One integer atomic per workgroup and count.  Integer sums: the order never enters the result.
#include "gfl_common.hpp"

namespace gfl {

constexpr int SEG_BLOCK = 256;
constexpr int SEG_WAVES = SEG_BLOCK / 64;
constexpr int SEG_TH = 32;                                  // rows per tile
constexpr int SEG_RMAX = 64;                                // (the halo must fit the word beside the tile's)
constexpr int SEG_MROWS = SEG_TH + 2 * SEG_RMAX + 1;        // mask rows held: one more than boundary rows (the lower neighbour)
constexpr int SEG_BROWS = SEG_TH + 2 * SEG_RMAX;

// bits lo .. hi of a word (clipped to 0 .. 63; empty -> 0)
__device__ __forceinline__ unsigned long long bit_range(int lo, int hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > 63 ? 63 : hi;
    if (lo > hi) return 0ull;
    return (~0ull >> (63 - (hi - lo))) << lo;
}

__global__ void __launch_bounds__(SEG_BLOCK) seg_score_kernel(
        const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, const uint8_t* __restrict__ valid, int T, int H,
        int W, int R, uint32_t* __restrict__ counts) {
    // mask words: [mask][row][0..2 = the three words, 3 = the pixel right of word 2]; boundary words: [mask][row][0..2]
    __shared__ unsigned long long M[2][SEG_MROWS][4];
    __shared__ unsigned long long B[2][SEG_BROWS][3];
    __shared__ int hw[2 * SEG_RMAX + 1];
    __shared__ uint32_t acc[6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * SEG_TH;
    const int m_rows = SEG_TH + 2 * R + 1, b_rows = SEG_TH + 2 * R;
    for (int i = tid; i <= 2 * R; i += SEG_BLOCK) {
        const int dy = i - R, v = R * R - dy * dy;
        int h = (int)sqrtf((float)v);
        while (h * h > v) --h;
        while ((h + 1) * (h + 1) <= v) ++h;
        hw[i] = h;
    }
    for (int t = blockIdx.z; t < T; t += gridDim.z) {
        if (valid && !valid[t]) continue;
        const uint8_t* img[2] = {pred + (size_t)t * H * W, gt + (size_t)t * H * W};
        __syncthreads();                                    // (the previous frame's words are no longer read)
        if (tid < 6) acc[tid] = 0;
        // 1. mask words.  Columns that no boundary bit in reach needs stay zero: a boundary bit at column x reads the mask at
        //    x and x + 1, and the tests reach the columns x0 - R .. x0 + 63 + R
        for (int it = wave; it < m_rows * 3; it += SEG_WAVES) {
            const int r = it / 3, k = it - 3 * r;
            const int y = y0 - R + r, x = x0 - 64 + 64 * k + lane;
            const bool row_in = y >= 0 && y < H;
            const bool need = row_in && x >= x0 - R && x <= x0 + 64 + R && x >= 0 && x < W;
            const bool need_next = row_in && k == 2 && lane == 63 && R == SEG_RMAX && x + 1 < W;
            unsigned long long w[2], c[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const uint8_t* row = img[m] + (size_t)(row_in ? y : 0) * W;
                const bool p = need && row[x] != 0;
                const bool pn = need_next && row[x + 1] != 0;
                w[m] = __ballot(p);
                c[m] = __ballot(pn);
            }
            if (lane == 0) {
                M[0][r][k] = w[0];
                M[1][r][k] = w[1];
                if (k == 2) {
                    M[0][r][3] = c[0] ? 1ull : 0ull;
                    M[1][r][3] = c[1] ? 1ull : 0ull;
                }
            }
        }
        __syncthreads();
        // 2. boundary words: a pixel differs from its right, lower or lower-right neighbour; in the last row only the
        //    right one counts, in the last column only the lower one, the bottom-right pixel never
        for (int it = tid; it < 2 * b_rows * 3; it += SEG_BLOCK) {
            const int m = it / (b_rows * 3), rem = it - m * b_rows * 3;
            const int r = rem / 3, k = rem - 3 * r;
            const int y = y0 - R + r, xb = x0 - 64 + 64 * k;
            unsigned long long b = 0ull;
            if (y >= 0 && y < H) {
                const unsigned long long a = M[m][r][k], an = M[m][r][k + 1] & 1ull;
                const unsigned long long e = (a >> 1) | (an << 63);
                const unsigned long long inner = bit_range(-xb, W - 2 - xb);
                if (y < H - 1) {
                    const unsigned long long s = M[m][r + 1][k], sn = M[m][r + 1][k + 1] & 1ull;
                    const unsigned long long se = (s >> 1) | (sn << 63);
                    const unsigned long long last = bit_range(W - 1 - xb, W - 1 - xb);
                    b = (((a ^ e) | (a ^ s) | (a ^ se)) & inner) | ((a ^ s) & last);
                } else {
                    b = (a ^ e) & inner;
                }
            }
            B[m][r][k] = b;
        }
        __syncthreads();
        // 3. counts
        uint32_t n[6] = {0, 0, 0, 0, 0, 0};                 // inter, uni, n_fg, n_gt, fg_match, gt_match (wave-uniform)
        for (int ty = wave; ty < SEG_TH && y0 + ty < H; ty += SEG_WAVES) {
            const int rc = R + ty;
            const unsigned long long mp = M[0][rc][1], mg = M[1][rc][1];
            const unsigned long long bp = B[0][rc][1], bg = B[1][rc][1];
            n[0] += __popcll(mp & mg);
            n[1] += __popcll(mp | mg);
            n[2] += __popcll(bp);
            n[3] += __popcll(bg);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const unsigned long long own = m == 0 ? bp : bg;
                if (own == 0ull) continue;                  // (uniform)
                bool hit = false;
                if ((own >> lane) & 1ull) {
                    const int o = 1 - m;
                    for (int i = 0; i <= 2 * R && !hit; ++i) {
                        const int h = hw[i];
                        const int a = 64 + lane - h, z = 64 + lane + h;        // bit positions in the row's 192 bits
                        const unsigned long long* w = B[o][ty + i];
                        const unsigned long long f = (w[0] & bit_range(a, z)) | (w[1] & bit_range(a - 64, z - 64)) |
                                                     (w[2] & bit_range(a - 128, z - 128));
                        hit = f != 0ull;
                    }
                }
                n[4 + m] += __popcll(__ballot(hit));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (n[k]) atomicAdd(&acc[k], n[k]);
        }
        __syncthreads();
        if (tid < 6 && acc[tid]) atomicAdd(&counts[(size_t)t * 6 + tid], acc[tid]);
    }
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_seg_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* valid, int T, int H, int W, int radius,
                  uint32_t* counts, gfl_stream_t stream) {
    if (T < 0 || H <= 0 || W <= 0 || radius < 1 || radius > SEG_RMAX) return GFL_ERR_INVALID;
    if (T == 0) return GFL_OK;
    if (!pred || !gt || !counts) return GFL_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)T * 6 * sizeof(uint32_t), s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return GFL_ERR_HIP;
    }
    const dim3 grid((W + 63) / 64, (H + SEG_TH - 1) / SEG_TH, T < 65535 ? T : 65535);
    seg_score_kernel<<<grid, SEG_BLOCK, 0, s>>>(pred, gt, valid, T, H, W, radius, counts);
    return check_launch();
}

}  // extern "C"
