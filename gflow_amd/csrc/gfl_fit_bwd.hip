// Fused fit iteration, stage 4: the backward of the compositing -- back to front over the sorted per-tile lists, one
// 48-byte row of raw moments per (splat, tile) pair, no global atomics -- and, in iterations that cannot move the camera,
// the fold of the loss partials + the depth-affine step in one of its workgroups (loss_tail over LossTail, fold_loss_partials
// and finish_iteration, gfl_fit.hpp).  Block plan, alive box and the checkpoints' layout: gfl_fit_blend.hpp.
#include "gfl_fit_blend.hpp"

namespace gfl {

// gradient terms of one (pixel, splat) pair; branch-free: a lane that does not see the splat uses
// alpha = 0 (T, S unchanged, every term exactly 0).  v = s0..s4 (moments, below) do df0..3
__device__ __forceinline__ void blend_bwd_terms(const float4& p0, const float4& p1, const float4& p2, float fx, float fy,
                                                bool valid, float alpha, float G, float g0, float g1, float g2, float g3,
                                                float& T, float& S, float (&v)[10]) {
    const float a_eff = valid ? alpha : 0.f;
    const float rom = __builtin_amdgcn_rcpf(1.f - a_eff);
    T = T * rom;
    const float h = fmaf(g0, p1.z, fmaf(g1, p1.w, fmaf(g2, p2.x, g3 * p2.y)));
    const float dalpha = valid ? fmaf(T, h, -(S * rom)) : 0.f;
    const float w = a_eff * T;
    S = fmaf(h, w, S);
    v[6] = w * g0; v[7] = w * g1; v[8] = w * g2; v[9] = w * g3;
    const float dx = p0.x - fx, dy = p0.y - fy;
    v[5] = G * dalpha;
    const float dpow = p1.y * v[5];
    const float mx = -dx * dpow, my = -dy * dpow;
    // raw moments; the conic (A, B, C) is the same for every pixel of the splat, so the per-splat
    // kernel finishes them after the sums: du = A s0 + B s1, dv = C s1 + B s0, dA = s2 / 2,
    // dB = s3, dC = s4 / 2  (six VALU ops fewer per (splat, 8x8 block) unit than forming them here)
    v[0] = mx;
    v[1] = my;
    v[2] = dx * mx;
    v[3] = dx * my;
    v[4] = dy * my;
}

#ifdef GFL_TRACE
// analysis build only (make TRACE=1): per-tile timeline of the backward blend
__device__ long long g_bwd_trace[16384 * 8];
#endif
template <int B = 256>
__device__ void loss_tail(const LossTail& t) {
    constexpr int NV = 5;                   // mse, ssim, depth, d/da, d/db
    __shared__ float red[B / 64][NV];
    __shared__ float ge[NV];
    AffineRegs regs = {};
    request_affine(t, regs);
    float acc[NV] = {0.f, 0.f, 0.f, 0.f, 0.f};
    fold_loss_partials<B>(t.p_ssim, t.n_ssim, t.p_grad, t.n_grad, acc);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float s = wave_sum_to_lane63(acc[k]);
        if (lane == 63) red[wid][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        float x = 0.f;
#pragma unroll
        for (int w = 0; w < B / 64; ++w) x += red[w][threadIdx.x];
        ge[threadIdx.x] = x;
        t.sums[threadIdx.x] = x;            // sums[0..4] as gfl_loss_fwd_bwd documents
    }
    if (threadIdx.x >= NV && threadIdx.x < NV + 3) t.sums[threadIdx.x] = 0.f;
    if (threadIdx.x >= 16 && threadIdx.x < 28) t.d_extr_out[threadIdx.x - 16] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) finish_iteration(t, regs, ge + 3, [] {});
}

// DET (GFL_FIT_DETERMINISTIC): the four waves do not add their sums into one row with LDS float atomics, in whatever order they
// arrive; each leaves its sums in a row of its own 8x8 block with plain stores (one lane per component and splat: the
// reduce-scatter hands each component to one lane) and the tile folds the four rows in block order, ((b0 + b1) + b2) + b3.
// Rows by BLOCK, not by wave or SIMD: which wave walks which block depends on where the dispatcher put the waves (plan_ok).
// Fewer splats per batch (FBB_DET) keep the four rows inside the LDS that eight resident workgroups per CU leave.
//
// SUMS: how many of the ten per-pair sums somebody reads.  10: the first frame.  7: later frames, whose colours are frozen
// (freeze_rgb, trainer.py:537-540) -- the three colour sums are neither formed nor reduced (18 VALU ops in the wave
// reduce-scatter instead of 27 per unit).  6: the camera-only stage (freeze_all_splats) -- every splat gradient is zeroed
// afterwards, and the pose gradient needs only the five moments and the depth feature's gradient (16 ops).
template <int SUMS, bool DET = false>
__global__ void __launch_bounds__(256, 8) fused_blend_bwd_kernel(const float* __restrict__ rec,
                                                              const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ tile_range, float bg, int W,
                                                              int H, int gx, const float* __restrict__ final_T,
                                                              const int32_t* __restrict__ n_contrib,
                                                              const float* __restrict__ d_out,
                                                              float* __restrict__ pair_grad, TileQueue queue,
                                                              int32_t* __restrict__ tile_work,
                                                              const float* __restrict__ ckpt,
                                                              const float* __restrict__ render, LossTail ltail, int gy,
                                                              const int32_t* __restrict__ wide_off, long long wide_base,
                                                              const int32_t* __restrict__ stamp_ptr) {
    // (see LossTail.  The workgroup that holds the LAST pre-assigned slot of queue 0 does it before its first item: ~3 us
    //  that the seven other workgroups of its queue absorb.  A workgroup of its own behind the others only started when one
    //  of them -- all persistent -- had finished: +1 us at the end of the launch.)
    if (ltail.enabled && blockIdx.x == gridDim.x - queue.nq) loss_tail(ltail);
    // No global atomics: the four waves of the tile combine their per-splat sums in LDS and the tile writes ONE 48-byte row per
    // (splat, tile) pair with plain stores -- round 5: not at the pair's list position (the per-splat launch then needed a table
    // of positions, written by the tile sort from a gather of the records, and gathered rows scattered over 12.7 MB: 41 MB of
    // traffic, docs/history.md section 5) but at row g * SLOT_MAX + (the tile's index in the splat's own tile rectangle), which the
    // per-splat launch computes for itself and reads as ONE contiguous run per splat.  The scattered side of the exchange is
    // now the stores of this kernel, which is bound by instruction issue and does not wait for them.  A row carries the number
    // of the forward it belongs to (FitWs.stamp) in its eleventh float: pairs nobody walks -- behind the tile's deepest
    // contributor -- need no zero row.
    constexpr int NB = DET ? FBB_DET : FBB;          // splats staged per batch
    constexpr int NACC = DET ? 4 : 1;                // rows of sums per staged splat
    static_assert(!DET || NACC * NB * REC == 3 * 4 * 256, "the deterministic rows are cleared with three float4 per lane");
    __shared__ RecLDS recs[NB];
    __shared__ int32_t s_gid[NB];
    __shared__ float acc[NACC][NB][REC];
    __shared__ unsigned char s_mask[NB];
    __shared__ int32_t s_max_last;
    __shared__ int32_t s_ticket;
    __shared__ int32_t s_simd[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the component this lane adds into acc[][] (SUMS 6 / 7: the last value is the depth feature's gradient, column 9)
    const int comp_own = reduce_scatter_component<SUMS>(lane);
    const int comp = (SUMS != 10 && comp_own == SUMS - 1) ? 9 : comp_own;
    // block plan (gfl_fit_blend.hpp): which 8x8 block of a tile this wave walks follows from the SIMD it sits on
    const int simd = wave_simd();
    const bool simd_ok = simds_distinct(s_simd, simd);
  for (bool first = true;; first = false) {
    const TileItem item = next_item(queue, &s_ticket, first, HEAVY_PARTS, gridDim.x);
    const int tile = item.tile;
    if (tile < 0) break;
    // (the segments of a heavy first tile turning the plan by one SIMD each was measured slower: tools/experiments/README.md)
    const int blk = plan_block(item.plan, simd, simd_ok, wave);          // the 8x8 block of the tile this wave walks
    const int tx = tile % gx, ty = tile / gx;
    const int px = tx * GFL_TILE + (blk & 1) * 8 + (lane & 7);
    const int py = ty * GFL_TILE + (blk >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float fx = pixf(px), fy = pixf(py);
    const int start = tile_range[2 * tile], end = tile_range[2 * tile + 1];
    const int total = end - start;
    const int parts = item.part >= 0 ? heavy_parts(total) : 1;
    if (item.part >= parts) continue;                // this tile has fewer segments
    const int seg = heavy_seg(total, parts);
    const bool last_part = item.part < 0 || item.part == parts - 1;      // the farthest segment (or the whole tile)
    int units = 0;
#ifdef GFL_TRACE
    const long long trace_t0 = wall_clock64();
    int trace_lanes = 0;
#endif

    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, T = 1.f, S = 0.f;
    int last = 0;
    if (inside) {
        const size_t pix = (size_t)py * W + px, plane = (size_t)H * W;
        last = n_contrib[pix];
        g0 = d_out[pix]; g1 = d_out[plane + pix]; g2 = d_out[2 * plane + pix]; g3 = d_out[3 * plane + pix];
        if (last_part) {
            T = final_T[pix];
            S = T * bg * (g0 + g1 + g2 + g3);
        } else {
            // state in front of this segment's far boundary, from the forward checkpoint: T as it
            // was there and S = sum_c g_c * (everything blended behind it) = sum_c g_c * (out_c - C_c)
            float C[4];
            ckpt_load(ckpt_at(ckpt, item.queue, item.part) + tile_place(blk, lane), T, C);
            S = g0 * (render[pix] - C[0]) + g1 * (render[plane + pix] - C[1]) +
                g2 * (render[2 * plane + pix] - C[2]) + g3 * (render[3 * plane + pix] - C[3]);
        }
    }
    if (tid == 0) s_max_last = 0;
    __syncthreads();
    const unsigned long long alive0 = __ballot(inside);
    const int px0w = tx * GFL_TILE + (blk & 1) * 8, py0w = ty * GFL_TILE + (blk >> 1) * 8;
    const int wave_last = wave_max(last);
    if (lane == 0) atomicMax(&s_max_last, wave_last);
    __syncthreads();
    const int depth_n = min(total, (int)s_max_last);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // this item walks list positions hi-1 down to lo
    const int lo = item.part > 0 ? item.part * seg : 0;
    const int hi = last_part ? depth_n : min((item.part + 1) * seg, depth_n);

    const int stamp = *stamp_ptr;
    for (int r0 = 0; r0 < hi - lo; r0 += NB) {
        const int pos_t = tid < NB ? hi - 1 - r0 - tid : -1;           // slot tid <-> list position pos_t
        __syncthreads();
        if (pos_t >= lo) {
            const int g = ids[start + pos_t];
            const float4* r4 = reinterpret_cast<const float4*>(rec + (size_t)g * REC);
            const float4 p0 = r4[0], p1 = r4[1], p2 = r4[2];
            recs[tid].p0 = p0; recs[tid].p1 = p1; recs[tid].p2 = p2;
            s_gid[tid] = g;
            s_mask[tid] = (unsigned char)block_mask(p0, p1, p2.z, tx * GFL_TILE, ty * GFL_TILE);
        }
        if constexpr (DET) {
            float4* az = reinterpret_cast<float4*>(&acc[0][0][0]);
            az[tid] = zero4; az[tid + 256] = zero4; az[tid + 512] = zero4;
        } else if (tid < NB) {
            float4* az = reinterpret_cast<float4*>(&acc[0][tid][0]);
            az[0] = zero4; az[1] = zero4; az[2] = zero4;
        }
        __syncthreads();
        const int cnt = min(NB, hi - lo - r0);
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int slot = c0 + lane;
            const int spos = hi - 1 - r0 - slot;
            bool hit = slot < cnt && spos < wave_last && ((s_mask[slot] >> blk) & 1);
            {
                // as in the forward pass: only the pixels whose last contributor lies at or behind this group of 64
                // positions can receive anything from it; splats that do not reach their bounding box are skipped
                // before their alpha is evaluated (the test of block_mask on a smaller box)
                const unsigned long long alive = __ballot(last > hi - 1 - r0 - c0 - 63);
                if (alive != alive0 && alive != 0ull) cull_to_alive_box(hit, alive, recs[slot], px0w, py0w);
            }
            unsigned long long bits = __ballot(hit);
            while (bits) {
                const int j = c0 + (int)__builtin_ctzll(bits);
                bits &= bits - 1;
                const int pos = hi - 1 - r0 - j;
                const float4 p0 = recs[j].p0, p1 = recs[j].p1, p2 = recs[j].p2;
                float alpha, G;
                const bool valid = splat_alpha2(p0, p1, fx, fy, alpha, G) && (pos < last);
                if (__ballot(valid) == 0ull) continue;
#ifdef GFL_TRACE
                trace_lanes += __popcll(__ballot(valid));
#endif
                ++units;                     // wave-uniform: work feedback for the tile scheduler
                // (an interleaved two-splat version of this body was measured slower, twice)
                float v[10];
                blend_bwd_terms(p0, p1, p2, fx, fy, valid, alpha, G, g0, g1, g2, g3, T, S, v);
                float s[SUMS];               // the sums somebody reads: v[0 .. SUMS - 2] and, last, v[9] (SUMS)
#pragma unroll
                for (int k = 0; k < SUMS; ++k) s[k] = v[k < SUMS - 1 ? k : 9];
                const float mine = wave_reduce_scatter<SUMS>(s, lane);
                if constexpr (DET) {
                    if (comp >= 0) acc[blk][j][comp] = mine;
                } else {
                    if (comp >= 0) atomicAdd(&acc[0][j][comp], mine);
                }
            }
        }
        __syncthreads();
        if (pos_t >= lo) {
            // the pair's row: the tile's index inside the splat's tile rectangle (tile_rect of the staged u, v, radius: what the
            // binning walked and the per-splat launch will walk)
            const int g = s_gid[tid];
            const float4 p0 = recs[tid].p0;
            int x0, x1, y0, y1;
            tile_rect(p0.x, p0.y, __float_as_int(recs[tid].p2.w), gx, gy, x0, x1, y0, y1);
            const int nx = x1 - x0, j = (ty - y0) * nx + (tx - x0);
            long long row = (long long)g * SLOT_MAX + j;
            if (nx * (y1 - y0) > SLOT_MAX) {
                const int off = wide_off[g];
                row = off >= 0 ? wide_base + off + j : -1;
            }
            if (row >= 0) {
                float4* o = reinterpret_cast<float4*>(pair_grad + (size_t)row * PG);
                if constexpr (DET) {
                    float4 s[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float4 b0 = reinterpret_cast<const float4*>(&acc[0][tid][0])[k];
                        const float4 b1 = reinterpret_cast<const float4*>(&acc[1][tid][0])[k];
                        const float4 b2 = reinterpret_cast<const float4*>(&acc[2][tid][0])[k];
                        const float4 b3 = reinterpret_cast<const float4*>(&acc[3][tid][0])[k];
                        s[k] = make_float4(((b0.x + b1.x) + b2.x) + b3.x, ((b0.y + b1.y) + b2.y) + b3.y,
                                           ((b0.z + b1.z) + b2.z) + b3.z, ((b0.w + b1.w) + b2.w) + b3.w);
                    }
                    o[0] = s[0]; o[1] = s[1];
                    o[2] = make_float4(s[2].x, s[2].y, __int_as_float(stamp), 0.f);
                } else {
                    const float4* a4 = reinterpret_cast<const float4*>(&acc[0][tid][0]);
                    o[0] = a4[0]; o[1] = a4[1];
                    o[2] = make_float4(a4[2].x, a4[2].y, __int_as_float(stamp), 0.f);
                }
            }
        }
    }
    // work feedback for the next iteration's schedule, per 8x8 block (gfl_sched.hpp)
    if (lane == 0) atomicAdd(&tile_work[4 * tile + blk], units + 1);
#ifdef GFL_TRACE
    if (lane == 0 && tile < 2048) {
        const unsigned hw = wave_hw_id(), xcc = wave_xcc_id();
        long long* tr = g_bwd_trace + (size_t)(tile + (last_part ? 0 : 2048 * (1 + item.part))) * 8;
        if (wave == 0) {
            tr[0] = trace_t0; tr[1] = wall_clock64();
            tr[2] = ((long long)total << 32) | (unsigned)depth_n;
            tr[3] = ((long long)(xcc & 15) << 32) | hw;
        }
        tr[4 + wave] = ((long long)(trace_lanes | simd << 28) << 32) | (unsigned)units;   // bits 60-61: this wave's SIMD
    }
#endif
  }
}

// ---- launcher (gfl_fit.hpp).  sums: 10 / 7 / 6 (see the kernel); the deterministic instantiations with the state's flag
void launch_blend_bwd(const gfl_fit_state* st, float bg, int gx, int gy, int grid, int sums, const float* d_out, const TileQueue& q,
                      const FitWs& w, const LossTail& lt, hipStream_t s) {
    auto kern = sums == 6 ? fused_blend_bwd_kernel<6> : (sums == 7 ? fused_blend_bwd_kernel<7> : fused_blend_bwd_kernel<10>);
    if (st->flags & GFL_FIT_DETERMINISTIC)
        kern = sums == 6 ? fused_blend_bwd_kernel<6, true>
                         : (sums == 7 ? fused_blend_bwd_kernel<7, true> : fused_blend_bwd_kernel<10, true>);
    kern<<<grid, 256, 0, s>>>(st->rec, st->ids, st->tile_range, bg, st->W, st->H, gx, st->final_T, st->n_contrib, d_out, w.pair_grad,
                              q, w.sched.work, w.ckpt, st->render, lt, gy, w.wide_off, w.wide_base, w.stamp);
}

#ifdef GFL_TRACE
int read_bwd_trace(long long* out, int n_tiles) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_trace), (size_t)n_tiles * 8 * sizeof(long long));
}
#endif

}  // namespace gfl
