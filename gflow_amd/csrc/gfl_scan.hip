// Deterministic inclusive scan of doubles (gfl_scan_f64, include/gflow_hip.h): the CDFs the densification and the
// initialisation draw from in the deterministic mode (gflow_amd/trainer.py: sample_pixels,
// gflow_amd/sampling.py: complex_texture_sampling_device), in place of torch.cumsum, which torch classes as
// nondeterministic on the device.
//
// The fold order is a function of n alone: the values are cut into chunks of GFL_SCAN_CHUNK (a workgroup of SCAN_BLOCK
// lanes, SCAN_PER consecutive values per lane).  Inside a chunk: a lane's values in order, then an inclusive scan of the
// lane sums over its wave (shuffles, log steps), then the wave sums in wave order.  Launch 1 leaves every chunk's sum in
// the workspace; launch 2 adds, to every value of chunk c, the sum of the chunk sums 0 .. c-1 (folded by a fixed tree:
// lane l sums the sums l, l + SCAN_BLOCK, ... in order, then the lanes in the same order as above).  Two launches, no
// atomics, no dependence on the grid or the device.
#include "gfl_common.hpp"

namespace gfl {

constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_PER = GFL_SCAN_CHUNK / SCAN_BLOCK;
static_assert(SCAN_PER * SCAN_BLOCK == GFL_SCAN_CHUNK, "a chunk is SCAN_PER values per lane");

// this lane's SCAN_PER values of chunk blockIdx.x (zeros behind n) and their running sums
__device__ __forceinline__ void scan_lane_values(const double* __restrict__ in, int n, double (&v)[SCAN_PER]) {
    const long long base = (long long)blockIdx.x * GFL_SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) v[k] = base + k < n ? in[base + k] : 0.0;
#pragma unroll
    for (int k = 1; k < SCAN_PER; ++k) v[k] += v[k - 1];
}

__global__ void __launch_bounds__(SCAN_BLOCK) scan_chunk_sums_kernel(const double* __restrict__ in, int n,
                                                                     double* __restrict__ chunk_sum) {
    __shared__ double wsum[SCAN_BLOCK / 64];
    double v[SCAN_PER];
    scan_lane_values(in, n, v);
    double total;
    block_scan_excl<SCAN_BLOCK>(v[SCAN_PER - 1], wsum, total);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_BLOCK) scan_apply_kernel(const double* __restrict__ in, int n,
                                                                const double* __restrict__ chunk_sum, double* __restrict__ out) {
    __shared__ double wsum[SCAN_BLOCK / 64];
    // the sum of the chunks in front of this one: lane l folds sums l, l + SCAN_BLOCK, ... in order, then the lanes
    double front = 0.0;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += SCAN_BLOCK) front += chunk_sum[c];
    double offset;
    block_scan_excl<SCAN_BLOCK>(front, wsum, offset);
    double v[SCAN_PER];
    scan_lane_values(in, n, v);
    double dummy;
    const double lane_front = offset + block_scan_excl<SCAN_BLOCK>(v[SCAN_PER - 1], wsum, dummy);
    const long long base = (long long)blockIdx.x * GFL_SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k)
        if (base + k < n) out[base + k] = lane_front + v[k];
}

}  // namespace gfl

using namespace gfl;

extern "C" {

static inline int scan_chunks(int n) { return (n + GFL_SCAN_CHUNK - 1) / GFL_SCAN_CHUNK; }

size_t gfl_scan_f64_workspace_bytes(int n) {
    if (n < 0) return 0;
    return (size_t)(scan_chunks(n) > 0 ? scan_chunks(n) : 1) * sizeof(double);
}

int gfl_scan_f64(const double* in, int n, double* out, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (n < 0 || (n > 0 && (!in || !out || !workspace))) return GFL_ERR_INVALID;
    if (n == 0) return GFL_OK;
    if (workspace_bytes < gfl_scan_f64_workspace_bytes(n)) return GFL_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* sums = (double*)workspace;
    const int chunks = scan_chunks(n);
    scan_chunk_sums_kernel<<<chunks, SCAN_BLOCK, 0, s>>>(in, n, sums);
    scan_apply_kernel<<<chunks, SCAN_BLOCK, 0, s>>>(in, n, sums, out);
    return check_launch();
}

}  // extern "C"
