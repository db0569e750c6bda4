// The vertex-target term (include/mvfit.h: mvfit_vertex_target_loss): squared distance of a problem's vertices to up to four
// weighted target vertex sets, with its vertex gradient.  A problem's vertices are n = 3 nv flat floats; the term is
// separable per float.
//
//   vtgt_kernel<GATED, VEC>  grid (B, vertex_target_blocks(nv)), VT_NT threads.  The floats are taken in pairs (2p, 2p + 1);
//       workgroup y owns pairs [y VT_PAIRS, (y + 1) VT_PAIRS), thread t of it the pairs y VT_PAIRS + u VT_NT + t, u = 0 ..
//       VT_UNROLL - 1, so a wave reads 512 contiguous bytes per load.  A problem's row starts at a multiple of 4 n bytes:
//       8-byte loads (VEC) when n is even and every base is 8-byte aligned, else two 4-byte loads per pair - the same pairs
//       in the same order either way, and a last pair with one float when n is odd.  Per float e: d_k = V[e] - T_k[e] in
//       fp32 for the k with a_k > 0 in ascending k (a row with a_k == 0 is never read), the gradient 2 sum_k a_k d_k and
//       the loss sum_k a_k d_k^2 in float64.  A thread adds its floats in ascending (u, float, k); the wave total is
//       wave_ops.h's wave64_sum, the workgroup's the four wave totals in wave order; one float64 partial per workgroup.
//   vtgt_sum_kernel<GATED>   grid (B), one wave: the problem's partials, lane l those of index l, l + 64, .. in ascending
//       order, then wave64_sum; rounded to fp32 once.
// No atomics and no counters: the second step is an ordinary launch behind the first.  Nothing a problem gets depends on B,
// on its position in the batch or on the other problems.  GATED (the fit's chained rounds): gate[b] == 0 - a finished
// problem, or a stage without the term - ends the workgroup at once; a null gate keeps every problem.
#include "vertex_target.h"

#include <cstdint>

#include "wave_ops.h"

namespace mvfit {

constexpr int VT_NT = 256;
constexpr int VT_UNROLL = 4;
constexpr int VT_PAIRS = VT_NT * VT_UNROLL;       // pairs of floats per workgroup (8 KB of a row)

template <bool GATED> struct VtGate { __device__ __forceinline__ bool off(int) const { return false; } };
template <> struct VtGate<true> {
    const int* gate;
    __device__ __forceinline__ bool off(int b) const { return gate && !gate[b]; }
};

template <bool VEC>
__device__ __forceinline__ float2 vt_load(const float* __restrict__ row, int p, bool two) {
    if (VEC) return *reinterpret_cast<const float2*>(row + 2 * (size_t)p);
    return make_float2(row[2 * (size_t)p], two ? row[2 * (size_t)p + 1] : 0.f);
}

template <bool GATED, bool VEC>
__global__ __launch_bounds__(VT_NT) void vtgt_kernel(const float* __restrict__ verts, int n, int K,
                                                     const float* __restrict__ targets, const float* __restrict__ weights,
                                                     double* __restrict__ partial, float* __restrict__ g_verts,
                                                     VtGate<GATED> gate) {
    __shared__ double sh[VT_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (GATED && gate.off(b)) return;                                  // (uniform)
    const int npairs = (n + 1) >> 1;
    float a[VT_MAX_K];
#pragma unroll
    for (int k = 0; k < VT_MAX_K; ++k) a[k] = k < K ? weights[(size_t)b * K + k] : 0.f;      // (uniform: scalar loads)
    const float* V = verts + (size_t)b * n;
    const float* T = targets + (size_t)b * K * n;
    float* G = g_verts ? g_verts + (size_t)b * n : nullptr;
    const int p0 = blockIdx.y * VT_PAIRS + tid;
    // every load of the thread is issued before the first use: one wait per row instead of one per (pair, row)
    float2 v[VT_UNROLL], t[VT_MAX_K][VT_UNROLL];
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
        const int p = p0 + u * VT_NT;
        v[u] = p < npairs ? vt_load<VEC>(V, p, VEC || 2 * p + 1 < n) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < VT_MAX_K; ++k) {
#pragma unroll
        for (int u = 0; u < VT_UNROLL; ++u) t[k][u] = make_float2(0.f, 0.f);
        if (a[k] > 0.f) {                                              // (uniform)
#pragma unroll
            for (int u = 0; u < VT_UNROLL; ++u) {
                const int p = p0 + u * VT_NT;
                if (p < npairs) t[k][u] = vt_load<VEC>(T + (size_t)k * n, p, VEC || 2 * p + 1 < n);
            }
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < VT_UNROLL; ++u) {
        const int p = p0 + u * VT_NT;
        if (p >= npairs) break;
        const bool two = VEC || 2 * p + 1 < n;
        double gx = 0.0, gy = 0.0, lx = 0.0, ly = 0.0;
#pragma unroll
        for (int k = 0; k < VT_MAX_K; ++k) {
            if (a[k] > 0.f) {                                          // (uniform)
                const double ak = (double)a[k];
                const double dx = (double)(v[u].x - t[k][u].x), dy = (double)(v[u].y - t[k][u].y);
                gx += ak * dx; gy += ak * dy;
                lx += ak * (dx * dx); ly += ak * (dy * dy);
            }
        }
        acc += lx;
        if (two) acc += ly;
        if (G) {
            const float rx = (float)(2.0 * gx), ry = (float)(2.0 * gy);
            if (VEC) *reinterpret_cast<float2*>(G + 2 * (size_t)p) = make_float2(rx, ry);
            else { G[2 * (size_t)p] = rx; if (two) G[2 * (size_t)p + 1] = ry; }
        }
    }
    acc = wave64_sum(acc);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = sh[0];
#pragma unroll
        for (int w = 1; w < VT_NT / 64; ++w) s += sh[w];
        partial[(size_t)b * gridDim.y + blockIdx.y] = s;
    }
}

template <bool GATED>
__global__ __launch_bounds__(64) void vtgt_sum_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ loss,
                                                      VtGate<GATED> gate) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (GATED && gate.off(b)) return;
    double s = 0.0;
    for (int i = lane; i < nblk; i += 64) s += partial[(size_t)b * nblk + i];
    s = wave64_sum(s);
    if (lane == 0) loss[b] = (float)s;
}

int vertex_target_blocks(int nv) { return ((3 * nv + 1) / 2 + VT_PAIRS - 1) / VT_PAIRS; }

template <bool GATED>
static void vt_launch(bool vec, dim3 grid, hipStream_t stream, const float* verts, int n, int K, const float* targets,
                      const float* weights, double* partial, float* g_verts, VtGate<GATED> gate) {
    if (vec) hipLaunchKernelGGL((vtgt_kernel<GATED, true>), grid, dim3(VT_NT), 0, stream, verts, n, K, targets, weights, partial, g_verts, gate);
    else hipLaunchKernelGGL((vtgt_kernel<GATED, false>), grid, dim3(VT_NT), 0, stream, verts, n, K, targets, weights, partial, g_verts, gate);
}

hipError_t launch_vertex_target(const float* verts, int nv, int B, int K, const float* targets, const float* weights,
                                const int* gate, double* partial, float* loss, float* g_verts, hipStream_t stream) {
    const int n = 3 * nv, nblk = vertex_target_blocks(nv);
    const bool vec = n % 2 == 0 && ((reinterpret_cast<uintptr_t>(verts) | reinterpret_cast<uintptr_t>(targets) |
                                     reinterpret_cast<uintptr_t>(g_verts)) & 7) == 0;
    const dim3 grid(B, nblk);
    if (gate) {
        vt_launch<true>(vec, grid, stream, verts, n, K, targets, weights, partial, g_verts, VtGate<true>{gate});
        hipLaunchKernelGGL(vtgt_sum_kernel<true>, dim3(B), dim3(64), 0, stream, (const double*)partial, nblk, loss, VtGate<true>{gate});
    } else {
        vt_launch<false>(vec, grid, stream, verts, n, K, targets, weights, partial, g_verts, VtGate<false>{});
        hipLaunchKernelGGL(vtgt_sum_kernel<false>, dim3(B), dim3(64), 0, stream, (const double*)partial, nblk, loss, VtGate<false>{});
    }
    return hipGetLastError();
}

}  // namespace mvfit
