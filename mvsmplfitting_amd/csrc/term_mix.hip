// The term mix (include/mvfit.h: mvfit_set_term_mix): the two kernels that let one closure round carry a weighted sum of the
// scene, silhouette, vertex-target and scan terms.  The terms' own kernels and the dense pull-back run unchanged; these stand
// between them.
//
//   term_mix_cotangent_kernel<GATED, VEC>  grid (B, term_mix_blocks(nv)), TM_NT threads.  A problem's n = 3 nv floats are flat
//       and taken in pairs (2p, 2p + 1) exactly as vtgt_kernel takes them: workgroup y owns pairs [y TM_PAIRS, (y + 1)
//       TM_PAIRS), thread t the pairs y TM_PAIRS + u TM_NT + t, so a wave reads 512 contiguous bytes per load.  8-byte loads
//       (VEC) when n is even and every base is 8-byte aligned, else two 4-byte loads per pair in the same pair order.  Per
//       float g = (fl32(lam_sil g_sil) + fl32(lam_vt g_vt)) + fl32(lam_scan g_scan), rounded products and rounded adds in the
//       order silhouette, vertex targets, scan; a component with share 0 is skipped (never read, not added).  Thread 0 of
//       workgroup 0 writes L_v = fp32((double(lam_sil) L_sil + double(lam_vt) L_vt) + double(lam_scan) L_scan) - the products
//       are exact in float64 - and, when asked, the four parts and their sum.
//   term_mix_record_kernel<GATED>  grid (B), one thread per float of an SdfAdj.  In float64, every operation rounded on its
//       own: Q = lam_sc (S_sc S_sc) + S_v S_v, S = fp32(sqrt(Q)), entry e = fp32(((lam_sc S_sc) a_sc[e] + S_v a_v[e]) /
//       sqrt(Q)); Q < FLT_MIN: an all-zero record, as vjp_record_kernel writes it.  With lam_sc = 1 and S_v = 0 every step is
//       exact: the scene record passes through bit for bit.
// No atomics, no scratch, no host work; nothing a problem gets depends on B, on its position or on the other problems.
// GATED (the fit's chained rounds): gate[b] == 0 ends the workgroup at once, its rows keep what they held.
#include "term_mix.h"

#include <cstdint>

#include "mvfit_device.h"

#pragma clang fp contract(off)

namespace mvfit {

constexpr int TM_NT = 256;
constexpr int TM_UNROLL = 4;
constexpr int TM_PAIRS = TM_NT * TM_UNROLL;       // pairs of floats per workgroup (8 KB of a row)
constexpr int TM_REC = (int)(sizeof(SdfAdj) / sizeof(float));      // floats of a record: S first
constexpr int TM_REC_NT = (TM_REC + 63) / 64 * 64;

template <bool GATED> struct TmGate { __device__ __forceinline__ bool off(int) const { return false; } };
template <> struct TmGate<true> {
    const int* gate;
    __device__ __forceinline__ bool off(int b) const { return gate && !gate[b]; }
};

template <bool VEC>
__device__ __forceinline__ float2 tm_load(const float* __restrict__ row, int p, bool two) {
    if (VEC) return *reinterpret_cast<const float2*>(row + 2 * (size_t)p);
    return make_float2(row[2 * (size_t)p], two ? row[2 * (size_t)p + 1] : 0.f);
}

// (0, L_sil, L_vt, L_scan) or (S_sc^2, L_sil, L_vt, L_scan) and the weighted sum, the products exact in float64 and the adds in
// this order; the scan's add is made only with a scan share > 0: the sums of a mix without it keep their bits
__device__ __forceinline__ void tm_write_parts(float* __restrict__ parts, float* __restrict__ sums, int b, float lam_sc, float p_sc,
                                               float lam_sil, float p_sil, float lam_vt, float p_vt, float lam_scan, float p_scan) {
    parts[(size_t)b * 4 + 0] = p_sc; parts[(size_t)b * 4 + 1] = p_sil; parts[(size_t)b * 4 + 2] = p_vt; parts[(size_t)b * 4 + 3] = p_scan;
    double s = ((double)lam_sc * (double)p_sc + (double)lam_sil * (double)p_sil) + (double)lam_vt * (double)p_vt;
    if (lam_scan > 0.f) s = s + (double)lam_scan * (double)p_scan;
    sums[b] = (float)s;
}

template <bool GATED, bool VEC>
__global__ __launch_bounds__(TM_NT) void term_mix_cotangent_kernel(int n, float lam_sil, const float* __restrict__ g_sil,
                                                                   const float* __restrict__ L_sil, float lam_vt,
                                                                   const float* __restrict__ g_vt, const float* __restrict__ L_vt,
                                                                   float lam_scan, const float* __restrict__ g_scan,
                                                                   const float* __restrict__ L_scan, float* __restrict__ g,
                                                                   float* __restrict__ L_v, float* __restrict__ parts,
                                                                   float* __restrict__ sums, TmGate<GATED> gate) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (GATED && gate.off(b)) return;                                  // (uniform)
    const int npairs = (n + 1) >> 1;
    const bool sil = lam_sil > 0.f, vt = lam_vt > 0.f, scan = lam_scan > 0.f;      // (uniform)
    const float* A = sil ? g_sil + (size_t)b * n : nullptr;
    const float* T = vt ? g_vt + (size_t)b * n : nullptr;
    const float* C = scan ? g_scan + (size_t)b * n : nullptr;
    float* G = g + (size_t)b * n;
    const int p0 = blockIdx.y * TM_PAIRS + tid;
    // every load of the thread - up to three operand rows - is issued before the first use
    float2 a[TM_UNROLL], t[TM_UNROLL], c[TM_UNROLL];
#pragma unroll
    for (int u = 0; u < TM_UNROLL; ++u) {
        const int p = p0 + u * TM_NT;
        a[u] = sil && p < npairs ? tm_load<VEC>(A, p, VEC || 2 * p + 1 < n) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < TM_UNROLL; ++u) {
        const int p = p0 + u * TM_NT;
        t[u] = vt && p < npairs ? tm_load<VEC>(T, p, VEC || 2 * p + 1 < n) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < TM_UNROLL; ++u) {
        const int p = p0 + u * TM_NT;
        c[u] = scan && p < npairs ? tm_load<VEC>(C, p, VEC || 2 * p + 1 < n) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < TM_UNROLL; ++u) {
        const int p = p0 + u * TM_NT;
        if (p >= npairs) break;
        const bool two = VEC || 2 * p + 1 < n;
        // the live components in the order silhouette, vertex targets, scan: the first one starts the sum, the others are added
        float rx, ry;
        if (sil) {
            rx = lam_sil * a[u].x; ry = lam_sil * a[u].y;
            if (vt) { rx = rx + lam_vt * t[u].x; ry = ry + lam_vt * t[u].y; }
            if (scan) { rx = rx + lam_scan * c[u].x; ry = ry + lam_scan * c[u].y; }
        } else if (vt) {
            rx = lam_vt * t[u].x; ry = lam_vt * t[u].y;
            if (scan) { rx = rx + lam_scan * c[u].x; ry = ry + lam_scan * c[u].y; }
        } else { rx = lam_scan * c[u].x; ry = lam_scan * c[u].y; }
        if (VEC) *reinterpret_cast<float2*>(G + 2 * (size_t)p) = make_float2(rx, ry);
        else { G[2 * (size_t)p] = rx; if (two) G[2 * (size_t)p + 1] = ry; }
    }
    if (blockIdx.y == 0 && tid == 0) {
        const float ls = sil ? L_sil[b] : 0.f, lv = vt ? L_vt[b] : 0.f, lc = scan ? L_scan[b] : 0.f;
        double s = 0.0;
        if (sil) {
            s = (double)lam_sil * (double)ls;
            if (vt) s = s + (double)lam_vt * (double)lv;
            if (scan) s = s + (double)lam_scan * (double)lc;
        } else if (vt) {
            s = (double)lam_vt * (double)lv;
            if (scan) s = s + (double)lam_scan * (double)lc;
        } else s = (double)lam_scan * (double)lc;
        L_v[b] = (float)s;
        if (parts) tm_write_parts(parts, sums, b, 0.f, 0.f, lam_sil, ls, lam_vt, lv, lam_scan, lc);
    }
}

template <bool GATED>
__global__ __launch_bounds__(TM_REC_NT) void term_mix_record_kernel(float lam_sc, const SdfAdj* __restrict__ rec_scene,
                                                                    const SdfAdj* __restrict__ rec_verts, float lam_sil,
                                                                    const float* __restrict__ L_sil, float lam_vt,
                                                                    const float* __restrict__ L_vt, float lam_scan,
                                                                    const float* __restrict__ L_scan, SdfAdj* __restrict__ rec,
                                                                    float* __restrict__ parts, float* __restrict__ sums,
                                                                    TmGate<GATED> gate) {
    const int b = blockIdx.x, e = threadIdx.x;
    if (GATED && gate.off(b)) return;                                  // (uniform)
    if (e >= TM_REC) return;
    const float* sc = reinterpret_cast<const float*>(rec_scene + b);
    const float* rv = reinterpret_cast<const float*>(rec_verts + b);
    const float a_sc = sc[e], a_v = rv[e];                             // (entry 0 is S itself)
    const double S_sc = (double)sc[0], S_v = (double)rv[0];            // (uniform)
    const double Q = (double)lam_sc * (S_sc * S_sc) + S_v * S_v;
    const bool zero = Q < 1.17549435e-38;                              // FLT_MIN
    const double root = sqrt(Q);
    float out;
    if (e == 0) out = zero ? 0.f : (float)root;
    else out = zero ? 0.f : (float)((((double)lam_sc * S_sc) * (double)a_sc + S_v * (double)a_v) / root);
    reinterpret_cast<float*>(rec + b)[e] = out;
    if (e == 0 && parts)
        tm_write_parts(parts, sums, b, lam_sc, (float)(S_sc * S_sc), lam_sil, L_sil ? L_sil[b] : 0.f, lam_vt, L_vt ? L_vt[b] : 0.f,
                       lam_scan, L_scan ? L_scan[b] : 0.f);
}

int term_mix_blocks(int nv) { return ((3 * nv + 1) / 2 + TM_PAIRS - 1) / TM_PAIRS; }

template <bool GATED>
static void tm_launch(bool vec, dim3 grid, hipStream_t stream, int n, float lam_sil, const float* g_sil, const float* L_sil,
                      float lam_vt, const float* g_vt, const float* L_vt, float lam_scan, const float* g_scan, const float* L_scan,
                      float* g, float* L_v, float* parts, float* sums, TmGate<GATED> gate) {
    if (vec) hipLaunchKernelGGL((term_mix_cotangent_kernel<GATED, true>), grid, dim3(TM_NT), 0, stream, n, lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt, lam_scan, g_scan, L_scan, g, L_v, parts, sums, gate);
    else hipLaunchKernelGGL((term_mix_cotangent_kernel<GATED, false>), grid, dim3(TM_NT), 0, stream, n, lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt, lam_scan, g_scan, L_scan, g, L_v, parts, sums, gate);
}

hipError_t launch_term_mix_cotangent(int nv, int B, float lam_sil, const float* g_sil, const float* L_sil, float lam_vt,
                                     const float* g_vt, const float* L_vt, float lam_scan, const float* g_scan,
                                     const float* L_scan, const int* gate, float* g, float* L_v, float* parts, float* sums,
                                     hipStream_t stream) {
    if (!(lam_sil > 0.f) && !(lam_vt > 0.f) && !(lam_scan > 0.f)) return hipErrorInvalidValue;
    const int n = 3 * nv;
    uintptr_t bases = reinterpret_cast<uintptr_t>(g);
    if (lam_sil > 0.f) bases |= reinterpret_cast<uintptr_t>(g_sil);
    if (lam_vt > 0.f) bases |= reinterpret_cast<uintptr_t>(g_vt);
    if (lam_scan > 0.f) bases |= reinterpret_cast<uintptr_t>(g_scan);
    const bool vec = n % 2 == 0 && (bases & 7) == 0;
    const dim3 grid(B, term_mix_blocks(nv));
    if (gate) tm_launch<true>(vec, grid, stream, n, lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt, lam_scan, g_scan, L_scan, g, L_v, parts, sums, TmGate<true>{gate});
    else tm_launch<false>(vec, grid, stream, n, lam_sil, g_sil, L_sil, lam_vt, g_vt, L_vt, lam_scan, g_scan, L_scan, g, L_v, parts, sums, TmGate<false>{});
    return hipGetLastError();
}

hipError_t launch_term_mix_record(int B, float lam_sc, const SdfAdj* rec_scene, const SdfAdj* rec_verts, float lam_sil,
                                  const float* L_sil, float lam_vt, const float* L_vt, float lam_scan, const float* L_scan,
                                  const int* gate, SdfAdj* rec, float* parts, float* sums, hipStream_t stream) {
    if (gate)
        hipLaunchKernelGGL(term_mix_record_kernel<true>, dim3(B), dim3(TM_REC_NT), 0, stream, lam_sc, rec_scene, rec_verts, lam_sil,
                           L_sil, lam_vt, L_vt, lam_scan, L_scan, rec, parts, sums, TmGate<true>{gate});
    else
        hipLaunchKernelGGL(term_mix_record_kernel<false>, dim3(B), dim3(TM_REC_NT), 0, stream, lam_sc, rec_scene, rec_verts, lam_sil,
                           L_sil, lam_vt, L_vt, lam_scan, L_scan, rec, parts, sums, TmGate<false>{});
    return hipGetLastError();
}

}  // namespace mvfit
