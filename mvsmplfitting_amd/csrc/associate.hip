// Association of 2-D detections across the views of a frame (mvfit_associate_views): which detection of view A and
// which of view B show the same person.  A detector run per view lists its people in its own order; the multi-person
// fit needs one identity per (frame, person).  The reference fits people[0] only and has no such step; its one matching
// helper (module_utils.matching: pair_by_L2_distance) weights a distance by sqrt(conf_a * conf_b), which is the weight
// used here.  Three kernels per group of frames, all float64 with contraction off (include/mvfit.h states the order of
// every operation; tests/associate_oracle.py restates it in NumPy and the bits agree):
//
//   assoc_ray_kernel      thread = (frame, detection, joint): the world-space direction of the pixel's ray and the
//                         joint's confidence, 32 B per joint; the thread of (first frame, slot 0, joint 0) of a view also
//                         writes the view's ray origin.
//   assoc_cost_kernel     workgroup = a 16 x 16 tile of a frame's D x D cost matrix (upper-triangle tiles only), thread =
//                         one pair.  The 2 x 16 detections' rays are staged in LDS joint-major ([17][16][4] doubles per
//                         side, 17 KB: the 16 lanes of a row read 512 contiguous bytes, the 4 rows of a wave broadcast);
//                         the thread walks the 17 joints in ascending order and stores cost(a, b) and its mirror.
//   assoc_cluster_kernel  workgroup = a frame, thread = a detection.  Complete linkage with the cannot-link constraint:
//                         the linkage of two clusters is the MAXIMUM pair cost, and two detections of one view cost +inf,
//                         so a pair of clusters whose view sets overlap has linkage +inf by itself - the constraint needs
//                         no view sets, and L(A u B, X) = max(L(A, X), L(B, X)) carries it along.  A cluster lives in the
//                         slot of its smallest member, a dead slot's row and column are +inf.  Per step: thread c scans
//                         column c of the upper triangle (rows r < c, coalesced over c, eight independent loads in
//                         flight; skipping the dead rows through an LDS flag in front of each load was measured
//                         and is slower: the step is a latency chain, not a bandwidth limit), keeping its smallest (cost bits, r * D + c) - the bit pattern of a non-negative double
//                         orders like the value -, then the workgroup-wide minimum of that key: DPP butterflies inside
//                         the rows of a wave, v_permlane swaps across them (wave_ops.h), the four waves through LDS.  A
//                         minimum of integer keys does not depend on the order it is formed in: no float atomics, no
//                         dependence on wave scheduling.  The matrix of a frame (up to 512 KB) lives in the workspace.
//
// Nothing a frame computes depends on F, on the frame's position in the call or on the group it falls into.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "camera_math.h"
#include "wave_ops.h"
#include "launchers.h"

namespace mvfit {

constexpr int ASSOC_NT = 256;           // threads of a workgroup = the largest D (MVFIT_MAX_VIEWS * MVFIT_ASSOC_MAX_DET)
constexpr int ASSOC_J = 17;
constexpr int ASSOC_T = 16;             // tile edge of the cost kernel
constexpr int ASSOC_RAY = ASSOC_J * 4;  // doubles per detection: (d0, d1, d2, confidence) per joint

// thread = (frame of the group, detection, joint)
__global__ __launch_bounds__(ASSOC_NT) void assoc_ray_kernel(const float* __restrict__ kps, const int32_t* __restrict__ count,
                                                             const double* __restrict__ intris,
                                                             const double* __restrict__ extris, int f0, int nf, int V,
                                                             int Nmax, double* __restrict__ org, double* __restrict__ rays) {
    const int D = V * Nmax;
    const int idx = blockIdx.x * ASSOC_NT + threadIdx.x;
    if (idx >= nf * D * ASSOC_J) return;
    const int fl = idx / (D * ASSOC_J), rem = idx - fl * (D * ASSOC_J), a = rem / ASSOC_J, j = rem - a * ASSOC_J;
    const int v = a / Nmax, k = a - v * Nmax, f = f0 + fl;
    const double* E = extris + 16 * v;
    if (fl == 0 && k == 0 && j == 0)                                   // o_v = -R^T t
        for (int i = 0; i < 3; ++i) org[3 * v + i] = -((E[i] * E[3] + E[4 + i] * E[7]) + E[8 + i] * E[11]);
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, cf = 0.0;
    if (k < count[(size_t)f * V + v]) {
        double Ki[9];
        inv3(intris + 9 * v, Ki);
        const float* kp = kps + (((size_t)f * D + a) * ASSOC_J + j) * 3;
        const double x = (double)kp[0], y = (double)kp[1];
        cf = (double)kp[2];
        double n0 = Ki[0] * x + Ki[1] * y + Ki[2], n1 = Ki[3] * x + Ki[4] * y + Ki[5], n2 = Ki[6] * x + Ki[7] * y + Ki[8];
        const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        n0 /= nn; n1 /= nn; n2 /= nn;
        d0 = (E[0] * n0 + E[4] * n1) + E[8] * n2;                      // R^T n
        d1 = (E[1] * n0 + E[5] * n1) + E[9] * n2;
        d2 = (E[2] * n0 + E[6] * n1) + E[10] * n2;
    }
    double* o = rays + (size_t)idx * 4;
    o[0] = d0; o[1] = d1; o[2] = d2; o[3] = cf;
}

// grid (tile pairs of the upper triangle * frames of the group).  link: [nf, D, D] of the workspace; cost_out: the
// caller's matrix of the group's first frame, or null.
__global__ __launch_bounds__(ASSOC_NT) void assoc_cost_kernel(const double* __restrict__ rays, const double* __restrict__ org,
                                                              const int32_t* __restrict__ count, int f0, int V, int Nmax,
                                                              int ntile, int min_joints, double* __restrict__ link,
                                                              double* __restrict__ cost_out) {
    __shared__ double shA[ASSOC_J][ASSOC_T][4];
    __shared__ double shB[ASSOC_J][ASSOC_T][4];
    const int D = V * Nmax, ntp = ntile * (ntile + 1) / 2;
    const int fl = blockIdx.x / ntp, tid = threadIdx.x;
    int p = blockIdx.x - fl * ntp, ti = 0;
    while (p >= ntile - ti) { p -= ntile - ti; ++ti; }                 // row ti of the triangle holds ntile - ti tiles
    const int tj = ti + p;
    const double* fr = rays + (size_t)fl * D * ASSOC_RAY;
    for (int q = tid; q < 2 * ASSOC_T * ASSOC_RAY; q += ASSOC_NT) {
        const int side = q / (ASSOC_T * ASSOC_RAY), r = q - side * (ASSOC_T * ASSOC_RAY);
        const int det = r / ASSOC_RAY, e = r - det * ASSOC_RAY, g = (side ? tj : ti) * ASSOC_T + det;
        const double x = g < D ? fr[(size_t)g * ASSOC_RAY + e] : 0.0;
        (side ? shB : shA)[e >> 2][det][e & 3] = x;
    }
    __syncthreads();
    const int la = tid >> 4, lb = tid & 15, a = ti * ASSOC_T + la, b = tj * ASSOC_T + lb;
    if (a >= D || b >= D || a > b) return;
    double cost = INFINITY;
    const int va = a / Nmax, vb = b / Nmax;
    const int32_t* cnt = count + (size_t)(f0 + fl) * V;
    if (va != vb && a - va * Nmax < cnt[va] && b - vb * Nmax < cnt[vb]) {
        const double b0 = org[3 * vb] - org[3 * va], b1 = org[3 * vb + 1] - org[3 * va + 1], b2 = org[3 * vb + 2] - org[3 * va + 2];
        double num = 0.0, den = 0.0;
        int n = 0;
        for (int j = 0; j < ASSOC_J; ++j) {
            const double ca = shA[j][la][3], cb = shB[j][lb][3];
            if (!(ca > 0.0 && cb > 0.0)) continue;
            const double a0 = shA[j][la][0], a1 = shA[j][la][1], a2 = shA[j][la][2];
            const double e0 = shB[j][lb][0], e1 = shB[j][lb][1], e2 = shB[j][lb][2];
            const double c0 = a1 * e2 - a2 * e1, c1 = a2 * e0 - a0 * e2, c2 = a0 * e1 - a1 * e0;
            const double s2 = (c0 * c0 + c1 * c1) + c2 * c2;
            double dist;
            if (s2 > 1e-18) {
                dist = fabs((b0 * c0 + b1 * c1) + b2 * c2) / sqrt(s2);
            } else {                                                   // parallel rays: distance of o_b from the line a
                const double x0 = b1 * a2 - b2 * a1, x1 = b2 * a0 - b0 * a2, x2 = b0 * a1 - b1 * a0;
                dist = sqrt((x0 * x0 + x1 * x1) + x2 * x2);
            }
            const double w = sqrt(ca * cb);
            num += w * dist;
            den += w;
            ++n;
        }
        if (n >= min_joints) cost = num / den;
    }
    const size_t o = (size_t)fl * D * D, ab = o + (size_t)a * D + b, ba = o + (size_t)b * D + a;
    link[ab] = cost;
    if (cost_out) cost_out[ab] = cost;
    if (a != b) {
        link[ba] = cost;
        if (cost_out) cost_out[ba] = cost;
    }
}

struct AssocKey { unsigned long long c; unsigned i; };                 // cost bits (major), pair index (minor)

__device__ __forceinline__ AssocKey key_min(AssocKey p, AssocKey q) {
    return (q.c < p.c || (q.c == p.c && q.i < p.i)) ? q : p;
}
template <int CTRL>
__device__ __forceinline__ AssocKey key_dpp(AssocKey v) {
    AssocKey r;
    r.c = dpp_u64<CTRL>(v.c);
    r.i = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.i, CTRL, 0xf, 0xf, true);
    return r;
}
template <bool HALF>
__device__ __forceinline__ AssocKey key_swap_min(AssocKey v) {
    double da, db;
    swap_pair<HALF>(__builtin_bit_cast(double, v.c), da, db);
    unsigned ia, ib;
    if (HALF) swap32(v.i, ia, ib); else swap16(v.i, ia, ib);
    const AssocKey a = {__builtin_bit_cast(unsigned long long, da), ia}, b = {__builtin_bit_cast(unsigned long long, db), ib};
    return key_min(a, b);
}
// the wave's smallest key in every lane; all 64 lanes take part
__device__ __forceinline__ AssocKey wave64_key_min(AssocKey v) {
    v = key_min(v, key_dpp<DPP_XOR1>(v));
    v = key_min(v, key_dpp<DPP_XOR2>(v));
    v = key_min(v, key_dpp<DPP_HALF_MIRROR>(v));
    v = key_min(v, key_dpp<DPP_MIRROR>(v));
    v = key_swap_min<false>(v);
    v = key_swap_min<true>(v);
    return v;
}

// grid (frames of the group).  link: [nf, D, D], overwritten; labels / num_clusters: the caller's, indexed by f0 + frame.
__global__ __launch_bounds__(ASSOC_NT) void assoc_cluster_kernel(unsigned long long* link,
                                                                 const int32_t* __restrict__ count, int f0, int V, int Nmax,
                                                                 unsigned long long max_bits, int min_views,
                                                                 int32_t* __restrict__ labels, int32_t* __restrict__ num_clusters) {
    __shared__ int sh_cl[ASSOC_NT];                                    // slot of the detection's cluster, -1: no detection
    __shared__ int sh_size[ASSOC_NT];
    __shared__ int sh_rank[ASSOC_NT];
    __shared__ int sh_cnt[ASSOC_NT / 64];
    __shared__ unsigned long long sh_kc[ASSOC_NT / 64];
    __shared__ unsigned sh_ki[ASSOC_NT / 64];
    const int D = V * Nmax, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = f0 + blockIdx.x;
    unsigned long long* L = link + (size_t)blockIdx.x * D * D;
    const unsigned long long INF_BITS = 0x7ff0000000000000ull;
    const bool in = tid < D;
    const int c = in ? tid : D - 1;                                    // (a thread past D loads in bounds and keeps nothing)
    {
        const int v = c / Nmax;
        sh_cl[tid] = (in && c - v * Nmax < count[(size_t)f * V + v]) ? tid : -1;
        sh_size[tid] = 0;
    }
    __syncthreads();
    const int rmax = 64 * wave < D ? min(D, 64 * wave + 63) : 0;       // rows above the diagonal of this wave's columns
    for (int step = 0; step < D; ++step) {
        AssocKey best = {~0ull, 0u};
        for (int r0 = 0; r0 < rmax; r0 += 8) {
            unsigned long long x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = L[(size_t)min(r0 + k, D - 1) * D + c];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (in && r0 + k < c && x[k] < best.c) { best.c = x[k]; best.i = (unsigned)((r0 + k) * D + c); }
        }
        best = wave64_key_min(best);
        if (lane == 0) { sh_kc[wave] = best.c; sh_ki[wave] = best.i; }
        __syncthreads();
        AssocKey win = {sh_kc[0], sh_ki[0]};
        for (int w = 1; w < ASSOC_NT / 64; ++w) win = key_min(win, AssocKey{sh_kc[w], sh_ki[w]});
        if (win.c > max_bits) break;                                   // the same decision in every thread
        const int A = (int)(win.i / (unsigned)D), B = (int)(win.i - (unsigned)A * (unsigned)D);      // A < B
        if (in && tid != B) {
            // entry (s, x) of the upper triangle
            const size_t ax = tid < A ? (size_t)tid * D + A : (size_t)A * D + tid;
            const size_t bx = tid < B ? (size_t)tid * D + B : (size_t)B * D + tid;
            if (tid != A) {
                const unsigned long long la = L[ax], lb = L[bx];
                L[ax] = la > lb ? la : lb;
            }
            L[bx] = INF_BITS;                                          // slot B is dead; for tid == A: the pair itself
        }
        if (sh_cl[tid] == B) sh_cl[tid] = A;
        __syncthreads();
    }
    // sizes, the kept clusters in ascending slot order, labels
    if (sh_cl[tid] >= 0) atomicAdd(&sh_size[sh_cl[tid]], 1);
    __syncthreads();
    const bool kept = sh_cl[tid] == tid && sh_size[tid] >= min_views;
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) sh_cnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < ASSOC_NT / 64; ++w) { if (w < wave) base += sh_cnt[w]; total += sh_cnt[w]; }
    sh_rank[tid] = kept ? base + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
    __syncthreads();
    if (in) labels[(size_t)f * D + tid] = sh_cl[tid] >= 0 ? sh_rank[sh_cl[tid]] : -1;
    if (tid == 0 && num_clusters) num_clusters[f] = total;
}

size_t assoc_frame_bytes(int D) { return (size_t)D * ASSOC_RAY * 8 + (size_t)D * D * 8; }
size_t assoc_head_bytes() { return 512; }                              // the views' ray origins, [MVFIT_MAX_VIEWS, 3] doubles

// One group of nf frames (f0 ..) through the three kernels.  ws: assoc_head_bytes() + nf * assoc_frame_bytes(D) bytes.
hipError_t launch_associate_group(const float* kps, const int32_t* count, const double* intris, const double* extris, int f0,
                                  int nf, int V, int Nmax, double max_cost, int min_joints, int min_views, void* ws,
                                  double* cost_out, int32_t* labels, int32_t* num_clusters, hipStream_t stream) {
    const int D = V * Nmax, ntile = (D + ASSOC_T - 1) / ASSOC_T, ntp = ntile * (ntile + 1) / 2;
    double* org = reinterpret_cast<double*>(ws);
    double* rays = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(ws) + assoc_head_bytes());
    double* link = rays + (size_t)nf * D * ASSOC_RAY;
    const long long nray = (long long)nf * D * ASSOC_J;
    hipLaunchKernelGGL(assoc_ray_kernel, dim3((unsigned)((nray + ASSOC_NT - 1) / ASSOC_NT)), dim3(ASSOC_NT), 0, stream, kps, count,
                       intris, extris, f0, nf, V, Nmax, org, rays);
    hipLaunchKernelGGL(assoc_cost_kernel, dim3((unsigned)(nf * ntp)), dim3(ASSOC_NT), 0, stream, (const double*)rays,
                       (const double*)org, count, f0, V, Nmax, ntile, min_joints, link,
                       cost_out ? cost_out + (size_t)f0 * D * D : nullptr);
    hipLaunchKernelGGL(assoc_cluster_kernel, dim3(nf), dim3(ASSOC_NT), 0, stream, reinterpret_cast<unsigned long long*>(link), count,
                       f0, V, Nmax, __builtin_bit_cast(unsigned long long, max_cost), min_views, labels, num_clusters);
    return hipGetLastError();
}

}  // namespace mvfit
