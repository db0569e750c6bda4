// Point-cloud loss between scans and posed bodies, with its gradient on the vertices (include/mvfit.h: mvfit_set_scans /
// mvfit_scan_loss).  New ground: the reference has no term on measured 3-D surface data.
//
// Prepared once per scan set (scan_set):
//   scan_pack_kernel: point i of body n -> (x, y, z, w) when it takes part (i < count[n] and w > 0), else (NaN, NaN, NaN, 0);
//       the point itself is read only when it takes part.
// Per evaluation (scan_loss; scan_round inside the fit's chained rounds - the same kernels behind a per-body gate):
//   scan_face_kernel: a thread per (body, face): the record (bounding sphere centre, padded radius | a | b - a | c - a), 64 B,
//       and vertex a of every SCAN_SEED-th face in a compact list (the seed of the cull's bound).
//   scan_s2m_kernel<CULL> (term S, the hot one): a workgroup owns 256 points of one body, the point in registers; the body's
//       face records stream through LDS in tiles of SCAN_FT, every lane reads the same address (a broadcast).  The running
//       minimum (bits of m, face) stays in registers: m >= 0 orders like its bits, a NaN compares above +inf, ascending
//       faces and a strict compare send ties to the lowest face.  CULL: a face is skipped when its sphere lies farther than
//       the bound sb - see "the cull" below.  The winner's gradient goes to a 64-bit fixed-point accumulator per (body,
//       vertex, axis) (integer atomics: the sum does not depend on the order), taken with the weight times 2^e_n - e_n puts
//       the body's largest weight into [1, 2), so the unit 2^-32 is relative to the body's weights, not absolute;
//       w rho to one float64 partial per workgroup.
//   scan_m2s_kernel<SEARCH> (term M and the gradient's last step): a thread per (body, vertex); the packed points stream
//       through LDS in tiles of SCAN_PT, same minimum.  Then g = w_m2s rho' 2 (v - p) + w_s2m 2^-e_n acc / 2^32 in float64,
//       rounded and stored once; rho to one float64 partial per workgroup.
//   scan_sum_kernel: a wave per body, the partials of each term in ascending order.
//   scan_clear_kernel (scan_round only): zeroes the accumulators of the bodies the gate keeps - a kernel node where scan_loss
//       has a memset, which a captured round graph must not hold.
// No float atomics; nothing a body gets depends on the other bodies of the call or on its position in it.
//
// The cull.  sb is an upper bound of the distance from p to the surface: at first the distance to the nearest of the seed
// vertices (each lies on a face), later the root of the running minimum.  Face f cannot win when
//     |p - c_f| - r_f > sb,
// c_f, r_f its bounding sphere.  Everything here is fp32, so the test is widened until rounding cannot turn it:
// r_f is stored as r (1 + 2^-10) + 2^-13 max|coordinate of the face|, sb carries (1 + 2^-11) and 2^-13 max|coordinate of p|,
// and the squared centre distance is shrunk by (1 - 2^-11).  The fp32 errors of the centre, the radius, the centre distance,
// the seed distance and of m itself are a few units of 2^-24 times the coordinates involved - more than a hundred times
// smaller than the pads - so a skipped face has a computed m above the running minimum, and the culled and the exhaustive
// search return the same bits.  A NaN anywhere fails the skip test: the face is evaluated, as in the exhaustive search.
#include "scan_loss.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "launchers.h"
#include "mvfit.h"
#include "wave_ops.h"

namespace mvfit {

constexpr int SCAN_NT = 256;
constexpr int SCAN_FT = 512;                     // face records per LDS tile: 32 KB, four workgroups per CU
constexpr int SCAN_PT = 2048;                    // packed points per LDS tile: 32 KB
constexpr int SCAN_SEED = 8;                     // every SCAN_SEED-th face gives a seed vertex
constexpr double SCAN_FIX = 4294967296.0;        // 2^32: fixed-point unit of term S's gradient accumulators (unit of the vertices)
constexpr float SCAN_LO = 1.f - 0x1p-11f, SCAN_HI = 1.f + 0x1p-11f, SCAN_ABS = 0x1p-13f;

#pragma clang fp contract(off)

__device__ __forceinline__ float scan_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Closest point q of triangle (a, a + ab, a + ac) to p by region (vertex a, b, edge ab, vertex c, edge ac, edge bc, interior;
// the first that matches): q = a + v ab + w ac, d = q - p = (v ab + w ac) - (p - a), returns m = |d|^2.  The barycentrics of
// (a, b, c) are ((1 - v) - w, v, w).  One expression tree for every caller: the same inputs give the same bits.
__device__ __forceinline__ float scan_closest(const float* p, const float* a, const float* ab, const float* ac, float& v,
                                              float& w, float* d) {
    const float ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const float bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
    const float cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
    const float d1 = scan_dot(ab, ap), d2 = scan_dot(ac, ap), d3 = scan_dot(ab, bp), d4 = scan_dot(ac, bp),
                d5 = scan_dot(ab, cp), d6 = scan_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    float nv = 0.f, nw = 0.f, den = 1.f;
    if (d1 <= 0.f && d2 <= 0.f) { }
    else if (d3 >= 0.f && d4 <= d3) { nv = 1.f; }
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { nv = d1; den = d1 - d3; }
    else if (d6 >= 0.f && d5 <= d6) { nw = 1.f; }
    else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { nw = d2; den = d2 - d6; }
    else if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) { nv = e2; nw = e1; den = e1 + e2; }
    else { nv = vb; nw = vc; den = (va + vb) + vc; }
    const float inv = 1.f / den;
    v = nv * inv; w = nw * inv;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (v * ab[c] + w * ac[c]) - ap[c];
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// rho(m) and rho'(m) in float64: m when sigma <= 0, else sigma^2 m / (sigma^2 + m)
__device__ __forceinline__ void scan_rho(float sigma, double m, double& rho, double& drho) {
    rho = m; drho = 1.0;
    if (sigma > 0.f) {
        const double s2 = (double)sigma * (double)sigma, den = s2 + m;
        rho = s2 * m / den;
        drho = (s2 / den) * (s2 / den);
    }
}

// the workgroup's total of s in wave order, written by thread 0
__device__ __forceinline__ void scan_block_sum(double s, double* sh_d, double* out) {
    const int tid = threadIdx.x;
    s = wave64_sum(s);
    if ((tid & 63) == 0) sh_d[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = sh_d[0];
        for (int w = 1; w < SCAN_NT / 64; ++w) t += sh_d[w];
        *out = t;
    }
}

// The gate of the term inside the fit's chained rounds (scan_round): gate[body] == 0 - a finished problem, or a stage without
// the term - ends the workgroup at once, so the body keeps its loss, gradient rows, partials and accumulators; a null pointer
// keeps every body.  The read is uniform per workgroup (blockIdx.y).  The ungated instantiations carry an empty argument and
// are the kernels as they were.
template <bool GATED> struct ScanGate { __device__ __forceinline__ bool off(int) const { return false; } };
template <> struct ScanGate<true> {
    const int* gate;
    __device__ __forceinline__ bool off(int body) const { return gate && !gate[body]; }
};

// ---------------------------------------------------------------------------------------------------------- prepared once
// grid (ceil(Pmax / SCAN_NT), N)
__global__ __launch_bounds__(SCAN_NT) void scan_pack_kernel(const float* __restrict__ pts, const float* __restrict__ wts, int Pmax,
                                                            float4* __restrict__ pk) {
    const int i = blockIdx.x * SCAN_NT + threadIdx.x, n = blockIdx.y;
    if (i >= Pmax) return;
    const size_t at = (size_t)n * Pmax + i;
    const float w = wts[at];
    const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
    float4 o = make_float4(qnan, qnan, qnan, 0.f);
    if (w > 0.f) o = make_float4(pts[at * 3], pts[at * 3 + 1], pts[at * 3 + 2], w);
    pk[at] = o;
}

// ---------------------------------------------------------------------------------------------------------- per evaluation
// grid (ceil(nf / SCAN_NT), N): rec[(n nf + f) 4 + {0..3}] = (centre, padded radius), (a, 0), (ab, 0), (ac, 0);
// seed[n ns + f / SCAN_SEED] = (a, 0) for f % SCAN_SEED == 0
template <bool GATED>
__global__ __launch_bounds__(SCAN_NT) void scan_face_kernel(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                            int nf, int ns, float4* __restrict__ rec, float4* __restrict__ seed,
                                                            ScanGate<GATED> G) {
    const int f = blockIdx.x * SCAN_NT + threadIdx.x, n = blockIdx.y;
    if (G.off(n)) return;
    if (f >= nf) return;
    const float* vb = verts + (size_t)n * nv * 3;
    const float *pa = vb + (size_t)faces[f * 3] * 3, *pb = vb + (size_t)faces[f * 3 + 1] * 3, *pc = vb + (size_t)faces[f * 3 + 2] * 3;
    float a[3], ab[3], ac[3], cen[3], big = 0.f, r2 = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        a[q] = pa[q]; ab[q] = pb[q] - pa[q]; ac[q] = pc[q] - pa[q];
        cen[q] = a[q] + (ab[q] + ac[q]) * (1.f / 3.f);
        big = fmaxf(big, fmaxf(fabsf(pa[q]), fmaxf(fabsf(pb[q]), fabsf(pc[q]))));
    }
    const float* corner[3] = {pa, pb, pc};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dx = corner[k][0] - cen[0], dy = corner[k][1] - cen[1], dz = corner[k][2] - cen[2];
        r2 = fmaxf(r2, (dx * dx + dy * dy) + dz * dz);
    }
    const float rpad = sqrtf(r2) * (1.f + 0x1p-10f) + SCAN_ABS * big;
    float4* o = rec + ((size_t)n * nf + f) * 4;
    o[0] = make_float4(cen[0], cen[1], cen[2], rpad);
    o[1] = make_float4(a[0], a[1], a[2], 0.f);
    o[2] = make_float4(ab[0], ab[1], ab[2], 0.f);
    o[3] = make_float4(ac[0], ac[1], ac[2], 0.f);
    if (f % SCAN_SEED == 0) seed[(size_t)n * ns + f / SCAN_SEED] = o[1];
}

// grid (ceil(3 nv / SCAN_NT), N): acc[n][nv][3] = 0 for the bodies the gate keeps
__global__ __launch_bounds__(SCAN_NT) void scan_clear_kernel(unsigned long long* __restrict__ acc, int nv, ScanGate<true> G) {
    const int i = blockIdx.x * SCAN_NT + threadIdx.x, n = blockIdx.y;
    if (G.off(n)) return;
    if (i < nv * 3) acc[(size_t)n * nv * 3 + i] = 0ull;
}

// grid (ceil(Pmax / SCAN_NT), N): 256 points of body n against its nf face records.
// acc[(n nv + vertex) 3 + axis] += round(2^32 (2^e_n w_p) rho'(m) 2 d[axis] b_k), e_n = expo[n] (scan_set: the body's largest
// weight scaled into [1, 2)); partS[n gridDim.x + blockIdx.x] = sum of w_p rho.
template <bool CULL, bool GATED>
__global__ __launch_bounds__(SCAN_NT) void scan_s2m_kernel(const float4* __restrict__ pk, const int* __restrict__ count,
                                                           const int* __restrict__ expo, int Pmax,
                                                           const float4* __restrict__ rec, const float4* __restrict__ seed,
                                                           int nf, int ns, const int32_t* __restrict__ faces, int nv, float sigma,
                                                           unsigned long long* __restrict__ acc, double* __restrict__ partS,
                                                           int32_t* __restrict__ nearest, ScanGate<GATED> G) {
    __shared__ __attribute__((aligned(16))) float4 sh[SCAN_FT * 4];
    __shared__ double sh_d[SCAN_NT / 64];
    const int tid = threadIdx.x, n = blockIdx.y, i = blockIdx.x * SCAN_NT + tid;
    if (G.off(n)) return;                                            // (uniform)
    const bool inside = i < Pmax;
    if (blockIdx.x * SCAN_NT >= count[n]) {                          // (uniform) no point of this workgroup takes part
        if (inside && nearest) nearest[(size_t)n * Pmax + i] = -1;
        if (tid == 0) partS[(size_t)n * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    const float4 P = inside ? pk[(size_t)n * Pmax + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool live = P.w > 0.f;
    const float p[3] = {live ? P.x : 0.f, live ? P.y : 0.f, live ? P.z : 0.f};
    float sb = 0.f;
    const float slack = SCAN_ABS * fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2])));
    if (CULL) {
        float smin = __builtin_bit_cast(float, 0x7f800000u);
        const float4* sd = seed + (size_t)n * ns;
        for (int s0 = 0; s0 < ns; s0 += SCAN_FT * 4) {
            const int cnt = min(SCAN_FT * 4, ns - s0);
            __syncthreads();
            for (int j = tid; j < cnt; j += SCAN_NT) sh[j] = sd[s0 + j];
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const float4 a = sh[j];
                const float dx = a.x - p[0], dy = a.y - p[1], dz = a.z - p[2];
                smin = fminf(smin, (dx * dx + dy * dy) + dz * dz);
            }
        }
        sb = sqrtf(smin) * SCAN_HI + slack;
    }
    unsigned best = 0x7f800001u;                 // above +inf: a face with a finite m always wins over "none"
    int bj = -1;
    const float4* rb = rec + (size_t)n * nf * 4;
    for (int f0 = 0; f0 < nf; f0 += SCAN_FT) {
        const int cnt = min(SCAN_FT, nf - f0);
        __syncthreads();
        for (int j = tid; j < cnt * 4; j += SCAN_NT) sh[j] = rb[(size_t)f0 * 4 + j];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            bool test = live;
            if (CULL) {
                const float4 c = sh[j * 4];
                const float dx = c.x - p[0], dy = c.y - p[1], dz = c.z - p[2], t = sb + c.w;
                if (((dx * dx + dy * dy) + dz * dz) * SCAN_LO > t * t) test = false;
            }
            if (test) {
                const float4 A = sh[j * 4 + 1], B = sh[j * 4 + 2], C = sh[j * 4 + 3];
                const float a[3] = {A.x, A.y, A.z}, ab[3] = {B.x, B.y, B.z}, ac[3] = {C.x, C.y, C.z};
                float v, w, d[3];
                const float m = scan_closest(p, a, ab, ac, v, w, d);
                const unsigned mb = __builtin_bit_cast(unsigned, m);
                if (mb < best) {
                    best = mb; bj = f0 + j;
                    if (CULL) sb = fminf(sb, sqrtf(m) * SCAN_HI + slack);
                }
            }
        }
    }
    if (inside && nearest) nearest[(size_t)n * Pmax + i] = live ? bj : -1;
    double s = 0.0;
    if (live && bj >= 0) {
        const float4 A = rb[(size_t)bj * 4 + 1], B = rb[(size_t)bj * 4 + 2], C = rb[(size_t)bj * 4 + 3];
        const float a[3] = {A.x, A.y, A.z}, ab[3] = {B.x, B.y, B.z}, ac[3] = {C.x, C.y, C.z};
        float v, w, d[3];
        const float m = scan_closest(p, a, ab, ac, v, w, d);          // the same bits as in the search
        double rho, drho;
        scan_rho(sigma, (double)m, rho, drho);
        s = (double)P.w * rho;
        if (acc) {
            const float bary[3] = {(1.f - v) - w, v, w};
            const double k2 = 2.0 * ldexp((double)P.w, expo[n]) * drho * SCAN_FIX;       // e_n = 0: the weight itself
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                unsigned long long* o = acc + ((size_t)n * nv + faces[(size_t)bj * 3 + k]) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double g = fmin(fmax(k2 * ((double)d[c] * (double)bary[k]), -9.0e18), 9.0e18);
                    atomicAdd(o + c, (unsigned long long)llrint(g));
                }
            }
        }
    }
    scan_block_sum(s, sh_d, partS + (size_t)n * gridDim.x + blockIdx.x);
}

// grid (ceil(nv / SCAN_NT), N): thread = (body n, vertex j).  SEARCH: the nearest participating point (term M).  Either way
// the vertex's gradient is finished here: g = w_m2s rho' 2 (v - p) + w_s2m 2^-e_n acc / 2^32.
template <bool SEARCH, bool GATED>
__global__ __launch_bounds__(SCAN_NT) void scan_m2s_kernel(const float* __restrict__ verts, int nv, const float4* __restrict__ pk,
                                                           const int* __restrict__ count, const int* __restrict__ expo, int Pmax,
                                                           float w_s2m, float w_m2s,
                                                           float sigma, const long long* __restrict__ acc,
                                                           float* __restrict__ g_verts, double* __restrict__ partM,
                                                           int32_t* __restrict__ nearest, ScanGate<GATED> G) {
    __shared__ __attribute__((aligned(16))) float4 sh[SEARCH ? SCAN_PT : 1];
    __shared__ double sh_d[SCAN_NT / 64];
    const int tid = threadIdx.x, n = blockIdx.y, j = blockIdx.x * SCAN_NT + tid;
    if (G.off(n)) return;                                            // (uniform)
    const bool live = j < nv;
    const float* pv = verts + ((size_t)n * nv + (live ? j : 0)) * 3;
    const float x[3] = {pv[0], pv[1], pv[2]};
    double g[3] = {0.0, 0.0, 0.0}, rho = 0.0;
    if (SEARCH) {
        const float4* pb = pk + (size_t)n * Pmax;
        const int np = count[n];
        unsigned best = 0x7f800001u;
        int bi = -1;
        for (int p0 = 0; p0 < np; p0 += SCAN_PT) {
            const int cnt = min(SCAN_PT, np - p0);
            __syncthreads();
            for (int t = tid; t < cnt; t += SCAN_NT) sh[t] = pb[p0 + t];
            __syncthreads();
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                const float4 q = sh[t];
                const float dx = x[0] - q.x, dy = x[1] - q.y, dz = x[2] - q.z;
                const unsigned mb = __builtin_bit_cast(unsigned, (dx * dx + dy * dy) + dz * dz);
                if (mb < best) { best = mb; bi = p0 + t; }
            }
        }
        if (live && nearest) nearest[(size_t)n * nv + j] = bi;
        if (live && bi >= 0) {
            const float4 q = pb[bi];
            const float d[3] = {x[0] - q.x, x[1] - q.y, x[2] - q.z};
            double drho;
            scan_rho(sigma, (double)((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), rho, drho);
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = (double)w_m2s * (drho * (2.0 * (double)d[c]));
        }
    }
    if (live && g_verts) {
        float* o = g_verts + ((size_t)n * nv + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double t = g[c];
            if (acc) t += (double)w_s2m * ldexp((double)acc[((size_t)n * nv + j) * 3 + c] / SCAN_FIX, -expo[n]);
            o[c] = (float)t;
        }
    }
    if (SEARCH) scan_block_sum(rho, sh_d, partM + (size_t)n * gridDim.x + blockIdx.x);
}

// grid (N), one wave: loss[n] = float32(w_s2m S_n + w_m2s M_n); a term whose partials are null is left out
template <bool GATED>
__global__ __launch_bounds__(64) void scan_sum_kernel(const double* __restrict__ partS, int nblkP, const double* __restrict__ partM,
                                                      int nblkV, float w_s2m, float w_m2s, float* __restrict__ loss, ScanGate<GATED> G) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (G.off(n)) return;
    double tot = 0.0;
    if (partS) {
        double s = 0.0;
        for (int k = lane; k < nblkP; k += 64) s += partS[(size_t)n * nblkP + k];
        tot += (double)w_s2m * wave64_sum(s);
    }
    if (partM) {
        double s = 0.0;
        for (int k = lane; k < nblkV; k += 64) s += partM[(size_t)n * nblkV + k];
        tot += (double)w_m2s * wave64_sum(s);
    }
    if (lane == 0) loss[n] = (float)tot;
}

// ========================================================================================================== host side
static int scan_fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}
#define SCAN_HIP(call)                                                                                       \
    do {                                                                                                     \
        hipError_t e__ = (call);                                                                             \
        if (e__ != hipSuccess) return scan_fail(err, MVFIT_E_HIP, "%s: %s", #call, hipGetErrorString(e__));  \
    } while (0)

static size_t scan_al(size_t x) { return (x + 255) & ~(size_t)255; }
static int scan_blocks(int n) { return (n + SCAN_NT - 1) / SCAN_NT; }

// arguments are checked by the caller (mvfit_scan.hip); a failure leaves no scan set behind
int scan_set(ScanState& S, int nv, int nf, int N, int Pmax, const float* points, const int32_t* count, const float* weights,
             hipStream_t stream, std::string& err) {
    S.on = false;
    const size_t np = (size_t)N * Pmax;
    const int ns = (nf + SCAN_SEED - 1) / SCAN_SEED;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += scan_al(bytes); return at; };
    const size_t o_pts = take(np * 12), o_w = take(np * 4), o_pk = take(np * 16), o_cnt = take((size_t)N * 8),
                 o_rec = take((size_t)N * nf * 64), o_seed = take((size_t)N * ns * 16), o_acc = take((size_t)N * nv * 24),
                 o_partS = take((size_t)N * scan_blocks(Pmax) * 8), o_partM = take((size_t)N * scan_blocks(nv) * 8);
    SCAN_HIP(hipStreamSynchronize(stream));      // an evaluation in flight may still read the workspace
    if (o != S.ws.size()) {                      // a set of the same sizes reuses the workspace
        S.ws.reset();
        SCAN_HIP(S.ws.reserve(o));
    }
    unsigned char* const ws = S.ws.as<unsigned char>();
    S.N = N; S.Pmax = Pmax; S.nv = nv; S.nf = nf; S.ns = ns;
    S.o_pts = o_pts; S.o_w = o_w; S.o_pk = o_pk; S.o_cnt = o_cnt; S.o_rec = o_rec; S.o_seed = o_seed; S.o_acc = o_acc;
    S.o_partS = o_partS; S.o_partM = o_partM;
    // effective weights: 0 beyond count[n], 1 without weights
    S.h_w.assign(np, 0.f);
    // and, behind the counts, e_n: term S's fixed-point sums of body n are taken with the weights times 2^e_n, which puts the
    // body's largest weight into [1, 2) - the accumulator's unit is then relative to the body's own weights, and a set
    // whose weights are scaled by a power of two keeps every bit of the sums (the scaling is undone in float64)
    S.h_cnt.assign((size_t)2 * N, 0);
    for (int n = 0; n < N; ++n) {
        float wmax = 0.f;
        for (int i = 0; i < count[n]; ++i) {
            const float w = weights ? weights[(size_t)n * Pmax + i] : 1.f;
            S.h_w[(size_t)n * Pmax + i] = w;
            wmax = std::fmax(wmax, w);
        }
        S.h_cnt[n] = count[n];
        S.h_cnt[(size_t)N + n] = wmax > 0.f ? -std::ilogb(wmax) : 0;
    }
    SCAN_HIP(hipMemcpyAsync(ws + o_pts, points, np * 12, hipMemcpyDefault, stream));
    SCAN_HIP(hipMemcpyAsync(ws + o_w, S.h_w.data(), np * 4, hipMemcpyHostToDevice, stream));
    SCAN_HIP(hipMemcpyAsync(ws + o_cnt, S.h_cnt.data(), (size_t)N * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(scan_pack_kernel, dim3(scan_blocks(Pmax), N), dim3(SCAN_NT), 0, stream,
                       reinterpret_cast<const float*>(ws + o_pts), reinterpret_cast<const float*>(ws + o_w), Pmax,
                       reinterpret_cast<float4*>(ws + o_pk));
    SCAN_HIP(hipGetLastError());
    SCAN_HIP(hipStreamSynchronize(stream));      // the caller's points and the staging vectors are free again
    S.on = true;
    return MVFIT_OK;
}

int scan_loss(ScanState& S, const int32_t* faces, const float* vertices, float w_s2m, float w_m2s, float sigma, bool exhaustive,
              float* loss, float* g_vertices, int32_t* nearest_face, int32_t* nearest_point, hipStream_t stream,
              std::string& err) {
    const int N = S.N, Pmax = S.Pmax, nv = S.nv, nf = S.nf, nblkP = scan_blocks(Pmax), nblkV = scan_blocks(nv);
    unsigned char* const ws = S.ws.as<unsigned char>();
    const float4* pk = reinterpret_cast<const float4*>(ws + S.o_pk);
    const int* count = reinterpret_cast<const int*>(ws + S.o_cnt);
    const int* expo = count + N;
    float4* rec = reinterpret_cast<float4*>(ws + S.o_rec);
    float4* seed = reinterpret_cast<float4*>(ws + S.o_seed);
    double* partS = reinterpret_cast<double*>(ws + S.o_partS);
    double* partM = reinterpret_cast<double*>(ws + S.o_partM);
    const bool termS = w_s2m > 0.f, termM = w_m2s > 0.f;
    unsigned long long* acc = termS && g_vertices ? reinterpret_cast<unsigned long long*>(ws + S.o_acc) : nullptr;
    if (termS) {
        if (acc) SCAN_HIP(hipMemsetAsync(acc, 0, (size_t)N * nv * 24, stream));
        hipLaunchKernelGGL(scan_face_kernel<false>, dim3(scan_blocks(nf), N), dim3(SCAN_NT), 0, stream, vertices, nv, faces, nf, S.ns,
                           rec, seed, ScanGate<false>{});
        if (exhaustive)
            hipLaunchKernelGGL((scan_s2m_kernel<false, false>), dim3(nblkP, N), dim3(SCAN_NT), 0, stream, pk, count, expo, Pmax,
                               (const float4*)rec, (const float4*)seed, nf, S.ns, faces, nv, sigma, acc, partS, nearest_face,
                               ScanGate<false>{});
        else
            hipLaunchKernelGGL((scan_s2m_kernel<true, false>), dim3(nblkP, N), dim3(SCAN_NT), 0, stream, pk, count, expo, Pmax,
                               (const float4*)rec, (const float4*)seed, nf, S.ns, faces, nv, sigma, acc, partS, nearest_face,
                               ScanGate<false>{});
    } else if (nearest_face) {
        SCAN_HIP(hipMemsetAsync(nearest_face, 0xff, (size_t)N * Pmax * 4, stream));
    }
    if (termM)
        hipLaunchKernelGGL((scan_m2s_kernel<true, false>), dim3(nblkV, N), dim3(SCAN_NT), 0, stream, vertices, nv, pk, count, expo, Pmax,
                           w_s2m, w_m2s, sigma, reinterpret_cast<const long long*>(acc), g_vertices, partM, nearest_point,
                           ScanGate<false>{});
    else {
        if (g_vertices)
            hipLaunchKernelGGL((scan_m2s_kernel<false, false>), dim3(nblkV, N), dim3(SCAN_NT), 0, stream, vertices, nv, pk, count, expo,
                               Pmax, w_s2m, w_m2s, sigma, reinterpret_cast<const long long*>(acc), g_vertices, partM,
                               (int32_t*)nullptr, ScanGate<false>{});
        if (nearest_point) SCAN_HIP(hipMemsetAsync(nearest_point, 0xff, (size_t)N * nv * 4, stream));
    }
    hipLaunchKernelGGL(scan_sum_kernel<false>, dim3(N), dim3(64), 0, stream, termS ? (const double*)partS : nullptr, nblkP,
                       termM ? (const double*)partM : nullptr, nblkV, w_s2m, w_m2s, loss, ScanGate<false>{});
    SCAN_HIP(hipGetLastError());
    return MVFIT_OK;
}

// One evaluation for the fit's chained rounds: scan_loss's sequence (culled search, loss and gradient, no nearest outputs) with
// the gated kernels.  No host work, no memset and no copy, so a stream capture records it as it is - kernel nodes only: the
// accumulators are cleared by scan_clear_kernel.  Per body the loss and the gradient are scan_loss's bits at the same vertices.
int scan_round(ScanState& S, const int32_t* faces, const float* vertices, float w_s2m, float w_m2s, float sigma, const int* gate,
               float* loss, float* g_vertices, hipStream_t stream, std::string& err) {
    const int N = S.N, Pmax = S.Pmax, nv = S.nv, nf = S.nf, nblkP = scan_blocks(Pmax), nblkV = scan_blocks(nv);
    unsigned char* const ws = S.ws.as<unsigned char>();
    const float4* pk = reinterpret_cast<const float4*>(ws + S.o_pk);
    const int* count = reinterpret_cast<const int*>(ws + S.o_cnt);
    const int* expo = count + N;
    float4* rec = reinterpret_cast<float4*>(ws + S.o_rec);
    float4* seed = reinterpret_cast<float4*>(ws + S.o_seed);
    double* partS = reinterpret_cast<double*>(ws + S.o_partS);
    double* partM = reinterpret_cast<double*>(ws + S.o_partM);
    const bool termS = w_s2m > 0.f, termM = w_m2s > 0.f;
    unsigned long long* acc = termS ? reinterpret_cast<unsigned long long*>(ws + S.o_acc) : nullptr;
    const ScanGate<true> G{gate};
    if (termS) {
        hipLaunchKernelGGL(scan_clear_kernel, dim3(scan_blocks(nv * 3), N), dim3(SCAN_NT), 0, stream, acc, nv, G);
        hipLaunchKernelGGL(scan_face_kernel<true>, dim3(scan_blocks(nf), N), dim3(SCAN_NT), 0, stream, vertices, nv, faces, nf, S.ns,
                           rec, seed, G);
        hipLaunchKernelGGL((scan_s2m_kernel<true, true>), dim3(nblkP, N), dim3(SCAN_NT), 0, stream, pk, count, expo, Pmax,
                           (const float4*)rec, (const float4*)seed, nf, S.ns, faces, nv, sigma, acc, partS, (int32_t*)nullptr, G);
    }
    if (termM)
        hipLaunchKernelGGL((scan_m2s_kernel<true, true>), dim3(nblkV, N), dim3(SCAN_NT), 0, stream, vertices, nv, pk, count, expo, Pmax,
                           w_s2m, w_m2s, sigma, reinterpret_cast<const long long*>(acc), g_vertices, partM, (int32_t*)nullptr, G);
    else
        hipLaunchKernelGGL((scan_m2s_kernel<false, true>), dim3(nblkV, N), dim3(SCAN_NT), 0, stream, vertices, nv, pk, count, expo, Pmax,
                           w_s2m, w_m2s, sigma, reinterpret_cast<const long long*>(acc), g_vertices, partM, (int32_t*)nullptr, G);
    hipLaunchKernelGGL(scan_sum_kernel<true>, dim3(N), dim3(64), 0, stream, termS ? (const double*)partS : nullptr, nblkP,
                       termM ? (const double*)partM : nullptr, nblkV, w_s2m, w_m2s, loss, G);
    SCAN_HIP(hipGetLastError());
    return MVFIT_OK;
}

}  // namespace mvfit
