// Silhouette loss against per-view person masks, with its gradient on the vertices (include/mvfit.h:
// mvfit_set_silhouettes / mvfit_silhouette_loss).  New ground: the reference has no term on the body's outline.
//
// Prepared once per mask set:
//   field D_i = float32(sqrt(float64(d2))), d2 the exact integer squared distance to the nearest on pixel: two separable
//       passes in integer arithmetic - sil_dt_cols_kernel (a thread per column: the squared vertical distance) and
//       sil_dt_rows_kernel (a workgroup per row, the row staged in LDS; per pixel a scan outwards that stops as soon as the
//       horizontal offset alone exceeds the best candidate, so it is exact) - in place in the field's own memory;
//   contour = on pixels with an off 4-neighbour inside the image, in raster order, every contour_stride-th kept:
//       count per row (a wave per row, ballots), prefix per image, fill - raster order without atomics.
// Per evaluation:
//   sil_search_kernel (the hot one): a workgroup owns 512 contour points of one image, projects the body's vertices in
//       tiles of SIL_VT into LDS ((u, v), NaN for pz <= 0.05) and every thread walks the tile for its two points - all lanes
//       read the same address (a broadcast, no bank conflict), two vertices per 128-bit read; the running minimum
//       (bits of m, j) stays in registers (unsigned compare: m >= 0 orders like its bits, a NaN compares above +inf).  The
//       winner's pixel-space gradient goes to a 64-bit fixed-point accumulator per (image, vertex) (integer atomics:
//       the sum does not depend on the order), rho_B to one float64 partial per workgroup (wave tree, waves in order).
//   sil_vertex_kernel: a thread per (body, vertex) walks the body's images in ascending order: projection, bilinear
//       sample of the field and its derivative (term A), plus term B's accumulated gradient, pulled back through the
//       projection into a float64 sum that is rounded and stored once.  Term A's loss: a float64 partial per (image, block).
//   sil_loss_kernel: a wave per body, its images in ascending order, per image the partials in order.
// No float atomics; nothing a body gets depends on the other bodies of the call or on its position in it.
// Inside the fit (mvfit_set_silhouette_term): sil_round launches the <GATED = true> instantiations of the three evaluation
// kernels on the stream a chained round is captured on; they skip the bodies whose gate word is 0.
// With occluders set (mvfit_set_silhouette_occluders, silhouette_occlusion.hip) the <., OCC = true> instantiations of the search
// and the vertex kernel run: hidden vertices and flagged contour points drop out of both terms.
#include "silhouette.h"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "mvfit.h"
#include "silhouette_device.h"
#include "wave_ops.h"

namespace mvfit {

constexpr int SIL_PPT = 2;                       // contour points per thread of the search
constexpr int SIL_CHUNK = SIL_NT * SIL_PPT;      // contour points per workgroup
constexpr int SIL_VT = 3456;                     // vertices per LDS tile: 27 KB, five workgroups per CU
constexpr int SIL_INF = 0x3fffffff;              // "no on pixel in this column": above every real d2 (< 2^28), sums stay in int32
constexpr int SIL_FAR = 1 << 20;
constexpr double SIL_FIX = 268435456.0;          // 2^28: fixed-point unit of term B's gradient accumulators (pixels)

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ distance transform
// grid (ceil(W / SIL_NT), M): a thread per column.  g2 = squared distance to the nearest on pixel of the column (SIL_INF:
// none); flags[i] |= 1 when image i has an on pixel (an idempotent integer atomic).
__global__ __launch_bounds__(SIL_NT) void sil_dt_cols_kernel(const uint8_t* __restrict__ mask, int H, int W,
                                                             int* __restrict__ g2, int* __restrict__ flags) {
    const int x = blockIdx.x * SIL_NT + threadIdx.x, i = blockIdx.y;
    if (x >= W) return;
    const uint8_t* m = mask + (size_t)i * H * W + x;
    int* g = g2 + (size_t)i * H * W + x;
    int d = -1;
    bool any = false;
    for (int y = 0; y < H; ++y) {
        if (m[(size_t)y * W]) { d = 0; any = true; } else if (d >= 0) ++d;
        g[(size_t)y * W] = d < 0 ? SIL_FAR : d;
    }
    d = -1;
    for (int y = H - 1; y >= 0; --y) {
        if (m[(size_t)y * W]) d = 0; else if (d >= 0) ++d;
        const int cur = g[(size_t)y * W];
        const int best = (d >= 0 && d < cur) ? d : cur;
        g[(size_t)y * W] = best >= SIL_FAR ? SIL_INF : best * best;
    }
    if (any) atomicOr(&flags[i], 1);
}

// grid (H, M), dynamic LDS W ints: a workgroup per row, in place.  d2(x) = min_x' (x - x')^2 + g2(x'): candidates are taken
// at growing offset k on both sides; once k^2 >= the best so far no further one can win.  An image without an on pixel
// reads back as zeros.
__global__ __launch_bounds__(SIL_NT) void sil_dt_rows_kernel(int* __restrict__ g2, int H, int W, const int* __restrict__ flags) {
    extern __shared__ int sil_row[];
    const int y = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    int* row = g2 + ((size_t)i * H + y) * W;
    float* out = reinterpret_cast<float*>(row);
    if (!flags[i]) {
        for (int x = tid; x < W; x += SIL_NT) out[x] = 0.f;
        return;
    }
    for (int x = tid; x < W; x += SIL_NT) sil_row[x] = row[x];
    __syncthreads();
    for (int x = tid; x < W; x += SIL_NT) {
        int best = sil_row[x];
        for (int k = 1; k < W; ++k) {
            const int kk = k * k;
            if (kk >= best) break;
            const bool l = x - k >= 0, r = x + k < W;
            if (!l && !r) break;
            if (l) best = min(best, kk + sil_row[x - k]);
            if (r) best = min(best, kk + sil_row[x + k]);
        }
        out[x] = (float)sqrt((double)best);
    }
}

// ------------------------------------------------------------------------------------------------------------ contour
__device__ __forceinline__ bool sil_is_contour(const uint8_t* __restrict__ m, int H, int W, int x, int y) {
    const uint8_t* p = m + (size_t)y * W + x;
    if (!p[0]) return false;
    return (x > 0 && !p[-1]) || (x < W - 1 && !p[1]) || (y > 0 && !p[-(ptrdiff_t)W]) || (y < H - 1 && !p[W]);
}

// grid (ceil(H / 4), M): a wave per row.  FILL = false: row_cnt[i * H + y] = contour pixels of the row.  FILL = true:
// row_cnt holds the row's exclusive offset within its image; the k-th point of the image is kept iff k % stride == 0 and
// goes to xy[first[i] + k / stride].
template <bool FILL>
__global__ __launch_bounds__(SIL_NT) void sil_contour_kernel(const uint8_t* __restrict__ mask, int H, int W,
                                                             int* __restrict__ row_cnt, int stride,
                                                             const int* __restrict__ first, int2* __restrict__ xy) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * (SIL_NT / 64) + (threadIdx.x >> 6), i = blockIdx.y;
    if (y >= H) return;
    const uint8_t* m = mask + (size_t)i * H * W;
    int run = FILL ? row_cnt[(size_t)i * H + y] : 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool c = x < W && sil_is_contour(m, H, W, x, y);
        const unsigned long long bal = __ballot(c);
        if (FILL && c) {
            const int k = run + __popcll(bal & ((1ull << lane) - 1ull));
            if (k % stride == 0) xy[(size_t)first[i] + k / stride] = make_int2(x, y);
        }
        run += __popcll(bal);
    }
    if (!FILL && lane == 0) row_cnt[(size_t)i * H + y] = run;
}

// grid (M): the rows' counts of image i -> exclusive offsets in place, total[i] = the image's contour pixels
__global__ __launch_bounds__(SIL_NT) void sil_scan_kernel(int* __restrict__ row_cnt, int H, int* __restrict__ total) {
    __shared__ int sh[SIL_NT];
    const int i = blockIdx.x, tid = threadIdx.x;
    int* r = row_cnt + (size_t)i * H;
    const int per = (H + SIL_NT - 1) / SIL_NT, y0 = min(H, tid * per), y1 = min(H, y0 + per);
    int s = 0;
    for (int y = y0; y < y1; ++y) s += r[y];
    sh[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int t = 0; t < SIL_NT; ++t) { const int c = sh[t]; sh[t] = a; a += c; }
        total[i] = a;
    }
    __syncthreads();
    int a = sh[tid];
    for (int y = y0; y < y1; ++y) { const int c = r[y]; r[y] = a; a += c; }
}

// The gate of the term inside the fit's chained rounds (sil_round): gate[body] == 0 - a finished problem, or a stage without
// the term - ends the workgroup at once; a null pointer keeps every body.  The ungated instantiations carry an empty
// argument and are the kernels as they were.
template <bool GATED> struct SilGate { __device__ __forceinline__ bool off(int) const { return false; } };
template <> struct SilGate<true> {
    const int* gate;
    __device__ __forceinline__ bool off(int body) const { return gate && !gate[body]; }
};

// What the search and the vertex kernel take beside their data: the gate and the occluders in one argument, so that the
// instantiations without occluders have the argument list - and with it the code - they had before occluders existed.
template <bool GATED, bool OCC> struct SilPolicy : SilGate<GATED>, SilOcc<OCC> {};

// ------------------------------------------------------------------------------------------------ term B: the search
// grid (chunks): SIL_CHUNK contour points of one image against all vertices of its body.
// acc[(image * nv + j) * 2 + {0, 1}] += round(2^28 * stride * rho_B'(m) * 2 (dx, dy)); partB[chunk] = sum of rho_B.
// OCC (occluders are set, silhouette_device.h: SilOcc): a hidden vertex is NaN in the tile like an invalid one, a flagged
// point contributes nothing and reports winner -2.
template <bool GATED, bool OCC>
__global__ __launch_bounds__(SIL_NT) void sil_search_kernel(const float* __restrict__ verts, int nv, const SilCam* __restrict__ cams,
                                                            const int* __restrict__ image_body,
                                                            const SilChunk* __restrict__ chunks, const int2* __restrict__ xy,
                                                            float sigma, int stride, unsigned long long* __restrict__ acc,
                                                            double* __restrict__ partB, int* __restrict__ winner,
                                                            SilPolicy<GATED, OCC> pol) {
    __shared__ __attribute__((aligned(16))) float2 sh_uv[SIL_VT];
    __shared__ double sh_d[SIL_NT / 64];
    static_assert(SIL_VT % 2 == 0, "two vertices per read");
    const int tid = threadIdx.x;
    const SilChunk ch = chunks[blockIdx.x];
    if (GATED && pol.off(image_body[ch.image])) return;           // (uniform)
    const SilCam cam = cams[ch.image];
    const float* vb = verts + (size_t)image_body[ch.image] * nv * 3;
    float cx[SIL_PPT], cy[SIL_PPT];
    unsigned best[SIL_PPT];
    int bj[SIL_PPT];
#pragma unroll
    for (int p = 0; p < SIL_PPT; ++p) {
        const int k = tid + p * SIL_NT;
        const int2 q = k < ch.count ? xy[(size_t)ch.first + k] : make_int2(0, 0);
        cx[p] = (float)q.x + 0.5f; cy[p] = (float)q.y + 0.5f;
        best[p] = 0x7f800001u;                   // above +inf: a valid vertex always wins over "none"
        bj[p] = -1;
    }
    const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
    for (int v0 = 0; v0 < nv; v0 += SIL_VT) {
        const int n = min(SIL_VT, nv - v0);
        __syncthreads();
        for (int j = tid; j < n; j += SIL_NT) {
            float px, py, pz, u, w;
            bool ok = sil_project(cam, vb + (size_t)(v0 + j) * 3, px, py, pz, u, w);
            if (OCC && ok && pol.hidden(ch.image, u, w, pz)) ok = false;
            sh_uv[j] = ok ? make_float2(u, w) : make_float2(qnan, qnan);
        }
        if (tid == 0 && (n & 1)) sh_uv[n] = make_float2(qnan, qnan);       // n odd => n < SIL_VT
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < n; j += 2) {
            const float4 q = *reinterpret_cast<const float4*>(&sh_uv[j]);
#pragma unroll
            for (int p = 0; p < SIL_PPT; ++p) {
                float dx = q.x - cx[p], dy = q.y - cy[p];
                unsigned mb = __builtin_bit_cast(unsigned, dx * dx + dy * dy);
                if (mb < best[p]) { best[p] = mb; bj[p] = v0 + j; }
                dx = q.z - cx[p]; dy = q.w - cy[p];
                mb = __builtin_bit_cast(unsigned, dx * dx + dy * dy);
                if (mb < best[p]) { best[p] = mb; bj[p] = v0 + j + 1; }
            }
        }
    }
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < SIL_PPT; ++p) {
        const int k = tid + p * SIL_NT;
        if (k >= ch.count) continue;
        if (OCC && pol.flagged((size_t)ch.first + k)) {
            if (winner) winner[(size_t)ch.first + k] = -2;
            continue;
        }
        if (winner) winner[(size_t)ch.first + k] = bj[p];
        if (bj[p] < 0) continue;
        float px, py, pz, u, w;
        sil_project(cam, vb + (size_t)bj[p] * 3, px, py, pz, u, w);       // the same bits as in the tile
        const float dx = u - cx[p], dy = w - cy[p];
        const double m = (double)(dx * dx + dy * dy);
        double rho = m, drho = 1.0;
        if (sigma > 0.f) {
            const double s2 = (double)sigma * (double)sigma, den = s2 + m;
            rho = s2 * m / den;
            drho = (s2 / den) * (s2 / den);
        }
        s += rho;
        if (acc) {
            const double k2 = 2.0 * (double)stride * drho * SIL_FIX;
            const double gx = fmin(fmax(k2 * (double)dx, -9.0e18), 9.0e18), gy = fmin(fmax(k2 * (double)dy, -9.0e18), 9.0e18);
            unsigned long long* a = acc + ((size_t)ch.image * nv + bj[p]) * 2;
            atomicAdd(a + 0, (unsigned long long)llrint(gx));
            atomicAdd(a + 1, (unsigned long long)llrint(gy));
        }
    }
    s = wave64_sum(s);
    if ((tid & 63) == 0) sh_d[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = sh_d[0];
        for (int w = 1; w < SIL_NT / 64; ++w) t += sh_d[w];
        partB[blockIdx.x] = t;
    }
}

// --------------------------------------------------------------------------------- term A and the pull-back of both terms
// first index s in sbody[0 .. M) with sbody[s] >= n
__device__ __forceinline__ int sil_lower_bound(const int* __restrict__ sbody, int M, int n) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sbody[mid] < n) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (ceil(nv / SIL_NT), N): thread = (body n, vertex j).  sbody / simg: the images sorted by (body, image).
// partA[i * gridDim.x + blockIdx.x] = the workgroup's sum of rho_A in image i.  OCC: a vertex hidden in image i gets
// nothing from it, like an invalid one.
template <bool GATED, bool OCC>
__global__ __launch_bounds__(SIL_NT) void sil_vertex_kernel(const float* __restrict__ verts, int nv, const SilCam* __restrict__ cams,
                                                            const int* __restrict__ sbody, const int* __restrict__ simg, int M,
                                                            const float* __restrict__ field, int H, int W,
                                                            const int* __restrict__ flags, float w_in, float w_out, float sigma,
                                                            const long long* __restrict__ acc, float* __restrict__ g_verts,
                                                            double* __restrict__ partA, SilPolicy<GATED, OCC> pol) {
    __shared__ double sh_d[SIL_NT / 64];
    const int n = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * SIL_NT + tid;
    if (GATED && pol.off(n)) return;                                // (uniform)
    const bool live = j < nv;
    const float* pv = verts + ((size_t)n * nv + (live ? j : 0)) * 3;
    double g[3] = {0.0, 0.0, 0.0};
    const double s2 = (double)sigma * (double)sigma;
    for (int s = sil_lower_bound(sbody, M, n); s < M && sbody[s] == n; ++s) {
        const int i = simg[s];
        double rho = 0.0;
        if (live && flags[i]) {
            const SilCam cam = cams[i];
            float px, py, pz, u, w;
            if (sil_project(cam, pv, px, py, pz, u, w) && !(OCC && pol.hidden(i, u, w, pz))) {
                const float x = u - 0.5f, y = w - 0.5f;
                const float xc = fminf(fmaxf(x, 0.f), (float)(W - 1)), yc = fminf(fmaxf(y, 0.f), (float)(H - 1));
                const int x0 = min((int)floorf(xc), W - 2), y0 = min((int)floorf(yc), H - 2);
                const double a = (double)(xc - (float)x0), b = (double)(yc - (float)y0);
                const float* f = field + (size_t)i * H * W + (size_t)y0 * W + x0;
                const double D00 = (double)f[0], D01 = (double)f[1], D10 = (double)f[W], D11 = (double)f[W + 1];
                const double d = (1.0 - b) * ((1.0 - a) * D00 + a * D01) + b * ((1.0 - a) * D10 + a * D11);
                const double ddx = x == xc ? (1.0 - b) * (D01 - D00) + b * (D11 - D10) : 0.0;
                const double ddy = y == yc ? (1.0 - a) * (D10 - D00) + a * (D11 - D01) : 0.0;
                double drdd = 2.0 * d;
                rho = d * d;
                if (sigma > 0.f) {
                    const double den = s2 + d * d;
                    rho = s2 * (d * d) / den;
                    drdd = 2.0 * d * ((s2 / den) * (s2 / den));
                }
                if (g_verts) {
                    double gu = (double)w_in * drdd * ddx, gv = (double)w_in * drdd * ddy;
                    if (acc) {
                        const long long* ac = acc + ((size_t)i * nv + j) * 2;
                        gu += (double)w_out * ((double)ac[0] / SIL_FIX);
                        gv += (double)w_out * ((double)ac[1] / SIL_FIX);
                    }
                    const double k = (double)cam.f / (double)pz;
                    const double gpx = k * gu, gpy = k * gv, gpz = -k * (gu * (double)px + gv * (double)py) / (double)pz;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        g[c] += ((double)cam.R[c] * gpx + (double)cam.R[3 + c] * gpy) + (double)cam.R[6 + c] * gpz;
                }
            }
        }
        rho = wave64_sum(rho);
        if ((tid & 63) == 0) sh_d[tid >> 6] = rho;
        __syncthreads();
        if (tid == 0) {
            double t = sh_d[0];
            for (int w = 1; w < SIL_NT / 64; ++w) t += sh_d[w];
            partA[(size_t)i * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();
    }
    if (live && g_verts) {
        float* o = g_verts + ((size_t)n * nv + j) * 3;
        o[0] = (float)g[0]; o[1] = (float)g[1]; o[2] = (float)g[2];
    }
}

// the wave's total of the lane-strided sums of p[0 .. n), valid in every lane
__device__ __forceinline__ double sil_ordered_sum(const double* __restrict__ p, int n, int lane) {
    double a = 0.0;
    for (int k = lane; k < n; k += 64) a += p[k];
    return wave64_sum(a);
}

// grid (N), one wave: loss[n] = sum over the body's images, ascending, of w_in A_i + w_out stride B_i
template <bool GATED>
__global__ __launch_bounds__(64) void sil_loss_kernel(const int* __restrict__ sbody, const int* __restrict__ simg, int M,
                                                      const double* __restrict__ partA, int nblk,
                                                      const double* __restrict__ partB, const int* __restrict__ chunk_first,
                                                      float w_in, float w_out, int stride, float* __restrict__ loss,
                                                      SilGate<GATED> gate) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (GATED && gate.off(n)) return;
    double tot = 0.0;
    for (int s = sil_lower_bound(sbody, M, n); s < M && sbody[s] == n; ++s) {
        const int i = simg[s];
        const double A = sil_ordered_sum(partA + (size_t)i * nblk, nblk, lane);
        const int c0 = chunk_first[i], c1 = chunk_first[i + 1];
        const double B = c1 > c0 ? sil_ordered_sum(partB + c0, c1 - c0, lane) : 0.0;
        tot += (double)w_in * A + (double)w_out * ((double)stride * B);
    }
    if (lane == 0) loss[n] = (float)tot;
}

// grid (ceil(nv / SIL_NT), M): term B's accumulators of the images whose body is live -> 0 (one 16-byte store per (image,
// vertex)).  The rounds' form of sil_loss's memset, as a kernel: a captured round then holds kernel nodes only.  A workaround
// for an observation, not for an understood mechanism: with a memset node here, a two-stage fit that
// replayed an earlier fit's graph on the idle stream behind its lead phase had the closure's loss and another gradient in its
// first round, for the bodies with images only.  A gated-off body's accumulators keep what they hold: its search and vertex
// workgroups return before they touch them.
__global__ __launch_bounds__(SIL_NT) void sil_clear_kernel(unsigned long long* __restrict__ acc, int nv,
                                                           const int* __restrict__ image_body, SilGate<true> gate) {
    const int j = blockIdx.x * SIL_NT + threadIdx.x, i = blockIdx.y;
    if (gate.off(image_body[i]) || j >= nv) return;
    *reinterpret_cast<ulonglong2*>(acc + ((size_t)i * nv + j) * 2) = make_ulonglong2(0ull, 0ull);
}

// ========================================================================================================== host side
static int sil_fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}
#define SIL_HIP(call)                                                                                        \
    do {                                                                                                     \
        hipError_t e__ = (call);                                                                             \
        if (e__ != hipSuccess) return sil_fail(err, MVFIT_E_HIP, "%s: %s", #call, hipGetErrorString(e__));   \
    } while (0)

static size_t sil_al(size_t x) { return (x + 255) & ~(size_t)255; }

int sil_set(SilState& S, int nv, int M, int H, int W, const uint8_t* masks, const int32_t* image_body, const float* cam_R,
            const float* cam_t, const float* cam_f, const float* cam_c, int stride, hipStream_t stream, std::string& err) {
    S.on = false;                                // a failed set leaves no mask set behind
    S.occ_on = false;                            // the occluders belong to the mask set: every set clears them
    const int nblk = (nv + SIL_NT - 1) / SIL_NT;
    const size_t npix = (size_t)M * H * W;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += sil_al(bytes); return at; };
    const size_t o_field = take(npix * 4), o_mask = take(npix), o_row = take((size_t)M * H * 4), o_flags = take((size_t)M * 4),
                 o_total = take((size_t)M * 4), o_cam = take((size_t)M * sizeof(SilCam)), o_body = take((size_t)M * 4),
                 o_sbody = take((size_t)M * 4), o_simg = take((size_t)M * 4), o_first = take((size_t)(M + 1) * 4),
                 o_cfirst = take((size_t)(M + 1) * 4), o_acc = take((size_t)M * nv * 16), o_partA = take((size_t)M * nblk * 8);
    if (o != S.ws.size()) {                      // a set of the same size reuses the workspace
        SIL_HIP(hipStreamSynchronize(stream));
        S.ws.reset();
        SIL_HIP(S.ws.reserve(o));
    }
    unsigned char* const ws = S.ws.as<unsigned char>();
    S.M = M; S.H = H; S.W = W; S.stride = stride; S.nv = nv; S.C = 0; S.nchunks = 0;
    S.o_field = o_field; S.o_mask = o_mask; S.o_row = o_row; S.o_flags = o_flags; S.o_total = o_total; S.o_cam = o_cam;
    S.o_body = o_body; S.o_sbody = o_sbody; S.o_simg = o_simg; S.o_first = o_first; S.o_cfirst = o_cfirst; S.o_acc = o_acc;
    S.o_partA = o_partA;
    // tables: cameras, image -> body, the images sorted by (body, image)
    std::vector<int> order(M);
    for (int i = 0; i < M; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return image_body[a] < image_body[b]; });
    S.body_min = INT_MAX; S.body_max = INT_MIN;
    S.h_body.assign(image_body, image_body + M);
    for (int i = 0; i < M; ++i) { S.body_min = std::min(S.body_min, image_body[i]); S.body_max = std::max(S.body_max, image_body[i]); }
    const size_t tab_bytes = o_first - o_cam;
    S.h_tab.assign(tab_bytes / 4, 0);
    unsigned char* hb = reinterpret_cast<unsigned char*>(S.h_tab.data());
    for (int i = 0; i < M; ++i) {
        SilCam c;
        memcpy(c.R, cam_R + (size_t)i * 9, 36);
        memcpy(c.t, cam_t + (size_t)i * 3, 12);
        c.f = cam_f[i]; c.cx = cam_c[2 * i]; c.cy = cam_c[2 * i + 1]; c.pad = 0.f;
        memcpy(hb + (size_t)i * sizeof(SilCam), &c, sizeof(SilCam));
        reinterpret_cast<int32_t*>(hb + (o_body - o_cam))[i] = image_body[i];
        reinterpret_cast<int32_t*>(hb + (o_sbody - o_cam))[i] = image_body[order[i]];
        reinterpret_cast<int32_t*>(hb + (o_simg - o_cam))[i] = order[i];
    }
    SIL_HIP(hipMemcpyAsync(ws + o_cam, hb, tab_bytes, hipMemcpyHostToDevice, stream));
    SIL_HIP(hipMemcpyAsync(ws + o_mask, masks, npix, hipMemcpyDefault, stream));
    SIL_HIP(hipMemsetAsync(ws + o_flags, 0, (size_t)M * 4, stream));
    const uint8_t* d_mask = ws + o_mask;
    int* g2 = reinterpret_cast<int*>(ws + o_field);
    int* flags = reinterpret_cast<int*>(ws + o_flags);
    int* row = reinterpret_cast<int*>(ws + o_row);
    int* total = reinterpret_cast<int*>(ws + o_total);
    hipLaunchKernelGGL(sil_dt_cols_kernel, dim3((W + SIL_NT - 1) / SIL_NT, M), dim3(SIL_NT), 0, stream, d_mask, H, W, g2, flags);
    hipLaunchKernelGGL(sil_dt_rows_kernel, dim3(H, M), dim3(SIL_NT), (size_t)W * 4, stream, g2, H, W, (const int*)flags);
    const dim3 cgrid((H + SIL_NT / 64 - 1) / (SIL_NT / 64), M);
    hipLaunchKernelGGL(sil_contour_kernel<false>, cgrid, dim3(SIL_NT), 0, stream, d_mask, H, W, row, stride,
                       (const int*)nullptr, (int2*)nullptr);
    hipLaunchKernelGGL(sil_scan_kernel, dim3(M), dim3(SIL_NT), 0, stream, row, H, total);
    SIL_HIP(hipGetLastError());
    std::vector<int32_t> h_total(M);
    SIL_HIP(hipMemcpyAsync(h_total.data(), total, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    SIL_HIP(hipStreamSynchronize(stream));
    // contour_first over the kept points, and the search's chunks: each image's points in runs of SIL_CHUNK from its own start
    std::vector<int32_t> first(M + 1, 0), cfirst(M + 1, 0);
    long long C = 0, nch = 0;
    for (int i = 0; i < M; ++i) {
        const long long kept = ((long long)h_total[i] + stride - 1) / stride;
        C += kept; nch += (kept + SIL_CHUNK - 1) / SIL_CHUNK;
        if (C > INT_MAX) return sil_fail(err, MVFIT_E_UNSUPPORTED, "mvfit_set_silhouettes: more than 2^31 - 1 contour points");
        first[i + 1] = (int32_t)C; cfirst[i + 1] = (int32_t)nch;
    }
    std::vector<SilChunk> chunks((size_t)nch);
    for (int i = 0; i < M; ++i)
        for (int c = cfirst[i]; c < cfirst[i + 1]; ++c) {
            const int off = (c - cfirst[i]) * SIL_CHUNK;
            chunks[c] = SilChunk{i, first[i] + off, std::min(SIL_CHUNK, first[i + 1] - first[i] - off), 0};
        }
    size_t oc = 0;
    auto takec = [&oc](size_t bytes) { const size_t at = oc; oc += sil_al(bytes); return at; };
    S.o_xy = takec((size_t)C * 8); S.o_chunk = takec((size_t)nch * sizeof(SilChunk)); S.o_partB = takec((size_t)nch * 8);
    SIL_HIP(S.cs.reserve(oc));
    unsigned char* const cs = S.cs.as<unsigned char>();
    SIL_HIP(hipMemcpyAsync(ws + o_first, first.data(), (size_t)(M + 1) * 4, hipMemcpyHostToDevice, stream));
    SIL_HIP(hipMemcpyAsync(ws + o_cfirst, cfirst.data(), (size_t)(M + 1) * 4, hipMemcpyHostToDevice, stream));
    if (nch) {
        SIL_HIP(hipMemcpyAsync(cs + S.o_chunk, chunks.data(), (size_t)nch * sizeof(SilChunk), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(sil_contour_kernel<true>, cgrid, dim3(SIL_NT), 0, stream, d_mask, H, W, row, stride,
                           reinterpret_cast<const int*>(ws + o_first), reinterpret_cast<int2*>(cs + S.o_xy));
        SIL_HIP(hipGetLastError());
    }
    SIL_HIP(hipStreamSynchronize(stream));       // the host tables above are free again
    S.C = (int)C; S.nchunks = (int)nch;
    S.on = true;
    return MVFIT_OK;
}

int sil_read(const SilState& S, float* field, int32_t* contour_first, int32_t* contour_xy, hipStream_t stream, std::string& err) {
    const unsigned char *ws = S.ws.as<unsigned char>(), *cs = S.cs.as<unsigned char>();
    if (field) SIL_HIP(hipMemcpyAsync(field, ws + S.o_field, (size_t)S.M * S.H * S.W * 4, hipMemcpyDeviceToDevice, stream));
    if (contour_first)
        SIL_HIP(hipMemcpyAsync(contour_first, ws + S.o_first, (size_t)(S.M + 1) * 4, hipMemcpyDeviceToDevice, stream));
    if (contour_xy && S.C)
        SIL_HIP(hipMemcpyAsync(contour_xy, cs + S.o_xy, (size_t)S.C * 8, hipMemcpyDeviceToDevice, stream));
    return MVFIT_OK;
}

static SilGate<false> sil_gate(std::false_type, const int*) { return {}; }
static SilGate<true> sil_gate(std::true_type, const int* gate) { return SilGate<true>{gate}; }
static SilOcc<false> sil_occ(std::false_type, const SilState&) { return {}; }
static SilOcc<true> sil_occ(std::true_type, const SilState& S) {
    const unsigned char* oc = S.occ.as<unsigned char>();
    return SilOcc<true>{reinterpret_cast<const float*>(oc + S.o_zocc), oc + S.o_pflag, S.H, S.W, S.occ_margin};
}

// search -> vertex kernel -> loss kernel of one evaluation; acc: the zeroed fixed-point accumulators, or null (loss only)
template <bool GATED, bool OCC>
static void sil_launch(SilState& S, const float* vertices, int num_bodies, float w_in, float w_out, float sigma, const int* gate,
                       unsigned long long* acc, float* loss, float* g_vertices, int32_t* winner, hipStream_t stream) {
    const int nv = S.nv, nblk = (nv + SIL_NT - 1) / SIL_NT;
    unsigned char *ws = S.ws.as<unsigned char>(), *cs = S.cs.as<unsigned char>();
    const SilCam* cams = reinterpret_cast<const SilCam*>(ws + S.o_cam);
    const int* sbody = reinterpret_cast<const int*>(ws + S.o_sbody);
    const int* simg = reinterpret_cast<const int*>(ws + S.o_simg);
    const SilGate<GATED> g = sil_gate(std::integral_constant<bool, GATED>{}, gate);
    const SilPolicy<GATED, OCC> pol{g, sil_occ(std::integral_constant<bool, OCC>{}, S)};
    if (S.nchunks)
        hipLaunchKernelGGL((sil_search_kernel<GATED, OCC>), dim3(S.nchunks), dim3(SIL_NT), 0, stream, vertices, nv, cams,
                           reinterpret_cast<const int*>(ws + S.o_body), reinterpret_cast<const SilChunk*>(cs + S.o_chunk),
                           reinterpret_cast<const int2*>(cs + S.o_xy), sigma, S.stride, acc,
                           reinterpret_cast<double*>(cs + S.o_partB), winner, pol);
    hipLaunchKernelGGL((sil_vertex_kernel<GATED, OCC>), dim3(nblk, num_bodies), dim3(SIL_NT), 0, stream, vertices, nv, cams, sbody,
                       simg, S.M, reinterpret_cast<const float*>(ws + S.o_field), S.H, S.W,
                       reinterpret_cast<const int*>(ws + S.o_flags), w_in, w_out, sigma, reinterpret_cast<const long long*>(acc),
                       g_vertices, reinterpret_cast<double*>(ws + S.o_partA), pol);
    hipLaunchKernelGGL(sil_loss_kernel<GATED>, dim3(num_bodies), dim3(64), 0, stream, sbody, simg, S.M,
                       reinterpret_cast<const double*>(ws + S.o_partA), nblk,
                       reinterpret_cast<const double*>(cs + S.o_partB), reinterpret_cast<const int*>(ws + S.o_cfirst), w_in,
                       w_out, S.stride, loss, g);
}

// with occluders set (mvfit_set_silhouette_occluders) the <., OCC = true> instantiations run, otherwise the kernels as they were
int sil_loss(SilState& S, const float* vertices, int num_bodies, float w_in, float w_out, float sigma, float* loss,
             float* g_vertices, int32_t* winner, hipStream_t stream, std::string& err) {
    const bool accumulate = g_vertices && S.nchunks;
    unsigned long long* acc = accumulate ? reinterpret_cast<unsigned long long*>(S.ws.as<unsigned char>() + S.o_acc) : nullptr;
    if (accumulate) SIL_HIP(hipMemsetAsync(acc, 0, (size_t)S.M * S.nv * 16, stream));
    if (S.occ_on) sil_launch<false, true>(S, vertices, num_bodies, w_in, w_out, sigma, nullptr, acc, loss, g_vertices, winner, stream);
    else sil_launch<false, false>(S, vertices, num_bodies, w_in, w_out, sigma, nullptr, acc, loss, g_vertices, winner, stream);
    SIL_HIP(hipGetLastError());
    return MVFIT_OK;
}

// One evaluation for the fit's chained rounds: sil_loss's sequence with the gated kernels, every body's loss and vertex
// gradient; no host work, so a stream capture records it as it is (four kernel nodes: the accumulators are cleared by a
// kernel, not by a memset node - sil_clear_kernel).
int sil_round(SilState& S, const float* vertices, int num_bodies, float w_in, float w_out, float sigma, const int* gate,
              float* loss, float* g_vertices, hipStream_t stream, std::string& err) {
    unsigned long long* acc = S.nchunks ? reinterpret_cast<unsigned long long*>(S.ws.as<unsigned char>() + S.o_acc) : nullptr;
    if (acc)
        hipLaunchKernelGGL(sil_clear_kernel, dim3((S.nv + SIL_NT - 1) / SIL_NT, S.M), dim3(SIL_NT), 0, stream, acc, S.nv,
                           reinterpret_cast<const int*>(S.ws.as<unsigned char>() + S.o_body), SilGate<true>{gate});
    if (S.occ_on) sil_launch<true, true>(S, vertices, num_bodies, w_in, w_out, sigma, gate, acc, loss, g_vertices, nullptr, stream);
    else sil_launch<true, false>(S, vertices, num_bodies, w_in, w_out, sigma, gate, acc, loss, g_vertices, nullptr, stream);
    SIL_HIP(hipGetLastError());
    return MVFIT_OK;
}

}  // namespace mvfit
