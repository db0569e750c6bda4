// Refinement of the rig's cameras against held bodies (mvfit_camera_normal_eqs, mvfit_refine_cameras): the keypoint data
// term of the closure restricted to one view, as a function of that view's camera, with its gradient and Gauss-Newton matrix,
// and a Levenberg-Marquardt loop over them.  Given the bodies the views are independent: one workgroup of 256 threads per
// view, all float64 with contraction off (include/mvfit.h states the arithmetic, tests/camera_refine_oracle.py restates it in
// NumPy).  A camera is 15 doubles in the order of project.hip's LDS rows: R (9, row-major), t (3), f, cx, cy; its 9 parameters
// are omega (3), dt (3), f, cx, cy, a perturbation of the camera frame: p' = exp([omega]x) p + dt.
//
//   cr_eval     points i = b * 17 + j strided over the threads; E, g (9), the upper triangle of H (45), the number of counted
//               points and of counted points behind the camera accumulate in registers (57 doubles), then meet per wave
//               through wave64_sum (DPP rows, permlane swaps) and across the four waves through LDS, added in wave order by
//               whoever reads them.  No atomics: a view's sums depend on that view's inputs and on B only.
//   cr_lm       the loop is wave-uniform: every pass of the workgroup over the points is followed by lane 0 of wave 0 deciding
//               (accept / reject / stop), factoring the damped matrix and publishing the next candidate camera through LDS.
//               A candidate pass is the full pass, so E' of a candidate and E of the accepted point are one summation.  The
//               9 x 9 Cholesky runs unrolled in registers over all nine parameters: a parameter that is not free has the
//               row and column of the identity and gradient 0, which leaves the free block's operations with added exact
//               zeros - the bits of the factorisation of H[free, free] - and its step at 0.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops.h"
#include "launchers.h"

namespace mvfit {

constexpr int CR_NT = 256;
constexpr int CR_J = 17;
constexpr int CR_NP = 9;                // parameters of a camera
constexpr int CR_NH = 45;               // upper triangle of H
constexpr int CR_NS = 1 + CR_NP + CR_NH + 2;   // E, g, H, count, behind
constexpr int CR_CAM = 15;

__host__ __device__ constexpr int cr_tri(int i, int j) { return i * CR_NP - i * (i - 1) / 2 + (j - i); }   // i <= j
__host__ __device__ constexpr int cr_group(int i) { return i < 3 ? 0 : i < 6 ? 1 : i == 6 ? 2 : 3; }        // bit of free_mask

// One pass of the workgroup over the view's points at camera cam; the per-wave sums land in part[wave][.].  The caller puts a
// barrier between this and the reads.
__device__ __forceinline__ void cr_eval(const double (&cam)[CR_CAM], const float* __restrict__ joints,
                                        const float* __restrict__ gt_xy, const float* __restrict__ w_conf, int B, int V, int v,
                                        double rho2, double k0, double (*part)[CR_NS]) {
    double acc[CR_NS];
#pragma unroll
    for (int q = 0; q < CR_NS; ++q) acc[q] = 0.0;
    const double rho4 = rho2 * rho2, f = cam[12];
    const int n = B * CR_J;
    for (int i = threadIdx.x; i < n; i += CR_NT) {
        const int b = i / CR_J, j = i - b * CR_J;
        const size_t o = ((size_t)b * V + v) * CR_J + j;
        const double w = (double)w_conf[o];
        if (w == 0.0) continue;
        acc[CR_NS - 2] += 1.0;
        const double X = (double)joints[(size_t)i * 3], Y = (double)joints[(size_t)i * 3 + 1], Z = (double)joints[(size_t)i * 3 + 2];
        const double px = ((cam[0] * X + cam[1] * Y) + cam[2] * Z) + cam[9];
        const double py = ((cam[3] * X + cam[4] * Y) + cam[5] * Z) + cam[10];
        const double pz = ((cam[6] * X + cam[7] * Y) + cam[8] * Z) + cam[11];
        if (!(pz > 1e-6)) { acc[CR_NS - 1] += 1.0; continue; }
        const double a = px / pz, bb = py / pz, fz = f / pz;
        const double r[2] = {(double)gt_xy[o * 2] - (f * a + cam[13]), (double)gt_xy[o * 2 + 1] - (f * bb + cam[14])};
        const double k = k0 * (w * w);
        const double J[2][CR_NP] = {
            {-((f * a) * bb), f + (f * a) * a, -(f * bb), fz, 0.0, -(fz * a), a, 1.0, 0.0},
            {-(f + (f * bb) * bb), (f * a) * bb, f * a, 0.0, fz, -(fz * bb), bb, 0.0, 1.0}};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double r2 = r[e] * r[e], d = r2 + rho2;
            acc[0] += k * ((rho2 * r2) / d);
            const double c = (2.0 * k) * (rho4 / (d * d)), cr = c * r[e];
#pragma unroll
            for (int p = 0; p < CR_NP; ++p) {
                acc[1 + p] -= cr * J[e][p];
                const double cj = c * J[e][p];
#pragma unroll
                for (int q = p; q < CR_NP; ++q) acc[1 + CR_NP + cr_tri(p, q)] += cj * J[e][q];
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < CR_NS; ++q) {
        const double s = wave64_sum<double>(acc[q]);
        if (lane == 0) part[wave][q] = s;
    }
}

// the four waves' sums in wave order
__device__ __forceinline__ double cr_total(const double (*part)[CR_NS], int q) {
    return ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
}

__global__ __launch_bounds__(CR_NT) void cr_normal_eqs_kernel(const float* __restrict__ joints, const float* __restrict__ gt_xy,
                                                              const float* __restrict__ w_conf, int B, int V,
                                                              const double* __restrict__ cams, double rho2, double k0,
                                                              double* __restrict__ E, double* __restrict__ g,
                                                              double* __restrict__ H, int32_t* __restrict__ count) {
    __shared__ double part[CR_NT / 64][CR_NS];
    const int v = blockIdx.x, tid = threadIdx.x;
    double cam[CR_CAM];
#pragma unroll
    for (int i = 0; i < CR_CAM; ++i) cam[i] = cams[(size_t)v * CR_CAM + i];
    cr_eval(cam, joints, gt_xy, w_conf, B, V, v, rho2, k0, part);
    __syncthreads();
    const bool behind = cr_total(part, CR_NS - 1) != 0.0;
    const double undef = __builtin_nan("");
    if (tid == 0) {
        E[v] = behind ? (double)INFINITY : cr_total(part, 0);
        if (count) count[v] = (int32_t)cr_total(part, CR_NS - 2);
    }
    if (g && tid < CR_NP) g[(size_t)v * CR_NP + tid] = behind ? undef : cr_total(part, 1 + tid);
    if (H && tid < CR_NP * CR_NP) {
        const int i = tid / CR_NP, j = tid - i * CR_NP, lo = i < j ? i : j, hi = i < j ? j : i;
        H[(size_t)v * CR_NP * CR_NP + tid] = behind ? undef : cr_total(part, 1 + CR_NP + cr_tri(lo, hi));
    }
}

struct CrOpts {
    uint32_t free_mask, fixed_views;
    int max_iter, min_points;
    double rho2, k0, lambda0, ftol;
};

// theta' = step(theta, d): R' = exp([omega]x) R, t' = exp([omega]x) t + dt, f' = f + df, c' = c + dc (Rodrigues in float64)
__device__ __forceinline__ void cr_step(const double* th, const double (&d)[CR_NP], double* out) {
    const double wx = d[0], wy = d[1], wz = d[2], t2 = (wx * wx + wy * wy) + wz * wz;
    double A = 1.0, Bc = 0.5;
    if (t2 >= 1e-24) {
        const double t = sqrt(t2);
        A = sin(t) / t;
        Bc = (1.0 - cos(t)) / t2;
    }
    // exp = I + A K + Bc K^2, K = [omega]x, K^2 = omega omega^T - t2 I
    const double Ex[9] = {1.0 + Bc * (wx * wx - t2), Bc * (wx * wy) - A * wz, Bc * (wx * wz) + A * wy,
                          Bc * (wx * wy) + A * wz, 1.0 + Bc * (wy * wy - t2), Bc * (wy * wz) - A * wx,
                          Bc * (wx * wz) - A * wy, Bc * (wy * wz) + A * wx, 1.0 + Bc * (wz * wz - t2)};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (Ex[3 * r] * th[c] + Ex[3 * r + 1] * th[3 + c]) + Ex[3 * r + 2] * th[6 + c];
        out[9 + r] = ((Ex[3 * r] * th[9] + Ex[3 * r + 1] * th[10]) + Ex[3 * r + 2] * th[11]) + d[3 + r];
    }
    out[12] = th[12] + d[6];
    out[13] = th[13] + d[7];
    out[14] = th[14] + d[8];
}

// d = -A^-1 g over the free parameters, A = H with its diagonal times (1 + lam); false: a pivot that is not > 0
__device__ __forceinline__ bool cr_solve(const double* cur, uint32_t free_mask, double lam, double (&d)[CR_NP]) {
    double L[CR_NH];                                                   // row i, column j <= i at cr_tri(j, i)
    double y[CR_NP];
#pragma unroll
    for (int i = 0; i < CR_NP; ++i) {
        const bool fi = (free_mask >> cr_group(i)) & 1u;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const bool fj = (free_mask >> cr_group(j)) & 1u;
            double s;
            if (i == j) s = fi ? cur[1 + CR_NP + cr_tri(i, i)] * (1.0 + lam) : 1.0;
            else s = (fi && fj) ? cur[1 + CR_NP + cr_tri(j, i)] : 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[cr_tri(k, i)] * L[cr_tri(k, j)];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[cr_tri(i, i)] = sqrt(s);
            } else {
                L[cr_tri(j, i)] = s / L[cr_tri(j, j)];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CR_NP; ++i) {                                  // L y = -g
        double s = ((free_mask >> cr_group(i)) & 1u) ? -cur[1 + i] : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[cr_tri(k, i)] * y[k];
        y[i] = s / L[cr_tri(i, i)];
    }
#pragma unroll
    for (int i = CR_NP - 1; i >= 0; --i) {                             // L^T d = y
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < CR_NP; ++k) s -= L[cr_tri(i, k)] * d[k];
        d[i] = s / L[cr_tri(i, i)];
    }
    return true;
}

__global__ __launch_bounds__(CR_NT) void cr_lm_kernel(const float* __restrict__ joints, const float* __restrict__ gt_xy,
                                                      const float* __restrict__ w_conf, int B, int V, const double* cams_in,
                                                      CrOpts o, double* cams_out, double* __restrict__ report) {
    __shared__ double part[CR_NT / 64][CR_NS];
    __shared__ double cur[1 + CR_NP + CR_NH];                          // E, g, H at theta
    __shared__ double theta[CR_CAM];
    __shared__ double cand[CR_CAM];
    __shared__ int go;
    const int v = blockIdx.x, tid = threadIdx.x;
    double cam[CR_CAM];
#pragma unroll
    for (int i = 0; i < CR_CAM; ++i) cam[i] = cams_in[(size_t)v * CR_CAM + i];
    // state of lane 0 of wave 0
    double E0 = 0.0, lam = o.lambda0, cnt = 0.0;
    int it = 0, nacc = 0, status = -1;
    bool first = true;
    for (;;) {
        cr_eval(cam, joints, gt_xy, w_conf, B, V, v, o.rho2, o.k0, part);
        __syncthreads();
        if (tid == 0) {
            const double Ec = cr_total(part, CR_NS - 1) != 0.0 ? (double)INFINITY : cr_total(part, 0);
            bool take = false;
            if (first) {
                first = false;
                E0 = Ec;
                cnt = cr_total(part, CR_NS - 2);
                cur[0] = Ec;
#pragma unroll
                for (int i = 0; i < CR_CAM; ++i) theta[i] = cam[i];
                if ((o.fixed_views >> v) & 1u) status = 3;
                else if (cnt < (double)o.min_points) status = 4;
                else if (Ec == (double)INFINITY) status = 5;
                else take = true;
            } else if (Ec < cur[0]) {
                const double dec = cur[0] - Ec;
                take = true;
                cur[0] = Ec;
#pragma unroll
                for (int i = 0; i < CR_CAM; ++i) theta[i] = cam[i];
                lam = fmax(lam / 10.0, 1e-9);
                ++nacc;
                if (dec <= o.ftol * fmax(Ec, 1.0)) status = 0;
            } else {
                lam *= 10.0;
                if (lam > 1e12) status = 2;
            }
            if (take)
                for (int q = 1; q < 1 + CR_NP + CR_NH; ++q) cur[q] = cr_total(part, q);
            while (status < 0) {
                if (it == o.max_iter) { status = 1; break; }
                ++it;
                double d[CR_NP];
                if (!cr_solve(cur, o.free_mask, lam, d)) { lam *= 10.0; continue; }
                cr_step(theta, d, cand);
                break;
            }
            go = status < 0;
        }
        __syncthreads();
        if (!go) break;
#pragma unroll
        for (int i = 0; i < CR_CAM; ++i) cam[i] = cand[i];
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < CR_CAM; ++i) cams_out[(size_t)v * CR_CAM + i] = theta[i];
        double* r = report + (size_t)v * 8;
        r[0] = E0; r[1] = cur[0]; r[2] = (double)it; r[3] = (double)nacc; r[4] = (double)status; r[5] = cnt; r[6] = lam; r[7] = 0.0;
    }
}

hipError_t launch_camera_normal_eqs(const float* joints, const float* gt_xy, const float* w_conf, int B, int V,
                                    const double* cams, float rho, float data_weight, double* E, double* g, double* H,
                                    int32_t* count, hipStream_t stream) {
    const double rho2 = (double)rho * (double)rho, k0 = (double)data_weight * (double)data_weight;
    hipLaunchKernelGGL(cr_normal_eqs_kernel, dim3(V), dim3(CR_NT), 0, stream, joints, gt_xy, w_conf, B, V, cams, rho2, k0, E, g, H,
                       count);
    return hipGetLastError();
}

hipError_t launch_camera_refine(const float* joints, const float* gt_xy, const float* w_conf, int B, int V,
                                const double* cams_in, uint32_t free_mask, uint32_t fixed_views, int max_iter, int min_points,
                                float rho, float data_weight, double lambda0, double ftol, double* cams_out, double* report,
                                hipStream_t stream) {
    CrOpts o;
    o.free_mask = free_mask; o.fixed_views = fixed_views; o.max_iter = max_iter; o.min_points = min_points;
    o.rho2 = (double)rho * (double)rho; o.k0 = (double)data_weight * (double)data_weight; o.lambda0 = lambda0; o.ftol = ftol;
    hipLaunchKernelGGL(cr_lm_kernel, dim3(V), dim3(CR_NT), 0, stream, joints, gt_xy, w_conf, B, V, cams_in, o, cams_out, report);
    return hipGetLastError();
}

}  // namespace mvfit
