// Reverse mode of mvfit_vertices (include/mvfit.h: mvfit_vertices_backward): the vector-Jacobian product of
// (vertices, keypoints) = SMPL.forward (body_models_scale.py:327-412, lbs.py:135-222) at the parameters x.
//
//   prep_kernel (fit_kernels.hip)   x -> blendshape coefficients (coefT), skinning transforms (Amat): the pass's operands
//   vjp_tile_kernel               one workgroup per (vertex slice, 32-problem chunk): the dense part of the adjoint over the
//                                 slice's vertices, from the vertex cotangent, into one partial record per problem
//   vjp_reduce_kernel             the slice partials of a problem, added in slice order -> one SdfAdj-shaped record
//   vjp_tile_kernel<gated>,       the same dense part for the silhouette term inside the fit's chained rounds: chunks without a
//   vjp_record_kernel             live problem skipped, the record published in the form the closure consumes (SdfAdj)
//   vjp_tail_kernel               one workgroup per problem: the closure's adjoint stages (closure_device.h: closure_backward)
//                                 with the record entering at factor 1 and the keypoint cotangent in place of the data
//                                 term's keypoint gradient; every prior off
//
// Dense part, per vertex v of problem p with cotangent g_v (lbs.py:203-222):
//   v_posed   = v_template + coef . basis                         (recomputed in fp32: the adjoint is that of the fp32
//                                                                  model whatever contraction the forward used)
//   T         = sum_j w_vj A_j                                     (3x4)
//   g_vposed  = T[:, :3]^T g_v
//   g_coef   += basis_v^T g_vposed                                 (pose-feature rows 0..206, betas 207..216)
//   g_A_j    += w_vj [g_v v_posed^T | g_v]                         (the accumulator order of the closure's E6)
//   g_tau    += g_v
// Every sum runs in one fixed order (rows ascending inside a thread, vertices ascending inside a slice, slices ascending in
// the reduction): no atomics, and a problem's result does not depend on the batch, its position in it or its chunk.
#include <hip/hip_runtime.h>

#include "closure_device.h"
#include "launchers.h"

namespace mvfit {

constexpr int VB_NT = 512;                 // threads of the tile kernel: (problem, vertex) of a sub-tile, one each
constexpr int VB_TV = 16;                  // vertices per sub-tile
constexpr int VB_ROWS = 3 * VB_TV;         // basis rows per sub-tile
constexpr int VB_SUB = 2;                  // sub-tiles per slice
constexpr int VB_SLICE_V = VB_TV * VB_SUB; // vertices per slice (fixed: the summation order depends on the model alone)
constexpr int VB_PSTR = 528;               // floats per partial record: g_coef[224] | g_A[288] | g_tau[3] | pad
constexpr int VB_CS = KROWS + 4;           // LDS row stride of the coefficients    (16 lanes x 16 B: conflict-free)
constexpr int VB_AS = NJ * 12 + 4;         // LDS row stride of the transforms      (the same)
constexpr int VB_GS = VB_ROWS + 1;         // LDS row stride of g_v / v_posed       (odd: lanes of different problems)
constexpr int VB_QS = 36;                  // LDS row stride of g_vposed [row][problem]
static_assert(VB_NT == 32 * VB_TV, "one (problem, vertex) item per thread");
static_assert(VB_PSTR >= KROWS + NJ * 12 + 3, "partial record");

struct VjpTileLds {
    __attribute__((aligned(16))) float coef[32][VB_CS];     // the chunk's coefficients, problem-major
    __attribute__((aligned(16))) float A[32][VB_AS];        // the chunk's skinning transforms
    __attribute__((aligned(16))) float bs[VB_ROWS][KROWS];  // basis rows of the sub-tile
    __attribute__((aligned(16))) float gvp[VB_ROWS][VB_QS]; // g_vposed [row][problem]
    float w[VB_TV][NJ];                                     // skinning weights of the sub-tile
    float vt[VB_ROWS];                                      // v_template of the sub-tile
    float gv[32][VB_GS];                                    // vertex cotangent [problem][row]
    float vp[32][VB_GS];                                    // v_posed [problem][row]
};

// GATED (the silhouette term of the fit's chained rounds): a chunk none of whose problems has its gate word set returns at
// once; otherwise the same arithmetic in the same order - a live problem's partial record has the bits of the ungated
// kernel's (a gated-off neighbour's cotangent rows are whatever the buffer holds: its record is never read, and no sum
// mixes problems).  A null gate keeps every chunk.  The ungated instantiation carries an empty argument and is the kernel
// as it was.
template <bool GATED> struct VjpGate {};
template <> struct VjpGate<true> { const int* gate; };

template <bool GATED>
__global__ __launch_bounds__(VB_NT) void vjp_tile_kernel(DevModel M, DevPose P, int B, int Bpad,
                                                         const float* __restrict__ g_verts, float* __restrict__ part,
                                                         VjpGate<GATED> G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    VjpTileLds& S = *reinterpret_cast<VjpTileLds*>(smem_raw);
    const int tid = threadIdx.x, slice = blockIdx.x, chunk = blockIdx.y;
    const int nv = M.nv, b0 = chunk * 32;
    if constexpr (GATED) {
        if (G.gate) {
            int live = 0;
            for (int p = 0; p < 32 && b0 + p < B; ++p) live |= G.gate[b0 + p];      // (uniform: scalar loads)
            if (!live) return;
        }
    }
    // the chunk's operands (problems past B: zero transforms, zero cotangent - their records are never read)
    for (int i = tid; i < 32 * KROWS; i += VB_NT) {
        const int k = i >> 5, p = i & 31;
        S.coef[p][k] = P.coefT[(size_t)chunk * KROWS * 32 + i];
    }
    for (int i = tid; i < 32 * NJ * 12; i += VB_NT) {
        const int p = i / (NJ * 12), e = i - p * (NJ * 12);
        S.A[p][e] = b0 + p < B ? P.Amat[(size_t)(b0 + p) * NJ * 12 + e] : 0.f;
    }
    // accumulators: g_coef (threads < 448: 4 problems x 4 rows), g_A (every thread: problem, joints jg and jg + 16),
    // g_tau (lanes 0-31 of wave 7)
    const int kq = tid % 56, pg = tid / 56;
    float gc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) gc[i][q] = 0.f;
    const int ap = tid & 31, jg = tid >> 5;
    const bool two = jg + 16 < NJ;
    float ga0[12], ga1[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) { ga0[e] = 0.f; ga1[e] = 0.f; }
    float gt[3] = {0.f, 0.f, 0.f};
    const int ip = tid & 31, iv = tid >> 5;                 // the (problem, vertex) item of phases 1
    for (int sub = 0; sub < VB_SUB; ++sub) {
        const int v0 = slice * VB_SLICE_V + sub * VB_TV;
        if (v0 >= nv) break;                                // uniform
        __syncthreads();                                    // the previous sub-tile's readers are done
        // ---- phase 0: basis rows, weights, v_template, cotangent of the sub-tile (zero past the model / the batch) ----
        {
            const float4* src = reinterpret_cast<const float4*>(M.bs_vm + (size_t)v0 * 3 * KROWS);
            constexpr int n4 = VB_ROWS * KROWS / 4;
            const int lim4 = (nv - v0) * 3 * KROWS / 4;     // words of the model from v0 on
            for (int i = tid; i < n4; i += VB_NT)
                reinterpret_cast<float4*>(&S.bs[0][0])[i] = i < lim4 ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < VB_TV * NJ) {
            const int v = v0 + tid / NJ;
            (&S.w[0][0])[tid] = v < nv ? M.w_vm[(size_t)v0 * NJ + tid] : 0.f;
        } else if (tid >= 448 && tid < 448 + VB_ROWS) {
            const int r = tid - 448, v = v0 + r / 3, a = r - 3 * (r / 3);
            S.vt[r] = v < nv ? M.vt_planes[(size_t)a * M.nv_pad + v] : 0.f;
        }
        for (int i = tid; i < 32 * VB_ROWS; i += VB_NT) {
            const int p = i / VB_ROWS, r = i - p * VB_ROWS;
            float g = 0.f;
            if (g_verts && b0 + p < B && v0 + r / 3 < nv) g = g_verts[((size_t)(b0 + p) * nv + v0) * 3 + r];
            S.gv[p][r] = g;
        }
        __syncthreads();
        // ---- phase 1: v_posed, skinning transform and g_vposed of item (problem ip, vertex iv) ----
        {
            const float4* cr = reinterpret_cast<const float4*>(S.coef[ip]);
            const float4* r0 = reinterpret_cast<const float4*>(S.bs[3 * iv]);
            const float4* r1 = reinterpret_cast<const float4*>(S.bs[3 * iv + 1]);
            const float4* r2 = reinterpret_cast<const float4*>(S.bs[3 * iv + 2]);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 8
            for (int k4 = 0; k4 < KROWS / 4; ++k4) {
                const float4 c = cr[k4], x0 = r0[k4], x1 = r1[k4], x2 = r2[k4];
                s0 = fmaf(c.x, x0.x, s0); s0 = fmaf(c.y, x0.y, s0); s0 = fmaf(c.z, x0.z, s0); s0 = fmaf(c.w, x0.w, s0);
                s1 = fmaf(c.x, x1.x, s1); s1 = fmaf(c.y, x1.y, s1); s1 = fmaf(c.z, x1.z, s1); s1 = fmaf(c.w, x1.w, s1);
                s2 = fmaf(c.x, x2.x, s2); s2 = fmaf(c.y, x2.y, s2); s2 = fmaf(c.z, x2.z, s2); s2 = fmaf(c.w, x2.w, s2);
            }
            const float vp0 = S.vt[3 * iv] + s0, vp1 = S.vt[3 * iv + 1] + s1, vp2 = S.vt[3 * iv + 2] + s2;
            float T[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] = 0.f;
            for (int j = 0; j < NJ; ++j) {
                const float w = S.w[iv][j];
                if (w == 0.f) continue;                     // (uniform across the item's problems)
                const float4* Aj = reinterpret_cast<const float4*>(&S.A[ip][12 * j]);
                const float4 a0 = Aj[0], a1 = Aj[1], a2 = Aj[2];
                T[0] = fmaf(w, a0.x, T[0]); T[1] = fmaf(w, a0.y, T[1]); T[2] = fmaf(w, a0.z, T[2]); T[3] = fmaf(w, a0.w, T[3]);
                T[4] = fmaf(w, a1.x, T[4]); T[5] = fmaf(w, a1.y, T[5]); T[6] = fmaf(w, a1.z, T[6]); T[7] = fmaf(w, a1.w, T[7]);
                T[8] = fmaf(w, a2.x, T[8]); T[9] = fmaf(w, a2.y, T[9]); T[10] = fmaf(w, a2.z, T[10]); T[11] = fmaf(w, a2.w, T[11]);
            }
            const float g0 = S.gv[ip][3 * iv], g1 = S.gv[ip][3 * iv + 1], g2 = S.gv[ip][3 * iv + 2];
#pragma unroll
            for (int c = 0; c < 3; ++c) S.gvp[3 * iv + c][ip] = T[c] * g0 + T[4 + c] * g1 + T[8 + c] * g2;
            S.vp[ip][3 * iv] = vp0; S.vp[ip][3 * iv + 1] = vp1; S.vp[ip][3 * iv + 2] = vp2;
        }
        __syncthreads();
        // ---- phase 2: g_coef += basis^T g_vposed ; g_A ; g_tau ----
        if (tid < 448) {
#pragma unroll 4
            for (int r = 0; r < VB_ROWS; ++r) {
                const float4 x = reinterpret_cast<const float4*>(S.bs[r])[kq];
                const float4 g = reinterpret_cast<const float4*>(S.gvp[r])[pg];
                const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    gc[i][0] = fmaf(gg[i], x.x, gc[i][0]); gc[i][1] = fmaf(gg[i], x.y, gc[i][1]);
                    gc[i][2] = fmaf(gg[i], x.z, gc[i][2]); gc[i][3] = fmaf(gg[i], x.w, gc[i][3]);
                }
            }
        } else if (tid < 480) {
            for (int v = 0; v < VB_TV; ++v) {
                gt[0] += S.gv[ap][3 * v]; gt[1] += S.gv[ap][3 * v + 1]; gt[2] += S.gv[ap][3 * v + 2];
            }
        }
        for (int v = 0; v < VB_TV; ++v) {
            const float w0 = S.w[v][jg], w1 = two ? S.w[v][jg + 16] : 0.f;
            if (w0 == 0.f && w1 == 0.f) continue;
            const float g[3] = {S.gv[ap][3 * v], S.gv[ap][3 * v + 1], S.gv[ap][3 * v + 2]};
            const float x[3] = {S.vp[ap][3 * v], S.vp[ap][3 * v + 1], S.vp[ap][3 * v + 2]};
            float X[12];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int m = 0; m < 3; ++m) X[3 * a + m] = g[a] * x[m];
                X[9 + a] = g[a];
            }
            if (w0 != 0.f) {
#pragma unroll
                for (int e = 0; e < 12; ++e) ga0[e] = fmaf(w0, X[e], ga0[e]);
            }
            if (w1 != 0.f) {
#pragma unroll
                for (int e = 0; e < 12; ++e) ga1[e] = fmaf(w1, X[e], ga1[e]);
            }
        }
    }
    // ---- the slice's partial records ----
    float* pb = part + ((size_t)slice * Bpad + b0) * VB_PSTR;
    if (tid < 448) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(pb + (size_t)(4 * pg + i) * VB_PSTR + 4 * kq) = make_float4(gc[i][0], gc[i][1], gc[i][2], gc[i][3]);
    } else if (tid < 480) {
#pragma unroll
        for (int a = 0; a < 3; ++a) pb[(size_t)ap * VB_PSTR + KROWS + NJ * 12 + a] = gt[a];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) pb[(size_t)ap * VB_PSTR + KROWS + 12 * jg + e] = ga0[e];
    if (two) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pb[(size_t)ap * VB_PSTR + KROWS + 12 * (jg + 16) + e] = ga1[e];
    }
}

// record of problem b = the slice partials in slice order; S (the SDF term's sum) = 0
__global__ __launch_bounds__(VB_PSTR) void vjp_reduce_kernel(const float* __restrict__ part, int nslices, int Bpad,
                                                             SdfAdj* __restrict__ rec) {
    const int b = blockIdx.x, e = threadIdx.x;
    if (e >= KROWS + NJ * 12 + 3) return;
    const float* p = part + (size_t)b * VB_PSTR + e;
    float s = 0.f;
#pragma unroll 16
    for (int y = 0; y < nslices; ++y) s += p[(size_t)y * Bpad * VB_PSTR];      // (loads ahead of the adds; the adds in order)
    SdfAdj& R = rec[b];
    if (e < KROWS) R.gcoef[e] = s;
    else if (e < KROWS + NJ * 12) R.gA[e - KROWS] = s;
    else R.gtau[e - KROWS - NJ * 12] = s;
    if (e == 0) R.S = 0.f;
}

// The silhouette term's record of a live problem b (gate null or gate[b] != 0): the slice partials in slice order, as
// vjp_reduce_kernel adds them, = the adjoint of L = loss[b] with respect to the pass's operands.  The closure forms (w S)^2
// and applies 2 w^2 S to the record (closure_device.h: loss_combine), so S = sqrt(L) and the adjoint times 1 / (2 sqrt(L))
// make it yield w^2 L and w^2 grad L unchanged.  L < FLT_MIN (no image, or nothing to pay): an all-zero record - the closure
// then adds 0 and never reads the adjoint.
__global__ __launch_bounds__(VB_PSTR) void vjp_record_kernel(const float* __restrict__ part, int nslices, int Bpad,
                                                             const float* __restrict__ loss, const int* __restrict__ gate,
                                                             SdfAdj* __restrict__ rec) {
    const int b = blockIdx.x, e = threadIdx.x;
    if (gate && !gate[b]) return;
    if (e >= KROWS + NJ * 12 + 3) return;
    const float* p = part + (size_t)b * VB_PSTR + e;
    float s = 0.f;
#pragma unroll 16
    for (int y = 0; y < nslices; ++y) s += p[(size_t)y * Bpad * VB_PSTR];      // (loads ahead of the adds; the adds in order)
    const float L = loss[b];
    const bool zero = L < 1.17549435e-38f;                                     // FLT_MIN
    const float S = zero ? 0.f : sqrtf(L);
    const float k = zero ? 0.f : 1.f / (2.f * S);
    s = zero ? 0.f : s * k;
    SdfAdj& R = rec[b];
    if (e < KROWS) R.gcoef[e] = s;
    else if (e < KROWS + NJ * 12) R.gA[e - KROWS] = s;
    else R.gtau[e - KROWS - NJ * 12] = s;
    if (e == 0) R.S = S;
}

// per problem: the closure's adjoint with the record at factor 1 (rec may be null: no vertex cotangent) and the keypoint
// cotangent g_joints (null: zero) where the data term's keypoint gradient goes; every prior weight 0 and both prior guards
// set (their gradients are then not formed at all - the angle prior's exp could overflow into 0 * inf)
__global__ __launch_bounds__(STEP_NT) void vjp_tail_kernel(DevModel M, const float* __restrict__ params, uint32_t flags,
                                                           const float* __restrict__ g_joints, const SdfAdj* __restrict__ rec,
                                                           float* __restrict__ g_params) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ClosureLds& L = *reinterpret_cast<ClosureLds*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    prologue(L, M, nullptr, nullptr, nullptr, nullptr, nullptr, params + (size_t)b * DV, tid, rec ? rec + b : nullptr);
    __syncthreads();
    pose_prep(M, L, flags, tid);
    sparse_forward(M, L, false, tid);       // chain, and v_posed / T of the vertices the keypoints read
    const float* gj = g_joints ? g_joints + (size_t)b * NKP * 3 : nullptr;
    if (tid < NKP * 3) (&L.gkp[0][0])[tid] = gj ? gj[tid] : 0.f;
    else if (tid >= 64 && tid < 67) {
        // d/d transl of the keypoints (each is its source + transl): sum over keypoints, ascending
        const int a = tid - 64;
        float s = 0.f;
        if (gj) for (int k = 0; k < NKP; ++k) s += gj[3 * k + a];
        L.gtau[a] = s;
    } else if (tid == 128) {
        L.sdf_fac = rec ? 1.f : 0.f;
        L.flags_dropped = 3;
        L.gmm_sel = 0;
    }
    DevWeights W{};
    W.flags = flags & (MVFIT_F_VPOSER | MVFIT_F_FIX_SHAPE | MVFIT_F_FIX_SCALE);
    closure_backward<false>(M, L, 0, W, tid);
    if (tid < DV) g_params[(size_t)b * DV + tid] = L.grad[tid];
}

int vjp_slices(int nv) { return (nv + VB_SLICE_V - 1) / VB_SLICE_V; }
size_t vjp_part_bytes(int Bpad, int nv) { return (size_t)vjp_slices(nv) * Bpad * VB_PSTR * sizeof(float); }

hipError_t vertex_backward_configure() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vjp_tile_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)sizeof(VjpTileLds));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(vjp_tile_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)sizeof(VjpTileLds));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(vjp_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((sizeof(ClosureLds) + 15) & ~(size_t)15));
}

// after prep_kernel has written the operands of params into P: the dense pass (g_verts != null) and the tail
hipError_t launch_vertices_backward(const DevModel& M, const DevPose& P, int B, int Bpad, const float* params, uint32_t flags,
                                    const float* g_verts, const float* g_joints, float* part, SdfAdj* rec, float* g_params,
                                    hipStream_t stream) {
    if (g_verts) {
        const int ns = vjp_slices(M.nv);
        hipLaunchKernelGGL(vjp_tile_kernel<false>, dim3(ns, Bpad / 32), dim3(VB_NT), sizeof(VjpTileLds), stream, M, P, B, Bpad, g_verts, part,
                           VjpGate<false>{});
        hipLaunchKernelGGL(vjp_reduce_kernel, dim3(B), dim3(VB_PSTR), 0, stream, (const float*)part, ns, Bpad, rec);
    }
    hipLaunchKernelGGL(vjp_tail_kernel, dim3(B), dim3(STEP_NT), (sizeof(ClosureLds) + 15) & ~(size_t)15, stream, M, params, flags,
                       g_joints, g_verts ? (const SdfAdj*)rec : (const SdfAdj*)nullptr, g_params);
    return hipGetLastError();
}

// the silhouette term's pull-back of a chained round: g_verts[B][nv][3] (rows of live problems) and loss[B] -> rec[B]
hipError_t launch_silhouette_pullback(const DevModel& M, const DevPose& P, int B, int Bpad, const int* gate, const float* g_verts,
                                      const float* loss, float* part, SdfAdj* rec, hipStream_t stream) {
    const int ns = vjp_slices(M.nv);
    hipLaunchKernelGGL(vjp_tile_kernel<true>, dim3(ns, Bpad / 32), dim3(VB_NT), sizeof(VjpTileLds), stream, M, P, B, Bpad, g_verts,
                       part, VjpGate<true>{gate});
    hipLaunchKernelGGL(vjp_record_kernel, dim3(B), dim3(VB_PSTR), 0, stream, (const float*)part, ns, Bpad, loss, gate, rec);
    return hipGetLastError();
}

}  // namespace mvfit
