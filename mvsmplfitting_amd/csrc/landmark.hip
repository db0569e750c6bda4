// The surface landmark term (include/mvfit.h: mvfit_landmark_loss): named points of the body's surface - affine combinations
// of up to four vertices - against the pixels they were seen at in every view and, optionally, against measured 3-D
// positions, with the gradient on the vertices.
//
//   landmark_kernel  grid (B), LM_NT threads, one workgroup per problem, five phases with a barrier between them:
//     0  the problem's 3 nv gradient floats are zeroed (16-byte stores between an unaligned head and tail), the cameras of
//        the V views go to LDS, and thread l gathers landmark l: p_l = sum_k w_lk V[vid_lk] in fp32 from 0, ascending k, the
//        slots of weight 0 never read.
//     1  the V L items (v, l), item i = v L + l on thread i mod LM_NT: projection as the closure's keypoint term has it
//        (closure_device.h: loss_and_keypoint_grad - fp32, 1 / z without a guard), residual u - xy, GMoF, the item's
//        value conf^2 (g_x + g_y) in fp32 added to the thread's float64 sum in ascending i, and the item's gradient on p_l
//        into LDS.  An item of confidence 0 is never read and leaves a zero gradient.
//     2  thread l sums landmark l's item gradients over the views in ascending v from 0, then adds the 3-D part
//        w3d conf3^2 GMoF(p - xyz; rho3d) - value into the thread's float64 sum, gradient onto the point's.
//        The loss: wave64_sum of the threads' sums, the four wave totals in wave order, rounded to fp32 once.
//     3  thread t writes touched vertex tv[t]: sum of w_lk g_l over its (landmark, slot) entries in ascending order from 0.
//   Phase 3's stores land on floats phase 0 zeroed: both come from one workgroup, with barriers in between.
// No atomics and nothing read from the output: a problem's bits depend on its own inputs alone.  gate[b] == 0 - a finished
// problem, or a stage without the term - ends the workgroup at once; a null gate keeps every problem.
#include "landmark.h"

#include "wave_ops.h"

namespace mvfit {

constexpr int LM_NT = 256;

// GMoF (utils.py:435-438) of a residual and its derivative; s2 = 0: the plain square
__device__ __forceinline__ void lm_gmof(float r, float s2, float& val, float& der) {
    const float r2 = r * r;
    if (s2 > 0.f) {
        const float id = 1.0f / (r2 + s2);
        val = s2 * (r2 * id);
        der = 2.f * r * s2 * s2 * (id * id);
    } else {
        val = r2;
        der = 2.f * r;
    }
}

__global__ __launch_bounds__(LM_NT) void landmark_kernel(const float* __restrict__ verts, int nv, int B, const int32_t* __restrict__ tab,
                                                         int L, int nt, const float* __restrict__ tgt, int has3d, LmCams cams,
                                                         float rho, float w3d, float rho3d, const int* __restrict__ gate,
                                                         float* __restrict__ loss, float* __restrict__ g_verts) {
    __shared__ float s_pos[3][LM_MAX];
    __shared__ float s_gp[3][LM_MAX];
    __shared__ float s_gi[3][LM_MAX * LM_MAX_VIEWS];
    __shared__ float s_cam[LM_MAX_VIEWS][16];
    __shared__ double s_red[LM_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (gate && !gate[b]) return;                                      // (uniform)
    const int V = cams.V, nitem = V * L, n = 3 * nv;
    const int32_t* vid = tab;
    const float* w = reinterpret_cast<const float*>(tab + 4 * L);
    const int32_t *tv = tab + 8 * L, *tptr = tv + nt, *tent = tptr + nt + 1;
    const float* Vb = verts + (size_t)b * n;
    float* G = g_verts ? g_verts + (size_t)b * n : nullptr;

    // ---- phase 0
    if (G) {
        const int head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(G) & 15u)) & 15u) >> 2));
        const int nq = (n - head) >> 2;
        if (tid < head) G[tid] = 0.f;
        float4* q = reinterpret_cast<float4*>(G + head);
        for (int i = tid; i < nq; i += LM_NT) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = head + 4 * nq + tid; i < n; i += LM_NT) G[i] = 0.f;
    }
    if (tid < V * 16) {
        const int v = tid >> 4, j = tid & 15;
        const size_t cv = (cams.batched ? (size_t)b * V : 0) + v;
        s_cam[v][j] = j < 9 ? cams.R[cv * 9 + j] : j < 12 ? cams.t[cv * 3 + (j - 9)] : j == 12 ? cams.f[cv] :
                      j < 15 ? cams.c[cv * 2 + (j - 13)] : 0.f;
    }
    for (int l = tid; l < L; l += LM_NT) {
        float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
        for (int k = 0; k < LM_NNZ; ++k) {
            const float wk = w[l * LM_NNZ + k];
            if (wk != 0.f) {
                const float* p = Vb + (size_t)vid[l * LM_NNZ + k] * 3;
                px += wk * p[0]; py += wk * p[1]; pz += wk * p[2];
            }
        }
        s_pos[0][l] = px; s_pos[1][l] = py; s_pos[2][l] = pz;
    }
    __syncthreads();

    // ---- phase 1
    double acc = 0.0;
    const float rho2 = rho * rho;
    const float2* xy = reinterpret_cast<const float2*>(tgt) + (size_t)b * nitem;
    const float* conf = tgt + (size_t)B * nitem * 2 + (size_t)b * nitem;
    for (int i = tid; i < nitem; i += LM_NT) {
        const int v = i / L, l = i - v * L;
        const float cf = conf[i];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (cf > 0.f) {
            const float2 t = xy[i];
            const float X = s_pos[0][l], Y = s_pos[1][l], Z = s_pos[2][l];
            const float* Rc = s_cam[v];
            const float f = Rc[12], cx = Rc[13], cy = Rc[14];
            const float px = Rc[0] * X + Rc[1] * Y + Rc[2] * Z + Rc[9];
            const float py = Rc[3] * X + Rc[4] * Y + Rc[5] * Z + Rc[10];
            const float pz = Rc[6] * X + Rc[7] * Y + Rc[8] * Z + Rc[11];
            const float ipz = 1.0f / pz;
            const float u = f * (px * ipz) + cx, w_ = f * (py * ipz) + cy;
            const float c2 = cf * cf;
            float vx, vy, dx, dy;
            lm_gmof(u - t.x, rho2, vx, dx);
            lm_gmof(w_ - t.y, rho2, vy, dy);
            acc += (double)(c2 * (vx + vy));
            if (G) {
                const float gu = c2 * dx, gv = c2 * dy;
                const float gpx = f * gu * ipz, gpy = f * gv * ipz;
                const float gpz = -f * (gu * px + gv * py) * (ipz * ipz);
                g0 = Rc[0] * gpx + Rc[3] * gpy + Rc[6] * gpz;
                g1 = Rc[1] * gpx + Rc[4] * gpy + Rc[7] * gpz;
                g2 = Rc[2] * gpx + Rc[5] * gpy + Rc[8] * gpz;
            }
        }
        if (G) { s_gi[0][i] = g0; s_gi[1][i] = g1; s_gi[2][i] = g2; }
    }
    __syncthreads();

    // ---- phase 2
    const float rho3d2 = rho3d * rho3d;
    const float* xyz = tgt + (size_t)B * nitem * 3 + (size_t)b * L * 3;
    const float* conf3 = tgt + (size_t)B * nitem * 3 + (size_t)B * L * 3 + (size_t)b * L;
    for (int l = tid; l < L; l += LM_NT) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        if (G)
            for (int v = 0; v < V; ++v) { s0 += s_gi[0][v * L + l]; s1 += s_gi[1][v * L + l]; s2 += s_gi[2][v * L + l]; }
        const float c3 = has3d ? conf3[l] : 0.f;
        if (c3 > 0.f) {
            const float k3 = w3d * (c3 * c3);
            float vx, vy, vz, dx, dy, dz;
            lm_gmof(s_pos[0][l] - xyz[l * 3 + 0], rho3d2, vx, dx);
            lm_gmof(s_pos[1][l] - xyz[l * 3 + 1], rho3d2, vy, dy);
            lm_gmof(s_pos[2][l] - xyz[l * 3 + 2], rho3d2, vz, dz);
            acc += (double)(k3 * ((vx + vy) + vz));
            s0 += k3 * dx; s1 += k3 * dy; s2 += k3 * dz;
        }
        if (G) { s_gp[0][l] = s0; s_gp[1][l] = s1; s_gp[2][l] = s2; }
    }
    acc = wave64_sum(acc);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = s_red[0];
#pragma unroll
        for (int wv = 1; wv < LM_NT / 64; ++wv) s += s_red[wv];
        loss[b] = (float)s;
    }
    if (!G) return;

    // ---- phase 3
    for (int t = tid; t < nt; t += LM_NT) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        const int e1 = tptr[t + 1];
        for (int e = tptr[t]; e < e1; ++e) {
            const int ent = tent[e];
            const float wk = w[ent];
            const int l = ent >> 2;
            s0 += wk * s_gp[0][l]; s1 += wk * s_gp[1][l]; s2 += wk * s_gp[2][l];
        }
        float* o = G + (size_t)tv[t] * 3;
        o[0] = s0; o[1] = s1; o[2] = s2;
    }
}

hipError_t launch_landmarks(const float* verts, int nv, int B, const void* tab, int L, int nt, const float* tgt, bool has3d,
                            const LmCams& cams, float rho, float w3d, float rho3d, const int* gate, float* loss, float* g_verts,
                            hipStream_t stream) {
    if (L < 1 || L > LM_MAX || cams.V < 1 || cams.V > LM_MAX_VIEWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(landmark_kernel, dim3(B), dim3(LM_NT), 0, stream, verts, nv, B, static_cast<const int32_t*>(tab), L, nt, tgt,
                       has3d ? 1 : 0, cams, rho, w3d, rho3d, gate, loss, g_verts);
    return hipGetLastError();
}

}  // namespace mvfit
