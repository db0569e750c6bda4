// Occlusion between the bodies of a scene for the silhouette term (include/mvfit.h: mvfit_set_silhouette_occluders).  A
// person mask shows the visible part of the person only; where another body of the scene stands in front, an off pixel says
// nothing about this body.  The other bodies are frozen as depth maps per mask image, and the evaluation (silhouette.hip,
// the <., OCC = true> instantiations) ignores what the maps hide.  Per freeze:
//   occ_transform_kernel  per (instance, vertex): an instance is one body seen by one mask image's camera, drawn into that
//                         image's z_own (the image's own body) or z_occ (a scene mate); the renderer's vertex record
//   occ_raster_kernel     per (instance, face): the renderer's face setup, coverage and depth (render_raster.h); a covered
//                         sample inside [znear, zfar] does a 32-bit integer atomicMin of the fp32 depth bits (positive floats
//                         order like their bits) - order-independent, so the maps do not depend on the order or the grouping
//                         of the instances.  Faces whose box exceeds RD_BIG_BOX pixels are listed for
//   occ_raster_big_kernel a workgroup per listed face at a time, its threads striding over the box (the same samples)
//   occ_flag_kernel       per kept contour point: flagged when every off 4-neighbour inside the image is explained by an
//                         occluder that is not known to lie behind the body at the point
// and, as a diagnostic, occ_hidden_kernel per (image, vertex): the hidden test the evaluation kernels apply.
// The instance list (own body plus scene mates per image) is built on the host at freeze time.  Only integer atomics and
// plain vector stores.
#include "silhouette.h"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <map>

#include "mvfit.h"
#include "silhouette_device.h"

#pragma clang fp contract(off)

#include "render_raster.h"

namespace mvfit {

constexpr int OCC_GROUP = 512;                   // instances rasterised per pass over the workspace
constexpr unsigned OCC_INF = 0x7f800000u;        // +inf: nothing covers the sample

struct OccInst { int image, body, map, pad; };   // map: 0 = the image's own body (z_own), 1 = a scene mate (z_occ)
static_assert(sizeof(OccInst) == 16, "table row");

// grid (ceil(nv / SIL_NT), instances of the group)
__global__ __launch_bounds__(SIL_NT) void occ_transform_kernel(const float* __restrict__ verts, int nv, const SilCam* __restrict__ cams,
                                                               const OccInst* __restrict__ inst, int H, int W,
                                                               RenderVert* __restrict__ vert) {
    const int j = blockIdx.y, v = blockIdx.x * SIL_NT + threadIdx.x;
    if (v >= nv) return;
    const OccInst in = inst[j];
    const SilCam cam = cams[in.image];
    float px, py, pz, u, w;
    sil_project(cam, verts + ((size_t)in.body * nv + v) * 3, px, py, pz, u, w);
    vert[(size_t)j * nv + v] = snap_vertex(u, w, pz, H, W);
}

__device__ __forceinline__ void occ_sample(const FaceSetup& s, long long e0, long long e1, long long e2, unsigned* px) {
    float z;
    if (raster_depth(s, e0, e1, e2, z)) atomicMin(px, __float_as_uint(z));
}

__device__ __forceinline__ unsigned* occ_map(const OccInst& in, unsigned* z_occ, unsigned* z_own, int H, int W) {
    return (in.map ? z_occ : z_own) + (size_t)in.image * H * W;
}

// grid (ceil(nf / SIL_NT), instances of the group): one thread per (instance, face); big[0 .. *nbig): entries instance nf + f
__global__ __launch_bounds__(SIL_NT) void occ_raster_kernel(const OccInst* __restrict__ inst, const RenderVert* __restrict__ vert,
                                                            const int32_t* __restrict__ faces, int nf, int nv, int H, int W,
                                                            unsigned* __restrict__ z_occ, unsigned* __restrict__ z_own,
                                                            unsigned* __restrict__ nbig, int32_t* __restrict__ big) {
    const int j = blockIdx.y, f = blockIdx.x * SIL_NT + threadIdx.x;
    if (f >= nf) return;
    FaceSetup s;
    if (!face_setup(vert + (size_t)j * nv, faces, f, H, W, s)) return;
    if ((long long)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) > RD_BIG_BOX) {
        const unsigned k = atomicAdd(nbig, 1u);                    // k < instances nf: each face of each instance at most once
        big[k] = j * nf + f;
        return;
    }
    const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
    const long long dx0 = -256ll * (v2.Y - v1.Y) * s.sgn, dx1 = -256ll * (v0.Y - v2.Y) * s.sgn, dx2 = -256ll * (v1.Y - v0.Y) * s.sgn;
    unsigned* map = occ_map(inst[j], z_occ, z_own, H, W);
    for (int y = s.y0; y <= s.y1; ++y) {
        const long long sy = 256ll * y + 128, sx = 256ll * s.x0 + 128;
        long long e0 = edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn;
        long long e1 = edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn;
        long long e2 = edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn;
        for (int x = s.x0; x <= s.x1; ++x, e0 += dx0, e1 += dx1, e2 += dx2) occ_sample(s, e0, e1, e2, map + (size_t)y * W + x);
    }
}

// grid (RD_BIG_BLOCKS): the listed large faces of the group, the edge values evaluated directly at each sample - the same
// integers the incremental walk reaches
__global__ __launch_bounds__(SIL_NT) void occ_raster_big_kernel(const OccInst* __restrict__ inst, const RenderVert* __restrict__ vert,
                                                                const int32_t* __restrict__ faces, int nf, int nv, int H, int W,
                                                                unsigned* __restrict__ z_occ, unsigned* __restrict__ z_own,
                                                                const unsigned* __restrict__ nbig, const int32_t* __restrict__ big) {
    const unsigned n = *nbig;
    for (unsigned q = blockIdx.x; q < n; q += gridDim.x) {
        const int e = big[q], j = e / nf, f = e - j * nf;
        FaceSetup s;
        if (!face_setup(vert + (size_t)j * nv, faces, f, H, W, s)) continue;
        const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
        unsigned* map = occ_map(inst[j], z_occ, z_own, H, W);
        const int bw = s.x1 - s.x0 + 1;
        const long long npx = (long long)bw * (s.y1 - s.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += SIL_NT) {
            const int y = s.y0 + (int)(p / bw), x = s.x0 + (int)(p % bw);
            const long long sx = 256ll * x + 128, sy = 256ll * y + 128;
            occ_sample(s, edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn, edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn,
                       edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn, map + (size_t)y * W + x);
        }
    }
}

// grid (ceil(C / SIL_NT)): one thread per kept contour point; first[M + 1]: the contour's CSR
__global__ __launch_bounds__(SIL_NT) void occ_flag_kernel(const uint8_t* __restrict__ mask, int M, int H, int W,
                                                          const int* __restrict__ first, const int2* __restrict__ xy, int C,
                                                          const float* __restrict__ z_occ, const float* __restrict__ z_own,
                                                          uint8_t* __restrict__ pflag) {
    const int k = blockIdx.x * SIL_NT + threadIdx.x;
    if (k >= C) return;
    int lo = 0, hi = M;                          // the image i with first[i] <= k < first[i + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= k) lo = mid; else hi = mid;
    }
    const size_t img = (size_t)lo * H * W;
    const int2 p = xy[k];
    const float own = z_own[img + (size_t)p.y * W + p.x];
    bool all = true;
    const int nx[4] = {p.x - 1, p.x + 1, p.x, p.x}, ny[4] = {p.y, p.y, p.y - 1, p.y + 1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (nx[d] < 0 || nx[d] >= W || ny[d] < 0 || ny[d] >= H) continue;
        const size_t q = img + (size_t)ny[d] * W + nx[d];
        if (mask[q]) continue;
        const float zq = z_occ[q];
        const bool explained = zq < INFINITY && !(own <= zq);      // own = +inf: not known to be in front
        all = all && explained;
    }
    pflag[k] = all ? 1 : 0;
}

// grid (ceil(nv / SIL_NT), M)
__global__ __launch_bounds__(SIL_NT) void occ_hidden_kernel(const float* __restrict__ verts, int nv, const SilCam* __restrict__ cams,
                                                            const int* __restrict__ image_body, const float* __restrict__ z_occ,
                                                            int H, int W, float margin, uint8_t* __restrict__ hidden) {
    const int i = blockIdx.y, v = blockIdx.x * SIL_NT + threadIdx.x;
    if (v >= nv) return;
    const SilCam cam = cams[i];
    float px, py, pz, u, w;
    const bool ok = sil_project(cam, verts + ((size_t)image_body[i] * nv + v) * 3, px, py, pz, u, w);
    hidden[(size_t)i * nv + v] = ok && sil_hidden(z_occ + (size_t)i * H * W, H, W, margin, u, w, pz) ? 1 : 0;
}

// ========================================================================================================== host side
static int occ_fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}
#define OCC_HIP(call)                                                                                        \
    do {                                                                                                     \
        hipError_t e__ = (call);                                                                             \
        if (e__ != hipSuccess) return occ_fail(err, MVFIT_E_HIP, "%s: %s", #call, hipGetErrorString(e__));   \
    } while (0)

static size_t occ_al(size_t x) { return (x + 255) & ~(size_t)255; }

int sil_occ_set(SilState& S, const float* vertices, int num_bodies, const int32_t* body_scene, float margin, const int32_t* faces,
                int nf, hipStream_t stream, std::string& err) {
    S.occ_on = false;                            // a failed freeze leaves no occluders behind
    const int M = S.M, H = S.H, W = S.W, nv = S.nv;
    const size_t npix = (size_t)M * H * W;
    // the instance list: per image its own body, then its scene mates in ascending body index
    std::map<int32_t, std::vector<int>> scenes;
    for (int n = 0; n < num_bodies; ++n)
        if (body_scene[n] >= 0) scenes[body_scene[n]].push_back(n);
    S.h_inst.clear();
    for (int i = 0; i < M; ++i) {
        const int n = S.h_body[i];
        S.h_inst.insert(S.h_inst.end(), {i, n, 0, 0});
        if (body_scene[n] < 0) continue;
        for (int m : scenes[body_scene[n]])
            if (m != n) S.h_inst.insert(S.h_inst.end(), {i, m, 1, 0});
    }
    const size_t m_total = S.h_inst.size() / 4;
    if (m_total > (size_t)INT_MAX) return occ_fail(err, MVFIT_E_UNSUPPORTED, "mvfit_set_silhouette_occluders: more than 2^31 - 1 instances");
    const int group = (int)std::min<size_t>(m_total, (size_t)std::min(OCC_GROUP, INT_MAX / std::max(nf, 1)));
    // maps and flags: the same layout for the same (M, H, W, C)
    const size_t o_zocc = 0, o_zown = occ_al(npix * 4), o_pflag = o_zown + occ_al(npix * 4);
    const size_t need = o_pflag + occ_al(std::max(S.C, 1));
    const size_t w_inst = 0, w_nbig = occ_al(m_total * sizeof(OccInst)), w_vert = w_nbig + 256,
                 w_big = w_vert + occ_al((size_t)group * nv * sizeof(RenderVert)), w_need = w_big + occ_al((size_t)group * nf * 4);
    if (need > S.occ.size() || w_need > S.occ_ws.size()) {
        OCC_HIP(hipStreamSynchronize(stream));   // (the buffers that grow may still be read)
        OCC_HIP(S.occ.reserve(need));
        OCC_HIP(S.occ_ws.reserve(w_need));
    }
    S.o_zocc = o_zocc; S.o_zown = o_zown; S.o_pflag = o_pflag;
    unsigned char *oc = S.occ.as<unsigned char>(), *ow = S.occ_ws.as<unsigned char>();
    unsigned char *ws = S.ws.as<unsigned char>(), *cs = S.cs.as<unsigned char>();
    unsigned *z_occ = reinterpret_cast<unsigned*>(oc + o_zocc), *z_own = reinterpret_cast<unsigned*>(oc + o_zown);
    const OccInst* inst = reinterpret_cast<const OccInst*>(ow + w_inst);
    unsigned* nbig = reinterpret_cast<unsigned*>(ow + w_nbig);
    RenderVert* vert = reinterpret_cast<RenderVert*>(ow + w_vert);
    int32_t* big = reinterpret_cast<int32_t*>(ow + w_big);
    const SilCam* cams = reinterpret_cast<const SilCam*>(ws + S.o_cam);
    OCC_HIP(hipMemcpyAsync(ow + w_inst, S.h_inst.data(), m_total * sizeof(OccInst), hipMemcpyHostToDevice, stream));
    OCC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(z_occ), (int)OCC_INF, npix, stream));
    OCC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(z_own), (int)OCC_INF, npix, stream));
    for (size_t j0 = 0; j0 < m_total; j0 += group) {
        const int g = (int)std::min<size_t>(group, m_total - j0);
        OCC_HIP(hipMemsetAsync(nbig, 0, sizeof(unsigned), stream));
        hipLaunchKernelGGL(occ_transform_kernel, dim3((nv + SIL_NT - 1) / SIL_NT, g), dim3(SIL_NT), 0, stream, vertices, nv, cams,
                           inst + j0, H, W, vert);
        hipLaunchKernelGGL(occ_raster_kernel, dim3((nf + SIL_NT - 1) / SIL_NT, g), dim3(SIL_NT), 0, stream, inst + j0,
                           (const RenderVert*)vert, faces, nf, nv, H, W, z_occ, z_own, nbig, big);
        hipLaunchKernelGGL(occ_raster_big_kernel, dim3(RD_BIG_BLOCKS), dim3(SIL_NT), 0, stream, inst + j0, (const RenderVert*)vert,
                           faces, nf, nv, H, W, z_occ, z_own, (const unsigned*)nbig, (const int32_t*)big);
    }
    if (S.C)
        hipLaunchKernelGGL(occ_flag_kernel, dim3((S.C + SIL_NT - 1) / SIL_NT), dim3(SIL_NT), 0, stream, (const uint8_t*)(ws + S.o_mask), M,
                           H, W, reinterpret_cast<const int*>(ws + S.o_first), reinterpret_cast<const int2*>(cs + S.o_xy), S.C,
                           reinterpret_cast<const float*>(z_occ), reinterpret_cast<const float*>(z_own), oc + o_pflag);
    OCC_HIP(hipGetLastError());
    OCC_HIP(hipStreamSynchronize(stream));       // the host table is free again, and a failure is known before the state is set
    S.occ_margin = margin;
    S.occ_on = true;
    return MVFIT_OK;
}

int sil_occ_read(const SilState& S, float* z_occ, float* z_own, uint8_t* point_flag, hipStream_t stream, std::string& err) {
    const unsigned char* oc = S.occ.as<unsigned char>();
    const size_t bytes = (size_t)S.M * S.H * S.W * 4;
    if (z_occ) OCC_HIP(hipMemcpyAsync(z_occ, oc + S.o_zocc, bytes, hipMemcpyDeviceToDevice, stream));
    if (z_own) OCC_HIP(hipMemcpyAsync(z_own, oc + S.o_zown, bytes, hipMemcpyDeviceToDevice, stream));
    if (point_flag && S.C) OCC_HIP(hipMemcpyAsync(point_flag, oc + S.o_pflag, (size_t)S.C, hipMemcpyDeviceToDevice, stream));
    return MVFIT_OK;
}

int sil_occ_hidden(const SilState& S, const float* vertices, uint8_t* hidden, hipStream_t stream, std::string& err) {
    if (!S.occ_on) {
        OCC_HIP(hipMemsetAsync(hidden, 0, (size_t)S.M * S.nv, stream));
        return MVFIT_OK;
    }
    const unsigned char* ws = S.ws.as<unsigned char>();
    hipLaunchKernelGGL(occ_hidden_kernel, dim3((S.nv + SIL_NT - 1) / SIL_NT, S.M), dim3(SIL_NT), 0, stream, vertices, S.nv,
                       reinterpret_cast<const SilCam*>(ws + S.o_cam), reinterpret_cast<const int*>(ws + S.o_body),
                       reinterpret_cast<const float*>(S.occ.as<unsigned char>() + S.o_zocc), S.H, S.W, S.occ_margin, hidden);
    OCC_HIP(hipGetLastError());
    return MVFIT_OK;
}

}  // namespace mvfit
