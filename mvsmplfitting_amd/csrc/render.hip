// Overlay rendering of the fitted body on each view's image: the reference's save_images path
// (code/utils/utils.py:866-883 save_results -> :574-597 project_to_img -> :659-712 visualize_results ->
// :977-1028 Renderer.__call__, pyrender + OpenCV on the host) as a depth-tested rasteriser with a fixed operation order,
// so that a NumPy restatement (tests/render_oracle.py) reproduces the face-ID image bit for bit.  The contract is
// include/mvfit.h:mvfit_render_overlay.  Passes, per group of images (the workspace stays bounded; nothing depends on the
// grouping):
//   render_normals_kernel    per (problem, vertex): world-space vertex normal through the vertex->face CSR, float64
//   render_transform_kernel  per image: camera-space vertices, snapped 1/256-px positions, camera-space normals, and the
//                            camera-space box that places the nine point lights
//   render_raster_kernel     per (image, face): walks the face's pixel box with incremental int64 edge functions; a covered
//                            sample inside [znear, zfar] does a 64-bit atomicMin of (fp32 depth bits << 32 | face id) into
//                            the visibility buffer - order-independent, so the result is deterministic.  Faces whose box
//                            exceeds 1024 pixels (close-ups) are listed instead of walked by one lane:
//   render_raster_big_kernel per listed face: a whole workgroup strides over its box (same samples, same keys)
//   render_resolve_kernel    per pixel: shade + opaque composite (or the input pixel), face id
//   render_dots_kernel       per (image, point, 17 x 17 neighbourhood): the keypoint dots, drawn last
// mvfit_render_scene (several bodies per image, depth-tested against one another) runs the same passes over (image, slot)
// instances - scene_*_kernel below: transform and raster per instance, lights / visibility / big-face list per image,
// resolve decoding slot and face from the key - on top of the same device functions, so one grey body per image gives
// the bytes of mvfit_render_overlay.
// Geometry is evaluated without FP contraction (the pragma below), the divide correctly rounded (hipcc's default).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvfit_device.h"
#include "launchers.h"

#pragma clang fp contract(off)

#include "render_raster.h"      // vertex records, edge functions, face setup, the depth of a sample: shared with the silhouette term's occluder maps

namespace mvfit {

constexpr int RD_NT = 256;
constexpr unsigned long long RD_EMPTY = ~0ull;

struct RenderImage {           // per image: the nine lights (camera space)
    double L[9][3];
    double r2;
};

struct RenderGroup {           // the images of one group: problem and view per image
    int prob[RENDER_GROUP_MAX];
    int view[RENDER_GROUP_MAX];
};

struct RenderWs {              // one group's workspace (mvfit_scene.hip sizes it)
    RenderVert* vert;          // [G][Nv]
    float4* pcam;              // [G][Nv] camera-space position (w unused)
    double* ncam;              // [G][Nv][3] camera-space unit normal
    RenderImage* img;          // [G]
    unsigned long long* vis;   // [G][H][W]
    unsigned* nbig;            // [G] faces listed for render_raster_big_kernel
    int32_t* big;              // [G][Nf] their ids
};

struct RenderCam { float R[9], t[3], f, cx, cy; };

__device__ inline RenderCam load_cam(const DevProblems& Q, int b, int v) {
    const size_t i = (Q.cam_batched ? (size_t)b * Q.V : 0) + v;
    RenderCam c;
    for (int k = 0; k < 9; ++k) c.R[k] = Q.cam_R[i * 9 + k];
    for (int k = 0; k < 3; ++k) c.t[k] = Q.cam_t[i * 3 + k];
    c.f = Q.cam_f[i];
    c.cx = Q.cam_c[i * 2 + 0];
    c.cy = Q.cam_c[i * 2 + 1];
    return c;
}

// p = ((R0 X + R1 Y) + R2 Z) + t row by row, fp32, no contraction
__device__ inline void cam_point(const RenderCam& c, float X, float Y, float Z, float& px, float& py, float& pz) {
    px = ((c.R[0] * X + c.R[1] * Y) + c.R[2] * Z) + c.t[0];
    py = ((c.R[3] * X + c.R[4] * Y) + c.R[5] * Z) + c.t[1];
    pz = ((c.R[6] * X + c.R[7] * Y) + c.R[8] * Z) + c.t[2];
}

// the nine point lights from the axis-aligned box [lo, hi] of an image's camera-space vertices
__device__ inline RenderImage place_lights(const float lo[3], const float hi[3]) {
    double cen[3], h[3];
    for (int k = 0; k < 3; ++k) {
        cen[k] = 0.5 * ((double)lo[k] + (double)hi[k]);
        h[k] = 0.5 * ((double)hi[k] - (double)lo[k]);
    }
    const double r = sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
    RenderImage im;
    im.r2 = r * r;
    // utils.py:937-950 add_pointLight: theta in {pi/6, pi/2, 5pi/6} x phi in {0, 2pi/3, 4pi/3}
    const double PI = 3.14159265358979323846;
    for (int a = 0; a < 3; ++a)
        for (int p = 0; p < 3; ++p) {
            const double th = PI * (double)(2 * a + 1) / 6.0, ph = 2.0 * PI * (double)p / 3.0;
            const double d[3] = {sin(th) * cos(ph), sin(th) * sin(ph), cos(th)};
            for (int k = 0; k < 3; ++k) im.L[a * 3 + p][k] = cen[k] + r * d[k];
        }
    return im;
}

__global__ __launch_bounds__(RD_NT) void render_normals_kernel(const float* __restrict__ verts, int Nv,
                                                               const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ vf_ptr,
                                                               const int32_t* __restrict__ vf_idx,
                                                               double* __restrict__ nrm) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * RD_NT + threadIdx.x;
    if (i >= Nv) return;
    const float* P = verts + (size_t)b * Nv * 3;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = vf_ptr[i]; k < vf_ptr[i + 1]; ++k) {          // the vertex's faces in ascending id
        const int f = vf_idx[k];
        const int a = faces[f * 3 + 0], bb = faces[f * 3 + 1], cc = faces[f * 3 + 2];
        const double ax = P[a * 3 + 0], ay = P[a * 3 + 1], az = P[a * 3 + 2];
        const double e1x = (double)P[bb * 3 + 0] - ax, e1y = (double)P[bb * 3 + 1] - ay, e1z = (double)P[bb * 3 + 2] - az;
        const double e2x = (double)P[cc * 3 + 0] - ax, e2y = (double)P[cc * 3 + 1] - ay, e2z = (double)P[cc * 3 + 2] - az;
        sx = sx + (e1y * e2z - e1z * e2y);
        sy = sy + (e1z * e2x - e1x * e2z);
        sz = sz + (e1x * e2y - e1y * e2x);
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    double* o = nrm + ((size_t)b * Nv + i) * 3;
    if (len > 0.0) { o[0] = sx / len; o[1] = sy / len; o[2] = sz / len; }
    else { o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; }
}

// one body under one camera, by a whole workgroup: vertex records, camera-space positions and normals into vert / pcam /
// ncam [Nv]; on return red[0..2][0] / red[3..5][0] hold the min / max corner of the camera-space box
__device__ inline void transform_body(const RenderCam& c, const float* __restrict__ P, const double* __restrict__ N, int Nv, int H,
                                      int W, RenderVert* vert, float4* pcam, double* ncam, float (*red)[RD_NT]) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < Nv; i += RD_NT) {
        float px, py, pz;
        cam_point(c, P[i * 3 + 0], P[i * 3 + 1], P[i * 3 + 2], px, py, pz);
        const float u = c.f * (px / pz) + c.cx;
        const float w = c.f * (py / pz) + c.cy;
        RenderVert rv;                                          // (render_raster.h: snap_vertex states the same record)
        rv.ok = (pz > RD_ZNEAR) && (u >= -RD_GUARD) && (u <= (float)W + RD_GUARD) && (w >= -RD_GUARD) && (w <= (float)H + RD_GUARD);
        rv.X = rv.ok ? (int)rintf(u * 256.f) : 0;
        rv.Y = rv.ok ? (int)rintf(w * 256.f) : 0;
        rv.pz = pz;
        vert[i] = rv;
        pcam[i] = make_float4(px, py, pz, 0.f);
        const double nx = N[i * 3 + 0], ny = N[i * 3 + 1], nz = N[i * 3 + 2];
        ncam[(size_t)i * 3 + 0] = ((double)c.R[0] * nx + (double)c.R[1] * ny) + (double)c.R[2] * nz;
        ncam[(size_t)i * 3 + 1] = ((double)c.R[3] * nx + (double)c.R[4] * ny) + (double)c.R[5] * nz;
        ncam[(size_t)i * 3 + 2] = ((double)c.R[6] * nx + (double)c.R[7] * ny) + (double)c.R[8] * nz;
        mn[0] = fminf(mn[0], px); mn[1] = fminf(mn[1], py); mn[2] = fminf(mn[2], pz);
        mx[0] = fmaxf(mx[0], px); mx[1] = fmaxf(mx[1], py); mx[2] = fmaxf(mx[2], pz);
    }
    for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = mn[k]; red[3 + k][threadIdx.x] = mx[k]; }
    __syncthreads();
    for (int s = RD_NT / 2; s > 0; s >>= 1) {                   // min / max: exact in any order
        if (threadIdx.x < s)
            for (int k = 0; k < 3; ++k) {
                red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]);
                red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
            }
        __syncthreads();
    }
}

// one workgroup per image of the group
__global__ __launch_bounds__(RD_NT) void render_transform_kernel(DevProblems Q, RenderGroup G, const float* __restrict__ verts,
                                                                 const double* __restrict__ nrm, int Nv, int H, int W,
                                                                 RenderWs ws) {
    __shared__ float red[6][RD_NT];
    const int g = blockIdx.x, b = G.prob[g], v = G.view[g];
    const RenderCam c = load_cam(Q, b, v);
    const size_t o = (size_t)g * Nv;
    transform_body(c, verts + (size_t)b * Nv * 3, nrm + (size_t)b * Nv * 3, Nv, H, W, ws.vert + o, ws.pcam + o, ws.ncam + o * 3, red);
    if (threadIdx.x == 0) {
        const float lo[3] = {red[0][0], red[1][0], red[2][0]}, hi[3] = {red[3][0], red[4][0], red[5][0]};
        ws.img[g] = place_lights(lo, hi);
    }
}

// one covered-or-not sample: e0 = edge v1->v2 (opposite v0), e1 = v2->v0, e2 = v0->v1, already oriented
__device__ inline void raster_sample(const FaceSetup& s, int f, long long e0, long long e1, long long e2, unsigned long long* px) {
    float z;
    if (!raster_depth(s, e0, e1, e2, z)) return;
    atomicMin(px, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)f);
}

// one thread per (image, face); a face whose pixel box exceeds RD_BIG_BOX pixels is handed to render_raster_big_kernel
__global__ __launch_bounds__(RD_NT) void render_raster_kernel(const int32_t* __restrict__ faces, int Nf, int Nv, int H, int W,
                                                              RenderWs ws) {
    const int g = blockIdx.y;
    const int f = blockIdx.x * RD_NT + threadIdx.x;
    if (f >= Nf) return;
    FaceSetup s;
    if (!face_setup(ws.vert + (size_t)g * Nv, faces, f, H, W, s)) return;
    if ((long long)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) > RD_BIG_BOX) {
        const unsigned k = atomicAdd(ws.nbig + g, 1u);             // k < Nf: each face is listed at most once
        ws.big[(size_t)g * Nf + k] = f;
        return;
    }
    const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
    // per-pixel steps along x (256 sub-pixel units)
    const long long dx0 = -256ll * (v2.Y - v1.Y) * s.sgn, dx1 = -256ll * (v0.Y - v2.Y) * s.sgn, dx2 = -256ll * (v1.Y - v0.Y) * s.sgn;
    unsigned long long* vis = ws.vis + (size_t)g * H * W;
    for (int y = s.y0; y <= s.y1; ++y) {
        const long long sy = 256ll * y + 128, sx = 256ll * s.x0 + 128;
        long long e0 = edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn;
        long long e1 = edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn;
        long long e2 = edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn;
        for (int x = s.x0; x <= s.x1; ++x, e0 += dx0, e1 += dx1, e2 += dx2)
            raster_sample(s, f, e0, e1, e2, vis + (size_t)y * W + x);
    }
}

// the listed large faces: one workgroup per face at a time, its threads striding over the face's pixel box; the edge
// values are evaluated directly at each sample - the same integers the incremental walk reaches, so the same keys
__global__ __launch_bounds__(RD_NT) void render_raster_big_kernel(const int32_t* __restrict__ faces, int Nf, int Nv, int H,
                                                                  int W, RenderWs ws) {
    const int g = blockIdx.y;
    const unsigned n = ws.nbig[g];
    unsigned long long* vis = ws.vis + (size_t)g * H * W;
    for (unsigned j = blockIdx.x; j < n; j += gridDim.x) {
        const int f = ws.big[(size_t)g * Nf + j];
        FaceSetup s;
        if (!face_setup(ws.vert + (size_t)g * Nv, faces, f, H, W, s)) continue;
        const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
        const int bw = s.x1 - s.x0 + 1;
        const long long npx = (long long)bw * (s.y1 - s.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += RD_NT) {
            const int y = s.y0 + (int)(p / bw), x = s.x0 + (int)(p % bw);
            const long long sx = 256ll * x + 128, sy = 256ll * y + 128;
            raster_sample(s, f, edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn, edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn,
                          edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn, vis + (size_t)y * W + x);
        }
    }
}

// the light sum of the pixel (x, y) that sees face f: V / pc / nc the records of the face's body in this image
__device__ inline double pixel_light(const int32_t* __restrict__ faces, const RenderVert* V, const float4* pc, const double* nc,
                                     int f, int x, int y, const RenderImage& im) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    const RenderVert v0 = V[i0], v1 = V[i1], v2 = V[i2];
    const long long sgn = edge_fn(v0.X, v0.Y, v1.X, v1.Y, v2.X, v2.Y) > 0 ? 1 : -1;
    const long long sx = 256ll * x + 128, sy = 256ll * y + 128;
    const double e0 = (double)(edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * sgn);
    const double e1 = (double)(edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * sgn);
    const double e2 = (double)(edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * sgn);
    const double w0 = e0 * (1.0 / (double)v0.pz), w1 = e1 * (1.0 / (double)v1.pz), w2 = e2 * (1.0 / (double)v2.pz);
    const double w = (w0 + w1) + w2;
    const double b0 = w0 / w, b1 = w1 / w, b2 = w2 / w;       // perspective-correct barycentrics
    const float4 p0 = pc[i0], p1 = pc[i1], p2 = pc[i2];
    const double q[3] = {(b0 * p0.x + b1 * p1.x) + b2 * p2.x, (b0 * p0.y + b1 * p1.y) + b2 * p2.y,
                         (b0 * p0.z + b1 * p1.z) + b2 * p2.z};
    const double* n0 = nc + (size_t)i0 * 3;
    const double* n1 = nc + (size_t)i1 * 3;
    const double* n2 = nc + (size_t)i2 * 3;
    double n[3];
    for (int k = 0; k < 3; ++k) n[k] = (b0 * n0[k] + b1 * n1[k]) + b2 * n2[k];
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len > 0.0) for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
    if ((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2] > 0.0)          // faces away from the camera: two-sided shading
        for (int k = 0; k < 3; ++k) n[k] = -n[k];
    double acc = 0.0;
    for (int k = 0; k < 9; ++k) {
        const double lx = im.L[k][0] - q[0], ly = im.L[k][1] - q[1], lz = im.L[k][2] - q[2];
        const double d2 = (lx * lx + ly * ly) + lz * lz;
        const double ndl = ((n[0] * lx + n[1] * ly) + n[2] * lz) / sqrt(d2);
        if (ndl > 0.0) acc = acc + im.r2 * ndl / d2;
    }
    return acc;
}

// one thread per pixel of the group's images
__global__ __launch_bounds__(RD_NT) void render_resolve_kernel(const int32_t* __restrict__ faces, int Nv, int H, int W,
                                                               RenderWs ws, const uint8_t* in, uint8_t* out,
                                                               int32_t* __restrict__ face_id) {
    const int g = blockIdx.y;
    const int pix = blockIdx.x * RD_NT + threadIdx.x;
    if (pix >= H * W) return;
    const size_t o = (size_t)g * H * W + pix;
    const unsigned long long key = ws.vis[o];
    if (key == RD_EMPTY) {
        if (face_id) face_id[o] = -1;
        if (in != out) { out[o * 3 + 0] = in[o * 3 + 0]; out[o * 3 + 1] = in[o * 3 + 1]; out[o * 3 + 2] = in[o * 3 + 2]; }
        return;
    }
    const int f = (int)(unsigned)(key & 0xffffffffull);
    if (face_id) face_id[o] = f;
    const int y = pix / W, x = pix - y * W;
    const size_t vb = (size_t)g * Nv;
    const double acc = pixel_light(faces, ws.vert + vb, ws.pcam + vb, ws.ncam + vb * 3, f, x, y, ws.img[g]);
    const double PI = 3.14159265358979323846;
    const double s = 0.5 * 0.3 + (0.5 / PI) * acc;
    const uint8_t val = (uint8_t)floor(255.0 * pow(fmin(1.0, s), 1.0 / 2.2) + 0.5);
    out[o * 3 + 0] = val; out[o * 3 + 1] = val; out[o * 3 + 2] = val;
}

// one dot by a workgroup, each thread one pixel of the point's 17 x 17 neighbourhood; out: the image
__device__ inline void draw_dot(const RenderCam& c, const float* P, int H, int W, uint8_t* out) {
    float px, py, pz;
    cam_point(c, P[0], P[1], P[2], px, py, pz);
    if (!(pz > RD_ZNEAR)) return;
    const float u = c.f * (px / pz) + c.cx, v = c.f * (py / pz) + c.cy;
    // beyond the guard band no dot pixel can reach the image (and the int conversion below stays defined)
    if (!(u >= -RD_GUARD && u <= (float)W + RD_GUARD && v >= -RD_GUARD && v <= (float)H + RD_GUARD)) return;
    const int cx = (int)u, cy = (int)v;                 // astype(np.int32): truncation toward zero
    for (int t = threadIdx.x; t < 17 * 17; t += RD_NT) {
        const int dy = t / 17 - 8, dx = t % 17 - 8;
        if (dx * dx + dy * dy > 64) continue;
        const int x = cx + dx, y = cy + dy;
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        const size_t o = (size_t)y * W + x;
        out[o * 3 + 0] = 255; out[o * 3 + 1] = 0; out[o * 3 + 2] = 0;
    }
}

// grid (num_points, group images)
__global__ __launch_bounds__(RD_NT) void render_dots_kernel(DevProblems Q, RenderGroup G, const float* __restrict__ points,
                                                            int num_points, int H, int W, uint8_t* out) {
    const int g = blockIdx.y, b = G.prob[g];
    const RenderCam c = load_cam(Q, b, G.view[g]);
    draw_dot(c, points + ((size_t)b * num_points + blockIdx.x) * 3, H, W, out + (size_t)g * H * W * 3);
}

// ---- mvfit_render_scene: several bodies per image.  The unit of work is an (image, slot) instance: body k of image i is the
// mesh whose vertex j is vertex k Nv + j and whose face f is face k Nf + f of the image's concatenated mesh.  The tables
// live in device memory (SceneImage per image, SceneInst per instance, in image order); the vertex records are per
// instance, the visibility buffer, the big-face list and the lights per image.
struct SceneImage { int first, count, view, cam_prob; };   // instances [first, first + count) of the call; cam_prob: the
                                                           // problem whose cameras draw the image (per-problem cameras)
struct SceneInst { int prob, image, slot; float col[3]; }; // image: index within the call

struct SceneWs {               // one group's workspace: n images, m instances
    RenderVert* vert;          // [m][Nv]
    float4* pcam;              // [m][Nv]
    double* ncam;              // [m][Nv][3]
    float* box;                // [m][6] camera-space min / max corner of the instance
    RenderImage* img;          // [n]
    unsigned long long* vis;   // [n][H][W]
    unsigned* nbig;            // [n]
    int32_t* big;              // [m][Nf]: the list of image g starts at its first instance; entries (instance in group) Nf + f
};

// one workgroup per instance of the group (instances j0 .. j0 + m of the call, images from i0 on)
__global__ __launch_bounds__(RD_NT) void scene_transform_kernel(DevProblems Q, const SceneImage* __restrict__ images,
                                                                const SceneInst* __restrict__ inst, int j0,
                                                                const float* __restrict__ verts, const double* __restrict__ nrm,
                                                                int Nv, int H, int W, SceneWs ws) {
    __shared__ float red[6][RD_NT];
    const int j = blockIdx.x;
    const SceneInst in = inst[j0 + j];
    const SceneImage im = images[in.image];
    const RenderCam c = load_cam(Q, im.cam_prob, im.view);
    const size_t o = (size_t)j * Nv;
    transform_body(c, verts + (size_t)in.prob * Nv * 3, nrm + (size_t)in.prob * Nv * 3, Nv, H, W, ws.vert + o, ws.pcam + o,
                   ws.ncam + o * 3, red);
    if (threadIdx.x < 6) ws.box[(size_t)j * 6 + threadIdx.x] = red[threadIdx.x][0];
}

// one thread per image of the group: the box of all its bodies (min / max: exact in any order), then the lights
__global__ __launch_bounds__(64) void scene_lights_kernel(const SceneImage* __restrict__ images, int i0, int n, int j0, SceneWs ws) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n) return;
    const SceneImage im = images[i0 + g];
    if (im.count == 0) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < im.count; ++k) {
        const float* b = ws.box + (size_t)(im.first - j0 + k) * 6;
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], b[a]); hi[a] = fmaxf(hi[a], b[3 + a]); }
    }
    ws.img[g] = place_lights(lo, hi);
}

// one thread per (instance, face)
__global__ __launch_bounds__(RD_NT) void scene_raster_kernel(const SceneInst* __restrict__ inst, int i0, int j0,
                                                             const int32_t* __restrict__ faces, int Nf, int Nv, int H, int W,
                                                             SceneWs ws) {
    const int j = blockIdx.y;
    const int f = blockIdx.x * RD_NT + threadIdx.x;
    if (f >= Nf) return;
    FaceSetup s;
    if (!face_setup(ws.vert + (size_t)j * Nv, faces, f, H, W, s)) return;
    const SceneInst in = inst[j0 + j];
    const int g = in.image - i0;
    if ((long long)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) > RD_BIG_BOX) {
        const unsigned k = atomicAdd(ws.nbig + g, 1u);             // k < count Nf: each face of each body at most once
        ws.big[(size_t)(j - in.slot) * Nf + k] = j * Nf + f;       // j - slot: the image's first instance
        return;
    }
    const int id = in.slot * Nf + f;
    const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
    const long long dx0 = -256ll * (v2.Y - v1.Y) * s.sgn, dx1 = -256ll * (v0.Y - v2.Y) * s.sgn, dx2 = -256ll * (v1.Y - v0.Y) * s.sgn;
    unsigned long long* vis = ws.vis + (size_t)g * H * W;
    for (int y = s.y0; y <= s.y1; ++y) {
        const long long sy = 256ll * y + 128, sx = 256ll * s.x0 + 128;
        long long e0 = edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn;
        long long e1 = edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn;
        long long e2 = edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn;
        for (int x = s.x0; x <= s.x1; ++x, e0 += dx0, e1 += dx1, e2 += dx2)
            raster_sample(s, id, e0, e1, e2, vis + (size_t)y * W + x);
    }
}

// the listed large faces of each image of the group, a workgroup per face at a time
__global__ __launch_bounds__(RD_NT) void scene_raster_big_kernel(const SceneImage* __restrict__ images,
                                                                 const SceneInst* __restrict__ inst, int i0, int j0,
                                                                 const int32_t* __restrict__ faces, int Nf, int Nv, int H, int W,
                                                                 SceneWs ws) {
    const int g = blockIdx.y;
    const unsigned n = ws.nbig[g];
    if (n == 0) return;
    const int32_t* list = ws.big + (size_t)(images[i0 + g].first - j0) * Nf;
    unsigned long long* vis = ws.vis + (size_t)g * H * W;
    for (unsigned q = blockIdx.x; q < n; q += gridDim.x) {
        const int e = list[q], j = e / Nf, f = e - j * Nf;
        FaceSetup s;
        if (!face_setup(ws.vert + (size_t)j * Nv, faces, f, H, W, s)) continue;
        const int id = inst[j0 + j].slot * Nf + f;
        const RenderVert &v0 = s.v0, &v1 = s.v1, &v2 = s.v2;
        const int bw = s.x1 - s.x0 + 1;
        const long long npx = (long long)bw * (s.y1 - s.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += RD_NT) {
            const int y = s.y0 + (int)(p / bw), x = s.x0 + (int)(p % bw);
            const long long sx = 256ll * x + 128, sy = 256ll * y + 128;
            raster_sample(s, id, edge_fn(v1.X, v1.Y, v2.X, v2.Y, sx, sy) * s.sgn, edge_fn(v2.X, v2.Y, v0.X, v0.Y, sx, sy) * s.sgn,
                          edge_fn(v0.X, v0.Y, v1.X, v1.Y, sx, sy) * s.sgn, vis + (size_t)y * W + x);
        }
    }
}

// one thread per pixel of the group's images: slot and face from the key, the body's colour per channel
__global__ __launch_bounds__(RD_NT) void scene_resolve_kernel(const SceneImage* __restrict__ images,
                                                              const SceneInst* __restrict__ inst, int i0, int j0,
                                                              const int32_t* __restrict__ faces, int Nf, int Nv, int H, int W,
                                                              SceneWs ws, const uint8_t* in, uint8_t* out,
                                                              int32_t* __restrict__ face_id, int32_t* __restrict__ body_id) {
    const int g = blockIdx.y;
    const int pix = blockIdx.x * RD_NT + threadIdx.x;
    if (pix >= H * W) return;
    const size_t o = (size_t)g * H * W + pix;
    const unsigned long long key = ws.vis[o];
    if (key == RD_EMPTY) {
        if (face_id) face_id[o] = -1;
        if (body_id) body_id[o] = -1;
        if (in != out) { out[o * 3 + 0] = in[o * 3 + 0]; out[o * 3 + 1] = in[o * 3 + 1]; out[o * 3 + 2] = in[o * 3 + 2]; }
        return;
    }
    const int id = (int)(unsigned)(key & 0xffffffffull);
    const int k = id / Nf, f = id - k * Nf;
    if (face_id) face_id[o] = f;
    if (body_id) body_id[o] = k;
    const int y = pix / W, x = pix - y * W;
    const int j = images[i0 + g].first - j0 + k;
    const size_t vb = (size_t)j * Nv;
    const double acc = pixel_light(faces, ws.vert + vb, ws.pcam + vb, ws.ncam + vb * 3, f, x, y, ws.img[g]);
    const double PI = 3.14159265358979323846;
    const float* col = inst[j0 + j].col;
    uint8_t val[3];
    for (int ch = 0; ch < 3; ++ch) {
        if (ch > 0 && col[ch] == col[ch - 1]) { val[ch] = val[ch - 1]; continue; }     // same colour, same byte
        const double c = (double)col[ch];
        const double s = c * 0.3 + (c / PI) * acc;
        val[ch] = (uint8_t)floor(255.0 * pow(fmin(1.0, s), 1.0 / 2.2) + 0.5);
    }
    out[o * 3 + 0] = val[0]; out[o * 3 + 1] = val[1]; out[o * 3 + 2] = val[2];
}

// grid (num_points, group instances): the dots of every body of every image
__global__ __launch_bounds__(RD_NT) void scene_dots_kernel(DevProblems Q, const SceneImage* __restrict__ images,
                                                           const SceneInst* __restrict__ inst, int i0, int j0,
                                                           const float* __restrict__ points, int num_points, int H, int W,
                                                           uint8_t* out) {
    const SceneInst in = inst[j0 + blockIdx.y];
    const SceneImage im = images[in.image];
    const RenderCam c = load_cam(Q, im.cam_prob, im.view);
    draw_dot(c, points + ((size_t)in.prob * num_points + blockIdx.x) * 3, H, W, out + (size_t)(in.image - i0) * H * W * 3);
}

size_t render_ws_bytes(int G, int Nv, int Nf, int H, int W) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    return up((size_t)G * Nv * sizeof(RenderVert)) + up((size_t)G * Nv * sizeof(float4)) + up((size_t)G * Nv * 3 * sizeof(double)) +
           up((size_t)G * sizeof(RenderImage)) + up((size_t)G * sizeof(unsigned)) + up((size_t)G * Nf * sizeof(int32_t)) +
           up((size_t)G * H * W * sizeof(unsigned long long));
}

hipError_t launch_render_normals(const float* verts, int B, int Nv, const int32_t* faces, const int32_t* vf_ptr,
                                 const int32_t* vf_idx, double* nrm, hipStream_t stream) {
    hipLaunchKernelGGL(render_normals_kernel, dim3((Nv + RD_NT - 1) / RD_NT, B), dim3(RD_NT), 0, stream, verts, Nv, faces,
                       vf_ptr, vf_idx, nrm);
    return hipGetLastError();
}

// one group of n <= RENDER_GROUP_MAX images; ws of render_ws_bytes(n, Nv, Nf, H, W) bytes; in / out / face_id at the group's
// first image
hipError_t launch_render_group(const DevProblems& Q, const int* prob, const int* view, int n, const float* verts,
                               const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points, int num_points,
                               int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, void* ws_mem,
                               hipStream_t stream) {
    RenderGroup G{};
    for (int i = 0; i < n; ++i) { G.prob[i] = prob[i]; G.view[i] = view[i]; }
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* p = static_cast<char*>(ws_mem);
    RenderWs ws;
    ws.vert = reinterpret_cast<RenderVert*>(p); p += up((size_t)n * Nv * sizeof(RenderVert));
    ws.pcam = reinterpret_cast<float4*>(p); p += up((size_t)n * Nv * sizeof(float4));
    ws.ncam = reinterpret_cast<double*>(p); p += up((size_t)n * Nv * 3 * sizeof(double));
    ws.img = reinterpret_cast<RenderImage*>(p); p += up((size_t)n * sizeof(RenderImage));
    ws.nbig = reinterpret_cast<unsigned*>(p); p += up((size_t)n * sizeof(unsigned));
    ws.big = reinterpret_cast<int32_t*>(p); p += up((size_t)n * Nf * sizeof(int32_t));
    ws.vis = reinterpret_cast<unsigned long long*>(p);
    hipError_t e = hipMemsetAsync(ws.vis, 0xff, (size_t)n * H * W * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(ws.nbig, 0, (size_t)n * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(render_transform_kernel, dim3(n), dim3(RD_NT), 0, stream, Q, G, verts, nrm, Nv, H, W, ws);
    hipLaunchKernelGGL(render_raster_kernel, dim3((Nf + RD_NT - 1) / RD_NT, n), dim3(RD_NT), 0, stream, faces, Nf, Nv, H, W, ws);
    hipLaunchKernelGGL(render_raster_big_kernel, dim3(RD_BIG_BLOCKS, n), dim3(RD_NT), 0, stream, faces, Nf, Nv, H, W, ws);
    hipLaunchKernelGGL(render_resolve_kernel, dim3((H * W + RD_NT - 1) / RD_NT, n), dim3(RD_NT), 0, stream, faces, Nv, H, W, ws,
                       in, out, face_id);
    if (points && num_points > 0)
        hipLaunchKernelGGL(render_dots_kernel, dim3(num_points, n), dim3(RD_NT), 0, stream, Q, G, points, num_points, H, W, out);
    return hipGetLastError();
}

size_t scene_ws_bytes(int n, int m, int Nv, int Nf, int H, int W) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    return up((size_t)m * Nv * sizeof(RenderVert)) + up((size_t)m * Nv * sizeof(float4)) + up((size_t)m * Nv * 3 * sizeof(double)) +
           up((size_t)m * 6 * sizeof(float)) + up((size_t)n * sizeof(RenderImage)) + up((size_t)n * sizeof(unsigned)) +
           up((size_t)m * Nf * sizeof(int32_t)) + up((size_t)n * H * W * sizeof(unsigned long long));
}

// one group of mvfit_render_scene: images i0 .. i0 + n of the call and their instances j0 .. j0 + m; tab: the call's tables
// (SCENE_IMAGE_WORDS int32 per image, then SCENE_INST_WORDS per instance); in / out / ids at the group's first image
hipError_t launch_scene_group(const DevProblems& Q, const int32_t* tab, int num_images, int i0, int n, int j0, int m,
                              const float* verts, const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points,
                              int num_points, int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, int32_t* body_id,
                              void* ws_mem, hipStream_t stream) {
    static_assert(sizeof(SceneImage) == SCENE_IMAGE_WORDS * 4 && sizeof(SceneInst) == SCENE_INST_WORDS * 4, "table layout");
    const SceneImage* images = reinterpret_cast<const SceneImage*>(tab);
    const SceneInst* inst = reinterpret_cast<const SceneInst*>(tab + (size_t)num_images * SCENE_IMAGE_WORDS);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* p = static_cast<char*>(ws_mem);
    SceneWs ws;
    ws.vert = reinterpret_cast<RenderVert*>(p); p += up((size_t)m * Nv * sizeof(RenderVert));
    ws.pcam = reinterpret_cast<float4*>(p); p += up((size_t)m * Nv * sizeof(float4));
    ws.ncam = reinterpret_cast<double*>(p); p += up((size_t)m * Nv * 3 * sizeof(double));
    ws.box = reinterpret_cast<float*>(p); p += up((size_t)m * 6 * sizeof(float));
    ws.img = reinterpret_cast<RenderImage*>(p); p += up((size_t)n * sizeof(RenderImage));
    ws.nbig = reinterpret_cast<unsigned*>(p); p += up((size_t)n * sizeof(unsigned));
    ws.big = reinterpret_cast<int32_t*>(p); p += up((size_t)m * Nf * sizeof(int32_t));
    ws.vis = reinterpret_cast<unsigned long long*>(p);
    hipError_t e = hipMemsetAsync(ws.vis, 0xff, (size_t)n * H * W * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(ws.nbig, 0, (size_t)n * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    if (m > 0) {
        hipLaunchKernelGGL(scene_transform_kernel, dim3(m), dim3(RD_NT), 0, stream, Q, images, inst, j0, verts, nrm, Nv, H, W, ws);
        hipLaunchKernelGGL(scene_lights_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, images, i0, n, j0, ws);
        hipLaunchKernelGGL(scene_raster_kernel, dim3((Nf + RD_NT - 1) / RD_NT, m), dim3(RD_NT), 0, stream, inst, i0, j0, faces, Nf,
                           Nv, H, W, ws);
        hipLaunchKernelGGL(scene_raster_big_kernel, dim3(RD_BIG_BLOCKS, n), dim3(RD_NT), 0, stream, images, inst, i0, j0, faces, Nf,
                           Nv, H, W, ws);
    }
    hipLaunchKernelGGL(scene_resolve_kernel, dim3((H * W + RD_NT - 1) / RD_NT, n), dim3(RD_NT), 0, stream, images, inst, i0, j0,
                       faces, Nf, Nv, H, W, ws, in, out, face_id, body_id);
    if (points && num_points > 0 && m > 0)
        hipLaunchKernelGGL(scene_dots_kernel, dim3(num_points, m), dim3(RD_NT), 0, stream, Q, images, inst, i0, j0, points,
                           num_points, H, W, out);
    return hipGetLastError();
}

}  // namespace mvfit
