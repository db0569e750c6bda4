// Scene collision loss between the bodies of a scene: SDFLoss.forward of the reference's sdf package
// (sdf/sdf/sdf_loss.py:51-99) as the unmodified reference executes it, batched over scenes, with its gradient.
//
// Per scene of P bodies (vertices already carry their translation):
//   box of body i (no gradient, :17-24,69-70): lo / hi over its vertices, c = (lo + hi) / 2 in float32 (boxes.mean(dim=1)),
//       s = float32((1 + scale_factor) * 0.5) * max_axis(hi - lo) - the Python-float factor is rounded to float32 and applied
//       to the float32 extent, as the expression at :70 evaluates;
//   phi_i = SDF(faces, (v_i - c_i) / s_i, G) (:72-76, no gradient): the voxel function of sdf_device.h over ALL faces,
//       voxelised by the kernels of the stand-alone op (sdf_voxelize.hip / the face lists of sdf_term.hip) - the same bits;
//   for every ordered pair i != j and every vertex v of body j (:81-98): x = (v - c_i) / s_i, p = grid_sample(phi_i, x)
//       (trilinear, zeros padding, align_corners = False, x the fastest grid axis), with a robustifier r:
//       f = (p / r)^2, p <- f / (f + 1); loss = sum p / P^2.
// The isolation filter (:39-49,59-68) is a no-op in the reference as it runs: `isolated` is a uint8 tensor, so `~isolated`
// is the bitwise complement (255 / 254), its sum is never 0 and indexing with it keeps every body.  Hence every body of a
// scene is kept - one far away from the others contributes 0 and still counts in P^2.  A scene of one body gives 0.
// The gradient flows through the sampled positions only:
//   d loss / d v_jv = sum_{i != j} (d p / d x) / s_i * [robustifier derivative] / P^2.
//
// MI355X mapping: the fields are materialised (N * G^3 * 4 B, grouped by the caller under a cap) and the one new hot kernel
// samples them: one thread owns a target vertex (j, v), walks the source bodies of its scene in ascending i, tests the
// source's box before it touches the field (most targets lie outside and read nothing), accumulates value and gradient in
// registers and stores g_vertices[j, v] once.  The loss is a fixed-order reduction: a shuffle tree per wave, the waves of a
// workgroup in order, one partial per (body, workgroup), then one pass per scene over its partials in ascending order - no
// float atomics, and nothing a scene computes depends on the other scenes of the call or on where it stands in it.
#include "sdf_device.h"
#include "mvfit_device.h"
#include "wave_ops.h"
#include "sdf_entries.h"
#include "launchers.h"

namespace mvfit {

constexpr int SCN_NT = 256;

struct SceneBody { int first, count, pad0, pad1; };      // the body's scene: first body (index in the call), body count
static_assert(sizeof(SceneBody) == 16, "table row");

#pragma clang fp contract(off)

// grid (bodies of the group), bodies b0 .. : the box of each body and its vertices in the box's coordinates (what the
// voxelisation reads).  min / max are exact in any order.
__global__ __launch_bounds__(SCN_NT) void scene_box_kernel(const float* __restrict__ verts, int nv, int b0, float factor,
                                                           float4* __restrict__ box, float* __restrict__ local) {
    __shared__ float sh[SCN_NT / 64][6];
    __shared__ float4 sh_box;
    const int b = b0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vb = verts + (size_t)b * nv * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = tid; v < nv; v += SCN_NT)
        for (int a = 0; a < 3; ++a) { const float x = vb[3 * v + a]; lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) { sh[wave][a] = lo[a]; sh[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SCN_NT / 64; ++w)
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], sh[w][a]); hi[a] = fmaxf(hi[a], sh[w][3 + a]); }
        const float ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
        const float4 bx = make_float4((lo[0] + hi[0]) / 2.0f, (lo[1] + hi[1]) / 2.0f, (lo[2] + hi[2]) / 2.0f, factor * ext);
        sh_box = bx;
        box[b] = bx;
    }
    __syncthreads();
    const float4 bx = sh_box;
    float* lb = local + (size_t)blockIdx.x * nv * 3;
    for (int v = tid; v < nv; v += SCN_NT) {
        lb[3 * v + 0] = (vb[3 * v + 0] - bx.x) / bx.w;
        lb[3 * v + 1] = (vb[3 * v + 1] - bx.y) / bx.w;
        lb[3 * v + 2] = (vb[3 * v + 2] - bx.z) / bx.w;
    }
}

// One target vertex (p0, p1, p2) against the field f of a source body with box bx: the sampled value is added to acc and
// its gradient with respect to the vertex to g.  Shared by scene_pair_kernel and scene_entries_kernel: the same
// expressions in the same order (contraction is off in this file), hence the same bits in both.
__device__ __forceinline__ void scene_sample_add(const float4 bx, const float* __restrict__ f, int G, float rob, float p0,
                                                 float p1, float p2, float& acc, float (&g)[3]) {
    const float fG = (float)G;
    // grid_sample's source index, align_corners = False: ((x + 1) * G - 1) / 2
    const float ix = (((p0 - bx.x) / bx.w + 1.f) * fG - 1.f) / 2.f;
    const float iy = (((p1 - bx.y) / bx.w + 1.f) * fG - 1.f) / 2.f;
    const float iz = (((p2 - bx.z) / bx.w + 1.f) * fG - 1.f) / 2.f;
    // outside the field and its border band of zeros padding: value and gradient 0, no memory access (also a NaN)
    if (!(ix > -1.f && ix < fG && iy > -1.f && iy < fG && iz > -1.f && iz < fG)) return;
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float tx = ix - fx, ty = iy - fy, tz = iz - fz;
    float c[2][2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int xx = x0 + dx, yy = y0 + dy, zz = z0 + dz;
                const bool in = xx >= 0 && xx < G && yy >= 0 && yy < G && zz >= 0 && zz < G;
                c[dz][dy][dx] = in ? f[((size_t)zz * G + yy) * G + xx] : 0.f;
            }
    const float wx[2] = {1.f - tx, tx}, wy[2] = {1.f - ty, ty}, wz[2] = {1.f - tz, tz};
    float p = 0.f, dpx = 0.f, dpy = 0.f, dpz = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float cv = c[dz][dy][dx];
                p += cv * (wx[dx] * wy[dy] * wz[dz]);
                dpx += cv * ((dx ? 1.f : -1.f) * wy[dy] * wz[dz]);
                dpy += cv * ((dy ? 1.f : -1.f) * wx[dx] * wz[dz]);
                dpz += cv * ((dz ? 1.f : -1.f) * wx[dx] * wy[dy]);
            }
    // d index / d vertex = G / 2 / s_i
    float k = fG / 2.f / bx.w;
    if (rob > 0.f) {
        const float q = p / rob, fr = q * q, den = fr + 1.f;
        k *= 2.f * q / rob / (den * den);
        p = fr / den;
    }
    acc += p;
    g[0] += dpx * k; g[1] += dpy * k; g[2] += dpz * k;
}

// grid (ceil(nv / SCN_NT), bodies of the group): thread = target vertex (j, v).  phi holds the fields of bodies b0 .. .
// part[(j - b0) * gridDim.x + blockIdx.x] = the workgroup's sum of sampled values (before the division by P^2).
__global__ __launch_bounds__(SCN_NT) void scene_pair_kernel(const float* __restrict__ verts, int nv, int b0,
                                                            const SceneBody* __restrict__ tab, const float4* __restrict__ box,
                                                            const float* __restrict__ phi, int G, float rob,
                                                            float* __restrict__ g_verts, float* __restrict__ part) {
    __shared__ float sh[SCN_NT / 64];
    const int j = b0 + blockIdx.y, tid = threadIdx.x, v = blockIdx.x * SCN_NT + tid;
    const SceneBody sb = tab[j];
    const bool live = v < nv;
    float acc = 0.f, g[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float* pv = verts + ((size_t)j * nv + v) * 3;
        const float p0 = pv[0], p1 = pv[1], p2 = pv[2];
        const size_t nvox = (size_t)G * G * G;
        for (int i = sb.first; i < sb.first + sb.count; ++i) {
            if (i == j) continue;
            scene_sample_add(box[i], phi + (size_t)(i - b0) * nvox, G, rob, p0, p1, p2, acc, g);
        }
        if (g_verts) {
            const float pp = (float)(sb.count * sb.count);
            float* o = g_verts + ((size_t)j * nv + v) * 3;
            o[0] = g[0] / pp; o[1] = g[1] / pp; o[2] = g[2] / pp;
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = sh[0];
        for (int w = 1; w < SCN_NT / 64; ++w) s += sh[w];
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// The collision term of a fit against FROZEN obstacles (mvfit_set_scene_obstacles): the scene counterpart of
// sdf_entries_kernel<false>.  Grid (SDF_NC, B): a workgroup owns one vertex chunk of problem j, every wave an ascending
// run of it, a thread one trial vertex of the vertex pass's output.  The thread walks the other bodies of j's scene in
// ascending i against their frozen boxes and fields (scene_sample_add: the box test comes before any field access; most
// vertices fail it for every source) and keeps value and gradient in registers.  The workgroup writes the chunk's
// record - S in float64, wave tree then the waves in order; the frozen boxes carry no gradient, so the box-adjoint sums
// are 0 - and its entries, the vertices with a non-zero gradient in ascending order at the chunk's own offset: what
// sdf_pullback_kernel reads.  S_j = sum_{i != j} sum_v rho(sample(phi_i, v)) carries no 1 / P^2 (the stage weight absorbs
// it).  No atomics, and nothing depends on B, on j's position in the call or on the other scenes.
__global__ __launch_bounds__(SDF_ADJ_NT) void scene_entries_kernel(int nv, const float* __restrict__ verts,
                                                                   const SceneBody* __restrict__ tab,
                                                                   const float4* __restrict__ box, const float* __restrict__ phi,
                                                                   int G, float rob, const int* __restrict__ gate,
                                                                   SdfEntry* __restrict__ entries, SdfChunk* __restrict__ chunks) {
    static_assert(SDF_NIT == 1, "one 64-vertex row per wave");
    __shared__ double sh_d[SDF_ADJ_NT / 64];
    __shared__ int sh_cnt[SDF_ADJ_NT / 64];
    const int j = blockIdx.y, y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (gate && !gate[j]) return;
    const SceneBody sb = tab[j];
    const int csz = (nv + SDF_NC - 1) / SDF_NC, k0 = y * csz, k1 = min(nv, k0 + csz);
    const int wsz = (csz + 7) / 8, c0 = k0 + wave * wsz, c1 = min(k1, c0 + wsz);
    const int v = c0 + lane;
    const bool in = v < c1;
    float acc = 0.f, g[3] = {0.f, 0.f, 0.f};
    if (in) {
        const float* pv = verts + ((size_t)j * nv + v) * 3;
        const float p0 = pv[0], p1 = pv[1], p2 = pv[2];
        const size_t nvox = (size_t)G * G * G;
        for (int i = sb.first; i < sb.first + sb.count; ++i) {
            if (i == j) continue;
            scene_sample_add(box[i], phi + (size_t)i * nvox, G, rob, p0, p1, p2, acc, g);
        }
    }
    const bool act = in && ((g[0] != 0.f) | (g[1] != 0.f) | (g[2] != 0.f));
    const unsigned long long bal = __ballot(act);
    const double S = wave64_sum((double)acc);
    if (lane == 0) { sh_d[wave] = S; sh_cnt[wave] = __popcll(bal); }
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += sh_cnt[w];
    if (act) {
        SdfEntry* eb = entries + (size_t)j * nv + k0;
        const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        *reinterpret_cast<float4*>(&eb[pos]) = make_float4(__builtin_bit_cast(float, v), g[0], g[1], g[2]);
    }
    if (tid == 0) {
        SdfChunk c;
        c.S = 0.0; c.cnt = 0;
        for (int w = 0; w < SDF_ADJ_NT / 64; ++w) { c.S += sh_d[w]; c.cnt += sh_cnt[w]; }
        c.gc0 = 0.0; c.gc1 = 0.0; c.gc2 = 0.0; c.gs = 0.0; c.pad = 0;
        chunks[(size_t)j * SDF_NC + y] = c;
    }
}

// grid (scenes of the group), one wave: the scene's partials in ascending (body, workgroup) order - lane l takes every
// 64th, then the shuffle tree - in float64, divided by P^2.  s0: first scene of the group, b0: its first body.
__global__ __launch_bounds__(64) void scene_loss_kernel(const float* __restrict__ part, int nblk, const int32_t* __restrict__ first,
                                                        int s0, int b0, float* __restrict__ loss) {
    const int s = s0 + blockIdx.x, lane = threadIdx.x;
    const int f = first[s], P = first[s + 1] - f;
    const float* p = part + (size_t)(f - b0) * nblk;
    const int n = P * nblk;
    double a = 0.0;
    for (int k = lane; k < n; k += 64) a += (double)p[k];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) loss[s] = (float)(a / (double)(P * P));
}

int scene_sdf_blocks(int nv) { return (nv + SCN_NT - 1) / SCN_NT; }

hipError_t launch_scene_boxes(const float* verts, int nv, int b0, int n, float factor, float4* box, float* local,
                              hipStream_t stream) {
    hipLaunchKernelGGL(scene_box_kernel, dim3(n), dim3(SCN_NT), 0, stream, verts, nv, b0, factor, box, local);
    return hipGetLastError();
}

// tab: [N] rows of SceneBody; first: the call's scene_first on the device
hipError_t launch_scene_pairs(const float* verts, int nv, int b0, int n, int s0, int ns, const void* tab, const int32_t* first,
                              const float4* box, const float* phi, int G, float rob, float* g_verts, float* part, float* loss,
                              hipStream_t stream) {
    const int nblk = scene_sdf_blocks(nv);
    hipLaunchKernelGGL(scene_pair_kernel, dim3(nblk, n), dim3(SCN_NT), 0, stream, verts, nv, b0,
                       reinterpret_cast<const SceneBody*>(tab), box, phi, G, rob, g_verts, part);
    hipLaunchKernelGGL(scene_loss_kernel, dim3(ns), dim3(64), 0, stream, (const float*)part, nblk, first, s0, b0, loss);
    return hipGetLastError();
}

// one box per problem for the pull-back of the scene term: no vertex matches its box-adjoint branch
__global__ void scene_null_box_kernel(SdfBox* __restrict__ box, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    SdfBox x;
    for (int a = 0; a < 3; ++a) { x.c[a] = 0.f; x.imin[a] = -1; x.imax[a] = -1; }
    x.s = 1.f; x.amax = 0; x.pad = 0;
    box[b] = x;
}

hipError_t launch_scene_null_boxes(SdfBox* box, int B, hipStream_t stream) {
    hipLaunchKernelGGL(scene_null_box_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, box, B);
    return hipGetLastError();
}

// The scene term of one closure round for all B problems of the ctx: entries against the frozen obstacles (tab, box, phi:
// [B] rows / [B] boxes / [B] fields by problem index), then the pull-back of sdf_term.hip into adj.  null_box: [B] boxes
// of launch_scene_null_boxes; entries: the work area of sdf_work_bytes(B, nv) bytes.
hipError_t launch_scene_term(const DevModel& M, const DevPose& P, const float* verts, int B, const void* tab, const float4* box,
                             const float* phi, int G, float rob, const int* gate, const SdfBox* null_box, void* entries,
                             SdfAdj* adj, hipStream_t stream) {
    if (M.nv > SDF_NC * 8 * SDF_NIT * 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_entries_kernel, dim3(SDF_NC, B), dim3(SDF_ADJ_NT), 0, stream, M.nv, verts,
                       reinterpret_cast<const SceneBody*>(tab), box, phi, G, rob, gate, reinterpret_cast<SdfEntry*>(entries),
                       sdf_work_chunks(entries, B, M.nv));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sdf_pullback(M, P, B, B, gate, null_box, entries, adj, stream);
}

}  // namespace mvfit
