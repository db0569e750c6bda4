// The rasteriser's coverage and depth rules as device functions (include/mvfit.h: mvfit_render_overlay, "coverage" and
// "depth"), shared by the renderer (render.hip) and the silhouette term's occluder depth maps (silhouette_occlusion.hip):
// one statement of the rules, so both draw the same samples at the same fp32 depths.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace mvfit {

constexpr float RD_ZNEAR = 0.05f, RD_ZFAR = 8000.f;
constexpr float RD_GUARD = 16384.f;                // a vertex further than this outside the image drops its triangle
constexpr long long RD_BIG_BOX = 1024;             // pixel boxes larger than this are walked by a whole workgroup
constexpr int RD_BIG_BLOCKS = 256;                 // workgroups per image of the large-face kernels

struct RenderVert {            // per (image, vertex)
    int X, Y;                  // rintf(u * 256), rintf(v * 256)
    float pz;
    int ok;                    // pz > znear and inside the guard band
};

// the record of a vertex projected to (u, w) at depth pz in an H x W image
__device__ __forceinline__ RenderVert snap_vertex(float u, float w, float pz, int H, int W) {
    RenderVert rv;
    rv.ok = (pz > RD_ZNEAR) && (u >= -RD_GUARD) && (u <= (float)W + RD_GUARD) && (w >= -RD_GUARD) && (w <= (float)H + RD_GUARD);
    rv.X = rv.ok ? (int)rintf(u * 256.f) : 0;
    rv.Y = rv.ok ? (int)rintf(w * 256.f) : 0;
    rv.pz = pz;
    return rv;
}

__device__ inline long long edge_fn(int xa, int ya, int xb, int yb, long long sx, long long sy) {
    return (long long)(xb - xa) * (sy - ya) - (long long)(yb - ya) * (sx - xa);
}

struct FaceSetup {             // a face's snapped vertices, orientation, pixel box and 1/z
    RenderVert v0, v1, v2;
    long long sgn, area;
    int x0, x1, y0, y1;
    double iz0, iz1, iz2;
};

// false: the face draws nothing (a vertex dropped, zero area, or its box misses the image)
__device__ inline bool face_setup(const RenderVert* V, const int32_t* faces, int f, int H, int W, FaceSetup& s) {
    s.v0 = V[faces[f * 3 + 0]]; s.v1 = V[faces[f * 3 + 1]]; s.v2 = V[faces[f * 3 + 2]];
    if (!(s.v0.ok && s.v1.ok && s.v2.ok)) return false;
    const long long area = edge_fn(s.v0.X, s.v0.Y, s.v1.X, s.v1.Y, s.v2.X, s.v2.Y);
    if (area == 0) return false;
    s.sgn = area > 0 ? 1 : -1;
    s.area = area * s.sgn;
    const int minX = min(s.v0.X, min(s.v1.X, s.v2.X)), maxX = max(s.v0.X, max(s.v1.X, s.v2.X));
    const int minY = min(s.v0.Y, min(s.v1.Y, s.v2.Y)), maxY = max(s.v0.Y, max(s.v1.Y, s.v2.Y));
    // pixel x is sampled at 256 x + 128: the columns whose centre lies in [minX, maxX] (arithmetic shifts = floor division)
    s.x0 = max(0, (minX - 128 + 255) >> 8); s.x1 = min(W - 1, (maxX - 128) >> 8);
    s.y0 = max(0, (minY - 128 + 255) >> 8); s.y1 = min(H - 1, (maxY - 128) >> 8);
    if (s.x0 > s.x1 || s.y0 > s.y1) return false;
    s.iz0 = 1.0 / (double)s.v0.pz; s.iz1 = 1.0 / (double)s.v1.pz; s.iz2 = 1.0 / (double)s.v2.pz;
    return true;
}

// one sample: e0 = edge v1->v2 (opposite v0), e1 = v2->v0, e2 = v0->v1, already oriented.  True when the sample is covered
// and its depth z lies inside [znear, zfar].
__device__ inline bool raster_depth(const FaceSetup& s, long long e0, long long e1, long long e2, float& z) {
    if ((e0 | e1 | e2) < 0) return false;
    const double w = ((double)e0 * s.iz0 + (double)e1 * s.iz1) + (double)e2 * s.iz2;
    z = (float)((double)s.area / w);
    return z >= RD_ZNEAR && z <= RD_ZFAR;
}

}  // namespace mvfit
