// Device side of the silhouette term that its two kernel files share (silhouette.hip: preparation and evaluation;
// silhouette_occlusion.hip: occluder depth maps, point flags, hidden bytes): the table rows, the projection and the
// hidden-vertex test of include/mvfit.h:mvfit_set_silhouette_occluders.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace mvfit {

constexpr int SIL_NT = 256;
constexpr float SIL_ZNEAR = 0.05f;

struct SilCam { float R[9], t[3], f, cx, cy, pad; };
static_assert(sizeof(SilCam) == 64, "table row");
struct SilChunk { int image, first, count, pad; };
static_assert(sizeof(SilChunk) == 16, "table row");

// the rasteriser's fp32 sequence (render.hip: cam_point), no contraction
__device__ __forceinline__ bool sil_project(const SilCam& c, const float* __restrict__ p, float& px, float& py, float& pz,
                                            float& u, float& w) {
    const float X = p[0], Y = p[1], Z = p[2];
    px = ((c.R[0] * X + c.R[1] * Y) + c.R[2] * Z) + c.t[0];
    py = ((c.R[3] * X + c.R[4] * Y) + c.R[5] * Z) + c.t[1];
    pz = ((c.R[6] * X + c.R[7] * Y) + c.R[8] * Z) + c.t[2];
    u = c.f * (px / pz) + c.cx;
    w = c.f * (py / pz) + c.cy;
    return pz > SIL_ZNEAR;
}

// a valid vertex projected to (u, w) at depth pz is hidden by the occluder map z_occ [H][W] of its image: inside the image
// (fp32 compares) and behind the map's depth at its pixel by more than margin (one rounded fp32 add)
__device__ __forceinline__ bool sil_hidden(const float* __restrict__ z_occ, int H, int W, float margin, float u, float w, float pz) {
    if (!(u >= 0.f && u < (float)W && w >= 0.f && w < (float)H)) return false;
    return z_occ[(size_t)(int)w * W + (int)u] + margin < pz;
}

// The occluders of the evaluation kernels (sil_loss / sil_round choose the instantiation from the mask set's state).  The
// instantiations without occluders carry an empty argument and are the kernels as they were.
template <bool OCC> struct SilOcc {
    __device__ __forceinline__ bool hidden(int, float, float, float) const { return false; }
    __device__ __forceinline__ bool flagged(size_t) const { return false; }
};
template <> struct SilOcc<true> {
    const float* z_occ;          // [M][H][W]
    const uint8_t* pflag;        // [C]
    int H, W;
    float margin;
    __device__ __forceinline__ bool hidden(int image, float u, float w, float pz) const {
        return sil_hidden(z_occ + (size_t)image * H * W, H, W, margin, u, w, pz);
    }
    __device__ __forceinline__ bool flagged(size_t point) const { return pflag[point] != 0; }
};

}  // namespace mvfit
