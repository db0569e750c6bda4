// Host interface of the silhouette term (silhouette.hip) as mvfit_scene.hip drives it: the mask set a ctx keeps between
// mvfit_set_silhouettes and the loss calls.  Every function returns an MVFIT_* code and, on failure, a message in err.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "dev_mem.h"

namespace mvfit {

struct SilState {
    bool on = false;
    int M = 0, H = 0, W = 0, stride = 1, nv = 0;
    int C = 0;                          // kept contour points of all images
    int nchunks = 0;                    // workgroups of the search kernel
    int body_min = 0, body_max = -1;    // range of image_body (checked against num_bodies at loss time)
    // device memory sized by (M, H, W, nv): fields, mask copy, row offsets, tables, fixed-point accumulators, term A partials
    DevBuf ws;
    size_t o_field = 0, o_mask = 0, o_row = 0, o_flags = 0, o_total = 0, o_cam = 0, o_body = 0, o_sbody = 0, o_simg = 0,
           o_first = 0, o_cfirst = 0, o_acc = 0, o_partA = 0;
    // device memory sized by the contour: points, chunk table, term B partials; grows to the largest set seen
    DevBuf cs;
    size_t o_xy = 0, o_chunk = 0, o_partB = 0;
    std::vector<int32_t> h_tab;         // host staging of the tables (kept while a copy may read it)
    std::vector<int32_t> h_body;        // image_body on the host (the occluder freeze builds its instance list from it)
    // occluder depth maps of mvfit_set_silhouette_occluders (silhouette_occlusion.hip): they belong to the mask set.
    // occ: z_occ [M][H][W] and z_own [M][H][W] (fp32 bits, +inf = nothing) and one flag byte per kept contour point; the
    // buffer only grows, so a re-freeze at unchanged (M, H, W, C) keeps its address.  occ_ws: the raster's instance table
    // and records of one group of instances, grown like the renderer's workspace.
    bool occ_on = false;
    float occ_margin = 0.f;
    DevBuf occ, occ_ws;
    size_t o_zocc = 0, o_zown = 0, o_pflag = 0;
    std::vector<int32_t> h_inst;        // host staging of the instance table
};

int sil_set(SilState& S, int nv, int M, int H, int W, const uint8_t* masks, const int32_t* image_body, const float* cam_R,
            const float* cam_t, const float* cam_f, const float* cam_c, int stride, hipStream_t stream, std::string& err);
int sil_read(const SilState& S, float* field, int32_t* contour_first, int32_t* contour_xy, hipStream_t stream, std::string& err);
int sil_loss(SilState& S, const float* vertices, int num_bodies, float w_in, float w_out, float sigma, float* loss,
             float* g_vertices, int32_t* winner, hipStream_t stream, std::string& err);
// the same evaluation for the fit's chained rounds (mvfit_set_silhouette_term): gate[body] == 0 skips the body (its loss and
// gradient rows keep what they held), null = every body; capturable
int sil_round(SilState& S, const float* vertices, int num_bodies, float w_in, float w_out, float sigma, const int* gate,
              float* loss, float* g_vertices, hipStream_t stream, std::string& err);


// Freeze the occluders of every image at vertices[num_bodies][nv][3] (dev): image i of body n = image_body[i] is occluded by
// the bodies m != n with body_scene[m] == body_scene[n] >= 0.  faces [nf][3] dev: the model's.  Arguments are checked by the
// caller (mvfit_scene.hip).  A failure leaves no occluders set.
int sil_occ_set(SilState& S, const float* vertices, int num_bodies, const int32_t* body_scene, float margin, const int32_t* faces,
                int nf, hipStream_t stream, std::string& err);
// z_occ / z_own [M][H][W] float32 and point_flag [C] uint8, dev out or null
int sil_occ_read(const SilState& S, float* z_occ, float* z_own, uint8_t* point_flag, hipStream_t stream, std::string& err);
// hidden [M][nv] uint8 dev out: 1 where vertex j of body image_body[i] is valid and hidden in image i; zeros without occluders
int sil_occ_hidden(const SilState& S, const float* vertices, uint8_t* hidden, hipStream_t stream, std::string& err);

}  // namespace mvfit
