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

}  // namespace mvfit
