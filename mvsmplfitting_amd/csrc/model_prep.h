// Host preparation of the model constants the kernels read (plain C++17, no HIP): prepare_model turns an mvfit_model into
// every table of DevModel and the ModelLds image, in host memory; mvfit_create_ex uploads them.  The layouts are
// documented here, once.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mvfit.h"
#include "model_layout.h"

namespace mvfit {

struct HostModel {
    int nv = 0, ntiles = 0, nv_pad = 0;  // vertices, MFMA tiles of TILE_V, ntiles * TILE_V
    // ---- blendshape basis: row p of vertex v, coordinate k (basis_value in model_prep.cpp) ----
    // bs4: [ntiles][3][KGROUPS][64 lanes][4] MFMA-B-operand order, element (T, k, g, l, q) = row 2 (4 g + q) + (l >> 5),
    // vertex 32 T + (l & 31), zero past the model
    std::vector<float> bs4;
    // bs_h2: the same basis split into fp16 pairs for the fp16 matrix pipe, scaled by bs_scale (the power of two that brings
    // max |x| into [2^13, 2^14)): [ntiles][3][14 blocks][hi, lo][64 lanes][8] = 8 fp16 of rows 16 G + 8 (lane >> 5) + t,
    // vertex 32 T + (lane & 31), x * bs_scale = hi + lo.  Empty for MVFIT_CONTRACTION_EXACT_FP32.
    std::vector<_Float16> bs_h2;
    float bs_scale = 1.f;
    int half_basis = 0;                  // MVFIT_CONTRACTION_HALF_BASIS: the contraction reads only the hi halves
    std::vector<float> bs_vm;            // [nv][3][KROWS] vertex-major, the coefficient vector's row order (SDF pull-back)
    // ---- rest pose and skinning ----
    std::vector<float> vt_planes;        // [3][nv_pad] v_template by coordinate
    std::vector<float> wt_tiles;         // [ntiles][NJ][32] lbs_weights per tile
    std::vector<float> w_vm;             // [nv][NJ] lbs_weights as given
    // sparse skinning: per padded vertex 4 weights and their joint indices, non-zeros in ascending joint order, zero-padded.
    // Empty when a vertex has more than 4 non-zero weights or dense_skinning is set.
    std::vector<float> wsp_w;            // [nv_pad][4]
    std::vector<int32_t> wsp_j;          // [nv_pad][4]
    // ---- the vertices the objective reads (non-zero columns of the 17 x nv keypoint selection, ascending) ----
    int ns = 0, nc = 0, nc_pad = 0;      // nc = 3 ns, nc_pad = nc rounded up to a multiple of 4
    std::vector<int32_t> sel_v;          // [ns]
    std::vector<float> pd_sub;           // [KROWS][nc_pad] basis rows of the selected coordinates c = 3 s + a
    std::vector<float> pd_subT;          // [nc_pad][KROWS]
    // vertex-pass side outputs: tile T's selected vertices are entries tile_sel_start[T] .. [T + 1] (ascending s)
    std::vector<int32_t> tile_sel_start; // [ntiles + 1]
    std::vector<int32_t> tile_sel_local; // [max(ns, 1)] vertex index inside its tile
    std::vector<int32_t> tile_sel_slot;  // [max(ns, 1)] selected-vertex slot s
    // ---- the LDS image of the per-problem kernels (model_layout.h) ----
    ModelLds lds;
    // E6's lane cells [NJ][16 lanes][E6_NZ]: the non-zero entries of wT[j][s], s = g, g + 16, ... in ascending s, each as
    // 4 s + t (the word of lds.selw that holds the weight), padded with E6_INVALID.  Uploaded behind the LDS image; used
    // when lds.e6_cells is 1 (no cell longer than E6_NZ, lds.sel_sparse set)
    std::vector<uint16_t> e6_cells;
    // ---- VPoser decoder (empty when the model has none) ----
    bool has_vposer = false;
    std::vector<float> vp_w1, vp_b1, vp_w2, vp_b2, vp_w3, vp_b3;   // [512][32], [512], [512][512], [512], [138][512], [138]
    std::vector<float> vp_w1T, vp_w2T, vp_w3T;                     // [32][512], [512][512], [512][144] (columns >= 138 zero)
    // register tiles of the decoder helpers (vposer_service.h: VpTiles), float4 words, thread-minor:
    //   vp_tw2[h][j = 2a + half][tid] = W2[64h + 8w + a][8l + 4 half .. + 3]                [VPS_SLICES][16][512][4]
    //   vp_tw3[h][j = 2r + half][tid] = W3[l + 64r][64h + 8w + 4 half .. + 3], zero rows for o >= 138   [VPS_SLICES][6][512][4]
    // (w = tid >> 6, l = tid & 63)
    std::vector<float> vp_tw2, vp_tw3;
    // ---- max-mixture prior (gmm_M = 0: none) ----
    int gmm_M = 0;
    std::vector<float> gmm_means;        // [M][69]
    std::vector<float> gmm_prec;         // [M][69][72] rows padded to 72 floats (16-byte aligned)
    std::vector<float> gmm_precT;        // [M][69][72] transposed precisions
    std::vector<float> gmm_lognw;        // [M] logf(nll_weights)
    // ---- faces of the renderer and the vertex -> face CSR its normals gather through (ascending face id per vertex);
    // empty when the model has no faces or one of them indexes outside the vertices ----
    int num_faces = 0;
    std::vector<int32_t> faces;          // [num_faces][3]
    std::vector<int32_t> vf_ptr;         // [nv + 1]
    std::vector<int32_t> vf_idx;         // [3 num_faces]
};

// Checks the model's arguments and builds every table.  Returns MVFIT_OK, or an MVFIT_E_* code with the message in err.
// contraction: mvfit_options::contraction; dense_skinning: mvfit_options::dense_skinning.
int prepare_model(const mvfit_model& m, int contraction, int dense_skinning, HostModel& out, std::string& err);

}  // namespace mvfit
