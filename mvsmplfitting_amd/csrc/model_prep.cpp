// Host preparation of the model constants (model_prep.h): plain C++17, no HIP.  Linked into libmvfit.so and, for
// tests/test_model_prep_cpu.py, into a host-only test library.
#include "model_prep.h"

#include <math.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace mvfit {
namespace {

constexpr int NPOSE = 207;    // blendshape rows 0..206: posedirs
constexpr int NBASIS = 217;   // rows 207..216: shapedirs (beta index); rows up to KROWS are zero

int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// blendshape row p of vertex v, coordinate k
inline float basis_value(const mvfit_model& m, int p, int v, int k) {
    if (p < NPOSE) return m.posedirs[(size_t)p * m.num_verts * 3 + 3 * v + k];
    if (p < NBASIS) return m.shapedirs[((size_t)v * 3 + k) * 10 + (p - NPOSE)];
    return 0.f;
}

// bs4, its split-fp16 form and scale, the vertex-major copy
void build_basis(const mvfit_model& m, int contraction, HostModel& h) {
    const int nv = h.nv;
    h.bs4.assign((size_t)h.ntiles * 3 * KGROUPS * 64 * 4, 0.f);
    for (int T = 0; T < h.ntiles; ++T)
        for (int k = 0; k < 3; ++k)
            for (int g = 0; g < KGROUPS; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int q = 0; q < 4; ++q) {
                        const int v = TILE_V * T + (l & 31);
                        if (v < nv) h.bs4[((((size_t)T * 3 + k) * KGROUPS + g) * 64 + l) * 4 + q] = basis_value(m, 2 * (4 * g + q) + (l >> 5), v, k);
                    }
    // MVFIT_CONTRACTION_HALF_BASIS (BASELINE configs[4]: half-width blendshape operands): the contraction streams only the
    // fp16 hi halves of the basis - 2 bytes per element like bf16, with 11 instead of 8 significant bits
    h.half_basis = contraction == MVFIT_CONTRACTION_HALF_BASIS ? 1 : 0;
    if (contraction != MVFIT_CONTRACTION_EXACT_FP32) {
        float mx = 0.f;
        for (float x : h.bs4) mx = std::max(mx, std::fabs(x));
        int ex = 0;
        if (mx > 0.f) std::frexp(mx, &ex);                 // mx = f * 2^ex, f in [0.5, 1)
        const float scale = std::ldexp(1.f, 14 - ex);       // max |x| * scale in [2^13, 2^14)
        constexpr int NB = KROWS / 16;
        h.bs_h2.resize((size_t)h.ntiles * 3 * NB * 2 * 64 * 8);
        for (int T = 0; T < h.ntiles; ++T)
            for (int k = 0; k < 3; ++k)
                for (int G16 = 0; G16 < NB; ++G16)
                    for (int l = 0; l < 64; ++l)
                        for (int t = 0; t < 8; ++t) {
                            const int v = TILE_V * T + (l & 31);
                            const float val = (v < nv ? basis_value(m, 16 * G16 + 8 * (l >> 5) + t, v, k) : 0.f) * scale;
                            const _Float16 hi = (_Float16)val;
                            const _Float16 lo = (_Float16)(val - (float)hi);
                            const size_t at = ((((size_t)(T * 3 + k) * NB + G16) * 2) * 64 + l) * 8 + t;
                            h.bs_h2[at] = hi;
                            h.bs_h2[at + 64 * 8] = lo;
                        }
        h.bs_scale = scale;
    }
    h.bs_vm.assign((size_t)nv * 3 * KROWS, 0.f);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k)
            for (int p = 0; p < NBASIS; ++p) h.bs_vm[((size_t)v * 3 + k) * KROWS + p] = basis_value(m, p, v, k);
}

// v_template planes, skinning weights per tile and vertex-major, the sparse skinning table when the model allows it
// (SMPL-family weights have <= 4 non-zeros per vertex; dense_skinning keeps the dense blend: tests compare the two bit for bit)
void build_skinning(const mvfit_model& m, int dense_skinning, HostModel& h) {
    const int nv = h.nv;
    h.vt_planes.assign((size_t)3 * h.nv_pad, 0.f);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k) h.vt_planes[(size_t)k * h.nv_pad + v] = m.v_template[3 * v + k];
    h.wt_tiles.assign((size_t)h.ntiles * NJ * 32, 0.f);
    for (int v = 0; v < nv; ++v)
        for (int j = 0; j < NJ; ++j) h.wt_tiles[((size_t)(v / 32) * NJ + j) * 32 + (v % 32)] = m.lbs_weights[(size_t)v * NJ + j];
    h.w_vm.assign(m.lbs_weights, m.lbs_weights + (size_t)nv * NJ);
    bool sparse_ok = !dense_skinning;
    for (int v = 0; v < nv && sparse_ok; ++v) {
        int nz = 0;
        for (int j = 0; j < NJ; ++j) nz += m.lbs_weights[(size_t)v * NJ + j] != 0.f;
        sparse_ok = nz <= 4;
    }
    if (!sparse_ok) return;
    h.wsp_w.assign((size_t)h.nv_pad * 4, 0.f);
    h.wsp_j.assign((size_t)h.nv_pad * 4, 0);
    for (int v = 0; v < nv; ++v) {
        int t = 0;
        for (int j = 0; j < NJ; ++j) {
            const float w = m.lbs_weights[(size_t)v * NJ + j];
            if (w != 0.f) { h.wsp_w[(size_t)v * 4 + t] = w; h.wsp_j[(size_t)v * 4 + t] = j; ++t; }
        }
    }
}

// joints as an affine function of beta (float64 accumulation over the regressor's non-zeros, ascending vertex)
void build_joint_affine(const mvfit_model& m, ModelLds& G) {
    const int nv = m.num_verts;
    for (int j = 0; j < NJ; ++j)
        for (int a = 0; a < 3; ++a) {
            double s = 0.0, sl[10] = {0};
            for (int v = 0; v < nv; ++v) {
                const double w = m.J_regressor[(size_t)j * nv + v];
                if (w == 0.0) continue;
                s += w * m.v_template[3 * v + a];
                for (int l = 0; l < 10; ++l) sl[l] += w * m.shapedirs[((size_t)v * 3 + a) * 10 + l];
            }
            G.J_t[j * 3 + a] = (float)s;
            for (int l = 0; l < 10; ++l) G.J_S[j * 3 + a][l] = (float)sl[l];
        }
}

// The vertices the objective reads: non-zero columns of the mapped 17 x nv selection.  joint_map indexes the model's joint
// tensor (include/mvfit.h): with a keypoint regressor 14 regressor rows + 5 face vertices ('smpllsp'), without one 24 posed
// skeleton joints + 5 face vertices ('smpl') - a skeleton keypoint has an empty selection row and its joint in kp_joint
// (closure_device.h: keypoints_from_xs, E6).  Also: their basis rows, weights, the selection in CSR form both ways and as
// padded lists, and the per-tile lists of the vertex pass's side outputs.
int build_selection(const mvfit_model& m, HostModel& h, std::string& err) {
    const int nv = h.nv;
    ModelLds& G = h.lds;
    const bool skel = m.kp_regressor == nullptr;
    const int n_rows = skel ? NJ : 14;                        // joints before the five face vertices
    for (int w = 0; w < 3; ++w) G.kp_joint[w] = 0x3fffffffu;  // 31 = vertex row, six per word
    G.n_skel = 0;
    std::vector<double> ksel((size_t)NKP * nv, 0.0);
    for (int k = 0; k < NKP; ++k) {
        const int src = m.joint_map[k];
        if (src < 0 || src >= n_rows + 5) return fail(err, MVFIT_E_ARG, "joint_map entry %d out of range (0..%d)", src, n_rows + 4);
        if (src < n_rows) {
            if (skel) {
                G.kp_joint[k / 6] &= ~(31u << (5 * (k % 6)));
                G.kp_joint[k / 6] |= (unsigned)src << (5 * (k % 6));
                ++G.n_skel;
            } else {
                for (int v = 0; v < nv; ++v) ksel[(size_t)k * nv + v] = m.kp_regressor[(size_t)src * nv + v];
            }
        } else {
            const int v = m.face_vertex_ids[src - n_rows];
            if (v < 0 || v >= nv) return fail(err, MVFIT_E_ARG, "face vertex id out of range");
            ksel[(size_t)k * nv + v] = 1.0;
        }
    }
    std::vector<int32_t>& sel = h.sel_v;
    for (int v = 0; v < nv; ++v) {
        bool nz = false;
        for (int k = 0; k < NKP; ++k) nz |= ksel[(size_t)k * nv + v] != 0.0;
        if (nz) sel.push_back(v);
    }
    if (sel.empty()) return fail(err, MVFIT_E_UNSUPPORTED, "the keypoints read no vertex (joint_map names no face vertex)");
    if ((int)sel.size() > NS_MAX) return fail(err, MVFIT_E_UNSUPPORTED, "keypoint regressor touches %d vertices (max %d)", (int)sel.size(), NS_MAX);
    const int ns = (int)sel.size();
    h.ns = G.ns = ns;
    h.nc = G.nc = 3 * ns;
    h.nc_pad = G.nc_pad = (3 * ns + 3) & ~3;
    h.pd_sub.assign((size_t)KROWS * h.nc_pad, 0.f);
    h.pd_subT.assign((size_t)h.nc_pad * KROWS, 0.f);
    int sel_sparse = 1;
    for (int s = 0; s < ns; ++s) {
        const int v = sel[s];
        G.sel_v[s] = v;
        for (int a = 0; a < 3; ++a) {
            const int cidx = 3 * s + a;
            G.vt_sub[cidx] = m.v_template[3 * v + a];
            for (int p = 0; p < NBASIS; ++p) {
                const float val = basis_value(m, p, v, a);
                h.pd_sub[(size_t)p * h.nc_pad + cidx] = val;
                h.pd_subT[(size_t)cidx * KROWS + p] = val;
            }
        }
        for (int j = 0; j < NJ; ++j) G.wT[j][s] = m.lbs_weights[(size_t)v * NJ + j];
        int np = 0;
        for (int j = 0; j < NJ; ++j) {
            const float w = m.lbs_weights[(size_t)v * NJ + j];
            if (w == 0.f) continue;
            if (np < 4) { G.selw[s][np] = w; G.selj[s] |= (unsigned)j << (8 * np); }
            ++np;
        }
        if (np > 4) sel_sparse = 0;
    }
    G.sel_sparse = sel_sparse;
    // E6's lane cells: lane g of joint j's 16-lane row adds the vertices s = g, g + 16, ... - their non-zero weights in that
    // order, each as the word of selw that holds it; a cell with more than E6_NZ of them (or a dense model) keeps the dense row
    h.e6_cells.assign((size_t)NJ * 16 * E6_NZ, (uint16_t)E6_INVALID);
    G.e6_cells = sel_sparse;
    for (int j = 0; j < NJ && sel_sparse; ++j)
        for (int g = 0; g < 16; ++g) {
            int n = 0;
            for (int s = g; s < ns; s += 16) {
                if (G.wT[j][s] == 0.f) continue;
                int t = 0;
                while (t < 3 && (((G.selj[s] >> (8 * t)) & 0xffu) != (unsigned)j || G.selw[s][t] == 0.f)) ++t;   // (byte 0 also names padding)
                if (n < E6_NZ) h.e6_cells[((size_t)j * 16 + g) * E6_NZ + n] = (uint16_t)(4 * s + t);
                ++n;
            }
            if (n > E6_NZ) G.e6_cells = 0;
        }
    // selection in CSR form, both ways
    int nnz = 0;
    for (int k = 0; k < NKP; ++k) {
        G.kp_start[k] = nnz;
        for (int s = 0; s < ns; ++s) {
            const double w = ksel[(size_t)k * nv + sel[s]];
            if (w == 0.0) continue;
            if (nnz >= KNNZ_MAX) return fail(err, MVFIT_E_UNSUPPORTED, "keypoint selection has more than %d non-zeros", KNNZ_MAX);
            G.kp_s[nnz] = s; G.kp_w[nnz] = (float)w; ++nnz;
        }
    }
    G.kp_start[NKP] = nnz;
    nnz = 0;
    for (int s = 0; s < ns; ++s) {
        G.vs_start[s] = nnz;
        for (int k = 0; k < NKP; ++k) {
            const double w = ksel[(size_t)k * nv + sel[s]];
            if (w == 0.0) continue;
            G.vs_k[nnz] = k; G.vs_w[nnz] = (float)w; ++nnz;
        }
    }
    for (int s = ns; s <= NS_MAX; ++s) G.vs_start[s] = nnz;
    // fixed-length zero-padded copies (entry 0 / weight 0 pads: fmaf(0, x, acc) == acc)
    G.padded = 1;
    for (int k = 0; k < NKP; ++k) {
        const int n0 = G.kp_start[k], cnt = G.kp_start[k + 1] - n0;
        if (cnt > KP_NZ) G.padded = 0;
        for (int t = 0; t < KP_NZ; ++t) { G.kpp_s[k][t] = t < cnt ? G.kp_s[n0 + t] : 0; G.kpp_w[k][t] = t < cnt ? G.kp_w[n0 + t] : 0.f; }
    }
    for (int s = 0; s < NS_MAX; ++s) {
        const int n0 = G.vs_start[s], cnt = G.vs_start[s + 1] - n0;
        if (cnt > VS_NZ) G.padded = 0;
        for (int t = 0; t < VS_NZ; ++t) { G.vsp_k[s][t] = t < cnt ? G.vs_k[n0 + t] : 0; G.vsp_w[s][t] = t < cnt ? G.vs_w[n0 + t] : 0.f; }
    }
    // per-tile lists for the vertex pass side outputs
    h.tile_sel_start.assign(h.ntiles + 1, 0);
    h.tile_sel_local.assign(ns, 0);
    h.tile_sel_slot.assign(ns, 0);
    int pos = 0;
    for (int T = 0; T < h.ntiles; ++T) {
        h.tile_sel_start[T] = pos;
        for (int s = 0; s < ns; ++s)
            if (sel[s] / TILE_V == T) { h.tile_sel_local[pos] = sel[s] % TILE_V; h.tile_sel_slot[pos] = s; ++pos; }
    }
    h.tile_sel_start[h.ntiles] = pos;
    return MVFIT_OK;
}

// kinematic tree: levels, child lists and the chain schedules of ModelLds
int build_chain(const mvfit_model& m, ModelLds& G, std::string& err) {
    int depth[NJ];
    for (int j = 0; j < NJ; ++j) {
        G.parents[j] = m.parents[j];
        if (j > 0 && (m.parents[j] < 0 || m.parents[j] >= j)) return fail(err, MVFIT_E_ARG, "parents must be topologically ordered");
        depth[j] = j == 0 ? 0 : depth[m.parents[j]] + 1;
    }
    int maxd = 0;
    for (int j = 0; j < NJ; ++j) maxd = std::max(maxd, depth[j]);
    G.nlevels = maxd + 1;
    int pos = 0;
    for (int lv = 0; lv <= maxd; ++lv) {
        G.level_start[lv] = pos;
        for (int j = 0; j < NJ; ++j) if (depth[j] == lv) G.level_joints[pos++] = j;
    }
    for (int lv = maxd + 1; lv <= NJ; ++lv) G.level_start[lv] = pos;
    pos = 0;
    for (int p = 0; p < NJ; ++p) {
        G.child_start[p] = pos;
        for (int j = 1; j < NJ; ++j) if (m.parents[j] == p) G.child_list[pos++] = j;
    }
    G.child_start[NJ] = pos;
    // forward schedule: each level in groups of 5 joints (one wave = 5 x 12 lanes)
    memset(G.fwd_tab, 0xff, sizeof(G.fwd_tab));
    memset(G.bwd_tab, 0xff, sizeof(G.bwd_tab));
    int np = 0;
    for (int lv = 1; lv <= maxd; ++lv)
        for (int base = G.level_start[lv]; base < G.level_start[lv + 1]; base += 5, ++np) {
            if (np >= NJ) return fail(err, MVFIT_E_UNSUPPORTED, "kinematic tree needs more than %d chain passes", NJ);
            for (int q = 0; q < 5 && base + q < G.level_start[lv + 1]; ++q) {
                const int j = G.level_joints[base + q];
                G.fwd_tab[np][q] = j | (m.parents[j] << 8);
            }
        }
    G.n_fwd = np;
    // pointer-jumping tables (chain_forward_block)
    for (int j = 0; j < NJ; ++j) G.anc_tab[0][j] = m.parents[j];
    for (int st = 1; st < 5; ++st)
        for (int j = 0; j < NJ; ++j) {
            const int a = G.anc_tab[st - 1][j];
            G.anc_tab[st][j] = a < 0 ? -1 : G.anc_tab[st - 1][a];
        }
    int nj = 0;
    while ((1 << nj) < maxd + 1) ++nj;
    if (nj > 5) return fail(err, MVFIT_E_UNSUPPORTED, "kinematic tree deeper than 32 joints");
    G.n_jump = nj;
    // backward schedule: parents with children, deepest level first; <= 3 children per entry
    // (a parent with more children appears in consecutive passes), <= 5 entries per pass.
    // Two entries of the same parent never share a pass (they would race on its row).
    np = 0;
    for (int lv = maxd - 1; lv >= 0; --lv) {
        std::vector<int> entries;     // packed words of this level
        for (int i = G.level_start[lv]; i < G.level_start[lv + 1]; ++i) {
            const int p = G.level_joints[i];
            const int nc = G.child_start[p + 1] - G.child_start[p];
            for (int k = 0; k < nc; k += 3) {
                int ch[3] = {31, 31, 31};
                for (int t = 0; t < 3 && k + t < nc; ++t) ch[t] = G.child_list[G.child_start[p] + k + t];
                entries.push_back(p | (k > 0 ? 0x80 : 0) | (ch[0] << 8) | (ch[1] << 16) | (ch[2] << 24));
            }
        }
        // greedy packing into passes: at most 5 entries, no repeated parent inside a pass
        std::vector<bool> used(entries.size(), false);
        size_t left = entries.size();
        while (left > 0) {
            if (np >= NJ) return fail(err, MVFIT_E_UNSUPPORTED, "kinematic tree needs more than %d adjoint passes", NJ);
            int q = 0;
            std::vector<int> parents_in_pass;
            for (size_t i = 0; i < entries.size() && q < 5; ++i) {
                if (used[i]) continue;
                const int p = entries[i] & 0x1f;
                bool clash = false;
                for (int pp : parents_in_pass) clash |= pp == p;
                if (clash) continue;
                G.bwd_tab[np][q++] = entries[i];
                parents_in_pass.push_back(p);
                used[i] = true;
                --left;
            }
            ++np;
        }
    }
    G.n_bwd = np;
    return MVFIT_OK;
}

// VPoser decoder: the weights, their transposes and the helpers' register tiles
int build_vposer(const mvfit_model& m, HostModel& h, std::string& err) {
    if (!m.vp_fc1_w) return MVFIT_OK;
    if (!m.vp_fc1_b || !m.vp_fc2_w || !m.vp_fc2_b || !m.vp_out_w || !m.vp_out_b) return fail(err, MVFIT_E_ARG, "incomplete vposer weights");
    const std::vector<float>&w1 = h.vp_w1, &w2 = h.vp_w2, &w3 = h.vp_w3;
    h.vp_w1.assign(m.vp_fc1_w, m.vp_fc1_w + 512 * 32); h.vp_b1.assign(m.vp_fc1_b, m.vp_fc1_b + 512);
    h.vp_w2.assign(m.vp_fc2_w, m.vp_fc2_w + 512 * 512); h.vp_b2.assign(m.vp_fc2_b, m.vp_fc2_b + 512);
    h.vp_w3.assign(m.vp_out_w, m.vp_out_w + 138 * 512); h.vp_b3.assign(m.vp_out_b, m.vp_out_b + 138);
    h.vp_w1T.assign(32 * 512, 0.f); h.vp_w2T.assign(512 * 512, 0.f); h.vp_w3T.assign(512 * 144, 0.f);
    for (int o = 0; o < 512; ++o) for (int i = 0; i < 32; ++i) h.vp_w1T[i * 512 + o] = w1[o * 32 + i];
    for (int o = 0; o < 512; ++o) for (int i = 0; i < 512; ++i) h.vp_w2T[i * 512 + o] = w2[o * 512 + i];
    for (int o = 0; o < 138; ++o) for (int i = 0; i < 512; ++i) h.vp_w3T[i * 144 + o] = w3[o * 512 + i];
    h.vp_tw2.assign((size_t)VPS_SLICES * 16 * 512 * 4, 0.f);
    h.vp_tw3.assign((size_t)VPS_SLICES * 6 * 512 * 4, 0.f);
    for (int hs = 0; hs < VPS_SLICES; ++hs)
        for (int tid = 0; tid < 512; ++tid) {
            const int w = tid >> 6, l = tid & 63;
            for (int j = 0; j < 16; ++j)
                for (int q = 0; q < 4; ++q)
                    h.vp_tw2[(((size_t)hs * 16 + j) * 512 + tid) * 4 + q] = w2[(size_t)(64 * hs + 8 * w + (j >> 1)) * 512 + 8 * l + 4 * (j & 1) + q];
            for (int j = 0; j < 6; ++j) {
                const int o = l + 64 * (j >> 1);
                if (o < 138)
                    for (int q = 0; q < 4; ++q)
                        h.vp_tw3[(((size_t)hs * 6 + j) * 512 + tid) * 4 + q] = w3[(size_t)o * 512 + 64 * hs + 8 * w + 4 * (j & 1) + q];
            }
        }
    h.has_vposer = true;
    return MVFIT_OK;
}

// max-mixture prior: precisions with rows padded to 72 floats, both orientations; log weights
int build_gmm(const mvfit_model& m, HostModel& h, std::string& err) {
    if (m.gmm_M <= 0) return MVFIT_OK;
    if (m.gmm_M > 8 || !m.gmm_means || !m.gmm_precisions || !m.gmm_nll_weights) return fail(err, MVFIT_E_ARG, "gmm: M <= 8 and all arrays required");
    const int M = m.gmm_M;
    h.gmm_M = M;
    h.gmm_means.assign(m.gmm_means, m.gmm_means + M * 69);
    h.gmm_prec.assign((size_t)M * 69 * 72, 0.f);
    h.gmm_precT.assign((size_t)M * 69 * 72, 0.f);
    for (int g = 0; g < M; ++g)
        for (int r = 0; r < 69; ++r)
            for (int q = 0; q < 69; ++q) {
                const float v = m.gmm_precisions[((size_t)g * 69 + r) * 69 + q];
                h.gmm_prec[((size_t)g * 69 + r) * 72 + q] = v;
                h.gmm_precT[((size_t)g * 69 + q) * 72 + r] = v;
            }
    h.gmm_lognw.resize(M);
    for (int i = 0; i < M; ++i) h.gmm_lognw[i] = logf(m.gmm_nll_weights[i]);
    return MVFIT_OK;
}

// faces for mvfit_render_overlay with the vertex -> face CSR (a model whose faces index outside the vertices keeps none:
// the renderer then reports MVFIT_E_STATE, nothing else uses them)
void build_faces(const mvfit_model& m, HostModel& h) {
    if (!m.faces || m.num_faces <= 0) return;
    const int nf = m.num_faces, nv = h.nv;
    for (size_t i = 0; i < (size_t)nf * 3; ++i)
        if (m.faces[i] < 0 || m.faces[i] >= nv) return;
    h.faces.assign(m.faces, m.faces + (size_t)nf * 3);
    h.vf_ptr.assign(nv + 1, 0);
    h.vf_idx.assign((size_t)nf * 3, 0);
    for (int32_t i : h.faces) ++h.vf_ptr[i + 1];
    for (int i = 0; i < nv; ++i) h.vf_ptr[i + 1] += h.vf_ptr[i];
    std::vector<int32_t> fill(h.vf_ptr.begin(), h.vf_ptr.end() - 1);
    for (int f = 0; f < nf; ++f)                          // ascending face id within each vertex's list
        for (int k = 0; k < 3; ++k) h.vf_idx[fill[h.faces[f * 3 + k]]++] = f;
    h.num_faces = nf;
}

}  // namespace

// m has passed mvfit_create_ex's checks: every required array is present and num_verts > 0
int prepare_model(const mvfit_model& m, int contraction, int dense_skinning, HostModel& h, std::string& err) {
    h = HostModel();
    memset(&h.lds, 0, sizeof(h.lds));
    if (m.parents[0] >= 0) return fail(err, MVFIT_E_ARG, "parents[0] must be -1");
    h.nv = m.num_verts;
    h.ntiles = (h.nv + TILE_V - 1) / TILE_V;
    h.nv_pad = h.ntiles * TILE_V;
    build_basis(m, contraction, h);
    build_skinning(m, dense_skinning, h);
    build_joint_affine(m, h.lds);
    int rc = build_selection(m, h, err);
    if (rc == MVFIT_OK) rc = build_chain(m, h.lds, err);
    if (rc == MVFIT_OK) rc = build_vposer(m, h, err);
    if (rc == MVFIT_OK) rc = build_gmm(m, h, err);
    if (rc == MVFIT_OK) build_faces(m, h);
    return rc;
}

}  // namespace mvfit
