// The one declaration of every host function that one .hip file of libmvfit defines and another calls (launchers, workspace
// sizes and offsets, per-file configure calls).  Included by the file that defines a function and by the files that call it, so
// a declaration cannot drift from its definition unnoticed: a changed signature there is an overload that nobody defines, and
// the link (-z defs) stops.  Default arguments live here only.  launch_sdf_pullback: sdf_entries.h; sil_*: silhouette.h; the
// optimiser kernels' launchers: fit_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace mvfit {

struct ScanState;
struct DevModel;
struct DevPose;
struct DevProblems;
struct ResidentArgs;
struct SdfBox;
struct SdfAdj;

hipError_t launch_vertex_pass(const DevModel& M, const DevPose& P, int B, float* verts, int pass_kernel,
                              hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
hipError_t vertex_pass_configure();
// gate / gate_round (service rounds of a fit with the SDF term): the gate kernel copies the problems' gate words into the round's own
// copy, which the term's kernels behind the pass read
hipError_t launch_pass_gate(const DevPose& P, int b_lo, int B, hipStream_t stream, const int* gate = nullptr, int* gate_round = nullptr);
hipError_t launch_vertex_pass_resident(const DevModel& M, const ResidentArgs& RA, int tpw, hipStream_t stream);
// B: the problems the grid covers; layout_B >= B: the problems `entries` and `cull` were allocated for (sdf_layout.h)
hipError_t launch_sdf_term(const DevModel& M, const DevPose& P, const float* verts, int B, int layout_B, const int32_t* faces, int num_faces,
                           int G, const int* gate, SdfBox* box, float4* samp, void* entries, SdfAdj* adj, hipStream_t stream,
                           void* cull, unsigned* answer_tag = nullptr, unsigned answer = 0u, const unsigned long long* box_parts = nullptr);
size_t sdf_cull_bytes(int B, int num_faces);
size_t sdf_op_ws_bytes(int B, int num_faces);
bool sdf_op_uses_lists(int num_faces);
hipError_t launch_sdf_voxelize_culled(const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices, int G,
                                      float* phi, void* ws, hipStream_t stream);
size_t sdf_cull_zero_offset(int B, int num_faces);
size_t sdf_cull_zero_bytes(int B);
int sdf_cull_min_faces();
size_t sdf_work_bytes(int B, int nv);
size_t sdf_ticket_offset(int B, int nv);
hipError_t launch_triangulate(const float* kps, const double* intris, const double* extris, int B, int V, int J, double* out,
                              hipStream_t stream);
hipError_t launch_depth_guess(const double* rest, const double* extri, const double* intri, const float* kps, int B, int J,
                              double* out, hipStream_t stream);
hipError_t launch_umeyama(const double* src, const double* dst, int B, int npts, int estimate_scale, double* rot, double* rvec,
                          double* trans, double* scale, hipStream_t stream);
hipError_t launch_project_points(const DevProblems& Q, const float* pts, int N, float* uv, hipStream_t stream);
hipError_t launch_sdf_voxelize(const int32_t* faces, int num_faces, const float* vertices, int B, int num_vertices, int G,
                               float* phi, hipStream_t stream);
size_t render_ws_bytes(int G, int Nv, int Nf, int H, int W);
hipError_t launch_render_normals(const float* verts, int B, int Nv, const int32_t* faces, const int32_t* vf_ptr,
                                 const int32_t* vf_idx, double* nrm, hipStream_t stream);
hipError_t vertex_backward_configure();
hipError_t launch_vertices_backward(const DevModel& M, const DevPose& P, int B, int Bpad, const float* params, uint32_t flags,
                                    const float* g_verts, const float* g_joints, float* part, SdfAdj* rec, float* g_params,
                                    hipStream_t stream);
size_t vjp_part_bytes(int Bpad, int nv);
hipError_t launch_silhouette_pullback(const DevModel& M, const DevPose& P, int B, int Bpad, const int* gate, const float* g_verts,
                                      const float* loss, float* part, SdfAdj* rec, hipStream_t stream);
hipError_t launch_render_group(const DevProblems& Q, const int* prob, const int* view, int n, const float* verts,
                               const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points, int num_points,
                               int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, void* ws_mem,
                               hipStream_t stream);
size_t scene_ws_bytes(int n, int m, int Nv, int Nf, int H, int W);
size_t assoc_frame_bytes(int D);
size_t assoc_head_bytes();
hipError_t launch_associate_group(const float* kps, const int32_t* count, const double* intris, const double* extris, int f0,
                                  int nf, int V, int Nmax, double max_cost, int min_joints, int min_views, void* ws,
                                  double* cost_out, int32_t* labels, int32_t* num_clusters, hipStream_t stream);
hipError_t launch_camera_normal_eqs(const float* joints, const float* gt_xy, const float* w_conf, int B, int V,
                                    const double* cams, float rho, float data_weight, double* E, double* g, double* H,
                                    int32_t* count, hipStream_t stream);
hipError_t launch_camera_refine(const float* joints, const float* gt_xy, const float* w_conf, int B, int V,
                                const double* cams_in, uint32_t free_mask, uint32_t fixed_views, int max_iter, int min_points,
                                float rho, float data_weight, double lambda0, double ftol, double* cams_out, double* report,
                                hipStream_t stream);
int scene_sdf_blocks(int nv);
hipError_t launch_scene_boxes(const float* verts, int nv, int b0, int n, float factor, float4* box, float* local,
                              hipStream_t stream);
hipError_t launch_scene_pairs(const float* verts, int nv, int b0, int n, int s0, int ns, const void* tab, const int32_t* first,
                              const float4* box, const float* phi, int G, float rob, float* g_verts, float* part, float* loss,
                              hipStream_t stream);
hipError_t launch_scene_null_boxes(SdfBox* box, int B, hipStream_t stream);
hipError_t launch_scene_term(const DevModel& M, const DevPose& P, const float* verts, int B, const void* tab, const float4* box,
                             const float* phi, int G, float rob, const int* gate, const SdfBox* null_box, void* entries,
                             SdfAdj* adj, hipStream_t stream);
hipError_t launch_scene_group(const DevProblems& Q, const int32_t* tab, int num_images, int i0, int n, int j0, int m,
                              const float* verts, const double* nrm, int Nv, const int32_t* faces, int Nf, const float* points,
                              int num_points, int H, int W, const uint8_t* in, uint8_t* out, int32_t* face_id, int32_t* body_id,
                              void* ws_mem, hipStream_t stream);
// The scan loss (scan_loss.hip; the state: scan_loss.h).  Both return an MVFIT_* code and, on failure, a message in err; the
// caller (mvfit_scan.hip) has checked the arguments.  scan_set: points [N][Pmax][3] dev or host, count [N] and weights
// [N][Pmax] (or null) host.  scan_loss: faces [nf][3] dev, the model's; exhaustive = the search without the cull.
int scan_set(ScanState& S, int nv, int nf, int N, int Pmax, const float* points, const int32_t* count, const float* weights,
             hipStream_t stream, std::string& err);
int scan_loss(ScanState& S, const int32_t* faces, const float* vertices, float w_s2m, float w_m2s, float sigma, bool exhaustive,
              float* loss, float* g_vertices, int32_t* nearest_face, int32_t* nearest_point, hipStream_t stream,
              std::string& err);
// scan_loss's culled evaluation for the fit's chained rounds: kernel launches only (a capture records it as it is); gate [N] dev
// or null - a body with gate 0 keeps everything it held; loss [N] and g_vertices [N][nv][3] dev, both written.
int scan_round(ScanState& S, const int32_t* faces, const float* vertices, float w_s2m, float w_m2s, float sigma, const int* gate,
               float* loss, float* g_vertices, hipStream_t stream, std::string& err);

}  // namespace mvfit
