// Records between the producers of an interpenetration term's entries (sdf_entries_kernel in sdf_term.hip, scene_entries_kernel
// in scene_sdf.hip) and the pull-back through skinning and the blendshape basis (sdf_pullback_kernel, sdf_term.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "mvfit_device.h"
#include "sdf_layout.h"

namespace mvfit {

constexpr int SDF_ADJ_NT = 512;      // threads of an entry / pull-back workgroup

// entry list of one problem: the vertices that carry gradient, in ascending vertex order
struct SdfEntry { int v; float g[3]; };                                  // vertex, dS/dvertex
static_assert(sizeof(SdfEntry) == 16, "entry layout");

// (SDF_NC, the vertex chunks per problem in the entry kernel - one workgroup each: sdf_layout.h)
constexpr int SDF_NIT = 1;           // 64-vertex rows per wave of a chunk: nv <= SDF_NC * 8 waves * SDF_NIT * 64 = 8192

// per (problem, vertex chunk): partial sums of S and of the box adjoint, entries written (at the chunk's own offset)
struct SdfChunk { double S, gc0, gc1, gc2, gs; int cnt, pad; };
static_assert(sizeof(SdfChunk) == 48, "chunk record");

// the chunk records inside the work area behind `entries` (sdf_work_bytes(layout_B, nv) bytes, layout: sdf_layout.h)
SdfChunk* sdf_work_chunks(void* entries, int layout_B, int nv);
// B: the problems the grid covers; layout_B >= B: the problems the work area was allocated for
hipError_t launch_sdf_pullback(const DevModel& M, const DevPose& P, int B, int layout_B, const int* gate, const SdfBox* box, void* entries,
                               SdfAdj* adj, hipStream_t stream);

}  // namespace mvfit
