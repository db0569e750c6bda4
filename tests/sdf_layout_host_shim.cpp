// Host build of csrc/sdf_layout.h for tests/test_sdf_layout_cpu.py (clang++ -O2 -shared -fPIC, no HIP): the byte layouts of the
// SDF term's work area and face-list workspace as flat int64 arrays, and the layout a launch over `grid` problems addresses
// inside a buffer allocated for `layout_B` - the functions the launchers of sdf_term.hip call.
#include <cstdint>

#include "../mvsmplfitting_amd/csrc/sdf_layout.h"

using namespace mvfit;

static void put_work(const SdfWorkLayout& w, int nv, int64_t* out9) {
    const int64_t v[9] = {(int64_t)w.entries, (int64_t)w.part, (int64_t)w.chunks, (int64_t)w.tickets, (int64_t)w.bytes,
                          (int64_t)sdf_work_entries_stride(nv), (int64_t)sdf_work_part_stride(), (int64_t)sdf_work_chunks_stride(), 4};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
}
static void put_cull(const SdfCullLayout& w, int F, int64_t* out12) {
    const int64_t v[12] = {(int64_t)w.tri, (int64_t)w.offs, (int64_t)w.cnt, (int64_t)w.ent, (int64_t)w.flag, (int64_t)w.bytes,
                           (int64_t)sdf_cull_tri_stride(F), (int64_t)sdf_cull_offs_stride(), (int64_t)sdf_cull_cnt_stride(),
                           (int64_t)sdf_cull_ent_stride(F), 4, (int64_t)w.cnt_bytes};
    for (int i = 0; i < 12; ++i) out12[i] = v[i];
}

// out9: offsets of entries, part, chunks, tickets; bytes; per-problem strides of the four regions
extern "C" void sdf_layout_work(int B, int nv, int64_t* out9) { put_work(sdf_work_layout(B, nv), nv, out9); }
// out12: offsets of tri, offs, cnt, ent, flag; bytes; per-problem strides of the five regions; bytes of the zeroed counters
extern "C" void sdf_layout_cull(int B, int F, int64_t* out12) { put_cull(sdf_cull_layout(B, F), F, out12); }

// what a launch over `grid` problems addresses in buffers allocated for layout_B; returns 0 when the grid does not fit
extern "C" int sdf_layout_launch_work(int grid, int layout_B, int nv, int64_t* out9) {
    SdfWorkLayout w;
    if (!sdf_launch_work_layout(grid, layout_B, nv, &w)) return 0;
    put_work(w, nv, out9);
    return 1;
}
extern "C" int sdf_layout_launch_cull(int grid, int layout_B, int F, int64_t* out12) {
    SdfCullLayout w;
    if (!sdf_launch_cull_layout(grid, layout_B, F, &w)) return 0;
    put_cull(w, F, out12);
    return 1;
}

// SDF_NS, SDF_NC, SDF_NBINS, SDF_OFFS_LD, SDF_CULL_CAP, and the record sizes: entry, adjoint, chunk, triangle
extern "C" void sdf_layout_constants(int64_t* out9) {
    const int64_t v[9] = {SDF_NS, SDF_NC, SDF_NBINS, SDF_OFFS_LD, SDF_CULL_CAP, (int64_t)SDF_ENTRY_BYTES, (int64_t)SDF_ADJ_BYTES,
                          (int64_t)SDF_CHUNK_BYTES, (int64_t)SDF_TRI_BYTES};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
}
