// Byte layouts of the interpenetration term's two workspaces (sdf_term.hip), plain C++ with no HIP: the host files, the
// launchers and tests/sdf_layout_host_shim.cpp share these functions.
//
// A layout is a property of the ALLOCATION: every region is [B][per-problem slice] for the B the buffer was allocated with,
// and what must be zero between rounds (the tickets, the bin counters) was zeroed at those offsets.  A launch that covers
// fewer problems (a sub-batch of a service tail) addresses the same regions and touches the first `grid` slices of each:
// launchers take the grid's problem count and the allocation's separately and come here with the allocation's.
#pragma once
#include <cstddef>

#include "model_layout.h"

namespace mvfit {

#ifndef SDF_NS_
#define SDF_NS_ 8                   // (-DSDF_NS_=1 reproduces the single-chain summation order bit for bit: the control experiment)
#endif
constexpr int SDF_NS = SDF_NS_;      // workgroups (entry slices) per problem in the pull-back
constexpr int SDF_NC = 16;           // vertex chunks per problem in the entry kernel (one workgroup each)

// sizes of the records (the structs live in device headers, which assert that they agree)
constexpr size_t SDF_ENTRY_BYTES = 16;                                   // SdfEntry
constexpr size_t SDF_ADJ_BYTES = (size_t)(4 + NJ * 12 + KROWS) * 4;      // SdfAdj
constexpr size_t SDF_CHUNK_BYTES = 48;                                   // SdfChunk
constexpr size_t SDF_TRI_BYTES = 128;                                    // SdfTri

constexpr size_t sdf_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// work area behind `entries`: [B][nv] SdfEntry | [B][SDF_NS] SdfAdj slice partials | [B][SDF_NC] SdfChunk | [B] tickets
// (the tickets must be zero before the first round: mvfit_api.hip clears them when it allocates the area; every round
// leaves them at zero)
struct SdfWorkLayout {
    size_t entries, part, chunks, tickets;       // byte offsets of the regions
    size_t bytes;                                // of the whole area
};
constexpr SdfWorkLayout sdf_work_layout(int B, int nv) {
    SdfWorkLayout w{};
    w.entries = 0;
    w.part = sdf_align256((size_t)B * nv * SDF_ENTRY_BYTES);
    w.chunks = w.part + (size_t)B * SDF_NS * SDF_ADJ_BYTES;
    w.tickets = sdf_align256(w.chunks + (size_t)B * SDF_NC * SDF_CHUNK_BYTES);
    w.bytes = w.tickets + (size_t)B * sizeof(int);
    return w;
}
// per-problem slice of each region, in bytes
constexpr size_t sdf_work_entries_stride(int nv) { return (size_t)nv * SDF_ENTRY_BYTES; }
constexpr size_t sdf_work_part_stride() { return (size_t)SDF_NS * SDF_ADJ_BYTES; }
constexpr size_t sdf_work_chunks_stride() { return (size_t)SDF_NC * SDF_CHUNK_BYTES; }

// face-list workspace of the culled sample kernel (bins, lists: sdf_term.hip)
constexpr int SDF_NB = 256;                         // projective bins per axis (ray structure)
constexpr int SDF_NC3 = 64;                         // cells per axis (distance structure)
constexpr int SDF_NBINS = SDF_NB * SDF_NB + SDF_NC3 * SDF_NC3 * SDF_NC3;
constexpr int SDF_OFFS_LD = SDF_NBINS + 4;           // row of the offsets (NBINS + 1 used), 16-byte aligned
constexpr int SDF_CULL_CAP = 64;                    // list entries per face the workspace holds

// [B][F] SdfTri | [B][SDF_OFFS_LD] offsets | [B][SDF_NBINS] counters (zero between rounds: cleared at allocation, count adds,
// fill takes away) | [B][SDF_CULL_CAP * F] int2 list entries | [B] flags
struct SdfCullLayout {
    size_t tri, offs, cnt, ent, flag;            // byte offsets of the regions
    size_t cnt_bytes;                            // of the counters, padded: what the allocation zeroes
    size_t bytes;
};
constexpr SdfCullLayout sdf_cull_layout(int B, int F) {
    SdfCullLayout w{};
    w.tri = 0;
    w.offs = w.tri + sdf_align256((size_t)B * F * SDF_TRI_BYTES);
    w.cnt = w.offs + sdf_align256((size_t)B * SDF_OFFS_LD * 4);
    w.cnt_bytes = sdf_align256((size_t)B * SDF_NBINS * 4);
    w.ent = w.cnt + w.cnt_bytes;
    w.flag = w.ent + sdf_align256((size_t)B * SDF_CULL_CAP * F * 8);
    w.bytes = w.flag + sdf_align256((size_t)B * 4);
    return w;
}
constexpr size_t sdf_cull_tri_stride(int F) { return (size_t)F * SDF_TRI_BYTES; }
constexpr size_t sdf_cull_offs_stride() { return (size_t)SDF_OFFS_LD * 4; }
constexpr size_t sdf_cull_cnt_stride() { return (size_t)SDF_NBINS * 4; }
constexpr size_t sdf_cull_ent_stride(int F) { return (size_t)SDF_CULL_CAP * F * 8; }

// A launch over `grid` problems inside a buffer allocated for `layout_B`: the layout it addresses, or false when the grid
// does not fit the allocation.  (The launchers of sdf_term.hip call these; nothing else turns a grid into offsets.)
constexpr bool sdf_launch_work_layout(int grid, int layout_B, int nv, SdfWorkLayout* out) {
    if (grid < 0 || grid > layout_B) return false;
    *out = sdf_work_layout(layout_B, nv);
    return true;
}
constexpr bool sdf_launch_cull_layout(int grid, int layout_B, int F, SdfCullLayout* out) {
    if (grid < 0 || grid > layout_B) return false;
    *out = sdf_cull_layout(layout_B, F);
    return true;
}

}  // namespace mvfit
