// Host build of csrc/model_prep.cpp for tests/test_e6_cells_cpu.py (clang++ -O2 -shared -fPIC, no HIP): E6's lane cells and
// the tables they index, copied into caller buffers (model_prep_host_shim.cpp names every other table).
#include <cstdio>
#include <cstring>
#include <string>

#include "../mvsmplfitting_amd/csrc/model_prep.h"

using mvfit::HostModel;

extern "C" void* e6_run(const mvfit_model* m, int contraction, int dense_skinning, int* rc, char* err, int errlen) {
    HostModel* h = new HostModel();
    std::string e;
    *rc = mvfit::prepare_model(*m, contraction, dense_skinning, *h, e);
    snprintf(err, errlen, "%s", e.c_str());
    return h;
}

extern "C" void e6_free(void* h) { delete static_cast<HostModel*>(h); }

// sizes: {NJ, lanes, E6_NZ, E6_INVALID, NS_STRIDE, NS_MAX}
extern "C" void e6_sizes(int* out) {
    const int v[6] = {mvfit::NJ, 16, mvfit::E6_NZ, (int)mvfit::E6_INVALID, mvfit::NS_STRIDE, mvfit::NS_MAX};
    memcpy(out, v, sizeof(v));
}

// cells [NJ][16][E6_NZ] uint16, wT [NJ][NS_STRIDE], selw [NS_MAX][4], selj [NS_MAX]; info = {ns, lds.e6_cells, lds.sel_sparse,
// number of cell entries}
extern "C" void e6_get(void* hp, uint16_t* cells, float* wT, float* selw, unsigned* selj, int* info) {
    const HostModel& h = *static_cast<HostModel*>(hp);
    info[0] = h.lds.ns; info[1] = h.lds.e6_cells; info[2] = h.lds.sel_sparse; info[3] = (int)h.e6_cells.size();
    if (cells && h.e6_cells.size() == (size_t)mvfit::NJ * 16 * mvfit::E6_NZ) memcpy(cells, h.e6_cells.data(), h.e6_cells.size() * 2);
    memcpy(wT, h.lds.wT, sizeof(h.lds.wT));
    memcpy(selw, h.lds.selw, sizeof(h.lds.selw));
    memcpy(selj, h.lds.selj, sizeof(h.lds.selj));
}
