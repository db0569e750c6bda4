// The scan set a ctx keeps between mvfit_set_scans and the loss calls (scan_loss.hip; driven by mvfit_scan.hip through
// launchers.h: scan_set / scan_loss; the fit's rounds evaluate on the same set through scan_round).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dev_mem.h"

namespace mvfit {

struct ScanState {
    bool on = false;
    int N = 0, Pmax = 0, nv = 0, nf = 0, ns = 0;            // ns: seed vertices per body (scan_loss.hip)
    // device memory sized by (N, Pmax, nv, nf): points, effective weights, packed points, counts and weight exponents, face
    // records, seed vertices, fixed-point accumulators, loss partials of both terms.  A set of the same sizes keeps the buffer
    // and with it every address.
    DevBuf ws;
    size_t o_pts = 0, o_w = 0, o_pk = 0, o_cnt = 0, o_rec = 0, o_seed = 0, o_acc = 0, o_partS = 0, o_partM = 0;
    std::vector<float> h_w;             // host staging of the effective weights and the counts (kept while a copy may read it)
    std::vector<int32_t> h_cnt;         // [2 N]: count[n], then e_n = -ilogb(largest participating weight of body n), 0 without one
};

}  // namespace mvfit
