// The dispatch table of devprobe_fns.h compiled by g++ with the flags of tests/emul: the reference side of tests/test_devprobe_gpu.py
// (same compiler and flags as the oracle and the CPU emulation).  A loop over rows, nothing else.
#include <cstddef>
#include <vector>

#include "devprobe_fns.h"

using namespace f3ds;

extern "C" {

int dp_host_shape(int fn, int* ni, int* no) { return dp_shape(fn, ni, no) ? 0 : -1; }

// fn < DP_TABLE: constants as literals (m_lit); fn >= DP_TABLE: read from a copy of the table (m_tab)
int dp_host_run(int fn, const uint32_t* in, uint32_t* out, size_t n) {
    int ni, no;
    if (!dp_shape(fn, &ni, &no)) return -1;
    static double table[MC_COUNT];
    static const bool filled = (m_table_fill(table, 0, 1), true);
    (void)filled;
    const m_tab tab{table};
    for (size_t r = 0; r < n; ++r) {
        if (fn >= DP_TABLE) dp_eval(fn - DP_TABLE, in + r * (size_t)ni, out + r * (size_t)no, tab);
        else dp_eval(fn, in + r * (size_t)ni, out + r * (size_t)no, m_lit());
    }
    return 0;
}

// T tables (devprobe_fns.h, dp_evl_one); nk / nm = the summed K / M of all tables (scratch sizes); out = 7 floats per table
int dp_host_evl(uint32_t T, const uint32_t* dims, const uint32_t* ssize, const uint32_t* tsize, const uint32_t* roff, const uint32_t* col, const uint32_t* cnt,
                size_t nk, size_t nm, uint32_t* out) {
    std::vector<unsigned char> visited(nm + 1), used(nk + 1);
    std::vector<uint32_t> order(nm + 1), match(nm + 1), in(nm + 1), ci(nk + 1), cc(nk + 1);
    const DpEvlArrays A{dims, ssize, tsize, roff, col, cnt, visited.data(), used.data(), order.data(), match.data(), in.data(), ci.data(), cc.data(), out};
    for (uint32_t t = 0; t < T; ++t) dp_evl_one(A, t);
    return 0;
}

}  // extern "C"
