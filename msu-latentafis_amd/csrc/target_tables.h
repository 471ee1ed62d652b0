// target_tables.h — the targets of a call as a CSR by row, built on the host alone: nothing here knows of a device, so the construction is a program of its own under
// the host sanitizers (target_tables_check.cpp, tests/test_target_tables_host.py).  Target i asks about row query[i]; dev [m] lists the targets that go to the device
// (NULL: all m of them), key [per target] a secondary key (NULL: none).  The device's tables begin rows [n_rows] | off [n_rows + 1] | row [m], the call's own column
// [m] behind them; order is the way back: place t of the CSR holds element order[t] of dev (NULL: target order[t]).  afis_rank_positions', afis_entries_at's, the case lists'.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace afis {

struct TargetTables {
    std::vector<int32_t> rows, off, order;                                  // the distinct rows ascending; row r's places off[r] .. off[r + 1] - 1; [m], stable: by key, else the caller's order
    int32_t max_row_targets = 0;                                            // the longest row
    int32_t* write(int32_t* tab) const                                      // rows | off | row [m] into tab; returns where the call's own column begins
    {
        tab = std::copy(off.begin(), off.end(), std::copy(rows.begin(), rows.end(), tab));
        for (size_t r = 0; r < rows.size(); ++r) tab = std::fill_n(tab, off[r + 1] - off[r], rows[r]);
        return tab;
    }
};

inline TargetTables build_target_tables(const int32_t* query, const int32_t* dev, size_t m, const int64_t* key)
{
    TargetTables t;
    std::vector<int32_t> row(m); std::vector<int64_t> key_of(m, 0);        // per element of dev: its row and its key, so that the comparator reads two arrays and tests for neither list
    for (size_t k = 0; k < m; ++k) { const size_t i = dev ? (size_t)dev[k] : k; row[k] = query[i]; if (key) key_of[k] = key[i]; }
    t.off.assign(1, 0); t.order.resize(m);
    std::iota(t.order.begin(), t.order.end(), 0);
    std::stable_sort(t.order.begin(), t.order.end(), [r = row.data(), k = key_of.data()](int32_t a, int32_t b) { return r[a] != r[b] ? r[a] < r[b] : k[a] < k[b]; });   // (pointers by value: nothing to reload per comparison)
    for (size_t p = 0; p < m; ++p) {
        const int32_t q = row[(size_t)t.order[p]];
        if (t.rows.empty() || q != t.rows.back()) { t.rows.push_back(q); t.off.push_back(t.off.back()); }
        t.max_row_targets = std::max(t.max_row_targets, ++t.off.back() - t.off[t.off.size() - 2]);
    }
    return t;
}

}  // namespace afis
