// column_names.h — which column a name refers to: the names of a score matrix's columns, or of a subject handle's slots, ascending and distinct, as a view.  Standard
// library only.  names [n] (a subset's listed indices sorted; a subject handle's ids) or, names == NULL, base + 0 .. n - 1 (the resident shard's positions).  Made for
// the last search by column_names() (afis_ctx.h); link_groups.h's column nodes are this view, and target_tables_check.cpp holds it against a linear search.
#pragma once
#include <algorithm>
#include <cstdint>

namespace afis {

struct ColumnNames {
    const int64_t* names; int64_t n; int64_t base;
    int64_t name(int64_t v) const { return names ? names[v] : base + v; }
    // the columns whose names lie below name_ — where a column of that name stands, or would: afis_count_before's tie position
    int64_t lower(int64_t name_) const { return names ? (int64_t)(std::lower_bound(names, names + n, name_) - names) : std::min(std::max<int64_t>(name_ - base, 0), n); }
    int64_t find(int64_t name_) const                                       // the column of that name, -1: none (a search of its own: one move fewer on the critical path of a step than through lower())
    {
        if (!names) return name_ >= base && name_ - base < n ? name_ - base : -1;
        const int64_t* const it = std::lower_bound(names, names + n, name_); return it != names + n && *it == name_ ? (int64_t)(it - names) : -1;
    }
};

}  // namespace afis
