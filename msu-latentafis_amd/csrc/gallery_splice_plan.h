// gallery_splice_plan.h — the host plan of afis_gallery_commit_at (afis_gallery.cpp): staged template i takes the place of resident entry idx[i] - index_base.
// From what the host keeps of the resident shard (CSR offsets, empty flags) and the staged templates' offsets and flags it validates the call, writes the CSR
// offsets and the empty flags of the shard AFTER the edit, and one source table per point kind for the splice kernel (gallery_edit.hip: k_splice_ranges):
//   src[t] >= 0 : template t keeps its points; they start at point src[t] of the RESIDENT array (its old offset)
//   src[t] <  0 : template t is replaced; its points start at point ~src[t] of the STAGED array
// Pure host code, no HIP: gallery_splice_plan_check.cpp runs it under the host sanitizers (tests/test_gallery_replace_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace afis {

enum SplicePlanError {
    kSpliceOk = 0,
    kSpliceNullIdx,                                                         // n > 0 without an index list
    kSpliceCount,                                                           // n is not the number of staged templates
    kSpliceRange,                                                           // an index outside [index_base, index_base + G)
    kSpliceDuplicate,                                                       // an index listed twice
    kSpliceTooLarge,                                                        // the edited shard's points (or the staged ones) beyond 32-bit offsets, or its 32-point tiles beyond the bound pass's stream
};

struct SplicePlan {
    std::vector<int32_t> mo, to;                                            // [G + 1] CSR offsets after the edit
    std::vector<uint8_t> empty;                                             // [G]
    std::vector<int32_t> src_m, src_t;                                      // [G] source tables, minutiae and texture points (above)
    int64_t first = 0;                                                      // the first replaced entry (local): offsets before it do not move
};

inline const char* splice_plan_message(int e)
{
    switch (e) {
    case kSpliceNullIdx: return "null index list";
    case kSpliceCount: return "n differs from the number of staged templates";
    case kSpliceRange: return "gallery index outside this shard";
    case kSpliceDuplicate: return "a gallery index listed twice";
    case kSpliceTooLarge: return "shard too large for 32-bit point offsets or the bound pass's code stream; split the gallery into more shards";
    default: return "";
    }
}

// res_mo / res_to [G + 1], res_empty [G]: the resident shard.  idx [n]: global indices.  st_mo / st_to [n_staged + 1]: the staged templates' offsets, from any base (a slice
// of a mapped container starts where the slice starts: the staged arrays on the device start at st_mo[0] / st_to[0]); st_empty [n_staged].  `out` is written on kSpliceOk only.
inline int plan_gallery_splice(const int32_t* res_mo, const int32_t* res_to, const uint8_t* res_empty, int64_t G, int64_t index_base, const int64_t* idx, int64_t n,
                               int64_t n_staged, const int64_t* st_mo, const int64_t* st_to, const uint8_t* st_empty, SplicePlan& out)
{
    if (n > 0 && !idx) return kSpliceNullIdx;
    if (n != n_staged || n < 0) return kSpliceCount;
    std::vector<int64_t> slot((size_t)G, -1);                               // local entry -> the staged template that replaces it
    for (int64_t i = 0; i < n; ++i) {
        if (idx[i] < index_base || idx[i] >= index_base + G) return kSpliceRange;
        const size_t g = (size_t)(idx[i] - index_base);
        if (slot[g] >= 0) return kSpliceDuplicate;
        slot[g] = i;
    }
    const int64_t kMax = 0x7fffffff;
    if (n > 0 && (st_mo[n] - st_mo[0] > kMax || st_to[n] - st_to[0] > kMax)) return kSpliceTooLarge;
    SplicePlan p;
    p.mo.assign((size_t)G + 1, 0); p.to.assign((size_t)G + 1, 0); p.empty.assign((size_t)G, 0); p.src_m.assign((size_t)G, 0); p.src_t.assign((size_t)G, 0);
    p.first = G;
    int64_t nm = 0, nt = 0, t32 = 0;
    for (int64_t t = 0; t < G; ++t) {
        const int64_t j = slot[(size_t)t];
        int64_t cm, ct;
        if (j < 0) {
            cm = res_mo[t + 1] - res_mo[t]; ct = res_to[t + 1] - res_to[t];
            p.src_m[(size_t)t] = res_mo[t]; p.src_t[(size_t)t] = res_to[t];
            p.empty[(size_t)t] = res_empty[t];
        } else {
            cm = st_mo[j + 1] - st_mo[j]; ct = st_to[j + 1] - st_to[j];
            p.src_m[(size_t)t] = ~(int32_t)(st_mo[j] - st_mo[0]); p.src_t[(size_t)t] = ~(int32_t)(st_to[j] - st_to[0]);
            p.empty[(size_t)t] = st_empty[j];
            if (t < p.first) p.first = t;
        }
        nm += cm; nt += ct; t32 += (ct + 31) / 32;
        if (nm > kMax || nt > kMax) return kSpliceTooLarge;
        p.mo[(size_t)t + 1] = (int32_t)nm; p.to[(size_t)t + 1] = (int32_t)nt;
    }
    if (t32 > kMax / 32) return kSpliceTooLarge;
    out = std::move(p);
    return kSpliceOk;
}

}  // namespace afis
