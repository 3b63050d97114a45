// mm_adjacency.h -- the host mesh adjacency shared by the labelling (mm_ccta.cpp) and the trimming (mm_trim.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace mm {

// build_adjacency_map (ccta_py.rs:507-525) as sorted, de-duplicated neighbour lists (a face with a repeated corner
// makes that vertex its own neighbour, as in the reference)
struct Adjacency {
    std::vector<int64_t> off, nb;
    const int64_t* begin(int64_t v) const { return nb.data() + off[(size_t)v]; }
    const int64_t* end(int64_t v) const { return nb.data() + off[(size_t)v + 1]; }
};
// Edges with an end outside [0, nv) are left out: such a vertex is in no subset the callers walk (keep_largest takes
// indices >= nv as the reference does; the other callers reject them up front).
inline void build_adjacency(const int64_t* faces, int64_t nf, int64_t nv, Adjacency& adj)
{
    std::vector<std::pair<int64_t, int64_t>> ed;
    ed.reserve((size_t)nf * 6);
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t* v = faces + 3 * f;
        const int64_t e[3][2] = {{v[0], v[1]}, {v[1], v[2]}, {v[2], v[0]}};
        for (const auto& p : e)
            if (p[0] >= 0 && p[0] < nv && p[1] >= 0 && p[1] < nv) { ed.emplace_back(p[0], p[1]); ed.emplace_back(p[1], p[0]); }
    }
    std::sort(ed.begin(), ed.end());
    ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
    adj.off.assign((size_t)nv + 1, 0);
    for (const auto& p : ed) ++adj.off[(size_t)p.first + 1];
    for (int64_t v = 0; v < nv; ++v) adj.off[(size_t)v + 1] += adj.off[(size_t)v];
    adj.nb.resize(ed.size());
    for (size_t k = 0; k < ed.size(); ++k) adj.nb[k] = ed[k].second;   // sorted by first: already in CSR order
}

}  // namespace mm
