// fpfh_batch_plan.hpp -- what pcc_fpfh_descriptors_batch (fpfh_batch.hip) plans of its own: the output splice.
// Plain C++ (no HIP): tests/cpp/test_fpfh_batch_plan.cpp compiles it on its own.
//
// Routes, bases and work items are range_batch_plan.hpp's (range_batch_plan with min_points = 0: an empty cluster is on the
// batch route with no point).  Once the slice bounds of the batch route and the row counts of the work handle are known,
// fpfh_batch_splice puts both back into cluster order: the caller's bounds, and the row copies that move the batch route's
// rows to their places.
#pragma once
#include "range_batch_plan.hpp"

namespace pcc {

// one copy of the output splice: `count` rows from row `src` of the batch route's rows to row `dst` of the caller's
struct FpfhBatchCopy {
    size_t src, dst, count;
};
// slice[n_clusters + 1]: the batch route's slice bounds (a cluster off that route owns none); single_m[c]: the rows the work
// handle found for a cluster on it.  offsets: the caller's n_clusters + 1 bounds; copies: the batch route's runs in cluster
// order, merged where neighbours stay neighbours.
template <class Slice>
inline void fpfh_batch_splice(const RangeBatchPlan& p, const Slice* slice, const size_t* single_m, std::vector<size_t>* offsets,
                              std::vector<FpfhBatchCopy>* copies) {
    const size_t n_clusters = p.n.size();
    offsets->assign(n_clusters + 1, 0);
    copies->clear();
    size_t at = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        (*offsets)[c] = at;
        if (p.on_work_handle(c)) {
            at += single_m[c];
            continue;
        }
        const size_t src = (size_t)slice[c], m = (size_t)slice[c + 1] - src;
        if (m) {
            if (!copies->empty() && copies->back().src + copies->back().count == src && copies->back().dst + copies->back().count == at)
                copies->back().count += m;
            else
                copies->push_back({src, at, m});
        }
        at += m;
    }
    (*offsets)[n_clusters] = at;
}

}  // namespace pcc
