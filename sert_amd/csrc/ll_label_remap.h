// The column layout of a loglinear fold-in handle that refreshes trained columns (include/sert_hip_ll_foldin.h:
// sert_ll_foldin_create_refresh; host/api_ll_foldin.inc) and the remap of CSR label rows into it.  Host only: plain C++, no
// HIP, so that a stand-alone program can run it under a sanitizer on the CPU (tools/ll_label_remap_check.cpp).
//
// PUBLIC columns are the caller's: e < V_e trained entity e, V_e + j new entity j.  INTERNAL columns are the handle's: the
// V_f = V_e - R frozen columns first, in ascending trained index, the R refreshed slots behind them in the order of
// refresh_ids, the N new columns last.  The step kernels see a model of V_f frozen entities and Nt = R + N new ones.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace sert {

enum { LL_LAYOUT_OK = 0, LL_LAYOUT_ID_RANGE = 1, LL_LAYOUT_ID_DUPLICATE = 2 };

// internal_of (V_e + N): the internal column of every public one.  refresh_ids: R distinct ids in [0, V_e), any order (not
// read when R == 0).  -> LL_LAYOUT_OK, or what is wrong with the ids (internal_of is then unspecified).
inline int ll_layout(int32_t Ve, int32_t N, const int32_t* refresh_ids, int32_t R, std::vector<int32_t>& internal_of) {
    internal_of.assign((size_t)Ve + (size_t)N, -1);
    for (int32_t s = 0; s < R; ++s) {
        const int32_t e = refresh_ids[s];
        if (e < 0 || e >= Ve) return LL_LAYOUT_ID_RANGE;
        if (internal_of[(size_t)e] >= 0) return LL_LAYOUT_ID_DUPLICATE;
        internal_of[(size_t)e] = s;                      // (the slot for now: V_f is added below)
    }
    const int32_t Vf = Ve - R;
    int32_t frozen = 0;
    for (int32_t e = 0; e < Ve; ++e) {
        if (internal_of[(size_t)e] < 0) internal_of[(size_t)e] = frozen++;
        else internal_of[(size_t)e] += Vf;
    }
    for (int32_t j = 0; j < N; ++j) internal_of[(size_t)Ve + (size_t)j] = Vf + R + j;
    return LL_LAYOUT_OK;
}

// CSR label rows on public columns, already validated (indptr from 0, non-decreasing; the columns of a row in [0, V_e + N),
// strictly increasing) -> the same rows on internal columns, strictly increasing again: out_indices / out_data hold
// indptr[M] entries, indptr is unchanged.  Frozen and new columns keep their relative order under internal_of; a refreshed
// column moves from among the frozen ones to the trainable tail [V_f, ..), so a row's frozen entries are written first, as
// they come, and its tail is sorted by internal column, values along with their columns.
inline void ll_remap_csr(const int64_t* indptr, const int32_t* indices, const float* data, int64_t M,
                         const std::vector<int32_t>& internal_of, int32_t Vf, int32_t* out_indices, float* out_data) {
    std::vector<std::pair<int32_t, float>> tail;
    for (int64_t r = 0; r < M; ++r) {
        int64_t o = indptr[r];
        tail.clear();
        for (int64_t i = indptr[r]; i < indptr[r + 1]; ++i) {
            const int32_t c = internal_of[(size_t)indices[i]];
            if (c < Vf) { out_indices[o] = c; out_data[o] = data[i]; ++o; }
            else tail.emplace_back(c, data[i]);
        }
        std::sort(tail.begin(), tail.end(), [](const std::pair<int32_t, float>& a, const std::pair<int32_t, float>& b) {
            return a.first < b.first;                    // (distinct columns: the order is total)
        });
        for (const auto& t : tail) { out_indices[o] = t.first; out_data[o] = t.second; ++o; }
    }
}

}  // namespace sert
