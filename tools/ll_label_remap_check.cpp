// Stand-alone check of sert_amd/csrc/ll_label_remap.h (the column layout of a refreshing loglinear fold-in handle and the
// remap of CSR label rows into it) on the CPU, meant to be built with -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sert_amd/csrc \
//         tools/ll_label_remap_check.cpp -o ll_label_remap_check
//     ll_label_remap_check < rows.txt > remapped.txt
// Input, whitespace-separated integers: V_e N R M, then R refresh ids, M + 1 indptr values, nnz public columns, nnz values as
// the BITS of their float32.  Output: the status of ll_layout; then, if it is 0, V_e + N internal columns, nnz internal
// columns and nnz value bits, one array per line.  The program checks itself that every remapped row is strictly increasing,
// that its frozen prefix is the row's frozen entries in their order and that (column, value) pairs are a permutation of the
// row's own; it exits 1 with a message if not.  tests/test_ll_refresh_inputs_cpu.py feeds it the rows of
// tests/ll_refresh_cases.py and compares the output with NumPy.
#include <cstdio>
#include <cstring>
#include <map>

#include "ll_label_remap.h"

static bool read_i64(long long* v) { return scanf("%lld", v) == 1; }

int main() {
    long long Ve, N, R, M;
    if (!read_i64(&Ve) || !read_i64(&N) || !read_i64(&R) || !read_i64(&M) || Ve < 0 || N < 0 || R < 0 || M < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int32_t> ids((size_t)R);
    for (auto& e : ids) { long long v; if (!read_i64(&v)) return 2; e = (int32_t)v; }
    std::vector<int64_t> indptr((size_t)M + 1);
    for (auto& p : indptr) { long long v; if (!read_i64(&v)) return 2; p = v; }
    const int64_t nnz = indptr[(size_t)M];
    std::vector<int32_t> indices((size_t)nnz);
    for (auto& c : indices) { long long v; if (!read_i64(&v)) return 2; c = (int32_t)v; }
    std::vector<float> data((size_t)nnz);
    for (auto& x : data) {
        long long v;
        if (!read_i64(&v)) return 2;
        const uint32_t bits = (uint32_t)v;
        memcpy(&x, &bits, sizeof x);
    }
    std::vector<int32_t> internal_of;
    const int status = sert::ll_layout((int32_t)Ve, (int32_t)N, ids.empty() ? nullptr : ids.data(), (int32_t)R, internal_of);
    printf("%d\n", status);
    if (status != sert::LL_LAYOUT_OK) return 0;
    const int32_t Vf = (int32_t)(Ve - R);
    // exactly nnz entries each: a write past the end is the sanitizer's to find
    std::vector<int32_t> out_indices((size_t)nnz);
    std::vector<float> out_data((size_t)nnz);
    sert::ll_remap_csr(indptr.data(), indices.data(), data.data(), M, internal_of, Vf, out_indices.data(), out_data.data());
    for (int64_t r = 0; r < M; ++r) {
        std::map<int32_t, uint32_t> want;
        std::vector<int32_t> frozen;
        for (int64_t i = indptr[(size_t)r]; i < indptr[(size_t)r + 1]; ++i) {
            uint32_t bits;
            memcpy(&bits, &data[(size_t)i], sizeof bits);
            const int32_t c = internal_of[(size_t)indices[(size_t)i]];
            want[c] = bits;
            if (c < Vf) frozen.push_back(c);
        }
        size_t k = 0;
        for (int64_t i = indptr[(size_t)r]; i < indptr[(size_t)r + 1]; ++i, ++k) {
            uint32_t bits;
            memcpy(&bits, &out_data[(size_t)i], sizeof bits);
            const int32_t c = out_indices[(size_t)i];
            const bool increasing = i == indptr[(size_t)r] || out_indices[(size_t)i - 1] < c;
            const auto it = want.find(c);
            if (!increasing || it == want.end() || it->second != bits || (k < frozen.size() && frozen[k] != c)) {
                fprintf(stderr, "row %lld: entry %lld is wrong after the remap\n", (long long)r, (long long)i);
                return 1;
            }
        }
    }
    for (size_t i = 0; i < internal_of.size(); ++i) printf("%d ", internal_of[i]);
    printf("\n");
    for (int64_t i = 0; i < nnz; ++i) printf("%d ", out_indices[(size_t)i]);
    printf("\n");
    for (int64_t i = 0; i < nnz; ++i) {
        uint32_t bits;
        memcpy(&bits, &out_data[(size_t)i], sizeof bits);
        printf("%u ", bits);
    }
    printf("\n");
    return 0;
}
