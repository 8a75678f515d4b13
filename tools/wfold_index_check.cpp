// Stand-alone check of sert_amd/csrc/wfold_index.h (the per-batch inverted index new word -> batch rows of a word fold-in) on
// the CPU, meant to be built with -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sert_amd/csrc \
//         tools/wfold_index_check.cpp -o wfold_index_check && ./wfold_index_check
// It builds the index of random token arrays -- no new word, every position new, one position in three -- at shapes with one,
// two and three levels and walks it the way the segmented-sum kernels do: every entry names a batch row, every item holds 1 to
// kWfoldChunk entries, a level's partial rows are numbered in item order, and every word's occurrences are counted exactly
// once.  Prints "ok", or a message and exit status 1.  With the argument "probe" it builds one trivial index only: a caller uses
// that to learn whether a sanitized build runs at all here, and then holds the full run to exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "wfold_index.h"
using namespace sert;
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "probe")) {
        const int32_t tok[2] = {0, -1};
        WfoldIndex ix;
        build_wfold_index(tok, 1, 1, 2, 1, ix);
        printf("probe ok\n");
        return 0;
    }
    srand(7);
    const int shapes[][4] = {{3, 32, 3, 5}, {2, 200, 3, 1}, {2, 1366, 3, 1}, {4, 64, 10, 300}, {1, 1, 1, 1}, {2, 5000, 2, 2}};
    for (auto& sh : shapes) {
        const int nb = sh[0], B = sh[1], n = sh[2], Nw = sh[3];
        for (int mode = 0; mode < 3; ++mode) {
            std::vector<int32_t> tok((size_t)nb * B * n);
            for (auto& t : tok) t = mode == 0 ? -1 : mode == 1 ? rand() % Nw : (rand() % 3 ? -1 : rand() % Nw);
            WfoldIndex ix;
            build_wfold_index(tok.data(), nb, B, n, Nw, ix);
            // walk the index as the kernels do: every entry in range, every word's occurrences counted once
            for (int b = 0; b < nb; ++b) {
                const WfoldBatch& bx = ix.batches[b];
                std::vector<long> cnt(Nw, 0), want(Nw, 0);
                for (int p = 0; p < B * n; ++p) if (tok[(size_t)b * B * n + p] >= 0) ++want[tok[(size_t)b * B * n + p]];
                std::vector<std::vector<long>> part(bx.nlevels + 1);
                for (int l = 0; l < bx.nlevels; ++l) {
                    std::vector<long> out;
                    for (int k = 0; k < bx.item_cnt[l]; ++k) {
                        const SegItem it = ix.items[bx.item_off[l] + k];
                        if (it.end - it.begin > kWfoldChunk || it.end <= it.begin) { printf("bad item\n"); return 1; }
                        long s = 0;
                        for (int e = it.begin; e < it.end; ++e) {
                            if (l == 0) { const int r = ix.rows[bx.rows_off + e]; if (r < 0 || r >= B) { printf("bad row\n"); return 1; } s += 1; }
                            else s += part[l - 1].at(e);
                        }
                        if (it.dst >= 0) cnt.at(it.dst) += s;
                        else { if ((size_t)(-(it.dst + 1)) != out.size()) { printf("bad part\n"); return 1; } out.push_back(s); }
                    }
                    part[l] = out;
                }
                if (cnt != want) { printf("count mismatch\n"); return 1; }
            }
        }
    }
    printf("ok\n");
    return 0;
}
