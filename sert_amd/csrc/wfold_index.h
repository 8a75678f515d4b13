// Host-side builder of a word fold-in's per-batch inverted index NEW word -> batch rows of its occurrences
// (include/sert_hip_wfold.h; driven by host/api_wfold.inc over the kernels of kernels_seg.h).  Host code only.
//
// Batches are the fixed slices [iB, (i + 1)B) of the upload, so the index is built once, as word_index.h builds the full
// model's.  Per batch:
//   rows[]    one entry per occurrence of a new word: the batch row of the occurrence.  A word's entries are consecutive and
//             ascend by (row, position) -- a word twice in one window is two entries --, the words ascend.
//   level 0   one item per word with at most kWfoldChunk occurrences: {begin, end, dst = word, 0}; a longer list is cut into
//             chunks of kWfoldChunk entries (the last one shorter), each an item {begin, end, dst = -(p + 1), 0} that writes
//             partial row p of the level
//   level l   the same over the partial rows of level l - 1: a word's partial rows are consecutive and in chunk order, so
//             the chunk sums are added in chunk order
// until every word has a final item.  The item is word_index.h's SegItem, read as int4 by segsum_rows.  The association is
// a function of the upload alone.  Frozen positions (token -1) have no entry; a batch without a new word has no level.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "word_index.h"   // (SegItem, kSegChunk)

namespace sert {

constexpr int kWfoldChunk = kSegChunk;   // 64: the entries one lane group walks
constexpr int kWfoldMaxLevels = 6;       // 64^6 entries: more than a batch can hold

struct WfoldBatch {
    int64_t rows_off = 0;                      // offset of this batch's entries in rows[]
    int32_t num_entries = 0;
    int nlevels = 0;
    int64_t item_off[kWfoldMaxLevels] = {};    // offset into items[]
    int32_t item_cnt[kWfoldMaxLevels] = {};
    int64_t part_off[kWfoldMaxLevels] = {};    // partial-row offset of level l's OUTPUT space
    int64_t part_rows = 0;
};

struct WfoldIndex {
    std::vector<int32_t> rows;
    std::vector<SegItem> items;
    std::vector<WfoldBatch> batches;
    int64_t max_part_rows = 0;
};

// tok: (num_batches * B * n) the new word of every position in [0, num_words), or a negative value for a frozen position
// (validated by the caller).
inline void build_wfold_index(const int32_t* tok, int64_t num_batches, int B, int n, int num_words, WfoldIndex& out) {
    const int64_t T = (int64_t)B * n;
    out = WfoldIndex();
    out.batches.resize((size_t)num_batches);
    std::vector<int32_t> count((size_t)num_words, 0), touched;
    struct Seg { int32_t begin, end, word; };
    std::vector<Seg> segs, next;
    for (int64_t bi = 0; bi < num_batches; ++bi) {
        const int32_t* x = tok + bi * T;
        WfoldBatch& bx = out.batches[(size_t)bi];
        bx.rows_off = (int64_t)out.rows.size();
        // counting sort by word, stable in position
        touched.clear();
        for (int64_t p = 0; p < T; ++p)
            if (x[p] >= 0 && count[(size_t)x[p]]++ == 0) touched.push_back(x[p]);
        std::sort(touched.begin(), touched.end());
        segs.clear();
        int32_t acc = 0;
        for (int32_t v : touched) {
            const int32_t c = count[(size_t)v];
            segs.push_back({acc, acc + c, v});
            count[(size_t)v] = acc;            // write cursor
            acc += c;
        }
        bx.num_entries = acc;
        out.rows.resize((size_t)(bx.rows_off + acc));
        int32_t* rows = out.rows.data() + bx.rows_off;
        for (int64_t p = 0; p < T; ++p)
            if (x[p] >= 0) rows[count[(size_t)x[p]]++] = (int32_t)(p / n);
        for (int32_t v : touched) count[(size_t)v] = 0;
        // the levels
        int level = 0;
        int64_t part_base = 0;
        while (!segs.empty() && level < kWfoldMaxLevels) {
            bx.item_off[level] = (int64_t)out.items.size();
            bx.part_off[level] = part_base;
            next.clear();
            int32_t nparts = 0;
            for (const Seg& s : segs) {
                if (s.end - s.begin <= kWfoldChunk || level == kWfoldMaxLevels - 1) {
                    out.items.push_back({s.begin, s.end, s.word, 0});
                } else {
                    const int32_t first = nparts;
                    for (int32_t b = s.begin; b < s.end; b += kWfoldChunk) {
                        out.items.push_back({b, std::min(s.end, b + kWfoldChunk), -(nparts + 1), 0});
                        ++nparts;
                    }
                    next.push_back({first, nparts, s.word});
                }
            }
            bx.item_cnt[level] = (int32_t)((int64_t)out.items.size() - bx.item_off[level]);
            part_base += nparts;
            segs.swap(next);
            ++level;
        }
        bx.nlevels = level;
        bx.part_rows = part_base;
        out.max_part_rows = std::max(out.max_part_rows, part_base);
    }
}

}  // namespace sert
