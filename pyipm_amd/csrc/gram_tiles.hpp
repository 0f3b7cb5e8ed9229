// gram_tiles.hpp -- which 128 x 128 tiles of J'J = [Je | Ji]'[Je | Ji] a partial restaging of the Jacobians leaves stale
// (include/pyipm_newton.h, pyipm_lbfgs_stage_jacobian_columns), and the tile list the restricted Gram launch walks.
// No HIP in here: tests/gram_tiles_replay.cpp compiles it under the host compiler alone.
//
// Column c of J belongs to tile index c / 128.  When the columns of tile index d change, the lower-triangle tiles
// (i, j), i >= j, with i == d or j == d change and no other: a handle keeps the set of such d between two directions.
#pragma once
#include <stdint.h>
#include <vector>

namespace pyipm {

constexpr int64_t GT_TILE = 128;                 // = BM = the column tile of k_update<128>
constexpr unsigned GT_PAD = 0xffffffffu;         // a list entry without a tile (k_update skips it)

struct GramTiles {
    int nt = 0;                                  // tile indices of the padded matrix (p_pad / 128)
    int ndirty = 0;
    std::vector<unsigned char> dirty;            // per tile index

    void init(int64_t p_pad) { nt = (int)(p_pad / GT_TILE); dirty.assign((size_t)nt, 0); ndirty = 0; }
    void clear() { dirty.assign((size_t)nt, 0); ndirty = 0; }
    bool any() const { return ndirty > 0; }
    bool all() const { return ndirty == nt; }
    // columns [c0, c0 + count) changed; 0 <= c0, c0 + count <= p_pad (the caller has checked)
    void mark(int64_t c0, int64_t count) {
        if (count <= 0) return;
        for (int64_t t = c0 / GT_TILE; t <= (c0 + count - 1) / GT_TILE; ++t)
            if (!dirty[(size_t)t]) { dirty[(size_t)t] = 1; ++ndirty; }
    }
    // lower-triangle tiles with a dirty row or column index: all of them but those among the clean indices
    int64_t tile_count() const {
        const int64_t clean = nt - ndirty;
        return (int64_t)nt * (nt + 1) / 2 - clean * (clean + 1) / 2;
    }
    static int64_t list_capacity(int64_t p_pad) {               // entries list() can produce for this order, padding included
        const int64_t t = p_pad / GT_TILE;
        return t * (t + 1) / 2 + 8;
    }
    // The dirty tiles as k_update's tile list: entry = row tile | column tile << 16, length a multiple of 8, entry b going
    // to the XCD b % 8 serves.  As in the full launch's list (tile_list, pyipm_newton.hip) the matrix is walked in 8 x 8
    // super-tiles, column by column, each super-tile's tiles staying on one XCD so that its operand strips are reused from
    // that L2; the sequences are then evened out and the shorter ones padded.  The order decides no bit of the result:
    // every tile is owned by one workgroup.
    void list(std::vector<unsigned>& out) const {
        std::vector<unsigned> seq[8];
        const int ns = (nt + 7) / 8;
        int next = 0;
        for (int sJ = 0; sJ < ns; ++sJ)
            for (int sI = sJ; sI < ns; ++sI) {
                std::vector<unsigned>& s = seq[next & 7];
                const size_t before = s.size();
                for (int w = 0; w < 64; ++w) {
                    const int rt = sI * 8 + (w & 7), ct = sJ * 8 + (w >> 3);
                    if (rt >= nt || ct >= nt || rt < ct) continue;
                    if (dirty[(size_t)rt] || dirty[(size_t)ct]) s.push_back((unsigned)rt | ((unsigned)ct << 16));
                }
                if (s.size() != before) ++next;
            }
        size_t total = 0;
        for (const auto& s : seq) total += s.size();
        const size_t target = (total + 7) / 8;
        std::vector<unsigned> spare;
        for (auto& s : seq) while (s.size() > target) { spare.push_back(s.back()); s.pop_back(); }
        for (auto& s : seq) while (s.size() < target && !spare.empty()) { s.push_back(spare.back()); spare.pop_back(); }
        out.assign(8 * target, GT_PAD);
        for (int x = 0; x < 8; ++x)
            for (size_t j = 0; j < seq[x].size(); ++j) out[8 * j + (size_t)x] = seq[x][j];
    }
};

}  // namespace pyipm
