// Replays pyipm_amd/csrc/gram_tiles.hpp (the header the library compiles) for tests/test_lbfgs_columns_abi.py.
// stdin, one case per line:  p_pad nranges (c0 count)*      stdout, one line per case:
//   ndirty all tile_count list_capacity list_length code*      (the codes of list(), padding included)
#include <stdio.h>
#include <vector>
#include "gram_tiles.hpp"

int main() {
    long long p_pad; int nr;
    while (scanf("%lld %d", &p_pad, &nr) == 2) {
        pyipm::GramTiles t;
        t.init(p_pad);
        for (int k = 0; k < nr; ++k) {
            long long c0, count;
            if (scanf("%lld %lld", &c0, &count) != 2) return 2;
            t.mark(c0, count);
        }
        std::vector<unsigned> list;
        t.list(list);
        printf("%d %d %lld %lld %zu", t.ndirty, t.all() ? 1 : 0, (long long)t.tile_count(),
               (long long)pyipm::GramTiles::list_capacity(p_pad), list.size());
        for (unsigned c : list) printf(" %u", c);
        printf("\n");
        // a handle's life: cleared by the next Gram launch, marked again
        t.clear();
        if (t.any() || t.tile_count() != 0) return 3;
        t.mark(0, p_pad);
        if (!t.all()) return 4;
    }
    return 0;
}
