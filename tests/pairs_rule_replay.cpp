// Replay of the L-BFGS pair store's host rule on the CPU (tests/test_pairs_rule.py compiles and runs it with the address and
// undefined-behaviour sanitizers): pyipm_amd/csrc/pairs_rule.hpp, the source the library compiles, fed with products that NumPy
// computed.  All floating-point numbers travel as C99 hexadecimal literals, so a comparison of the output is bit for bit.
// Input, one case:  memory constrained zeta0 eps offers  and then per offer  k inner_0 .. inner_{k-1} cross_0 .. cross_{k-1} curv den
// with k = kept() + 1 -- checked here against the rule's own count.  Output per offer, one line:
// outcome m fail zeta SS (m*m) L (m*m) D (m*m).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pairs_rule.hpp"

using namespace pyipm;

static bool rd(double* v) {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) return false;
    char* end = nullptr;
    *v = std::strtod(tok, &end);
    return end && *end == 0;
}

int main() {
    int memory, con, offers;
    while (std::scanf("%d %d", &memory, &con) == 2) {
        double zeta0, eps;
        if (!rd(&zeta0) || !rd(&eps) || std::scanf("%d", &offers) != 1) { std::fprintf(stderr, "bad case header\n"); return 2; }
        PairsRule rule;
        rule.init(memory, con != 0, zeta0);
        for (int t = 0; t < offers; ++t) {
            int k;
            if (std::scanf("%d", &k) != 1) { std::fprintf(stderr, "short case\n"); return 2; }
            if (k != rule.kept() + 1) { std::fprintf(stderr, "offer %d: %d products, the rule expects %d\n", t, k, rule.kept() + 1); return 3; }
            std::vector<double> inner((size_t)k), cross((size_t)k);
            double curv, den;
            for (int i = 0; i < k; ++i) if (!rd(&inner[(size_t)i])) return 2;
            for (int i = 0; i < k; ++i) if (!rd(&cross[(size_t)i])) return 2;
            if (!rd(&curv) || !rd(&den)) return 2;
            const int out = rule.offer(inner.data(), cross.data(), curv, den, eps);
            const size_t mm = (size_t)rule.m * (size_t)rule.m;
            if (rule.SS.size() != mm || rule.L.size() != mm || rule.D.size() != mm) { std::fprintf(stderr, "SS / L / D are not m x m\n"); return 3; }
            std::printf("%d %d %lld %a", out, rule.m, (long long)rule.fail, rule.zeta);
            for (const std::vector<double>* a : {&rule.SS, &rule.L, &rule.D})
                for (double v : *a) std::printf(" %a", v);
            std::printf("\n");
        }
    }
    return 0;
}
