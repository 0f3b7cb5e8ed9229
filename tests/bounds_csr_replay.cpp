// bounds_csr_replay.cpp -- pyipm_amd/csrc/bounds_csr.hpp (the bounds of a bounded L-BFGS handle grouped by variable) under
// the host compiler and its sanitizers: tests/test_lbfgs_bounds_abi.py feeds cases on stdin and checks the lines.
//   in : n mb  var_0 sign_0 ... var_{mb-1} sign_{mb-1}        (one case per line; sign as an integer)
//   out: "ok" start_0 .. start_n | ent_0 .. ent_{mb-1}         or   "refused" <reason>
// A refused case is followed by a check that the structure still holds what the case before it built.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "bounds_csr.hpp"

int main() {
    pyipm::BoundsCsr csr;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        long long n = 0, mb = 0;
        in >> n >> mb;
        std::vector<int64_t> var;
        std::vector<double> sign;
        for (long long j = 0; j < mb; ++j) {
            long long v = 0, s = 0;
            in >> v >> s;
            var.push_back((int64_t)v);
            sign.push_back((double)s);
        }
        const std::vector<int64_t> start0 = csr.start, ent0 = csr.ent;
        const char* why = csr.build((int64_t)n, (int64_t)mb, mb > 0 ? var.data() : nullptr, mb > 0 ? sign.data() : nullptr);
        if (why) {
            if (csr.start != start0 || csr.ent != ent0) { std::printf("refused but changed\n"); return 1; }
            std::printf("refused %s\n", why);
            continue;
        }
        std::printf("ok");
        for (int64_t v : csr.start) std::printf(" %lld", (long long)v);
        std::printf(" |");
        for (int64_t c : csr.ent)
            std::printf(" %lld:%d", (long long)pyipm::BoundsCsr::index_of(c), (int)pyipm::BoundsCsr::sign_of(c));
        std::printf("\n");
    }
    return 0;
}
