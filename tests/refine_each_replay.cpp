// Replay of one problem's adaptive refinement on the CPU (tests/test_refine_each_plan.py compiles and runs it with the address and
// undefined-behaviour sanitizers): the state k_b_ref_round keeps per problem -- going / stopped, the steps taken, the error before
// the last step, the record -- moved by refine_each_verdict / refine_each_close of pyipm_amd/csrc/refine_each_plan.hpp, the source
// the kernel compiles, through the max_steps + 1 rounds the host enqueues.  The iterate is a number: a step adds one, a save keeps
// it, a take-back restores it.  Input, one case per line:  max_steps target count e_0 .. e_{count-1}  -- e_k is what the k-th
// measurement gives.  Output per case:  steps berr0 berr converged iterate visits  (%.17g; nan as printf writes it).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "refine_each_plan.hpp"

using namespace pyipm;

// the decision is usable in a constant expression (the kernel relies on nothing else of it)
static_assert(refine_each_verdict(0, -1.0, 1e-15, 8, 1e-14) == REFINE_EACH_CONVERGED, "");
static_assert(refine_each_verdict(0, -1.0, 1e-8, 8, 1e-14) == REFINE_EACH_GO_ON, "");
static_assert(refine_each_verdict(8, 1e-8, 1e-10, 8, 1e-14) == REFINE_EACH_STOP, "");
static_assert(refine_each_verdict(1, 1e-8, 2e-8, 8, 1e-14) == REFINE_EACH_TAKE_BACK, "");

int main() {
    int max_steps, count;
    double target;
    while (std::scanf("%d %lf %d", &max_steps, &target, &count) == 3) {
        std::vector<double> e((size_t)count);
        for (int k = 0; k < count; ++k)
            if (std::scanf("%lf", &e[(size_t)k]) != 1) { std::fprintf(stderr, "short case\n"); return 2; }
        int go = 1, it = 0, iterate = 0, saved = -1, visits = 0;
        double prev = -1.0;
        double info[4] = {-1.0, -1.0, -1.0, -1.0};
        for (int round = 0; round <= max_steps; ++round) {
            if (!go) continue;                                   // (the workgroups of a stopped problem return at once)
            if (visits >= count) { std::fprintf(stderr, "the script is too short: visit %d\n", visits); return 2; }
            const double berr = e[(size_t)visits++];
            if (it == 0) info[1] = berr;
            const RefineEachVerdict v = refine_each_verdict(it, prev, berr, max_steps, target);
            if (v == REFINE_EACH_GO_ON) {
                if (round == max_steps) { std::fprintf(stderr, "GO ON in the last round: no correction follows it\n"); return 3; }
                prev = berr; it += 1;
                saved = iterate;
                iterate += 1;                                    // the correction and the sum of this round
            } else {
                const RefineEachInfo o = refine_each_close(v, it, prev, berr, info[1]);
                info[0] = o.steps; info[2] = o.berr; info[3] = o.converged;
                go = 0;
                if (v == REFINE_EACH_TAKE_BACK) {
                    if (saved < 0) { std::fprintf(stderr, "take-back without a saved iterate\n"); return 3; }
                    iterate = saved;
                }
            }
        }
        if (go) { std::fprintf(stderr, "still going after max_steps + 1 rounds\n"); return 3; }
        std::printf("%.17g %.17g %.17g %.17g %d %d\n", info[0], info[1], info[2], info[3], iterate, visits);
    }
    return 0;
}
