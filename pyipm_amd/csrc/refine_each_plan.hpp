// refine_each_plan.hpp -- what one problem of a batch does after a measurement of its backward error during adaptive
// refinement (pyipm_newton_refine_batched; k_b_ref_round, kernels_brefine.hpp): the rule of drv::refine_loop with refine < 0
// (driver.hpp), stated for ONE problem as a function of its own state.  Plain C++: nothing of HIP or of the handle in it; the
// functions are constexpr so that the kernel and a stand-alone replay (tests/test_refine_each_plan.py) compile this one source.
//
// A visit: `it` steps have been taken, `prev` is the error measured before the last of them (< 0: none yet), `berr` the error
// just measured from the blocks.  The order of the tests is refine_loop's:
//   the last step made it worse, or the measurement is not a number    -> TAKE BACK the saved iterate; that step is not counted
//   NaN / Inf with no step taken                                        -> STOP, nothing done
//   berr <= target                                                      -> CONVERGED
//   it == max_steps, or the last step gained less than 4x               -> STOP
//   otherwise                                                           -> GO ON: save the iterate, take a step
#pragma once
namespace pyipm {
enum RefineEachVerdict : int { REFINE_EACH_CONVERGED = 0, REFINE_EACH_TAKE_BACK = 1, REFINE_EACH_STOP = 2, REFINE_EACH_GO_ON = 3 };

constexpr RefineEachVerdict refine_each_verdict(int it, double prev, double berr, int max_steps, double target) {
    if (prev >= 0.0 && !(berr <= prev)) return REFINE_EACH_TAKE_BACK;
    if (!(berr <= 1.0e300)) return REFINE_EACH_STOP;
    if (berr <= target) return REFINE_EACH_CONVERGED;
    if (it >= max_steps || (prev >= 0.0 && berr > 0.25 * prev)) return REFINE_EACH_STOP;
    return REFINE_EACH_GO_ON;
}

// The record of a problem: the layout of pyipm_newton_solve_info.  berr0 is written at the first visit; a verdict other than
// GO ON closes the record (TAKE BACK: the kept iterate is the saved one -- its error, one step fewer).
struct RefineEachInfo { double steps, berr0, berr, converged; };
constexpr RefineEachInfo refine_each_close(RefineEachVerdict v, int it, double prev, double berr, double berr0) {
    return v == REFINE_EACH_TAKE_BACK ? RefineEachInfo{(double)(it - 1), berr0, prev, 0.0}
                                      : RefineEachInfo{(double)it, berr0, berr, v == REFINE_EACH_CONVERGED ? 1.0 : 0.0};
}
}  // namespace pyipm
