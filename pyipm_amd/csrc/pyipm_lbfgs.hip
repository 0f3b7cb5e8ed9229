// pyipm_lbfgs.hip -- the L-BFGS search direction (include/pyipm_lbfgs.h) as a translation unit of its own.  gfx950 only.
#include "driver.hpp"
using namespace pyipm;
using namespace pyipm::drv;
#include "kernels_lbfgs.hpp"
#pragma GCC visibility push(default)
#include "lbfgs_impl.hpp"
#include "qn_impl.hpp"                     // its quasi-Newton KKT operator (include/pyipm_newton.h, pyipm_qn_*)
#include "qnmany_impl.hpp"                 // ... for k columns per call (pyipm_lbfgs_kkt_matvec_many / _solve_many)
#include "pairs_impl.hpp"                  // the pair store that feeds it (include/pyipm_newton.h, "pair store")
#pragma GCC visibility pop
