// kernels_lbbounds.hpp — simple bounds of the L-BFGS direction as structure (include/pyipm_newton.h,
// pyipm_lbfgs_bounded_*).  A bound column +-e_k has one entry, so its slack and multiplier eliminate in closed form:
//
//   theta_k = zeta + sum_{j: var[j]=k} Sigma_j ,   ghat_x[k] = g_x[k] + sum_j sigma_j (Sigma_j g_li,j + g_s,j)
//   omega_k = sqrt(zeta / theta_k) ,  J~ = diag(omega) J_g ,  W~ = diag(omega) W ,  g~_x = omega ghat_x ,  dx = omega dx~
//   ds_j = sigma_j dx_k - g_li,j ,   dlambda_j = Sigma_j ds_j - g_s,j
//
// and the system in (dx~, ds_g, dlambda_g) is the one lbfgs_impl.hpp solves, on the scaled operands.  Everything here is
// HBM-bound glue around that pipeline: the weights (a gather from the variable's side over bounds_csr.hpp's CSR: no atomics,
// a fixed order), the scaled copy of the Jacobian operand, the weighted pack of V, and the tail.
// Vectors of the caller's layout ("full": mi = mg + mb, the bounds last in each inequality block) carry an F below.
#pragma once
#include "ctx.hpp"

namespace pyipm {

// One thread per variable: omega[k], and g[k] = ghat_x[k] of the reduced right-hand side.
//   gF: [g_x (n) | g_s (mg + mb) | g_le (me) | g_li (mg + mb)],  sigF: Sigma of all mg + mb inequalities.
__global__ __launch_bounds__(256) void k_bd_weights(double* __restrict__ om, double* __restrict__ g,
                                                    const double* __restrict__ gF, const double* __restrict__ sigF,
                                                    const int64_t* __restrict__ start, const int64_t* __restrict__ ent,
                                                    int64_t n, int64_t me, int64_t mg, int64_t mb, double zeta)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double* gs = gF + n + mg;                         // g_s of the bounds
    const double* gl = gF + n + (mg + mb) + me + mg;        // g_li of the bounds
    const double* sg = sigF + mg;
    double theta = zeta, corr = 0.0;
    const int64_t e1 = start[k + 1];
    for (int64_t e = start[k]; e < e1; ++e) {
        const int64_t code = ent[e];
        const int64_t j = code >= 0 ? code : ~code;
        const double sj = sg[j], t = fma(sj, gl[j], gs[j]);
        theta += sj;
        corr += code >= 0 ? t : -t;
    }
    om[k] = sqrt(zeta / theta);
    g[k] = gF[k] + corr;
}

// The rows below x of the reduced right-hand side: g[n + i] = [g_s,g (mg) | g_le (me) | g_li,g (mg)]
__global__ __launch_bounds__(256) void k_bd_gather_g(double* __restrict__ g, const double* __restrict__ gF, int64_t n,
                                                     int64_t me, int64_t mg, int64_t mb)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * mg + me) return;
    g[n + i] = gF[n + (i < mg ? i : i + mb)];
}

// JTs[c + k*ld] = omega[k] * JT[c + k*ld], k < n, c < ld (ld = p_pad, a multiple of 128; the padding rows of JT are zero
// and stay zero, the columns k >= n are not touched: they were cleared when the handle was made).
// A wave on one column of the operand at a time, 16 bytes per lane (1 KB contiguous per access), omega[k] wave-uniform,
// four columns in flight; a workgroup covers a run of 16 variables.
__global__ __launch_bounds__(256) void k_bd_scale(double* __restrict__ JTs, const double* __restrict__ JT, int64_t ld,
                                                  const double* __restrict__ om, int64_t n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t half = ld / 2;
    for (int64_t k0 = ((int64_t)blockIdx.x * 4 + wave) * 4; k0 < n; k0 += (int64_t)gridDim.x * 16) {
        const bool h1 = k0 + 1 < n, h2 = k0 + 2 < n, h3 = k0 + 3 < n;
        const double w0 = om[k0], w1 = h1 ? om[k0 + 1] : 0.0, w2 = h2 ? om[k0 + 2] : 0.0, w3 = h3 ? om[k0 + 3] : 0.0;
        const double2* src = reinterpret_cast<const double2*>(JT + k0 * ld);
        double2* dst = reinterpret_cast<double2*>(JTs + k0 * ld);
        for (int64_t c = lane; c < half; c += 64) {
            double2 a0 = src[c], a1, a2, a3;
            if (h1) a1 = src[c + half];
            if (h2) a2 = src[c + 2 * half];
            if (h3) a3 = src[c + 3 * half];
            a0.x *= w0; a0.y *= w0;
            dst[c] = a0;
            if (h1) { a1.x *= w1; a1.y *= w1; dst[c + half] = a1; }
            if (h2) { a2.x *= w2; a2.y *= w2; dst[c + 2 * half] = a2; }
            if (h3) { a3.x *= w3; a3.y *= w3; dst[c + 3 * half] = a3; }
        }
    }
}

// k_lb_pack with the row weights: V[k][0] = om[k] g[k] ; V[k][1+c] = om[k] cS S[k][c] ; V[k][1+m+c] = om[k] cY Y[k][c]
__global__ __launch_bounds__(256) void k_bd_pack(double* __restrict__ V, int rr, const double* __restrict__ g,
                                                 const double* __restrict__ S, int64_t ldS,
                                                 const double* __restrict__ Y, int64_t ldY, int64_t n, int m,
                                                 double cS, double cY, const double* __restrict__ om)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * rr) return;
    const int64_t k = idx / rr;
    const int c = (int)(idx - k * rr);
    double v;
    if (c == 0) v = g[k];
    else if (c <= m) v = cS * S[k * ldS + (c - 1)];
    else v = cY * Y[k * ldY + (c - 1 - m)];
    V[idx] = om[k] * v;
}

// The tail, one thread per variable.  With t~ = W~ v11 + J~ u of the reduced solve (dx~ = (g~_x - t~) / zeta) and
// a_k = g_x[k] - t~_k / omega_k, c_i = Sigma_i g_li,i + g_s,i over the bounds i of variable k:
//   dx_k = (a_k + sum_i sigma_i c_i) / theta_k                                              (= omega_k dx~_k)
//   ds_j = sigma_j dx_k - g_li,j
//        = (sigma_j a_k + g_s,j + sum_{i != j} sigma_j sigma_i c_i - (zeta + sum_{i != j} Sigma_i) g_li,j) / theta_k
//   dlambda_j = Sigma_j ds_j - g_s,j  -> sgn * .
// The second form of ds_j has the term Sigma_j g_li,j cancelled on paper: at a nearly active bound (Sigma_j large) dx_k and
// g_li,j agree to many digits, and their difference taken in floating point would lose those digits of ds_j, which
// Sigma_j then multiplies in dlambda_j.  A variable's bounds are walked in CSR order, twice (a segment is a few entries).
__global__ __launch_bounds__(256) void k_bd_tail(double* __restrict__ dzF, const double* __restrict__ V, int rr,
                                                 const double* __restrict__ v, int r, const double* __restrict__ Ju,
                                                 const double* __restrict__ om, const double* __restrict__ gF,
                                                 const double* __restrict__ sigF, const int64_t* __restrict__ start,
                                                 const int64_t* __restrict__ ent, int64_t n, int64_t me, int64_t mg,
                                                 int64_t mb, double zeta, double sgn)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t os = n + mg, ol = n + (mg + mb) + me + mg;
    const double* row = V + k * rr;
    double tt = Ju[k];
    for (int c = 0; c < r; ++c) tt = fma(row[1 + c], v[c], tt);
    const double a = gF[k] - tt / om[k];
    const int64_t e0 = start[k], e1 = start[k + 1];
    double theta = zeta, corr = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t code = ent[e];
        const int64_t j = code >= 0 ? code : ~code;
        const double sj = sigF[mg + j], c = fma(sj, gF[ol + j], gF[os + j]);
        theta += sj;
        corr += code >= 0 ? c : -c;
    }
    dzF[k] = (a + corr) / theta;
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t code = ent[e];
        const int64_t j = code >= 0 ? code : ~code;
        const double sgj = code >= 0 ? 1.0 : -1.0;
        double rest = zeta, num = fma(sgj, a, gF[os + j]);
        for (int64_t f = e0; f < e1; ++f) {
            if (f == e) continue;
            const int64_t cf = ent[f];
            const int64_t i = cf >= 0 ? cf : ~cf;
            const double si = sigF[mg + i], c = fma(si, gF[ol + i], gF[os + i]);
            rest += si;
            num += (cf >= 0) == (code >= 0) ? c : -c;
        }
        const double ds = fma(-rest, gF[ol + j], num) / theta;
        dzF[os + j] = ds;
        dzF[ol + j] = sgn * fma(sigF[mg + j], ds, -gF[os + j]);
    }
}

// The rows of the general constraints, as the pipeline left them (multiplier rows already flipped):
//   dzF_s[i] = dz_s[i], i < mg ;   dzF_l[j] = dz_l[j], j < me + mg
__global__ __launch_bounds__(256) void k_bd_scatter_dz(double* __restrict__ dzF, const double* __restrict__ dz, int64_t n,
                                                       int64_t me, int64_t mg, int64_t mb)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * mg + me) return;
    dzF[n + (i < mg ? i : i + mb)] = dz[n + i];
}

}  // namespace pyipm
