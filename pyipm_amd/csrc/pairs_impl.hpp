// pairs_impl.hpp -- host orchestration + C-ABI of the L-BFGS pair store (include/pyipm_newton.h, "pair store").
// Included at the end of pyipm_lbfgs.hip.  The device half is kernels_pairs.hpp, the accept / skip / reset rule and the
// SS / L / D bookkeeping are pairs_rule.hpp (host only).
#pragma once
#include "../../include/pyipm_newton.h"
#include "kernels_pairs.hpp"
#include "pairs_rule.hpp"

namespace {

struct PairsCtx {
    int64_t n = 0;
    int memory = 0, cap = 0, lg = 2, device = 0;
    hipStream_t stream = nullptr;
    DevBuf<char> ws;
    double *St = nullptr;               // n x 2 cap: [S | Y] row by row (kernels_pairs.hpp)
    double *dx = nullptr, *dg = nullptr;            // the offered pair, until it is committed
    double *in[4] = {nullptr, nullptr, nullptr, nullptr};   // staging of host x_old, x_new, g_old, g_new
    double *part = nullptr;             // PAIRS_GBLK x PAIRS_PSTRIDE partial sums
    double *prods = nullptr;            // [inner | cross | curv | den]: ONE device buffer (a later all-reduce goes here)
    PinnedBuf<double> hprods;           // where the one copy per offer lands
    PairsRule rule;
    std::string err;
};

inline PairsCtx* PR(pyipm_pairs* h) { return reinterpret_cast<PairsCtx*>(h); }

#define PR_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e__ = (call);                                                          \
        if (e__ != hipSuccess) {                                                          \
            pr->err = std::string(#call) + ": " + hipGetErrorString(e__);                 \
            return PYIPM_E_HIP;                                                           \
        }                                                                                 \
    } while (0)

inline bool pairs_geometry_ok(int64_t n, int memory) { return n > 0 && memory >= 1 && memory <= 31; }

// Device layout of a store; returns total bytes, sets pointers when base != nullptr.
size_t pairs_carve(PairsCtx* c, int64_t n, int cap, char* base) {
    Carve cv;
    const size_t D = sizeof(double);
    const size_t oSt = cv.take((size_t)n * (size_t)(2 * cap) * D);
    const size_t odx = cv.take((size_t)n * D), odg = cv.take((size_t)n * D);
    size_t oin[4];
    for (int i = 0; i < 4; ++i) oin[i] = cv.take((size_t)n * D);
    const size_t opart = cv.take((size_t)PAIRS_GBLK * PAIRS_PSTRIDE * D);
    const size_t oprods = cv.take((size_t)PAIRS_PSTRIDE * D);
    if (base) {
        c->St = (double*)(base + oSt); c->dx = (double*)(base + odx); c->dg = (double*)(base + odg);
        for (int i = 0; i < 4; ++i) c->in[i] = (double*)(base + oin[i]);
        c->part = (double*)(base + opart); c->prods = (double*)(base + oprods);
    }
    return cv.off;
}

}  // namespace

#undef PYIPM_CATCH_H
#define PYIPM_SETERR_PAIRS(msg_) set_err_noexcept(reinterpret_cast<PairsCtx*>(p), (msg_))
#define PYIPM_CATCH_H(h_)  PYIPM_CATCH_CORE(PYIPM_SETERR_PAIRS, PYIPM_E_NOMEM, PYIPM_E_HIP)

extern "C" {

size_t pyipm_pairs_workspace_bytes(int64_t n, int memory) try {
    if (!pairs_geometry_ok(n, memory)) return 0;
    return pairs_carve(nullptr, n, memory + 1, nullptr);
} PYIPM_CATCH_SIZE

int pyipm_pairs_create(pyipm_pairs** out, int64_t n, int memory, int constrained, double zeta0, int device,
                       void* stream) try {
    if (!out) return PYIPM_E_BADARG;
    *out = nullptr;
    if (!pairs_geometry_ok(n, memory) || !(zeta0 > 0.0)) return PYIPM_E_BADARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PYIPM_E_NODEVICE;
    if (hipSetDevice(device) != hipSuccess) return PYIPM_E_NODEVICE;
    std::unique_ptr<PairsCtx> pr(new PairsCtx());      // an early return releases what the store owns by then
    pr->n = n; pr->memory = memory; pr->cap = memory + 1; pr->lg = pairs_lanes_log2(pr->cap);
    pr->device = device; pr->stream = (hipStream_t)stream;
    pr->rule.init(memory, constrained != 0, zeta0);
    const size_t bytes = pairs_carve(nullptr, n, pr->cap, nullptr);
    if (pr->ws.reserve(bytes) != hipSuccess) return PYIPM_E_NOMEM;
    if (getenv("PYIPM_POISON_WORKSPACE")) hipMemset(pr->ws, 0xFF, bytes);      // test hook, as in pyipm_lbfgs_create
    pairs_carve(pr.get(), n, pr->cap, pr->ws);
    if (pr->hprods.reserve(PAIRS_PSTRIDE) != hipSuccess) return PYIPM_E_NOMEM;
    *out = reinterpret_cast<pyipm_pairs*>(pr.release());
    return PYIPM_OK;
} PYIPM_CATCH_NOH

int pyipm_pairs_destroy(pyipm_pairs* p) try {
    if (!p) return PYIPM_E_BADARG;
    PairsCtx* pr = PR(p);
    hipSetDevice(pr->device);
    hipStreamSynchronize(pr->stream);
    delete pr;
    return PYIPM_OK;
} PYIPM_CATCH_H(p)

const char* pyipm_pairs_last_error(pyipm_pairs* p) {
    if (!p) return "null handle";
    return PR(p)->err.c_str();
}

int pyipm_pairs_set_stream(pyipm_pairs* p, void* stream) try {
    if (!p) return PYIPM_E_BADARG;
    PR(p)->stream = (hipStream_t)stream;
    return PYIPM_OK;
} PYIPM_CATCH_H(p)

int pyipm_pairs_reset(pyipm_pairs* p) try {
    if (!p) return PYIPM_E_BADARG;
    PR(p)->rule.reset();                 // (the columns stay where they are: m = 0 hides them)
    return PYIPM_OK;
} PYIPM_CATCH_H(p)

int pyipm_pairs_offer(pyipm_pairs* p, const double* x_old, const double* x_new, const double* g_old,
                      const double* g_new, double eps, int memkind, int* outcome) try {
    if (!p) return PYIPM_E_BADARG;
    PairsCtx* pr = PR(p);
    if (!x_old || !x_new || !g_old || !g_new || !outcome) { pr->err = "offer: null x / g / outcome pointer"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_HOST && memkind != PYIPM_MEM_DEVICE) { pr->err = "offer: unknown memkind"; return PYIPM_E_BADARG; }
    PR_HIP(hipSetDevice(pr->device));
    hipStream_t st = pr->stream;
    const int64_t n = pr->n;
    const double* src[4] = {x_old, x_new, g_old, g_new};
    if (memkind == PYIPM_MEM_HOST)
        for (int i = 0; i < 4; ++i) {
            PR_HIP(hipMemcpyAsync(pr->in[i], src[i], (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
            src[i] = pr->in[i];
        }
    PairsRule& rule = pr->rule;
    const int m = rule.m, drop = rule.drops() ? 1 : 0, k = rule.kept() + 1, con = rule.constrained ? 1 : 0;
    hipLaunchKernelGGL(k_pairs_products, dim3(PAIRS_GBLK), dim3(256), 0, st, pr->part, pr->dx, pr->dg, pr->St, pr->cap, m, drop,
                       pr->lg, src[0], src[1], src[2], src[3], n, con);
    PR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pairs_reduce, dim3(1), dim3(512), 0, st, pr->prods, pr->part, pr->cap, m, drop, con);
    PR_HIP(hipGetLastError());
    double* h = pr->hprods;
    PR_HIP(hipMemcpyAsync(h, pr->prods, (size_t)(2 * k + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
    PR_HIP(hipStreamSynchronize(st));            // the one synchronisation of an offer (host inputs are free from here on)
    const int res = rule.offer(h, h + k, h[2 * k], h[2 * k + 1], eps);
    if (res == PAIRS_ACCEPTED) {
        const int64_t rows_per_block = drop ? 4 * (64 >> pr->lg) : 256;
        hipLaunchKernelGGL(k_pairs_commit, dim3((unsigned)((n + rows_per_block - 1) / rows_per_block)), dim3(256), 0, st,
                           pr->St, pr->cap, m, drop, pr->lg, pr->dx, pr->dg, n);
        PR_HIP(hipGetLastError());
    }
    *outcome = res;
    return PYIPM_OK;
} PYIPM_CATCH_H(p)

int pyipm_pairs_view_get(pyipm_pairs* p, pyipm_pairs_view* v) try {
    if (!p) return PYIPM_E_BADARG;
    PairsCtx* pr = PR(p);
    if (!v) { pr->err = "view_get: null view pointer"; return PYIPM_E_BADARG; }
    v->m = pr->rule.m; v->ld = 2 * pr->cap;
    v->S = pr->St; v->Y = pr->St + pr->cap;
    v->SS = pr->rule.SS.data(); v->L = pr->rule.L.data(); v->D = pr->rule.D.data();
    v->zeta = pr->rule.zeta; v->fail = pr->rule.fail;
    return PYIPM_OK;
} PYIPM_CATCH_H(p)

}  // extern "C"
