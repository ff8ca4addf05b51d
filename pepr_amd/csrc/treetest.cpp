// treetest.cpp -- tree selection tests (include/peprml.h: pml_au_fit, pml_rell_tests, pml_tree_tests, pml_debug_rell, their
// *_weighted forms and pml_catpv_table):
// what TreeComparison.runConsel (TreeComparison.java:812-885) gets from `makermt -b 10 --puzzle | consel | catpv -v`.
// The resampling and the counting run on the device (rell.hip); the host fits the AU curve to ten integers per tree.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <numeric>

#include "../../include/peprml.h"
#include "api_types.hpp"

using namespace pml;

namespace {

// Phi^-1: Wichura's algorithm AS 241, routine PPND16 (Appl. Statist. 37 (1988) 477-484), relative accuracy about 1e-16
double ppnd16(double p) {
    static const double a[8] = {3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                                4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3};
    static const double b[8] = {1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
                                2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3};
    static const double c[8] = {1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                                1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4};
    static const double d[8] = {1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
                                1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};
    static const double e[8] = {6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                                2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7};
    static const double f[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                                7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15};
    auto poly = [](const double *k, double x) { double s = k[7]; for (int i = 6; i >= 0; --i) s = s * x + k[i]; return s; };
    const double q = p - 0.5;
    if (std::fabs(q) <= 0.425) { const double r = 0.180625 - q * q; return q * poly(a, r) / poly(b, r); }
    double r = q < 0 ? p : 1.0 - p;
    if (!(r > 0)) return q < 0 ? -HUGE_VAL : HUGE_VAL;
    r = std::sqrt(-std::log(r));
    const double v = r <= 5.0 ? poly(c, r - 1.6) / poly(d, r - 1.6) : poly(e, r - 5.0) / poly(f, r - 5.0);
    return q < 0 ? -v : v;
}
double norm_cdf(double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); }
double norm_pdf(double x) { return 0.39894228040143267794 * std::exp(-0.5 * x * x); }

// the scale whose n_k / N is closest to 1, the first of equals
int scale_k1(int K, const double *r) {
    int k1 = 0;
    for (int k = 1; k < K; ++k) if (std::fabs(r[k] - 1.0) < std::fabs(r[k1] - 1.0)) k1 = k;
    return k1;
}

int au_fit(int K, const double *r, const long long *count, long long B, double *au, double *d_out, double *c_out, double *rss_out, int *nused_out) {
    if (K <= 0 || !r || !count || B <= 0 || !au) return PML_EINVAL;
    for (int k = 0; k < K; ++k) if (!(r[k] > 0) || !std::isfinite(r[k]) || count[k] < 0 || count[k] > B) return PML_EINVAL;
    // weighted least squares z_k ~ d sqrt(r_k) + c / sqrt(r_k) (Shimodaira 2002, Syst. Biol. 51:492-508, eq. 9-11): normal equations
    double sxx = 0, sxy = 0, syy = 0, sxz = 0, syz = 0;
    int used = 0;
    std::vector<double> X(K), Y(K), Z(K), W(K, 0.0);
    for (int k = 0; k < K; ++k) {
        if (count[k] <= 0 || count[k] >= B) continue;
        const double p = (double)count[k] / (double)B, z = -ppnd16(p), ph = norm_pdf(z);
        const double w = (double)B * ph * ph / (p * (1.0 - p));
        X[k] = std::sqrt(r[k]); Y[k] = 1.0 / X[k]; Z[k] = z; W[k] = w;
        sxx += w * X[k] * X[k]; sxy += w * X[k] * Y[k]; syy += w * Y[k] * Y[k]; sxz += w * X[k] * Z[k]; syz += w * Y[k] * Z[k];
        ++used;
    }
    const double det = sxx * syy - sxy * sxy;
    double d = 0, c = 0, rss = 0, p_au;
    if (used >= 2 && det > 1e-12 * sxx * syy) {
        d = (sxz * syy - syz * sxy) / det;
        c = (syz * sxx - sxz * sxy) / det;
        for (int k = 0; k < K; ++k) if (W[k] > 0) { const double e = Z[k] - (d * X[k] + c * Y[k]); rss += W[k] * e * e; }
        p_au = 1.0 - norm_cdf(d - c);
    } else {
        // no curve to fit (fewer than two usable scales, or usable scales that do not determine d and c: all of one r):
        // the plain bootstrap probability; nused = 0 or 1 says that no fit was made
        p_au = (double)count[scale_k1(K, r)] / (double)B;
        used = std::min(used, 1);
    }
    *au = p_au;
    if (d_out) *d_out = d;
    if (c_out) *c_out = c;
    if (rss_out) *rss_out = rss;
    if (nused_out) *nused_out = used;
    return PML_OK;
}

struct DevBuf {          // device allocations of one call, released together
    std::vector<void *> p;
    ~DevBuf() { for (void *q : p) hipFree(q); }
    template <class T> hipError_t get(T **out, size_t n) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};
#define TCHK(expr)                                                                                               \
    do { const hipError_t e_ = (expr);                                                                           \
         if (e_ != hipSuccess) return c.fail(e_ == hipErrorOutOfMemory ? PML_ENOMEM : PML_EDEVICE, std::string("tree tests: " #expr ": ") + hipGetErrorString(e_)); } while (0)

struct Scales { std::vector<double> r; std::vector<int> nk; int k1 = 0; };

// what a weighted run (the weighted arm of k_rell) takes and gives on top of the plain one
struct Weighted {
    const double *isig_in = nullptr;        // host [T][T] 1 / sigma, or null: k_rell_pairsd
    std::vector<double> isig;               // [T][T] the matrix that was used
    std::vector<long long> wkh, wsh;        // [T]
};

// the resampling launch on a packed table: counts (and optionally every replicate sum and the kernel's HIP-event time) back
// path: 0 = LDS when the table fits, 1 = LDS or PML_EINVAL, 2 = global;  w: null = the plain arm, exactly as ever
int rell_run(Ctx &c, DevBuf &mem, const double *d_X, const double *d_L, int N, int T, const Scales &sc, long long B, unsigned long long seed,
             int path, double *y_out, long long *bp, long long *kh, long long *sh, int *path_used, double *ms_out, Weighted *w = nullptr) {
    const int K = (int)sc.nk.size(), tpad = (T + 1) & ~1;
    const bool fits = w ? rell_weighted_lds_fits(N, tpad, c.device) : rell_lds_fits(N, tpad, c.device);
    if (path == 1 && !fits) return c.fail(PML_EINVAL, w ? "the table and the 1 / sigma matrix do not fit the LDS path" : "the table does not fit the LDS path");
    bool lds = path == 2 ? false : fits;
    int *d_nk = nullptr; double *d_scale = nullptr, *d_Y = nullptr, *d_isig = nullptr; unsigned long long *d_cnt = nullptr;
    const size_t ncnt = (size_t)K * T + 2 * (size_t)T + (w ? 2 * (size_t)T : 0);
    std::vector<double> scale(K);
    for (int k = 0; k < K; ++k) scale[k] = (double)N / (double)sc.nk[k];
    TCHK(mem.get(&d_nk, K)); TCHK(mem.get(&d_scale, K)); TCHK(mem.get(&d_cnt, ncnt));
    if (y_out) TCHK(mem.get(&d_Y, (size_t)K * (size_t)B * T));
    TCHK(hipMemcpyAsync(d_nk, sc.nk.data(), sizeof(int) * K, hipMemcpyHostToDevice, c.stream));
    TCHK(hipMemcpyAsync(d_scale, scale.data(), sizeof(double) * K, hipMemcpyHostToDevice, c.stream));
    if (w) {
        TCHK(mem.get(&d_isig, (size_t)tpad * tpad));
        if (w->isig_in) {
            std::vector<double> pad((size_t)tpad * tpad, 0.0);
            for (int u = 0; u < T; ++u) for (int t = 0; t < T; ++t) pad[(size_t)u * tpad + t] = w->isig_in[(size_t)u * T + t];
            TCHK(hipMemcpy(d_isig, pad.data(), sizeof(double) * pad.size(), hipMemcpyHostToDevice));
        } else {
            launch_rell_pairsd(d_X, d_isig, N, T, tpad, c.stream);
            TCHK(hipGetLastError());
        }
    }
    RellWReq r;
    r.isig = d_isig; r.wkh = w ? d_cnt + (size_t)K * T + 2 * (size_t)T : nullptr; r.wsh = w ? r.wkh + T : nullptr;
    r.X = d_X; r.L = d_L; r.ndraws = d_nk; r.scale = d_scale; r.bp = d_cnt; r.kh = d_cnt + (size_t)K * T; r.sh = r.kh + T; r.Y = d_Y;
    r.base = (seed + 1ull) * 0x9E3779B97F4A7C15ull; r.B = (unsigned)B; r.N = N; r.T = T; r.tpad = tpad; r.K = K; r.k1 = sc.k1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct DropEv { hipEvent_t &a, &b; ~DropEv() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); } } dropev{ev0, ev1};
    if (ms_out) { TCHK(hipEventCreate(&ev0)); TCHK(hipEventCreate(&ev1)); }
    for (;;) {
        TCHK(hipMemsetAsync(d_cnt, 0, ncnt * sizeof(unsigned long long), c.stream));
        if (ms_out) TCHK(hipEventRecord(ev0, c.stream));
        const hipError_t e = w ? launch_rell_weighted(r, lds, c.stream) : launch_rell(r, lds, c.stream);
        if (e != hipSuccess && lds && path == 0) { lds = false; continue; }       // the runtime refused the LDS size: global path, same bits
        if (e != hipSuccess && lds) return c.fail(PML_EINVAL, std::string("the runtime refused the LDS path: ") + hipGetErrorString(e));
        TCHK(e);
        break;
    }
    if (ms_out) TCHK(hipEventRecord(ev1, c.stream));
    TCHK(hipStreamSynchronize(c.stream));
    TCHK(hipGetLastError());
    if (ms_out) { float ms = 0; TCHK(hipEventElapsedTime(&ms, ev0, ev1)); *ms_out = ms; }
    std::vector<unsigned long long> cnt(ncnt);
    TCHK(hipMemcpy(cnt.data(), d_cnt, ncnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)K * T; ++i) bp[i] = (long long)cnt[i];
    for (int t = 0; t < T; ++t) { kh[t] = (long long)cnt[(size_t)K * T + t]; sh[t] = (long long)cnt[(size_t)K * T + T + t]; }
    if (y_out) TCHK(hipMemcpy(y_out, d_Y, sizeof(double) * (size_t)K * (size_t)B * T, hipMemcpyDeviceToHost));
    if (w) {
        w->wkh.resize(T); w->wsh.resize(T); w->isig.resize((size_t)T * T);
        for (int t = 0; t < T; ++t) { w->wkh[t] = (long long)cnt[(size_t)K * T + 2 * (size_t)T + t]; w->wsh[t] = (long long)cnt[(size_t)K * T + 3 * (size_t)T + t]; }
        std::vector<double> pad((size_t)tpad * tpad);
        TCHK(hipMemcpy(pad.data(), d_isig, sizeof(double) * pad.size(), hipMemcpyDeviceToHost));
        for (int u = 0; u < T; ++u) for (int t = 0; t < T; ++t) w->isig[(size_t)u * T + t] = pad[(size_t)u * tpad + t];
    }
    if (path_used) *path_used = lds ? 1 : 2;
    return PML_OK;
}

// a host matrix (ntrees x nsites, the layout of RAxML_perSiteLLs) -> the packed table and its column sums on the device
int pack_host(Ctx &c, DevBuf &mem, int N, int T, const double *site_lnl, double **d_X, double **d_L) {
    const int tpad = (T + 1) & ~1;
    double *d_H = nullptr; const double **d_ptr = nullptr;
    TCHK(mem.get(&d_H, (size_t)T * N)); TCHK(mem.get(&d_ptr, T)); TCHK(mem.get(d_X, (size_t)N * tpad)); TCHK(mem.get(d_L, T));
    std::vector<const double *> ptr(T);
    for (int t = 0; t < T; ++t) ptr[t] = d_H + (size_t)t * N;
    TCHK(hipMemcpyAsync(d_H, site_lnl, sizeof(double) * (size_t)T * N, hipMemcpyHostToDevice, c.stream));
    TCHK(hipMemcpyAsync(d_ptr, ptr.data(), sizeof(double *) * T, hipMemcpyHostToDevice, c.stream));
    launch_rell_pack(d_ptr, nullptr, *d_X, *d_L, N, T, tpad, c.stream);
    TCHK(hipStreamSynchronize(c.stream));        // ptr (pageable) is free again
    return PML_OK;
}

int scales_from_opts(long long N, const pml_tree_test_opts *o, Scales &sc, long long &B, std::string &err) {
    const int K = (o && o->nscales > 0) ? o->nscales : 10;
    if (o && o->nscales < 0) { err = "nscales < 0"; return PML_EINVAL; }
    if (o && o->scales == nullptr && o->nscales > 0 && o->nscales != 10) { err = "nscales other than 10 needs the scales"; return PML_EINVAL; }
    B = (o && o->reps_per_scale > 0) ? o->reps_per_scale : 10000;
    if (o && o->reps_per_scale < 0) { err = "reps_per_scale < 0"; return PML_EINVAL; }
    if ((unsigned long long)K * (unsigned long long)B >= (1ull << 32)) { err = "nscales * reps_per_scale must stay below 2^32"; return PML_EINVAL; }
    sc.r.resize(K); sc.nk.resize(K);
    for (int k = 0; k < K; ++k) {
        const double rk = (o && o->scales) ? o->scales[k] : (5 + k) / 10.0;
        if (!(rk > 0) || !std::isfinite(rk) || rk * (double)N + 0.5 >= 2147483648.0) { err = "a scale must be positive and keep n_k below 2^31"; return PML_EINVAL; }
        sc.nk[k] = (int)std::max(1.0, std::floor(rk * (double)N + 0.5));
        sc.r[k] = (double)sc.nk[k] / (double)N;          // the scale actually drawn
    }
    sc.k1 = scale_k1(K, sc.r.data());
    return PML_OK;
}

template <class T> T *alloc_n(size_t n) { return (T *)std::calloc(std::max<size_t>(n, 1), sizeof(T)); }

// counts + column sums -> the table of p-values
int fill_result(int N, int T, const Scales &sc, long long B, const double *L, const double *lnl_report, std::vector<long long> &bp,
                std::vector<long long> &kh, std::vector<long long> &sh, pml_tree_test_result *out) {
    const int K = (int)sc.nk.size();
    pml_tree_test_result &R = *out;
    R.ntrees = T; R.nscales = K; R.k1 = sc.k1; R.nsites = N; R.reps = B;
    R.scales = alloc_n<double>(K); R.ndraws = alloc_n<long long>(K);
    R.lnl = alloc_n<double>(T); R.obs = alloc_n<double>(T); R.au = alloc_n<double>(T); R.np = alloc_n<double>(T); R.bp = alloc_n<double>(T);
    R.kh = alloc_n<double>(T); R.sh = alloc_n<double>(T); R.pp = alloc_n<double>(T); R.au_d = alloc_n<double>(T); R.au_c = alloc_n<double>(T);
    R.au_rss = alloc_n<double>(T); R.au_nused = alloc_n<int>(T); R.rank = alloc_n<int>(T);
    R.bp_count = alloc_n<long long>((size_t)K * T); R.kh_count = alloc_n<long long>(T); R.sh_count = alloc_n<long long>(T);
    if (!R.scales || !R.ndraws || !R.lnl || !R.obs || !R.au || !R.np || !R.bp || !R.kh || !R.sh || !R.pp || !R.au_d || !R.au_c || !R.au_rss ||
        !R.au_nused || !R.rank || !R.bp_count || !R.kh_count || !R.sh_count) return PML_ENOMEM;
    for (int k = 0; k < K; ++k) { R.scales[k] = sc.r[k]; R.ndraws[k] = sc.nk[k]; }
    std::memcpy(R.bp_count, bp.data(), sizeof(long long) * (size_t)K * T);
    std::memcpy(R.kh_count, kh.data(), sizeof(long long) * T);
    std::memcpy(R.sh_count, sh.data(), sizeof(long long) * T);
    int a = 0;
    for (int t = 1; t < T; ++t) if (L[t] > L[a]) a = t;
    int a2 = a == 0 ? 1 : 0;
    for (int t = a2 + 1; t < T; ++t) if (t != a && L[t] > L[a2]) a2 = t;
    double psum = 0;
    for (int t = 0; t < T; ++t) psum += std::exp(L[t] - L[a]);
    std::vector<int> order(T);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return L[x] > L[y]; });
    std::vector<long long> col(K);
    for (int t = 0; t < T; ++t) {
        R.lnl[t] = lnl_report ? lnl_report[t] : L[t];
        R.obs[t] = L[t == a ? a2 : a] - L[t];
        R.pp[t] = std::exp(L[t] - L[a]) / psum;
        R.np[t] = R.bp[t] = (double)bp[(size_t)sc.k1 * T + t] / (double)B;
        R.kh[t] = (double)kh[t] / (double)B; R.sh[t] = (double)sh[t] / (double)B;
        for (int k = 0; k < K; ++k) col[k] = bp[(size_t)k * T + t];
        if (int rc = au_fit(K, sc.r.data(), col.data(), B, &R.au[t], &R.au_d[t], &R.au_c[t], &R.au_rss[t], &R.au_nused[t])) return rc;
    }
    for (int i = 0; i < T; ++i) R.rank[order[i]] = i + 1;
    return PML_OK;
}

// counts + the matrix -> the weighted columns
int fill_weighted(int T, long long B, const double *L, const Weighted &w, pml_tree_test_weighted *out) {
    pml_tree_test_weighted &R = *out;
    R.ntrees = T;
    R.wkh = alloc_n<double>(T); R.wsh = alloc_n<double>(T); R.wkh_count = alloc_n<long long>(T); R.wsh_count = alloc_n<long long>(T);
    R.sigma = alloc_n<double>((size_t)T * T); R.wkh_other = alloc_n<int>(T);
    if (!R.wkh || !R.wsh || !R.wkh_count || !R.wsh_count || !R.sigma || !R.wkh_other) return PML_ENOMEM;
    for (int t = 0; t < T; ++t) {
        R.wkh_count[t] = w.wkh[t]; R.wsh_count[t] = w.wsh[t];
        R.wkh[t] = (double)w.wkh[t] / (double)B; R.wsh[t] = (double)w.wsh[t] / (double)B;
        // u* as the kernel chooses it: the same two rounded operations, the lowest index of equals
        int us = -1; double S = -HUGE_VAL;
        for (int u = 0; u < T; ++u) {
            const double is = w.isig[(size_t)t * T + u];
            R.sigma[(size_t)t * T + u] = is > 0.0 ? 1.0 / is : 0.0;
            if (u == t || !(is > 0.0)) continue;
            const double d = L[u] - L[t], q = d * is;
            if (q > S) { S = q; us = u; }
        }
        R.wkh_other[t] = us;
    }
    return PML_OK;
}

// a caller's 1 / sigma matrix: finite, >= 0, symmetric, 0 on the diagonal
bool isig_ok(const double *m, int T) {
    for (int u = 0; u < T; ++u) {
        if (m[(size_t)u * T + u] != 0.0) return false;
        for (int t = 0; t < T; ++t) {
            const double v = m[(size_t)u * T + t];
            if (!std::isfinite(v) || v < 0.0 || v != m[(size_t)t * T + u]) return false;
        }
    }
    return true;
}

bool shape_ok(long long N, int T) { return N >= 1 && N < 2147483648ll && T >= 2 && T <= 64; }

}  // namespace

extern "C" {

int pml_au_fit(int nscales, const double *r, const long long *count, long long B, double *au, double *d, double *c, double *rss, int *nused) {
    pml_fpguard fpg;
    try { return au_fit(nscales, r, count, B, au, d, c, rss, nused); }
    catch (const std::exception &) { return PML_ENOMEM; }
}

void pml_tree_test_result_free(pml_tree_test_result *R) {
    if (!R) return;
    void *p[] = {R->scales, R->ndraws, R->lnl, R->obs, R->au, R->np, R->bp, R->kh, R->sh, R->pp, R->au_d, R->au_c, R->au_rss, R->au_nused,
                 R->rank, R->bp_count, R->kh_count, R->sh_count};
    for (void *q : p) std::free(q);
    std::memset(R, 0, sizeof *R);
}

static int debug_rell(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, int nscales, const long long *ndraws, long long reps,
                      unsigned long long seed, int path, double *y_out, long long *bp_out, long long *kh_out, long long *sh_out, int *path_used,
                      double *kernel_ms_out, Weighted *w) {
    if (!ctx || !site_lnl || !ndraws || !bp_out || !kh_out || !sh_out || !shape_ok(nsites, ntrees) || nscales <= 0 || reps <= 0 || path < 0 || path > 2)
        return PML_EINVAL;
    if ((unsigned long long)nscales * (unsigned long long)reps >= (1ull << 32)) return PML_EINVAL;
    if (y_out && (double)nscales * (double)reps * ntrees > 134217728.0) return PML_EINVAL;          // every sum back: small shapes only (1 GiB)
    pml_fpguard fpg;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    Ctx &c = ctx->c;
    try {
        Scales sc; sc.r.resize(nscales); sc.nk.resize(nscales);
        for (int k = 0; k < nscales; ++k) {
            if (ndraws[k] < 1 || ndraws[k] >= 2147483648ll) return c.fail(PML_EINVAL, "n_k must be in [1, 2^31)");
            sc.nk[k] = (int)ndraws[k]; sc.r[k] = (double)ndraws[k] / (double)nsites;
        }
        sc.k1 = scale_k1(nscales, sc.r.data());
        pml_drop_worker_caches(ctx);
        TCHK(hipSetDevice(c.device));
        DevBuf mem; double *d_X = nullptr, *d_L = nullptr;
        if (int rc = pack_host(c, mem, (int)nsites, ntrees, site_lnl, &d_X, &d_L)) return rc;
        return rell_run(c, mem, d_X, d_L, (int)nsites, ntrees, sc, reps, seed, path, y_out, bp_out, kh_out, sh_out, path_used, kernel_ms_out, w);
    } catch (const std::bad_alloc &) { return c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return c.fail(PML_EINVAL, e.what()); }
}

int pml_debug_rell(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, int nscales, const long long *ndraws, long long reps,
                   unsigned long long seed, int path, double *y_out, long long *bp_out, long long *kh_out, long long *sh_out, int *path_used,
                   double *kernel_ms_out) {
    return debug_rell(ctx, nsites, ntrees, site_lnl, nscales, ndraws, reps, seed, path, y_out, bp_out, kh_out, sh_out, path_used, kernel_ms_out, nullptr);
}

int pml_debug_rell_weighted(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, int nscales, const long long *ndraws,
                            long long reps, unsigned long long seed, int path, double *y_out, long long *bp_out, long long *kh_out,
                            long long *sh_out, int *path_used, double *kernel_ms_out, const double *inv_sigma_in, double *inv_sigma_out,
                            long long *wkh_out, long long *wsh_out) {
    if (!ctx || !wkh_out || !wsh_out || !shape_ok(nsites, ntrees)) return PML_EINVAL;
    if (inv_sigma_in && !isig_ok(inv_sigma_in, ntrees)) return PML_EINVAL;
    try {
        Weighted w; w.isig_in = inv_sigma_in;
        const int rc = debug_rell(ctx, nsites, ntrees, site_lnl, nscales, ndraws, reps, seed, path, y_out, bp_out, kh_out, sh_out, path_used, kernel_ms_out, &w);
        if (rc) return rc;
        std::copy(w.wkh.begin(), w.wkh.end(), wkh_out); std::copy(w.wsh.begin(), w.wsh.end(), wsh_out);
        if (inv_sigma_out) std::copy(w.isig.begin(), w.isig.end(), inv_sigma_out);
        return PML_OK;
    } catch (const std::exception &) { return PML_ENOMEM; }
}

static int rell_tests(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, const pml_tree_test_opts *opts, pml_tree_test_result *out,
                      pml_tree_test_weighted *wout) {
    if (out) std::memset(out, 0, sizeof *out);
    if (wout) std::memset(wout, 0, sizeof *wout);
    if (!ctx || !site_lnl || !out || !shape_ok(nsites, ntrees)) return PML_EINVAL;
    pml_fpguard fpg;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    Ctx &c = ctx->c;
    int rc;
    try {
        Scales sc; long long B = 0; std::string err;
        if ((rc = scales_from_opts(nsites, opts, sc, B, err))) return c.fail(rc, err);
        const int N = (int)nsites, T = ntrees, K = (int)sc.nk.size();
        pml_drop_worker_caches(ctx);
        TCHK(hipSetDevice(c.device));
        DevBuf mem; double *d_X = nullptr, *d_L = nullptr;
        if ((rc = pack_host(c, mem, N, T, site_lnl, &d_X, &d_L))) return rc;
        std::vector<long long> bp((size_t)K * T), kh(T), sh(T); std::vector<double> L(T);
        TCHK(hipMemcpy(L.data(), d_L, sizeof(double) * T, hipMemcpyDeviceToHost));
        Weighted w;
        rc = rell_run(c, mem, d_X, d_L, N, T, sc, B, opts ? opts->seed : 0ull, 0, nullptr, bp.data(), kh.data(), sh.data(), nullptr, nullptr, wout ? &w : nullptr);
        if (!rc) rc = fill_result(N, T, sc, B, L.data(), nullptr, bp, kh, sh, out);
        if (!rc && wout) rc = fill_weighted(T, B, L.data(), w, wout);
        if (rc == PML_ENOMEM) c.fail(rc, "allocation failed");
    } catch (const std::bad_alloc &) { rc = c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = c.fail(PML_EINVAL, e.what()); }
    if (rc) { pml_tree_test_result_free(out); pml_tree_test_weighted_free(wout); }
    return rc;
}

int pml_rell_tests(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, const pml_tree_test_opts *opts, pml_tree_test_result *out) {
    return rell_tests(ctx, nsites, ntrees, site_lnl, opts, out, nullptr);
}
int pml_rell_tests_weighted(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, const pml_tree_test_opts *opts,
                            pml_tree_test_result *out, pml_tree_test_weighted *wout) {
    if (!wout) { if (out) std::memset(out, 0, sizeof *out); return PML_EINVAL; }
    return rell_tests(ctx, nsites, ntrees, site_lnl, opts, out, wout);
}

// The T candidate trees are the genes of ONE batch (the same alignment in each), optimised together as `raxmlHPC -f g` optimises
// each tree before it writes its per-site lnL; a gene's arithmetic does not depend on what shares its batch, so tree t carries
// the numbers of a pml_optimize call on it alone.  The table is gathered from the per-pattern lnL the last evaluation left
// in HBM: nothing but T scalars and the counts crosses the bus (plus the table itself when the caller asks for it).
static int tree_tests(pml_ctx *ctx, const pml_alignment *aln, int ntrees, const char *const *newicks, const pml_model *model,
                      const pml_search_opts *search_opts, const pml_tree_test_opts *test_opts, pml_tree_test_result *out,
                      pml_tree_test_weighted *wout, double *site_lnl_out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (wout) std::memset(wout, 0, sizeof *wout);
    if (!ctx || !aln || !newicks || !out || !shape_ok(aln->nsites, ntrees)) return PML_EINVAL;
    for (int t = 0; t < ntrees; ++t) if (!newicks[t]) return PML_EINVAL;
    pml_fpguard fpg;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    Ctx &c = ctx->c;
    Batch b;
    struct Drop { Batch &b; ~Drop() { b.destroy(); } } drop{b};
    int rc;
    try {
        const int N = aln->nsites, T = ntrees, tpad = (T + 1) & ~1;
        Scales sc; long long B = 0; std::string err;
        if ((rc = scales_from_opts(N, test_opts, sc, B, err))) return c.fail(rc, err);
        const int K = (int)sc.nk.size();
        pml_drop_worker_caches(ctx);
        static_assert(sizeof(pml_alignment) == sizeof(pml_alignment_view), "alignment view layout");
        std::vector<pml_alignment_view> views((size_t)T, pml_alignment_view{aln->ntax, aln->nsites, aln->names, aln->rows});
        rc = b.create(&c, T, views.data(), newicks, model ? model->pi_mode : PML_PI_RAXML_3DP, model ? model->ncat : 4, model ? model->alpha : 1.0,
                      search_opts == nullptr);
        if (rc) return rc;
        std::vector<double> lnl(T), again(T);
        if (search_opts) rc = b.optimize(search_opts->optimize_alpha != 0, search_opts->epsilon > 0 ? search_opts->epsilon : 1e-4, lnl.data());
        else rc = b.score(std::vector<char>(), lnl.data());
        if (!rc) rc = b.evaluate(std::vector<char>((size_t)T, 1), again.data());      // every tree's per-pattern lnL of its final state in d_patlnl[0]
        if (rc) return rc;
        const std::vector<int> &s2p = b.genes[0].aln.site2pat;
        for (int t = 0; t < T; ++t)
            if ((int)b.genes[t].aln.site2pat.size() != N || b.genes[t].aln.npat != b.genes[0].aln.npat) return c.fail(PML_EINVAL, "tree tests need the site map of the alignment");
        TCHK(hipSetDevice(c.device));
        DevBuf mem; double *d_X = nullptr, *d_L = nullptr; const double **d_ptr = nullptr; int *d_s2p = nullptr;
        TCHK(mem.get(&d_X, (size_t)N * tpad)); TCHK(mem.get(&d_L, T)); TCHK(mem.get(&d_ptr, T)); TCHK(mem.get(&d_s2p, N));
        std::vector<const double *> ptr(T);
        for (int t = 0; t < T; ++t) ptr[t] = b.genes[t].d_patlnl[0];
        TCHK(hipMemcpyAsync(d_ptr, ptr.data(), sizeof(double *) * T, hipMemcpyHostToDevice, c.stream));
        TCHK(hipMemcpyAsync(d_s2p, s2p.data(), sizeof(int) * N, hipMemcpyHostToDevice, c.stream));
        launch_rell_pack(d_ptr, d_s2p, d_X, d_L, N, T, tpad, c.stream);
        TCHK(hipStreamSynchronize(c.stream));
        std::vector<long long> bp((size_t)K * T), kh(T), sh(T); std::vector<double> L(T);
        TCHK(hipMemcpy(L.data(), d_L, sizeof(double) * T, hipMemcpyDeviceToHost));
        Weighted w;
        rc = rell_run(c, mem, d_X, d_L, N, T, sc, B, test_opts ? test_opts->seed : 0ull, 0, nullptr, bp.data(), kh.data(), sh.data(), nullptr, nullptr,
                      wout ? &w : nullptr);
        if (!rc && site_lnl_out) {                       // the very values that were resampled
            std::vector<double> X((size_t)N * tpad);
            TCHK(hipMemcpy(X.data(), d_X, sizeof(double) * X.size(), hipMemcpyDeviceToHost));
            for (int t = 0; t < T; ++t) for (int s = 0; s < N; ++s) site_lnl_out[(size_t)t * N + s] = X[(size_t)s * tpad + t];
        }
        if (!rc) rc = fill_result(N, T, sc, B, L.data(), lnl.data(), bp, kh, sh, out);
        if (!rc && wout) rc = fill_weighted(T, B, L.data(), w, wout);
        if (rc == PML_ENOMEM) c.fail(rc, "allocation failed");
    } catch (const std::bad_alloc &) { rc = c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = c.fail(PML_EINVAL, e.what()); }
    if (rc) { pml_tree_test_result_free(out); pml_tree_test_weighted_free(wout); }
    return rc;
}

int pml_tree_tests(pml_ctx *ctx, const pml_alignment *aln, int ntrees, const char *const *newicks, const pml_model *model,
                   const pml_search_opts *search_opts, const pml_tree_test_opts *test_opts, pml_tree_test_result *out, double *site_lnl_out) {
    return tree_tests(ctx, aln, ntrees, newicks, model, search_opts, test_opts, out, nullptr, site_lnl_out);
}
int pml_tree_tests_weighted(pml_ctx *ctx, const pml_alignment *aln, int ntrees, const char *const *newicks, const pml_model *model,
                            const pml_search_opts *search_opts, const pml_tree_test_opts *test_opts, pml_tree_test_result *out,
                            pml_tree_test_weighted *wout, double *site_lnl_out) {
    if (!wout) { if (out) std::memset(out, 0, sizeof *out); return PML_EINVAL; }
    return tree_tests(ctx, aln, ntrees, newicks, model, search_opts, test_opts, out, wout, site_lnl_out);
}

void pml_tree_test_weighted_free(pml_tree_test_weighted *R) {
    if (!R) return;
    void *p[] = {R->wkh, R->wsh, R->wkh_count, R->wsh_count, R->sigma, R->wkh_other};
    for (void *q : p) std::free(q);
    std::memset(R, 0, sizeof *R);
}

int pml_catpv_table(const pml_tree_test_result *r, const pml_tree_test_weighted *w, char **out) {
    if (out) *out = nullptr;
    if (!r || !out || r->ntrees < 1 || !r->rank || !r->obs || !r->au || !r->np || !r->bp || !r->pp || !r->kh || !r->sh) return PML_EINVAL;
    if (w && (w->ntrees != r->ntrees || !w->wkh || !w->wsh)) return PML_EINVAL;
    try {
        const int T = r->ntrees;
        std::vector<int> order(T);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return r->rank[x] < r->rank[y]; });
        char buf[256];
        std::snprintf(buf, sizeof buf, "# %4s %4s %8s %6s %6s | %6s %6s %6s %6s %6s %6s |", "rank", "item", "obs", "au", "np", "bp", "pp", "kh", "sh", "wkh", "wsh");
        std::string txt = buf;
        for (int t : order) {
            std::snprintf(buf, sizeof buf, "\n# %4d %4d %8.1f %6.3f %6.3f | %6.3f %6.3f %6.3f %6.3f", r->rank[t], t + 1, r->obs[t], r->au[t], r->np[t], r->bp[t],
                          r->pp[t], r->kh[t], r->sh[t]);
            txt += buf;
            if (w) std::snprintf(buf, sizeof buf, " %6.3f %6.3f |", w->wkh[t], w->wsh[t]);
            else std::snprintf(buf, sizeof buf, " %6s %6s |", "-", "-");
            txt += buf;
        }
        char *p = (char *)std::malloc(txt.size() + 1);
        if (!p) return PML_ENOMEM;
        std::memcpy(p, txt.c_str(), txt.size() + 1);
        *out = p;
        return PML_OK;
    } catch (const std::exception &) { return PML_ENOMEM; }
}

}  // extern "C"
